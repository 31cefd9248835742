"""Host state of the turbulence stirring (sx_turb_*, sph-exa_amd/csrc/sx_turb.cpp) against the numpy / Python
restatement in turb_ref.py.  No GPU: the library is loaded, no device call is made.

The restatement repeats the library's operations in the same order with the same libm, so equality is expected; the
comparisons allow 4 ulp.
"""
import math

import numpy as np
import pytest

import sphexa_amd as sx
import turb_ref as tr

ULP = 4.0


def settings(**kw):
    s = dict(tr.DEFAULTS)
    s.update(kw)
    return s


@pytest.fixture
def make():
    made = []

    def f(**kw):
        t = sx.Turbulence(**kw)
        made.append(t)
        return t

    yield f
    for t in made:
        t.close()


@pytest.mark.parametrize("form", [1, 0])
def test_mode_table_and_constants(make, form):
    s = settings(stSpectForm=form)
    t = make(stSpectForm=form)
    c = tr.constants(s)
    modes, amps = tr.mode_table(s)
    assert t.num_modes == len(amps)
    if form == 1:
        assert t.num_modes == 112 and t.max_index() == 3
    sc, ar = t.scalars(), t.arrays()
    for k in ("variance", "decayTime", "solWeightNorm"):
        assert tr.ulp_diff(sc[k], c[k]) <= ULP, (k, sc[k], c[k])
    assert sc["solWeight"] == s["solWeight"]
    got = ar["modes"].reshape(-1, 3)
    assert np.array_equal(np.signbit(got), np.signbit(modes))  # -0.0 where the reference negates a zero component
    nz = modes != 0
    assert np.all(got[~nz] == 0)
    assert np.max(tr.ulp_diff(got[nz], modes[nz])) <= ULP
    assert np.max(tr.ulp_diff(ar["amplitudes"], amps)) <= ULP


def test_mode_cap(make):
    """createStirringModes refuses a lattice point once numModes + 4 would exceed stMaxModes"""
    s = settings(stMaxModes=30)
    t = make(stMaxModes=30)
    modes, amps = tr.mode_table(s)
    assert t.num_modes == len(amps) == 28
    assert np.max(tr.ulp_diff(t.arrays()["amplitudes"], amps)) <= ULP


def test_form2_structure(make):
    s = settings(stSpectForm=2)
    c = tr.constants(s)
    t = make(stSpectForm=2)
    m = t.num_modes
    assert 0 < m <= s["stMaxModes"]
    ar = t.arrays()
    modes = ar["modes"].reshape(-1, 3)
    r = modes * s["Lbox"] / (2.0 * math.pi)
    assert np.max(np.abs(r - np.rint(r))) < 1e-12  # integer multiples of 2 pi / L per axis
    k = np.sqrt(np.sum(modes * modes, axis=1))
    assert np.all(k >= c["stirMin"]) and np.all(k <= c["stirMax"])
    assert t.max_index() <= 3
    assert np.all(ar["amplitudes"] > 0)
    t2 = make(stSpectForm=2)
    assert np.array_equal(t2.arrays()["modes"], ar["modes"]) and np.array_equal(t2.arrays()["phases"], ar["phases"])
    t3 = make(stSpectForm=2, rngSeed=7)
    assert t3.num_modes != m or not np.array_equal(t3.arrays()["modes"], ar["modes"])
    capped = make(stSpectForm=2, stMaxModes=20)
    assert capped.num_modes <= 20


def test_initial_phases_seed_251299(make):
    t = make()
    c = tr.constants(tr.DEFAULTS)
    rng = tr.StdRng(251299)
    want = rng.normals(6 * t.num_modes, 0.0, c["variance"])
    got = t.arrays()["phases"]
    assert got.shape == want.shape
    assert np.max(tr.ulp_diff(got, want)) <= ULP
    assert abs(np.std(got) / c["variance"] - 1) < 0.1


def test_ou_step_and_projection(make):
    t = make()
    s = tr.DEFAULTS
    c = tr.constants(s)
    modes = t.arrays()["modes"].reshape(-1, 3)
    rng = tr.StdRng(s["rngSeed"])
    ph = rng.normals(6 * t.num_modes, 0.0, c["variance"])
    for dt in (1e-4, 3.7e-3, 0.9):
        ph = tr.ou_step(ph, c["variance"], dt, c["decayTime"], rng.normals(6 * t.num_modes))
        t.update_noise(dt)
        got = t.arrays()["phases"]
        tol = 1e-15 * (np.abs(ph) + c["variance"])
        assert np.all(np.abs(got - ph) <= tol), float(np.max(np.abs(got - ph) / tol))
        re, im = tr.project(ph, modes, s["solWeight"])
        gre, gim = t.compute_phases()
        for g, w in ((gre, re), (gim, im)):
            tol = 1e-15 * (np.abs(w.ravel()) + c["variance"])
            assert np.all(np.abs(g - w.ravel()) <= tol), float(np.max(np.abs(g - w.ravel()) / tol))
        # solenoidal weight 1 would make k . phases vanish; at 0.5 the projection keeps half of the compressive part
        assert np.any(re != 0) and np.any(im != 0)


def test_state_round_trip(make):
    a = make(rngSeed=99)
    a.update_noise(1e-3)
    st = a.state()
    assert list(st) == sx.TURBULENCE_ATTRIBUTES
    txt = a.rng_state()
    words = txt.split()
    # operator<< on std::mt19937: the 624 state words and the position, separated by single blanks
    assert len(words) == 625 and all(w.isdigit() for w in words) and txt == " ".join(words)
    assert all(int(w) < 2 ** 32 for w in words[:624]) and int(words[624]) <= 624
    b = make(rngSeed=1, stSpectForm=0)  # a different table and generator, replaced by the state
    b.set_state(st)
    assert b.num_modes == a.num_modes and b.rng_state() == txt
    for k, v in a.scalars().items():
        assert b.scalars()[k] == v
    for k, v in a.arrays().items():
        assert np.array_equal(b.arrays()[k], v)
    for dt in (2e-3, 5e-2):
        a.update_noise(dt)
        b.update_noise(dt)
        assert np.array_equal(a.arrays()["phases"], b.arrays()["phases"])
    assert a.rng_state() == b.rng_state() != txt
    with pytest.raises(sx.SxError):
        bad = dict(st)
        bad["rngEngineState"] = b"not a generator"
        b.set_state(bad)


def test_generator_text_matches_restatement(make):
    """a fresh mt19937(seed) in text form starts with the seed; a state restored from that text draws the restated
    generator's first normals"""
    fresh = make(stMaxModes=3)  # no lattice point fits: no modes, no draws
    assert fresh.num_modes == 0 and fresh.max_index() == 0
    txt = fresh.rng_state()
    assert txt.split()[0] == "251299"
    t = make()  # has drawn its 672 initial phases
    assert t.rng_state() != txt
    st = t.state()
    st["rngEngineState"] = txt
    st["turbulence::phases"] = np.zeros(6 * t.num_modes)
    t.set_state(st)
    c = tr.constants(tr.DEFAULTS)
    dt = 2e-3
    t.update_noise(dt)  # from zero phases: variance sqrt(1 - f^2) z
    want = tr.ou_step(np.zeros(6 * t.num_modes), c["variance"], dt, c["decayTime"],
                      tr.StdRng(251299).normals(6 * t.num_modes))
    assert np.max(tr.ulp_diff(t.arrays()["phases"], want)) <= ULP


def test_max_index_follows_the_table(make):
    """the largest lattice index is read from the mode table itself: it survives a restored state whose box length
    differs from the settings', and a table off every lattice reports -1"""
    a = make(Lbox=2.0)
    b = make()  # Lbox 1
    b.set_state(a.state())
    assert a.max_index() == b.max_index() == 3
    st = a.state()
    modes = st["turbulence::modes"].copy()
    modes[np.flatnonzero(modes)[0]] *= 1.0 + 1e-6
    st["turbulence::modes"] = modes
    b.set_state(st)
    assert b.max_index() == -1


def test_ic_turbulence():
    from sphexa_amd import ic

    f, lim, bnd, dt0 = ic.turbulence(6)
    n = 216
    assert all(len(f[k]) == n for k in sx.Sim.CONSERVED)
    assert lim == [-0.5, 0.5] * 3 and bnd == [1, 1, 1] and dt0 == 1e-4
    for k in "xyz":
        assert f[k].min() >= -0.5 and f[k].max() < 0.5
    assert np.all(f["m"] == np.float32(1.0 / n)) and np.all(f["alpha"] == np.float32(0.05))
    assert np.all(f["vx"] == 0) and np.all(f["x_m1"] == 0) and np.all(f["du_m1"] == 0)
    h = np.cbrt(3.0 / (4.0 * math.pi) * 100 * 1.0 / n) * 0.5
    assert np.all(f["h"] == np.float32(h))
    cv = np.float32(np.float64(np.float32(8.317e7) / np.float32(0.62)) / (1.001 - 1.0))
    assert np.all(f["temp"] == 1000.0 / np.float64(cv))
    p = ic.turbulence_params(sx.default_params())
    assert p.gamma == 1.001 and p.Kcour == 0.4 and abs(p.muiConst - 0.62) < 1e-7 and p.ng0 == 100 and p.ngmax == 150
