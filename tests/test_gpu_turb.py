"""Turbulence stirring on the GPU: the stirring kernel (sx_stir, exact and fast variants) against the double-precision
formula of turb_ref.py, the device noise advance inside sx_sim_step, restart, and the refusals.

Tolerance of an acceleration component (turb_ref.stir_bound), from the reference's own float accumulator and not from
what the kernels give: numModes 2^-24 S + 2^-23 |a_before|, S = solWeightNorm sum_m amplitude_m (|Re_m| + |Im_m|).  A
float-accumulated restatement of the reference loop sits near 1e-7 S, the bound is 6.7e-6 S at 112 modes, a wrong sign
or a dropped mode is about 1e-2 S.
"""
import ctypes as C

import numpy as np
import pytest

import sphexa_amd as sx
import turb_ref as tr
from sphexa_amd import ic

pytestmark = pytest.mark.gpu

N = 64 * 3 + 17
FIRST, LAST = 5, N - 3
LBOX = 1.0


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def particles(n, seed):
    """n particles in [-L/2, L/2)^3 with points exactly on -L/2, on 0 and within 1e-12 of +L/2, and O(1) float
    accelerations"""
    rng = np.random.default_rng(seed)
    p = {k: rng.uniform(-0.5 * LBOX, 0.5 * LBOX, n) for k in "xyz"}
    edge = 0.5 * LBOX - 1e-13
    p["x"][10], p["y"][11], p["z"][12] = -0.5 * LBOX, 0.0, edge
    p["x"][13], p["y"][13], p["z"][13] = edge, -0.5 * LBOX, 0.0
    p["x"][14], p["y"][14], p["z"][14] = 0.0, 0.0, 0.0
    for k in ("ax", "ay", "az"):
        p[k] = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return p


def custom_table(turb, index):
    """turb's state with the first mode moved to the lattice point (index, 0, 0)"""
    st = turb.state()
    modes = st["turbulence::modes"].copy()
    modes[0:3] = [2.0 * np.pi * index / LBOX, 0.0, 0.0]
    st["turbulence::modes"] = modes
    return st


_cache = {}


def table_case(name):
    """(Turbulence, reference acceleration of particles(N, 1), bound scale S) of a mode table, computed once"""
    if name not in _cache:
        form = {"default": 1, "form0": 0, "form2": 2, "beyond": 1}[name]
        t = sx.Turbulence(stSpectForm=form, Lbox=LBOX)
        if name == "beyond":
            t.set_state(custom_table(t, sx.lib().sx_turb_fast_limit() + 1))
        t.update_noise(1e-3)  # phases of a running sim, not the initial draw
        _cache[name] = (t,) + reference(t, particles(N, 1))
    return _cache[name]


def reference(t, p):
    ar, sc = t.arrays(), t.scalars()
    modes = ar["modes"].reshape(-1, 3)
    re, im = tr.project(ar["phases"], modes, sc["solWeight"])
    want = tr.stir(p["x"], p["y"], p["z"], modes, re, im, ar["amplitudes"], sc["solWeightNorm"])
    return want, tr.stir_scale(re, im, ar["amplitudes"], sc["solWeightNorm"])


def run_stir(ctx, p, groups_of, t, exact):
    ctx.set_exact(exact)
    ds = sx.DeviceState(ctx, p)
    try:
        g, keep = groups_of(ctx)
        sx.stir(ctx, g, ds.fields, t)
        return {k: ds.get(k) for k in ("ax", "ay", "az", "x", "y", "z")}
    finally:
        ctx.set_exact(False)
        ctx.free_all()


def check_stirred(got, p, want, scale, num_modes, active):
    before = np.stack([p[k] for k in ("ax", "ay", "az")], axis=1).astype(np.float64)
    after = np.stack([got[k] for k in ("ax", "ay", "az")], axis=1).astype(np.float64)
    bound = tr.stir_bound(num_modes, scale, before)
    err = np.abs(after - (before + want))
    print("stirring error / bound:", float(np.max(err[active] / bound[active])), "S =", scale)
    assert np.all(err[active] <= bound[active]), float(np.max(err[active] / bound[active]))
    assert np.max(np.abs(want[active])) > 1e-2 * np.max(scale)  # the sum is not lost in the bound
    for k in ("ax", "ay", "az"):  # outside the view: bit-unchanged
        assert np.array_equal(got[k][~active].view(np.uint32), p[k][~active].view(np.uint32)), k
    for k in "xyz":
        assert np.array_equal(got[k], p[k])


def range_view(ctx):
    return sx.SxGroups(firstBody=FIRST, lastBody=LAST, numGroups=(LAST - FIRST + 63) // 64), None


@pytest.mark.parametrize("table", ["default", "form0", "form2"])
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_stir_kernel_vs_formula(ctx, table, exact):
    t, want, scale = table_case(table)
    if table == "default":
        assert t.num_modes == 112
    assert 0 <= t.max_index() <= sx.lib().sx_turb_fast_limit()
    p = particles(N, 1)
    got = run_stir(ctx, p, range_view, t, exact)
    active = np.zeros(N, bool)
    active[FIRST:LAST] = True
    check_stirred(got, p, want, scale, t.num_modes, active)


@pytest.mark.parametrize("table", ["default", "form0", "form2"])
def test_fast_variant_is_the_one_that_runs(ctx, table):
    """for tables within the fast limit sx_stir does not fall back: the float lattice kernel and the reference's loop
    agree within the bound (above) but not bit for bit (the fallback test shows they are bit-equal when it declines)"""
    t = table_case(table)[0]
    p = particles(N, 1)
    fast, exact = run_stir(ctx, p, range_view, t, False), run_stir(ctx, p, range_view, t, True)
    differ = sum(int(np.count_nonzero(fast[k] != exact[k])) for k in ("ax", "ay", "az"))
    assert differ > (LAST - FIRST) // 2, differ


def test_borrowed_state_is_read_only(ctx):
    sim, f, dt0 = turb_sim(ctx, True, state=ic.turbulence(8, LBOX))
    try:
        t = sim.turbulence()
        with pytest.raises(sx.SxError):
            t.update_noise(1e-3)
        with pytest.raises(sx.SxError):
            t.set_state(t.state())
    finally:
        sim.close()


def test_turbulence_checkpoint_needs_a_stirred_sim(ctx, tmp_path):
    path = str(tmp_path / "turb.npz")
    state = ic.turbulence(8, LBOX)
    sim, f, dt0 = turb_sim(ctx, True, state=state)
    try:
        sim.step()
        sim.save_checkpoint(path)
    finally:
        sim.close()
    plain, _, _ = turb_sim(ctx, False, state=state)
    try:
        with pytest.raises(ValueError, match="not stirred"):
            plain.load_checkpoint(path)
    finally:
        plain.close()


def make_view(n, seed):
    """random-size groups (1..64 targets) tiling [0, n); every third one, in shuffled order (a ve-bdt active-rung view)"""
    rng = np.random.default_rng(seed)
    b = [0]
    while b[-1] < n:
        b.append(min(n, b[-1] + int(rng.integers(1, 65))))
    gs, ge = np.array(b[:-1], np.uint32), np.array(b[1:], np.uint32)
    sel = np.arange(gs.size)[seed % 3::3]
    rng.shuffle(sel)
    act = np.zeros(n, bool)
    for s, e in zip(gs[sel], ge[sel]):
        act[s:e] = True
    return gs[sel].copy(), ge[sel].copy(), act


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_stir_explicit_group_view(ctx, exact):
    n = 1500
    t = table_case("default")[0]
    p = particles(n, 2)
    want, scale = reference(t, p)
    gs, ge, act = make_view(n, 4)
    assert gs.size >= 8 and 0.15 * n < act.sum() < 0.6 * n

    def view(ctx):
        gsd, ged = ctx.upload(gs), ctx.upload(ge)
        return sx.SxGroups(firstBody=0, lastBody=0, numGroups=gs.size, groupStart=gsd.ptr, groupEnd=ged.ptr), None

    got = run_stir(ctx, p, view, t, exact)
    check_stirred(got, p, want, scale, t.num_modes, act)


def test_stir_fallback_beyond_the_fast_limit(ctx):
    t, want, scale = table_case("beyond")
    assert t.max_index() == sx.lib().sx_turb_fast_limit() + 1
    p = particles(N, 1)
    active = np.zeros(N, bool)
    active[FIRST:LAST] = True
    got = run_stir(ctx, p, range_view, t, False)
    check_stirred(got, p, want, scale, t.num_modes, active)
    exact = run_stir(ctx, p, range_view, t, True)
    for k in ("ax", "ay", "az"):  # the fast variant declined: the exact variant's result
        assert np.array_equal(got[k], exact[k])


# ---- in the step ---------------------------------------------------------------------------------------------------

SIDE = 16


def turb_sim(ctx, stirred, state=None, **params_kw):
    f, lim, bnd, dt0 = state if state is not None else ic.turbulence(SIDE, LBOX)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), ic.turbulence_params(sx.default_params(**params_kw)))
    sim.set_state(f, dt0, dt0)
    if stirred:
        sim.set_turbulence(Lbox=LBOX)
    return sim, f, dt0


def restated_turbulence():
    """(generator, constants, mode table, initial phases) of the default settings, restated"""
    s = dict(tr.DEFAULTS, Lbox=LBOX)
    c = tr.constants(s)
    modes, amps = tr.mode_table(s)
    rng = tr.StdRng(s["rngSeed"])
    ph = rng.normals(6 * len(amps), 0.0, c["variance"])
    return rng, s, c, modes, amps, ph


def test_step_adds_the_stirring_term(ctx):
    a, f, dt0 = turb_sim(ctx, True)
    b, _, _ = turb_sim(ctx, False)
    try:
        a.step()
        b.step()
        names = ["id", "ax", "ay", "az", "nc", "h"]
        ga, gb = a.get(names), b.get(names)
        times = a.turbulence_times()
    finally:
        a.close()
        b.close()
    oa, ob = np.argsort(ga["id"]), np.argsort(gb["id"])
    assert np.array_equal(ga["id"][oa], f["id"]) and np.array_equal(gb["id"][ob], f["id"])
    assert np.array_equal(ga["nc"][oa], gb["nc"][ob]) and np.array_equal(ga["h"][oa], gb["h"][ob])
    rng, s, c, modes, amps, ph = restated_turbulence()
    ph = tr.ou_step(ph, c["variance"], dt0, c["decayTime"], rng.normals(ph.size))  # set_state's minDt
    re, im = tr.project(ph, modes, s["solWeight"])
    want = tr.stir(f["x"], f["y"], f["z"], modes, re, im, amps, c["solWeightNorm"])  # the initial coordinates
    scale = tr.stir_scale(re, im, amps, c["solWeightNorm"])
    acc_a = np.stack([ga[k][oa] for k in ("ax", "ay", "az")], axis=1).astype(np.float64)
    acc_b = np.stack([gb[k][ob] for k in ("ax", "ay", "az")], axis=1).astype(np.float64)
    bound = tr.stir_bound(len(amps), scale, acc_b)
    err = np.abs(acc_a - acc_b - want)
    print("step stirring error / bound:", float(np.max(err / bound)), "times (ms):", times)
    assert np.all(err <= bound), float(np.max(err / bound))
    assert np.max(np.abs(want)) > 1e-2 * np.max(scale)
    assert times["noise"] > 0 and times["stirring"] > 0


def test_ou_sequence_over_steps(ctx):
    sim, f, dt0 = turb_sim(ctx, True)
    try:
        dts, ecin = [], []
        for _ in range(5):
            dts.append(sim.scalars()["minDt"])  # the minDt current when the step stirs: the previous step's
            sim.step()
            ecin.append(sim.conserved()["ecin"])
        state = sim.turbulence_state()
    finally:
        sim.close()
    assert dts[0] == dt0 and len(set(dts)) > 1
    assert ecin[0] > 0 and ecin[-1] > ecin[0]
    rng, s, c, modes, amps, ph = restated_turbulence()
    for dt in dts:
        ph = tr.ou_step(ph, c["variance"], dt, c["decayTime"], rng.normals(ph.size))
    got = state["turbulence::phases"]
    tol = 1e-13 * (np.abs(ph) + c["variance"])
    print("OU phases after 5 steps, error / tolerance:", float(np.max(np.abs(got - ph) / tol)))
    assert np.all(np.abs(got - ph) <= tol), float(np.max(np.abs(got - ph) / tol))
    assert int(state["turbulence::numModes"]) == len(amps)
    assert np.max(tr.ulp_diff(state["turbulence::amplitudes"], amps)) <= 4


FIELDS = ["x", "y", "z", "h", "temp", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "du_m1", "alpha", "ax", "ay", "az", "du"]


def snapshot(sim):
    g = sim.get(["id"] + FIELDS)
    o = np.argsort(g["id"])
    st = sim.turbulence_state()
    return {k: g[k][o] for k in g}, sim.scalars(), st


def test_restart_takes_the_same_steps(ctx, tmp_path):
    paths = [str(tmp_path / "turb.npz"), str(tmp_path / "turb.h5")]
    sim, f, dt0 = turb_sim(ctx, True)
    try:
        for _ in range(3):
            sim.step()
        for p in paths:
            sim.save_checkpoint(p)
        for _ in range(2):
            sim.step()
        want = snapshot(sim)
    finally:
        sim.close()
    with np.load(paths[0]) as d:
        assert [k for k in sx.TURBULENCE_ATTRIBUTES if k in d.files] == sx.TURBULENCE_ATTRIBUTES
        assert bytes(d["rngEngineState"]).decode().count(" ") == 624
    for p in paths:
        new = sx.Sim(ctx, len(f["x"]), sx.make_box([-0.5 * LBOX, 0.5 * LBOX] * 3, [1, 1, 1]),
                     ic.turbulence_params(sx.default_params()))
        try:
            new.set_turbulence(Lbox=LBOX, rngSeed=1)  # another seed: the state must come from the file
            new.load_checkpoint(p)
            assert new.iteration == 3
            for _ in range(2):
                new.step()
            got = snapshot(new)
        finally:
            new.close()
        for k in want[0]:
            assert np.array_equal(got[0][k], want[0][k]), (p, k)
        assert got[1] == want[1], (p, got[1], want[1])
        for k in sx.TURBULENCE_ATTRIBUTES:
            assert np.array_equal(got[2][k], want[2][k]), (p, k)


def test_unstirred_checkpoint_is_unchanged(ctx, tmp_path):
    sim, f, dt0 = turb_sim(ctx, False)
    try:
        sim.step()
        sim.save_checkpoint(str(tmp_path / "plain.npz"))
        with pytest.raises(sx.SxError):
            sim.turbulence_state()
    finally:
        sim.close()
    with np.load(str(tmp_path / "plain.npz")) as d:
        assert sorted(d.files) == sorted(sx.Sim.CONSERVED + sx.ATTRIBUTE_NAMES)


@pytest.mark.parametrize("kind", ["std", "bdt"])
def test_refused_propagators(ctx, kind):
    f, lim, bnd, dt0 = ic.turbulence(8, LBOX)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), ic.turbulence_params(sx.default_params(**{kind: True})))
    try:
        with pytest.raises(sx.SxError) as e:
            sim.set_turbulence(Lbox=LBOX)
        assert "sx_sim_set_turbulence" in str(e.value) and ("std" in str(e.value) or "ve-bdt" in str(e.value))
    finally:
        sim.close()


def test_refused_communicator(ctx):
    sim, f, dt0 = turb_sim(ctx, True, state=ic.turbulence(8, LBOX))
    try:
        rc = sim.L.sx_sim_set_comm(sim.h, None)
        assert rc == sx.SX_ERR_ARG
        assert b"one rank" in sim.L.sx_last_error(ctx.h)
    finally:
        sim.close()
