"""The fused observables pass on the GPU (sx_observables, sx_sim_observe) against the numpy restatement tests/obs_ref.py
and, for the gravitational waves, against the reference's own numbers (tests/golden/gravwaves_ref.npz).

Tolerance of every float64 sum: 1e-12 * sum|term| (the bound test_gpu_observables.py uses for the conserved sums).  The
terms are the restatement's bit for bit up to the last bits of exp/sin/cos, only the summation order differs, and a
fixed tree over n <= 2e6 terms errs by a few 1e-16 sum|term|.  A sum that cancels is judged on sum|term|, never on its
own value.  The wind bubble's count is exact.

The fixed grid of the pass is 1024 workgroups of 512-particle chunks: BIG gives every workgroup three or four chunks
and a ragged last one.
"""
import ctypes as C
import io
import os

import numpy as np
import pytest

import gpu_util as gutil
import obs_ref
import pyoracle as po
import sphexa_amd as sx
from sphexa_amd import ic

pytestmark = pytest.mark.gpu

KINDS = obs_ref.KINDS
RHO_BUBBLE, TEMP_WIND = 1.5625, 1.1  # thresholds 0.64 rhoBubble ~ 1.0 and 0.9 tempWind ~ 0.99, inside the inputs' range
SMALL, BIG = 2053, 2_000_003
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gravwaves_ref.npz")
REL = 1e-12


def random_fields(n, seed):
    """x, y (z) in [0, 1), v, a ~ N(0, 1), c, kx, xm, m (temp) in [0.5, 1.5]; no particle within a relative 1e-5 of
    either wind-bubble threshold"""
    rng = np.random.default_rng(seed)
    f = {k: rng.uniform(0.0, 1.0, n) for k in "xyz"}
    for k in ("vx", "vy", "vz", "ax", "ay", "az"):
        f[k] = rng.normal(0.0, 1.0, n).astype(np.float32)
    for k in ("c", "kx", "xm", "m"):
        f[k] = rng.uniform(0.5, 1.5, n).astype(np.float32)
    f["temp"] = rng.uniform(0.5, 1.5, n)
    f["nc"] = rng.integers(50, 150, n).astype(np.uint32)
    near = np.abs(obs_ref.wind_rho(f).astype(np.float64) / (0.64 * RHO_BUBBLE) - 1.0) < 2e-5
    f["m"][near] *= np.float32(1.001)
    near = np.abs(f["temp"] / (0.9 * TEMP_WIND) - 1.0) < 2e-5
    f["temp"][near] *= 1.001
    return f


def assert_clear_of_thresholds(f, s):
    rho = obs_ref.wind_rho({k: f[k][s] for k in ("kx", "xm", "m")}).astype(np.float64)
    assert np.all(np.abs(rho / (0.64 * RHO_BUBBLE) - 1.0) > 1e-5)
    assert np.all(np.abs(f["temp"][s] / (0.9 * TEMP_WIND) - 1.0) > 1e-5)


class Device:
    """the fields of a host dict on the device, as an SxFields holding just those"""

    def __init__(self, ctx, host):
        self.ctx, self.host = ctx, host
        self.arrays = {k: ctx.upload(np.ascontiguousarray(v, dtype=sx.DTYPES[k])) for k, v in host.items()}
        self.fields = sx.SxFields()
        self.fields.n = len(next(iter(host.values())))
        for k, d in self.arrays.items():
            setattr(self.fields, k, d.ptr)

    def without(self, *names):
        f = sx.SxFields()
        C.memmove(C.byref(f), C.byref(self.fields), C.sizeof(f))
        for k in names:
            setattr(f, k, None)
        return f

    def free(self):
        for d in self.arrays.values():
            self.ctx.free(d)


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    d = Device(ctx, random_fields(SMALL, 1))
    yield d
    d.free()


@pytest.fixture(scope="module")
def big(ctx):
    d = Device(ctx, random_fields(BIG, 2))
    yield d
    d.free()


BOX = sx.make_box([0.0, 1.0, 0.0, 1.0, 0.0, 1.0], [1, 1, 1])


def settings():
    return sx.SxObsSettings(rhoBubble=RHO_BUBBLE, tempWind=TEMP_WIND)


def observe(ctx, dev, kind, first, last, fields=None):
    return ctx.observables(fields if fields is not None else dev.fields, kind, first, last, box=BOX,
                           settings=settings())


def check_sums(got, host, kind, first, last, conserved=True):
    want, mag = obs_ref.sums(kind, host, first=first, last=last, ybox=1.0, rho_bubble=RHO_BUBBLE,
                             temp_wind=TEMP_WIND, conserved=conserved)
    assert list(got) == obs_ref.CONSERVED + obs_ref.EXTRA[kind]
    worst = 0.0
    for name in want:
        err = abs(got[name] - want[name])
        if name in ("totalNeighbors", "survivors"):
            assert got[name] == want[name], (kind, name, got[name], want[name])
            continue
        worst = max(worst, err / mag[name] if mag[name] else (0.0 if err == 0 else np.inf))
        assert err <= REL * mag[name], (kind, name, first, last, got[name], want[name], err / max(mag[name], 1e-300))
    print(f"{kind} [{first}, {last}): worst error / sum|term| = {worst:.3g}")
    return want


@pytest.mark.parametrize("kind", KINDS)
def test_small_shapes(ctx, small, kind):
    """one chunk and less: empty, one particle, around the wave and the block width; then a shifted range"""
    for n in (1, 63, 64, 65, 255, 256, 257):
        check_sums(observe(ctx, small, kind, 0, n), small.host, kind, 0, n)
    got = observe(ctx, small, kind, 5, 5)  # n = 0
    assert all(v == 0.0 for v in got.values()), got
    check_sums(observe(ctx, small, kind, 5, SMALL - 3), small.host, kind, 5, SMALL - 3)


@pytest.mark.parametrize("kind", KINDS)
def test_every_workgroup_several_chunks(ctx, big, kind):
    check_sums(observe(ctx, big, kind, 0, BIG), big.host, kind, 0, BIG)


@pytest.mark.parametrize("kind", KINDS)
def test_conserved_sums_equal_the_conserved_kernel(ctx, small, big, kind):
    for dev, first, last in ((small, 5, SMALL - 3), (big, 17, BIG - 5)):
        got = observe(ctx, dev, kind, first, last)
        out = (C.c_double * 9)()
        ctx.check(ctx.L.sx_conserved_quantities(ctx.h, C.byref(dev.fields), first, last, 10.0, 5.0 / 3.0, out), "cq")
        _, mag = obs_ref.sums("time_energy", dev.host, first=first, last=last)
        for k, name in enumerate(obs_ref.CONSERVED):
            if name == "totalNeighbors":
                assert got[name] == out[k] == float(np.sum(dev.host["nc"][first:last].astype(np.int64)))
            else:
                assert abs(got[name] - out[k]) <= REL * mag[name], (kind, name, got[name], out[k])


def test_wind_bubble_count_is_exact(ctx, small, big):
    for dev, first, last in ((small, 5, SMALL - 3), (big, 0, BIG)):
        s = slice(first, last)
        assert_clear_of_thresholds(dev.host, s)
        rho = obs_ref.wind_rho({k: dev.host[k][s] for k in ("kx", "xm", "m")}).astype(np.float64)
        dense, cold = rho >= 0.64 * RHO_BUBBLE, dev.host["temp"][s] <= 0.9 * TEMP_WIND
        for a in (dense, ~dense, cold, ~cold, dense & cold, dense & ~cold, ~dense & cold):
            assert a.any()  # each side of both conditions holds particles
        got = observe(ctx, dev, "wind_bubble", first, last)
        assert got["survivors"] == float(np.count_nonzero(dense & cold))
        frac = sx.obs_finalize("wind_bubble", got, last - first, sx.SxObsSettings(particleMass=0.5, initialMass=4.0))
        assert frac == [np.count_nonzero(dense & cold) * 0.5 / 4.0]


def test_grav_waves_against_the_reference(ctx):
    """the reference's own sums and polarisations of the committed 2053 particles"""
    with np.load(GOLDEN) as d:
        g = {k: d[k] for k in d.files}
    host = {k: g[k] for k in ("x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az", "m")}
    host["temp"] = np.ones(len(host["x"]))
    dev = Device(ctx, host)
    try:
        first, last, theta, phi = int(g["first"]), int(g["last"]), float(g["theta"]), float(g["phi"])
        got = observe(ctx, dev, "grav_waves", first, last)
        _, mag = obs_ref.sums("grav_waves", host, first=first, last=last)
        names = obs_ref.EXTRA["grav_waves"]
        for k, name in enumerate(names):
            err = abs(got[name] - g["d2q"][k])
            print(name, "error / sum|term| =", err / mag[name])
            assert err <= REL * mag[name], (name, got[name], g["d2q"][k])
        h = sx.obs_finalize("grav_waves", got, last - first, sx.SxObsSettings(gravWaveTheta=theta, gravWavePhi=phi))
        bound = obs_ref.htt_bound([REL * mag[name] for name in names], theta, phi)
        for k in range(2):
            assert abs(h[k] - g["htt"][k]) <= bound[k], (k, h[k], g["htt"][k], bound[k])
            assert abs(g["htt"][k]) > 1e3 * bound[k]  # the signal is not lost in the bound
    finally:
        dev.free()


@pytest.mark.parametrize("kind", KINDS)
def test_deterministic(ctx, big, kind):
    a = observe(ctx, big, kind, 3, BIG - 1)
    b = observe(ctx, big, kind, 3, BIG - 1)
    assert np.array_equal(np.array(list(a.values())).view(np.uint64), np.array(list(b.values())).view(np.uint64))


@pytest.mark.parametrize("kind,missing,words", [
    ("mach_rms", "c", "Mach RMS needs c"),
    ("kh_growth", "kx", "kx or xm is missing"),
    ("kh_growth", "xm", "kx or xm is missing"),
    ("wind_bubble", "kx", "kx or xm is missing"),
    ("wind_bubble", "xm", "kx or xm is missing"),
    ("grav_waves", "ax", "need ax, ay, az"),
    ("grav_waves", "ay", "need ax, ay, az"),
    ("grav_waves", "az", "need ax, ay, az"),
    ("time_energy", "m", "null field of the conserved sums"),
])
def test_missing_field_is_refused(ctx, small, kind, missing, words):
    with pytest.raises(sx.SxError) as e:
        observe(ctx, small, kind, 0, SMALL, fields=small.without(missing))
    assert f"code {sx.SX_ERR_ARG}" in str(e.value) and words in str(e.value)


@pytest.mark.parametrize("kind", KINDS)
def test_short_output_is_refused(ctx, small, kind):
    with pytest.raises(sx.SxError) as e:
        ctx.observables(small.fields, kind, 0, SMALL, box=BOX, settings=settings(),
                        cap=8 + len(obs_ref.EXTRA[kind]))
    assert f"code {sx.SX_ERR_ARG}" in str(e.value) and "sums" in str(e.value)


def test_kind_fields_alone(ctx, small):
    """the signatures of the reference's gpu_reductions.h hold only the kind's fields: the conserved sums read as zero"""
    first, last = 5, SMALL - 3
    for kind, keep in (("mach_rms", ("vx", "vy", "vz", "c")), ("kh_growth", ("x", "y", "vy", "xm", "kx")),
                       ("wind_bubble", ("temp", "kx", "xm", "m"))):
        f = small.without(*[k for k in small.host if k not in keep])
        got = observe(ctx, small, kind, first, last, fields=f)
        assert all(got[k] == 0.0 for k in obs_ref.CONSERVED)
        full = observe(ctx, small, kind, first, last)
        for name in obs_ref.EXTRA[kind]:
            assert got[name] == full[name]  # the same terms in the same order


# ---- in the step driver ------------------------------------------------------------------------------------------

HEAD = ["iteration", "ttot", "minDt", "etot", "ecin", "eint", "egrav"]


def check_row_head(sim, row, steps, momenta=True):
    sc, cq = sim.scalars(), sim.conserved()
    assert row["iteration"] == steps and isinstance(row["iteration"], int)
    assert row["ttot"] == sc["ttot"] and row["minDt"] == sc["minDt"] and row["egrav"] == cq["egrav"]
    for k in ("etot", "ecin", "eint") + (("linmom", "angmom") if momenta else ()):
        assert row[k] == pytest.approx(cq[k], rel=1e-12, abs=1e-12 * abs(cq["ecin"])), k


def test_sim_mach_rms(ctx):
    st, obox = po.sedov_state(20)
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        sim.set_observable("mach_rms")
        for _ in range(3):
            sim.step()
        row = sim.observe()
        assert list(row) == sx.OBS_COLUMNS["mach_rms"]
        check_row_head(sim, row, 3)
        got = sim.get(["vx", "vy", "vz", "c"])
        t = obs_ref.mach_terms(got)["machSquareSum"]
        want = np.sqrt(np.sum(t) / st.n)
        assert want > 0 and abs(row["machRms"] ** 2 * st.n - np.sum(t)) <= REL * np.sum(np.abs(t))
        assert row["machRms"] == pytest.approx(want, rel=1e-12)
        line = sx.format_constants_row(row, "mach_rms")
        assert line.startswith(" 3 ") and len(line.split()) == 10
        out = io.StringIO()
        assert sim.write_constants(out) == row and sim.write_constants(out) == row  # nothing moved in between
        assert out.getvalue() == 2 * line
    finally:
        sim.close()


def test_sim_grav_waves(ctx):
    st, obox = po.evrard_state(14)
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox), params=sx.default_params(g=1.0, theta=0.5))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        sim.set_observable("grav_waves", gravWaveTheta=0.3, gravWavePhi=0.4)
        for _ in range(3):
            sim.step()
        row = sim.observe()
        assert list(row) == sx.OBS_COLUMNS["grav_waves"]
        check_row_head(sim, row, 3, momenta=False)
        assert row["egrav"] < 0
        got = sim.get(["x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az", "m"])
        want, mag = obs_ref.sums("grav_waves", got, conserved=False)
        names = obs_ref.EXTRA["grav_waves"]
        for name in names:
            assert abs(row[name] - want[name]) <= REL * mag[name], (name, row[name], want[name])
        h = obs_ref.htt([want[k] for k in names], 0.3, 0.4)
        bound = obs_ref.htt_bound([2 * REL * mag[k] for k in names], 0.3, 0.4)
        assert abs(row["httplus"] - h[0]) <= bound[0] and abs(row["httcross"] - h[1]) <= bound[1]
    finally:
        sim.close()


def test_sim_refuses_kh_growth_on_std(ctx):
    st, obox = po.sedov_state(12)
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox), params=sx.default_params(std=True))
    try:
        for kind in ("kh_growth", "wind_bubble"):
            with pytest.raises(sx.SxError) as e:
                sim.set_observable(kind, **(dict(rhoInt=1.0, uExt=1.0, rSphere=1.0) if kind == "wind_bubble" else {}))
            assert "kx was empty" in str(e.value) and "--prop ve" in str(e.value)
        sim.set_observable("mach_rms")  # everything else is accepted
        sim.set_observable("grav_waves", gravWaveTheta=0.1, gravWavePhi=0.2)
    finally:
        sim.close()


def mid_gap(values):
    """a threshold inside the widest relative gap between the distinct values of the middle half: particles on both
    sides, none near it"""
    u = np.unique(np.asarray(values, dtype=np.float64))
    if u.size < 2:
        return 0.5 * float(u[0])
    lo, hi = u.size // 4, max(u.size // 4 + 1, 3 * u.size // 4)
    k = lo + int(np.argmax(np.diff(u)[lo:hi] / np.abs(u[lo:hi])))
    return 0.5 * float(u[k] + u[k + 1])


def test_sim_wind_bubble_and_kh_rows(ctx):
    """the driver's derived wind-bubble settings and both VE-only rows after a Sedov step, against the restatement"""
    st, obox = po.sedov_state(16)
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        sim.step()
        got = sim.get(["x", "y", "vy", "xm", "kx", "m", "temp"])
        rho = obs_ref.wind_rho(got).astype(np.float64)
        rho_int, temp_cut = mid_gap(rho) / 0.64, mid_gap(got["temp"])
        cv = float(obs_ref.ideal_gas_cv())
        u_ext = temp_cut / 0.9 / cv
        sim.set_observable("wind_bubble", rhoInt=rho_int, uExt=u_ext, rSphere=0.25)
        row = sim.observe()
        assert list(row) == sx.OBS_COLUMNS["wind_bubble"]
        check_row_head(sim, row, 1)
        count = np.count_nonzero((rho >= 0.64 * rho_int) & (got["temp"] <= 0.9 * (u_ext * np.float32(cv))))
        mass0 = 0.25 ** 3 * 4.0 / 3.0 * np.pi * rho_int
        assert row["bubbleFraction"] == pytest.approx(count * float(got["m"][0]) / mass0, rel=1e-14)
        assert row["normalizedTime"] == row["ttot"] / 0.0937
        sim.set_observable("kh_growth")
        row = sim.observe()
        t = obs_ref.kh_terms(got, obox.lim[3] - obox.lim[2])
        s = {k: np.sum(v) for k, v in t.items()}
        want = 2.0 * np.sqrt(s["sumsi"] ** 2 + s["sumci"] ** 2) / s["sumdi"]
        # errors e_s, e_c, e_d of the three sums move 2 sqrt(s^2 + c^2) / d by at most 2 (e_s + e_c) / d + value e_d / d,
        # and value e_d / d <= REL value <= REL scale (the di are positive): 2 REL scale, doubled for numpy's own sums
        scale = 2.0 * (np.sum(np.abs(t["sumsi"])) + np.sum(np.abs(t["sumci"]))) / s["sumdi"]
        assert abs(row["khgr"] - want) <= 4 * REL * scale
    finally:
        sim.close()


def test_stirred_sim_reports_its_mach_number(ctx):
    f, lim, bnd, dt0 = ic.turbulence(16, 1.0)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), ic.turbulence_params(sx.default_params()))
    try:
        sim.set_state(f, dt0, dt0)
        sim.set_turbulence(Lbox=1.0)
        sim.set_observable("mach_rms")
        assert sim.observe()["machRms"] == 0.0  # at rest before the first step
        sim.step()
        row = sim.observe()
        got = sim.get(["vx", "vy", "vz", "c"])
        t = obs_ref.mach_terms(got)["machSquareSum"]
        assert row["machRms"] > 0 and row["machRms"] == pytest.approx(np.sqrt(np.sum(t) / len(f["x"])), rel=1e-12)
        assert abs(row["machRms"] ** 2 * len(f["x"]) - np.sum(t)) <= REL * np.sum(t)
    finally:
        sim.close()
