"""Sim.profile (sx_sim_profile) on one rank: under every propagator it is Context.profile of the sim's own fields and
the oracle (tests/profile_ref.py) on the copied columns, bit for bit; quantities a layout does not keep are refused with
a reason; it changes no state; and whole runs are judged by it the way tests/test_gpu_trajectory.py judges them from
host copies: Sedov -n 50 -s 200 against the reference's analytic table, the Noh lattice -n 30 -s 100 against the closed
form.

Bounds of the whole-run cases.  The device's l1 is the exact sum of the N deviations rounded once, divided by N;
trajectory.analytic_l1 sums the same deviations with np.sum: N 2^-52 sum |q - s| / N, plus 4 ulp of the larger of |s|
and |q| per term for np.interp's (and noh_rho's) own rounding of s.  The bands against the reference's runs are those of
tests/test_gpu_trajectory.py: 0.01 on the Sedov L1, 1 % on the binned means, 2 % on the Noh L1.
"""
import numpy as np
import pytest

import golden_util as gu
import gpu_util as gutil
import nbody_ref as nr
import profile_ref as pr
import pyoracle as po
import sphexa_amd as sx
import trajectory as tj

pytestmark = pytest.mark.gpu
U = 2.0 ** -52
COLUMNS = ["x", "y", "z", "vx", "vy", "vz", "h", "m", "temp", "kx", "xm", "rho", "c", "divv", "curlv", "alpha"]
EDGES = np.linspace(0.0, 0.6, 13)


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def same(a, b):
    assert np.array_equal(a["count"], b["count"]) and a["nonfinite"][0] == b["nonfinite"][0]
    for k in ("W", "S1", "S2", "D"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    for k in ("min", "max"):
        assert np.array_equal(a[k], b[k]), k


def three_ways(ctx, sim, std, quantities, **kw):
    """Sim.profile, Context.profile on Sim.fields() and the oracle on Sim.get(): the same bits"""
    out = sim.profile(EDGES, quantities, **kw)
    spec = sim.profile_spec(EDGES, quantities, **kw)
    f, _ = sim.fields()
    seam = ctx.profile(f, sim.box, spec, params=sim.params, std=std)
    same(out["raw"], seam)
    assert sim.profile_stats() == ctx.profile_stats() and sim.profile_stats()["particles"] == sim.size()
    cols = sim.get([k for k in COLUMNS if k in sim.allocated_fields()])
    kw = dict(kw)
    kw.setdefault("center", [0.5 * (sim.box.lim[2 * k] + sim.box.lim[2 * k + 1]) for k in range(3)])
    ref = pr.profile(cols, list(sim.box.lim), list(sim.box.bnd), EDGES, quantities, std=std,
                     mui=sim.params.muiConst, gamma=sim.params.gamma, **kw)
    same(out["raw"], ref)
    nb = len(EDGES) - 1
    assert np.array_equal(out["count"], ref["count"][:nb])
    assert out["under"] == ref["count"][nb] and out["over"] == ref["count"][nb + 1]
    for k, name in enumerate(quantities):
        assert np.array_equal(out["sum"][name], ref["S1"][k][:nb])
        filled = ref["count"][:nb] > 0
        assert np.array_equal(out["mean"][name][filled], ref["S1"][k][:nb][filled] / ref["W"][:nb][filled])
    return out


def table():
    r = np.linspace(0.0, 0.9, 30)
    return ("table", r, 1.0 + 3.0 * np.exp(-((r - 0.2) / 0.05) ** 2))


@pytest.mark.parametrize("std", [False, True], ids=["ve", "std"])
def test_hydro_propagators(ctx, std):
    st, obox = po.sedov_state(12)
    sim = sx.Sim(ctx, st.n + 64, gutil.box_to_sx(obox), params=sx.default_params(std=std))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        for _ in range(3):
            sim.step()
        out = three_ways(ctx, sim, std, ("rho", "p", "vel", "u"), solutions={"rho": table()})
        assert out["l1"]["rho"] > 0 and out["nonfinite"] == 0 and abs(out["mean"]["rho"][5] - 1.0) < 0.2
        kept = [k for k in ("c", "divv", "curlv", "alpha") if k in sim.allocated_fields()]
        three_ways(ctx, sim, std, tuple(["vrad"] + kept[:3]), weight="mass", center=(0.4, -0.45, 0.1))
        three_ways(ctx, sim, std, tuple(["temp", "h"] + kept[3:]), coord="rho")
        for name in ("c", "divv", "curlv", "alpha"):
            if name not in kept:
                with pytest.raises(sx.SxError, match=f"{name} is not kept by this layout"):
                    sim.profile(EDGES, ("vel", name))
        with pytest.raises(sx.SxError, match="strictly ascending"):
            sim.profile([0.0, 0.2, 0.1], ("vel",))
    finally:
        sim.close()


def test_ve_bdt_between_substeps(ctx):
    st, obox = po.sedov_state(12)
    sim = sx.Sim(ctx, st.n + 64, gutil.box_to_sx(obox), params=sx.default_params(bdt=True))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt)
        for _ in range(3):
            sim.step()
            three_ways(ctx, sim, False, ("rho", "p", "vel", "u"), solutions={"rho": table()})
    finally:
        sim.close()


def test_gravity_only_propagator(ctx):
    st, obox = po.evrard_state(10)
    arr = {k: st.arrays[k].copy() for k in nr.FIELDS}
    sim = sx.Sim(ctx, len(arr["x"]), gutil.box_to_sx(obox), params=sx.default_params(g=1.0), propagator=3)
    try:
        sim.set_state(arr, st.minDt, st.minDt)
        sim.step()
        three_ways(ctx, sim, False, ("vel", "vrad", "h"), weight="mass")
        three_ways(ctx, sim, False, ("vrad",), coord="z")
        for name in ("p", "rho", "u", "temp", "c", "divv", "curlv", "alpha"):
            with pytest.raises(sx.SxError, match=f"{name} .*the gravity-only propagator keeps vel, vrad and h only"):
                sim.profile(EDGES, ("vel", name))
        with pytest.raises(sx.SxError, match="the gravity-only propagator keeps vel, vrad and h only"):
            sim.profile(EDGES, ("vel",), coord="rho")
    finally:
        sim.close()


def run_steps(ctx, profile_after):
    st, obox = po.sedov_state(12)
    sim = sx.Sim(ctx, st.n + 64, gutil.box_to_sx(obox))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        sim.step()
        sim.step()
        if profile_after:
            names = sim.allocated_fields()
            before, mem0 = sim.get(names), sim.memory()
            sim.profile(EDGES, solutions={"rho": table()})
            mem1 = sim.memory()
            after = sim.get(names)
            assert all(before[k].tobytes() == after[k].tobytes() for k in names)
            assert mem1["device"] > mem0["device"] and mem1["pinned"] > mem0["pinned"]  # the prof.* buffers, counted
            sim.profile(EDGES, solutions={"rho": table()})
            assert sim.memory() == mem1
        sim.step()
        return sim.get(["id", "x", "y", "z", "vx", "vy", "vz", "temp", "h"]), sim.scalars()
    finally:
        sim.close()


def test_a_profile_changes_no_state(ctx):
    """every field is the same before and after the call, and the next step is the one of a run that never asked"""
    asked, sc_a = run_steps(ctx, True)
    never, sc_n = run_steps(ctx, False)
    assert sc_a == sc_n
    for k in asked:
        assert asked[k].tobytes() == never[k].tobytes(), k


def whole_run(case):
    fname, init, side, steps, prof_steps, rmax, nbins = tj.CASES[case]
    fx = gu.load(fname)
    st, obox = getattr(po, init + "_state")(side)
    ctx = sx.Context(0)
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        for _ in range(steps):
            sim.step()
        yield fx, sim, rmax, nbins
    finally:
        sim.close()
        ctx.close()


def test_sedov_n50_200_steps_judged_on_the_device():
    for fx, sim, rmax, nbins in whole_run("sedov"):
        sol = fx["sol"]
        out = sim.profile(np.linspace(0.0, rmax, nbins + 1), ("rho", "p", "vel", "u"),
                          solutions={"rho": ("table", sol[:, 0], sol[:, 1])})
        final = sim.get(tj.FIELDS)
        rho, _ = tj.eos_rho_p(final)
        r = tj.radii(final)
        host = tj.analytic_l1(r, rho.astype(np.float64), sol[:, 0], sol[:, 1])
        s = np.interp(r, sol[:, 0], sol[:, 1])
        bound = U * np.sum(np.abs(s - rho)) + 4 * U * np.sum(np.maximum(np.abs(s), rho)) / rho.size
        ref = float(fx["ref_l1_density_subsampled"][0])
        print(f"Sedov -n 50 -s 200 density L1: device {out['l1']['rho']:.6f}, host {host:.6f} (bound {bound:.2e}), "
              f"reference {ref:.4f}")
        assert out["nonfinite"] == 0 and out["under"] == 0
        assert abs(out["l1"]["rho"] - host) <= bound, (out["l1"]["rho"], host, bound)
        assert abs(out["l1"]["rho"] - ref) <= 0.01, (out["l1"]["rho"], ref)
        for k in ("rho", "p", "vel", "u"):
            mean = np.where(out["count"] > 0, out["mean"][k], 0.0)  # an empty shell: 0, as trajectory.profiles has it
            d = tj.profile_l1(mean, fx[f"s200_{k}"], fx["s200_count"])
            print(f"  25-bin means of {k} at step 200 vs the reference run: {d:.2e}")
            assert d <= 0.01, (k, d)


def test_noh_n30_100_steps_judged_on_the_device():
    for fx, sim, rmax, nbins in whole_run("noh"):
        t = sim.scalars()["ttot"]
        final = sim.get(tj.FIELDS)
        rho, _ = tj.eos_rho_p(final)
        for key, rho0 in (("ref_l1_noh_density_attr", tj.NOH_RHO0_ATTR), ("ref_l1_noh_density_ic", tj.NOH_RHO0_IC)):
            out = sim.profile(np.linspace(0.0, rmax, nbins + 1), ("rho",), solutions={"rho": ("noh", dict(time=t, rho0=rho0))})
            host, ref = tj.noh_l1(final, t, rho0), float(fx[key][0])
            s = tj.noh_rho(tj.radii(final), t, rho0=rho0)
            bound = U * np.sum(np.abs(s - rho)) + 4 * U * np.sum(np.maximum(np.abs(s), rho)) / rho.size
            print(f"Noh -n 30 -s 100 density L1 (rho0 = {rho0:.4g}): device {out['l1']['rho']:.6f}, host {host:.6f} "
                  f"(bound {bound:.2e}), reference {ref:.4f}")
            assert abs(out["l1"]["rho"] - host) <= bound, (out["l1"]["rho"], host, bound)
            assert abs(out["l1"]["rho"] / ref - 1) <= 0.02, (key, out["l1"]["rho"], ref)
