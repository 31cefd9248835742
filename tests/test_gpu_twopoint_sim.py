"""Sim.twopoint (sx_sim_twopoint) on one rank: Sim.twopoint = Context.twopoint on Sim.fields() = the oracle
(tests/twopoint_ref.py) on the columns Sim.get copies, bit for bit, under the VE, std and gravity-only propagators after
five steps; the call changes no state; the lattice coordination numbers on the Sedov lattice at step 0 (a device result
against arithmetic); xi of uniform random points inside its Poisson band.

The refusal of a communicator with more than one rank is not tested here: one process holds one rank, so it would take
worker processes for a message (as for Sim.fof)."""
import numpy as np
import pytest

import gpu_util as gutil
import pyoracle as po
import sphexa_amd as sx
import twopoint_ref as tr
from sphexa_amd import ic

pytestmark = pytest.mark.gpu

SEDOV_BOX = ([-0.5, 0.5] * 3, [1, 1, 1])
COLUMNS = ["x", "y", "z", "m", "vx", "vy", "vz", "id"]


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def three_ways(ctx, sim, edges, **kw):
    """Sim.twopoint, Context.twopoint on Sim.fields() and the oracle on Sim.get(): the same bits"""
    out = sim.twopoint(edges, **kw)
    spec = sim.twopoint_spec(edges, **kw)
    f, idp = sim.fields()
    n = sim.size()
    seam = ctx.twopoint(f, sim.box, spec, id=sx.DeviceArray(ctx, idp, n, np.uint64), first=0, last=n)
    cols = sim.get(COLUMNS)
    ref = tr.twopoint(cols, list(sim.box.lim), list(sim.box.bnd), edges, series=spec.series, stride=spec.stride,
                      phase=spec.phase, ids=cols["id"])
    tr.assert_same(out, ref, spec.series)
    tr.assert_same(seam, ref, spec.series)
    assert sim.twopoint_stats() == ctx.twopoint_stats() and sim.twopoint_stats()["pairs_binned"] == ref["pairs"]
    filled = ref["count"] > 0
    if spec.series & tr.FLAGS["U2"]:
        assert np.array_equal(out["s2"][filled], ref["U2"][filled] / ref["count"][filled])
        assert np.all(np.isnan(out["s2"][~filled]))
    return out, ref


@pytest.mark.parametrize("std", [False, True], ids=["ve", "std"])
def test_sedov_after_five_steps(ctx, std):
    st, obox = po.sedov_state(16)
    sim = sx.Sim(ctx, st.n + 64, gutil.box_to_sx(obox), params=sx.default_params(std=std))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        for _ in range(5):
            sim.step()
        edges = np.linspace(0.0, 2.2 / 16, 12)
        out, ref = three_ways(ctx, sim, edges, mass=True)
        assert 5e4 < ref["pairs"] < 2e5 and out["nonfinite"] == 0 and out["targets"] == st.n
        assert out["pairs_expected"] == st.n * (st.n - 1) // 2 and out["xi"].shape == (11,)
        assert np.any(out["U1"] != 0), "the blast moves"
        three_ways(ctx, sim, edges, series=("count",), stride=4, phase=3)
        three_ways(ctx, sim, edges, series=("U1", "A3"), stride=2, phase=0)
        with pytest.raises(sx.SxError, match="exceeds a third of the periodic x extent"):
            sim.twopoint([0.0, 0.4])
        with pytest.raises(sx.SxError, match="phase 2 is not below stride 2"):
            sim.twopoint(edges, stride=2, phase=2)
    finally:
        sim.close()


def test_gravity_only_plummer_after_five_steps(ctx):
    f, lim, bnd, dt0 = ic.plummer(4000)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), sx.default_params(g=1.0, theta=0.5, nbody=True))
    try:
        sim.set_state(f, dt0, dt0)
        for _ in range(5):
            sim.step()
        edges = np.geomspace(0.02, 0.3, 10)
        out, ref = three_ways(ctx, sim, edges, mass=True)
        assert 2e4 < ref["pairs"] < 2e5 and out["xi"] is None, "xi needs a box periodic on all axes"
        # equal masses 1/n: WW is count / n^2, exactly (a power of two is not needed: the sum is of equal terms)
        m = np.float64(np.float32(1.0 / 4000))
        assert np.allclose(out["ww"], ref["count"] * (m * m), rtol=1e-15)
        three_ways(ctx, sim, edges, stride=8, phase=5)
    finally:
        sim.close()


def run_steps(ctx, ask):
    st, obox = po.sedov_state(12)
    sim = sx.Sim(ctx, st.n + 64, gutil.box_to_sx(obox))
    try:
        sim.set_state(st.arrays, st.minDt, st.minDt_m1)
        sim.step()
        sim.step()
        if ask:
            names = sim.allocated_fields()
            before, mem0, sc0 = sim.get(names), sim.memory(), sim.scalars()
            out = sim.twopoint(np.linspace(0.0, 0.2, 9), mass=True)
            assert out["targets"] == st.n and int(out["count"].sum()) > st.n
            mem1 = sim.memory()
            after = sim.get(names)
            assert all(before[k].tobytes() == after[k].tobytes() for k in names) and sim.scalars() == sc0
            assert mem1["device"] > mem0["device"] and mem1["pinned"] > mem0["pinned"]  # the twopoint.* buffers, counted
            again = sim.twopoint(np.linspace(0.0, 0.2, 9), mass=True)
            assert sim.memory() == mem1
            assert all(np.array_equal(out[k], again[k]) for k in ("count",) + tr.SERIES)
        sim.step()
        return sim.get(["id", "x", "y", "z", "vx", "vy", "vz", "temp", "h"]), sim.scalars()
    finally:
        sim.close()


def test_a_pair_count_changes_no_state(ctx):
    """every field is the same before and after the call, and the next step is the one of a run that never asked"""
    asked, sc_a = run_steps(ctx, True)
    never, sc_n = run_steps(ctx, False)
    assert sc_a == sc_n
    for k in asked:
        assert asked[k].tobytes() == never[k].tobytes(), k


def test_lattice_coordination_numbers_on_the_sedov_lattice(ctx):
    """init_sedov at step 0 is a simple cubic lattice of 16^3 points with spacing a = 1/16 in a periodic box: 6
    neighbours at a, 12 at sqrt(2) a, 8 at sqrt(3) a per point, every pair once: 3 N, 6 N and 4 N.  Arithmetic, not the
    oracle."""
    N, a = 16 ** 3, 1.0 / 16
    sim = sx.Sim(ctx, N + 64, sx.make_box(*SEDOV_BOX))
    try:
        sim.init_sedov(16)
        out = sim.twopoint([0.5 * a, 1.2 * a, 1.6 * a, 1.9 * a], series=("count",))
        assert out["count"].tolist() == [3 * N, 6 * N, 4 * N]
        assert (out["targets"], out["nonfinite"], out["coincident"]) == (N, 0, 0)
        # a lattice at rest: every velocity series is an exact zero
        out = sim.twopoint([0.5 * a, 1.2 * a, 1.6 * a, 1.9 * a])
        assert out["count"].tolist() == [3 * N, 6 * N, 4 * N] and all(np.all(out[k] == 0.0) for k in tr.SERIES[:5])
        # every second id a target: a pair is left out iff both members are odd
        half = sim.twopoint([0.5 * a, 1.2 * a], series=("count",), stride=2, phase=0)
        ids = sim.get(["id"])["id"]
        assert half["targets"] == int(np.count_nonzero(ids % 2 == 0)) and 0 < half["count"][0] < 3 * N
    finally:
        sim.close()


def test_xi_of_uniform_random_points(ctx):
    """4000 uniform random points in the periodic unit box have xi = 0 up to shot noise.  Seed 2024, five linear bins
    from 0.02 to 0.12.  The oracle on the CPU gives for this seed
        count = [1909, 4873, 9778, 16129, 24194]
        xi    = [0.01753, -0.04306, -0.01397, -0.01345, -0.00801]
    The band per bin is four times the Poisson expectation 1 / sqrt(count) of that count:
        band  = [0.09155, 0.0573, 0.04045, 0.0315, 0.02572]"""
    f = tr.uniform(4000, seed=2024)
    edges = np.linspace(0.02, 0.12, 6)
    count = np.array([1909, 4873, 9778, 16129, 24194])
    band = 4.0 / np.sqrt(count)
    ds = sx.DeviceState(ctx, f)
    try:
        got = ctx.twopoint(ds.fields, sx.make_box(*tr.PERIODIC), sx.SxTwoPoint(edges, ("count",)))
    finally:
        ctx.free_all()
    assert got["pairs_expected"] == 4000 * 3999 // 2
    print("count", got["count"].tolist(), "xi", got["xi"].tolist(), "band", band.tolist())
    assert np.all(np.abs(got["xi"]) <= band)
    assert np.array_equal(got["count"], count)
