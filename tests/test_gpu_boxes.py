"""The hydro path in non-cubic, off-origin and mixed-boundary boxes (tests/box_cases.py) against the CPU oracle, which
test_boxes_oracle.py pins bit for bit to the reference in the same boxes.

Every other parity test runs in a cube whose axes share one boundary type; the code is written per axis (keys
normalised by each axis' inverse length, node centres and sizes, the per-axis prefilter test of the search, the cluster
kernels' choice between folded coordinates and applyPBC, putInBox and the fixed-boundary skip, the spatial groups'
per-axis normalisation, the skin grid), and a cube never separates those branches.  The tolerances are the suite's own:
bit-exact keys, order, tree arrays, nc, h, neighbour sets, positions and group boundaries; RTOL 2e-5 of the oracle's
per-particle scales for the float sums (test_gpu_cluster_kernels.check_all, gpu_util.StepChecker).

The position-update kernels in these boxes are in test_gpu_timestep.py, two ranks in test_gpu_distributed.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import box_cases as bc
import gpu_util as gutil
import pyoracle as po
import sphexa_amd as sx
from test_gpu_cluster_kernels import advanced_state, reference_chain, run_cluster_kernels, run_std_chain
from test_gpu_gravity import check_acc, gpu_gravity
from test_gpu_group_views import make_view
from test_gpu_groups import gpu_groups
from test_gpu_parity import FLOATS
from test_gpu_search_builds import search
from test_gpu_skin import skin_vs_fresh

pytestmark = pytest.mark.gpu

HYDRO = ["thin_z", "gresho", "windshock", "mixed", "far_mixed", "far_pbc"]


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ora():
    return po.load_oracle()


@functools.lru_cache(maxsize=None)
def _advanced(name, prop):
    """the case's state after 2 oracle steps, key-sorted, with the oracle's neighbor list (computed once)"""
    ora = po.load_oracle()
    params = ora.params(av_clean=(prop == "avclean"), std=(prop == "std"))
    return advanced_state(ora, None, None, 2, params, state=bc.state(name))


def advanced(name, prop="ve"):
    st, box, nbr = _advanced(name, prop)
    return st.copy(), box, nbr


def assert_intent(name, ora):
    """the case reaches the code path it is sized for (box_cases.check_regime, on the oracle alone)"""
    st, box = bc.state(name)
    rule, waves = bc.check_regime(st, box, ora)
    if name in ("thin_z", "gresho"):
        assert rule >= 0.9, (name, rule)
    elif name in ("windshock", "far_pbc"):
        assert rule == 0.0 and waves == 0.0, (name, rule, waves)
    elif name in ("mixed", "far_mixed"):
        assert 0.0 < rule < 1.0 and 0.0 < waves < 1.0, (name, rule, waves)


# ---- 1. keys, sort, tree --------------------------------------------------------------------------------------

@pytest.mark.parametrize("bucket", [64, 1])
@pytest.mark.parametrize("name", list(bc.CASES))
def test_keys_sort_tree_exact(ctx, ora, name, bucket):
    """test_gpu_parity.test_keys_sort_tree_exact in every box, with a particle on each lower limit, on each upper
    limit (it clamps to the last cell) and a nextafter below each upper limit"""
    st, obox = bc.state(name)
    st = bc.with_edges(st, obox)
    box = gutil.box_to_sx(obox)
    n = st.n
    x, y, z = ctx.upload(st.x), ctx.upload(st.y), ctx.upload(st.z)
    keys = ctx.alloc(n, np.uint64)
    ctx.check(ctx.L.sx_sfc_keys(ctx.h, x.ptr, y.ptr, z.ptr, keys.ptr, n, C.byref(box)), "keys")
    ref_keys = ora.sfc_keys(st, obox).copy()
    got = keys.get()
    assert np.array_equal(got, ref_keys), np.nonzero(got != ref_keys)[0][:8]
    order = ctx.alloc(n, np.uint32)
    ctx.check(ctx.L.sx_sort_keys(ctx.h, keys.ptr, order.ptr, n), "sort")
    assert np.array_equal(order.get(), np.argsort(ref_keys, kind="stable"))
    skeys = np.sort(ref_keys)
    assert np.array_equal(keys.get(), skeys)
    tree, host = gutil.device_tree(ctx, keys, n, bucket, box)
    ref = ora.octree(skeys, bucket)
    for k in ["leaves", "counts", "prefixes", "childOffsets", "parents", "levelRange", "internalToLeaf",
              "leafToInternal"]:
        assert np.array_equal(host[k], ref[k]), k
    c, s = ora.node_centers(ref["prefixes"], obox)
    assert np.array_equal(host["centers"], c) and np.array_equal(host["sizes"], s)
    assert np.array_equal(host["layout"][:-1], np.concatenate([[0], np.cumsum(ref["counts"])[:-1]]))
    ctx.free_all()


# ---- 2. search ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", HYDRO)
def test_search_builds_identical_and_exact(ctx, ora, name):
    """the three search modes of test_gpu_search_builds.py (large, compact, forced fallback) with the h-nc iteration
    running (h0 = 1.35 h): identical lists, union sizes and statistics; nc and h bit-exact and the neighbour sets equal
    to the oracle's.  In the far boxes any absolute coordinate that passes through a float loses the particle spacing"""
    assert_intent(name, ora)
    st, obox = bc.state(name)
    gutil.sorted_state(st, obox, ora)
    h0 = (st.h * np.float32(1.35)).astype(np.float32)
    big = search(ctx, st, obox, 1, h0)
    small = search(ctx, st, obox, 2, h0)
    fb = search(ctx, st, obox, 3, h0)
    assert big["build"] == 1 and fb["build"] == 2 and small["build"] in (0, 2)
    assert not np.array_equal(big["h"], h0)  # the iteration iterated
    for other in (small, fb):
        assert np.array_equal(other["h"], big["h"])
        assert np.array_equal(other["nc"], big["nc"])
        assert np.array_equal(other["nbr"], big["nbr"])
        for k in ("sum", "max", "failed", "union", "cand"):
            assert other[k] == big[k], k
    ref = st.copy()
    ref.h[:] = h0
    rn, rnc = ora.find_neighbors(ref, obox, iterate_h=True)
    assert np.array_equal(big["h"], ref.h) and np.array_equal(big["nc"], rnc)
    a = gutil.rows_sorted(big["nbr"].ravel(), big["nc"], 150)
    b = gutil.rows_sorted(rn, rnc, 150)
    bad = [i for i, (p, q) in enumerate(zip(a, b)) if not np.array_equal(p, q)]
    assert not bad, (len(bad), bad[:5])


# ---- 3. cluster kernels in isolation --------------------------------------------------------------------------

@pytest.mark.parametrize("name,prop,view", [("thin_z", "ve", False), ("windshock", "ve", False),
                                            ("mixed", "ve", False), ("far_mixed", "ve", False),
                                            ("gresho", "avclean", False), ("mixed", "ve", True)])
def test_cluster_kernels_vs_oracle(ctx, ora, name, prop, view):
    """every VE cluster kernel in isolation on the oracle's inputs (test_gpu_cluster_kernels.run_cluster_kernels) on
    the case's state after 2 oracle steps; `view`: on a shuffled third of random-size explicit groups"""
    av_clean = prop == "avclean"
    params = ora.params(av_clean=av_clean)
    st, box, nbr = advanced(name, prop)
    chk = st.copy()
    ref, sc = reference_chain(ora, chk, box, nbr, params, st.minDt)
    inputs = {"h": st.h.copy(), "nc": st.nc.copy()}
    v = make_view(st.n, 1) if view else None
    worst = run_cluster_kernels(ctx, st, gutil.box_to_sx(box), inputs, ref, sc, params, st.minDt, av_clean, view=v)
    print("cluster", name, prop, "view" if view else "all", {k: f"{v:.2e}" for k, v in worst.items()})


def test_cluster_kernels_std_vs_oracle(ctx, ora):
    """the std chain (density, EOS, IAD, momentum/energy) on windshock after 2 std oracle steps"""
    st, box, nbr = advanced("windshock", "std")
    worst = run_std_chain(ctx, ora, st, box, nbr, ora.params(std=True))
    print("cluster std windshock", {k: f"{v:.2e}" for k, v in worst.items()})


# ---- 5. spatial groups ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["thin_z", "mixed", "far_pbc"])
def test_spatial_groups_match_oracle(ctx, ora, name):
    """sx_spatial_groups against the oracle's computeGroupSplits restatement: the whole range and the two sub-ranges
    of test_gpu_groups.py"""
    st, obox = bc.state(name)
    gutil.sorted_state(st, obox, ora)
    t = ora.octree(st.keys, 64)
    layout = np.concatenate([[0], np.cumsum(t["counts"])]).astype(np.uint32)
    n = st.n
    # tolFactor 2 is the propagator's (sph/groups.cu:38); on these lattices it leaves every group whole, so 0.4 is
    # run as well: there the criterion, a distance in box-scaled coordinates against the leaf size, cuts at the steps
    # along the axis with the fewest cells and not along the others, and the per-axis scaling decides the result
    for tol in (2.0, 0.4):
        for first, last in ((0, n), (37, n - 11), (n // 3, n // 3 + 130)):
            ref = ora.group_splits(first, last, st.x, st.y, st.z, t["leaves"], layout, obox, tol)
            got = gpu_groups(ctx, first, last, st.x, st.y, st.z, t["leaves"], layout, obox, tol)
            assert np.array_equal(got, ref), (name, tol, first, last, got.size, ref.size)
            assert np.all(np.diff(got) > 0) and np.all(np.diff(got) <= 64)
        if tol == 0.4:
            sizes = np.diff(ora.group_splits(0, n, st.x, st.y, st.z, t["leaves"], layout, obox, tol))
            assert (n + 63) // 64 < sizes.size < n and sizes.max() > 1, (name, sizes.size)


# ---- 6. sim steps ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,av_clean", [("thin_z", False), ("gresho", False), ("windshock", False),
                                           ("mixed", False), ("far_mixed", False), ("mixed", True)])
def test_sim_steps_vs_oracle(ctx, ora, name, av_clean):
    """3 sx_sim steps with the default skin settings, each checked per particle against an oracle step from the same
    state.  Steps 2 and 3 filter the first step's lists, except in the thin boxes (thin_z, gresho), where the skin
    lists of nearly every cluster outgrow the filter and the driver searches anew every step (measured: 3 builds,
    0 reuse steps): a matter of speed, the steps are checked all the same"""
    st, obox = bc.state(name)
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox), params=sx.default_params(av_clean=av_clean))
    sim.set_state(st.arrays, st.minDt, st.minDt_m1)
    try:
        chk = gutil.shadow_steps(ctx, ora, sim, obox, 3, ora.params(av_clean=av_clean), FLOATS)
        print("steps", name, "avclean" if av_clean else "ve", {k: f"{v:.2g}" for k, v in chk.worst.items()})
        ks = sim.skin_stats()
        print("skin", name, {k: ks[k] for k in ("builds", "reuse_steps", "exact_clusters")})
        if name not in ("thin_z", "gresho"):
            assert ks["reuse_steps"] >= 1, ks
    finally:
        sim.close()


# ---- 7. skin over more steps ----------------------------------------------------------------------------------

def test_skin_windshock_equal_fresh_search(ctx):
    """12 steps in windshock started near the Courant step (dt0 = 1e-3: the shear moves the particles by a few per
    cent of h per step, across the periodic faces of the long axis too): every step's neighbour sets, nc and h equal a
    fresh sync + search of the same state (test_gpu_skin.skin_vs_fresh), and the lists were reused"""
    st, obox = bc.state("windshock", dt0=1e-3)
    ks = skin_vs_fresh(ctx, st, obox, 12, 0.08, "windshock")
    assert ks["reuse_steps"] >= 1 and ks["builds"] >= 1, ks


# ---- 8. open gravity in a non-cubic box -----------------------------------------------------------------------

def test_open_gravity_vs_oracle(ctx, ora):
    """sx_gravity_upsweep / sx_gravity_traverse in the 2 x 1 x 0.5 open box: test_gpu_gravity.test_gravity_vs_oracle's
    bounds at theta 0.5 (centers and multipoles bit-identical, accelerations to the summation order, egrav 1e-10)"""
    st, box = bc.state("open_grav")
    gutil.sorted_state(st, box, ora)
    out = gpu_gravity(ctx, st, box, theta=0.5)
    ref = st.copy()
    eg, cen, mp = ora.gravity(ref, box, ora.params(g=1.0, theta=0.5))
    assert np.array_equal(out["centers"], cen)
    assert np.array_equal(out["multipoles"], mp)
    check_acc(out, ref.arrays)
    assert out["egrav"] == pytest.approx(eg, rel=1e-10)
    ctx.free_all()


def test_open_gravity_sim_steps(ctx, ora):
    """2 VE + self-gravity steps of sx_sim in that box, per particle against the oracle (test_sim_steps_with_gravity)"""
    st, obox = bc.state("open_grav")
    sim = sx.Sim(ctx, st.n, gutil.box_to_sx(obox), params=sx.default_params(g=1.0, theta=0.5))
    sim.set_state(st.arrays, st.minDt, st.minDt_m1)

    def egrav(s, sim, ref):
        assert sim.scalars()["egrav"] == pytest.approx(ref.egrav, rel=1e-5)

    try:
        chk = gutil.shadow_steps(ctx, ora, sim, obox, 2, ora.params(g=1.0, theta=0.5), FLOATS, on_step=egrav)
        print("steps open_grav g=1", {k: f"{v:.2g}" for k, v in chk.worst.items()})
    finally:
        sim.close()


@pytest.mark.parametrize("name", ["windshock", "mixed"])
def test_gravity_refused_in_periodic_box_cases(ctx, name):
    """self-gravity needs an open box or a periodic cube: a non-cubic periodic box and a box periodic along one axis
    are refused at creation with SX_ERR_ARG and a reason, not stepped wrongly"""
    st, obox = bc.state(name)
    box = gutil.box_to_sx(obox)
    p = sx.default_params(g=1.0)
    h = C.c_void_p()
    assert ctx.L.sx_sim_create(C.byref(h), ctx.h, st.n, C.byref(p), C.byref(box), 64) == sx.SX_ERR_ARG
    msg = ctx.L.sx_last_error(ctx.h)
    assert msg and len(msg) > 10, msg
