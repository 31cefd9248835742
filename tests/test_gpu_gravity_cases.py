"""Self-gravity on the GPU on the inputs of tests/gravity_cases.py: clumps in a sparse halo, six decades of mass, massless
bodies, coincident bodies and bodies on node boundaries, a box far from the origin, deep trees, tiny views, a periodic
box.  Through the C ABI like test_gpu_gravity.py (sx_gravity_upsweep / _traverse / _traverse_pbc) plus
sx_gravity_direct and the step driver.

References and bounds, none of them from what the kernels give:
* upsweep: the exact variant's centres and multipoles are the oracle's bit for bit; the fast variant passes
  test_gpu_gravity.check_upsweep_fast;
* the walk at theta = 0.5 and 0.9 against the oracle's walk (pinned to the reference's CPU functions): exact
  1e-6 |a_ref| + 1e-7 A, egrav to 1e-10; production 1e-5 |a_ref| + 1e-6 A, egrav to 1e-6 (A = max |a_ref|).  On `massless`
  the oracle, like the reference, is not finite for the body on the origin (0 * inf in the M2P of an empty node,
  tests/test_gravity_cases.py): that body and egrav are compared with direct_ref alone, below;
* the walk at theta = 1e-20, which opens every node, against the float64 direct sum of direct_ref: the two sides are then
  the same sum.  Per target and component, production |a - a_ref| <= 1e-5 S_i (test_gpu_direct.FAST_CAP on the sum of
  the absolute terms of target i), exact direct_ref.reorder_bound plus the float rounding of the output;
* sx_gravity_direct in key order and shuffled: the same two bounds.
Every test prints its worst error / bound.
"""
import ctypes as C

import numpy as np
import pytest

import direct_ref as dr
import gpu_util as gutil
import gravity_cases as gc
import nbody_ref as nr
import pyoracle as po
import sphexa_amd as sx
from sphexa_amd import ic
from test_gpu_direct import FAST_CAP, bits, check_view, make_view, run_direct
from test_gpu_gravity import check_upsweep_fast
from test_gpu_nbody import check_shadow_step, make_sim, state_of

pytestmark = pytest.mark.gpu

ALL_OPEN = 1e-20
VARIANTS = pytest.mark.parametrize("exact", [True, False], ids=["exact", "production"])
CASE_BUCKETS = [(name, b) for name in gc.CASES for b in ((64, 16, 8, 1) if name == "deep_uniform" else (64, 16))]
WALK_BOUNDS = {True: (1e-6, 1e-7, 1e-10), False: (1e-5, 1e-6, 1e-6)}  # (rtol, atol_frac, egrav rel)


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.set_exact(False)
    c.close()


@pytest.fixture(scope="module")
def ora():
    return po.load_oracle()


_prep, _direct, _walk = {}, {}, {}


def build(name):
    if name == "periodic":
        return gc.periodic()
    if name.startswith("picks"):
        return gc.picks(int(name[5:]))
    return gc.case(name)


def prepared(name, ora):
    """(state sorted by the oracle's keys, oracle box), built once and left unchanged"""
    if name not in _prep:
        _prep[name] = gc.oracle_state(*build(name), ora)
    return _prep[name]


def direct_of(name, ora, shells=0, targets=None):
    """float64 direct sum (out4, S) of the sorted state, once per case"""
    if name not in _direct:
        st, box = prepared(name, ora)
        _direct[name] = gc.direct(gc.fields_of(st), shells, L=1.0, targets=targets)
    return _direct[name]


def oracle_walk(name, ora, theta, bucket, first=0, last=None):
    key = (name, theta, bucket, first, last)
    if key not in _walk:
        st, box = prepared(name, ora)
        ref = st.copy()
        ref.keys[:] = st.keys
        eg, cen, mp = ora.gravity(ref, box, ora.params(g=1.0, theta=theta), first=first, last=last, bucket=bucket)
        _walk[key] = (np.column_stack([ref.ax, ref.ay, ref.az]).astype(np.float64), eg, cen, mp)
    return _walk[key]


def gpu_walk(ctx, st, obox, theta, bucket, exact, first=0, last=None, shells=None, a0=0.0):
    """upsweep and traversal of [first, last) on the device; the accelerations start at a0"""
    last = st.n if last is None else last
    ctx.set_exact(exact)
    try:
        box = gutil.box_to_sx(obox)
        host = gutil.host_dict(st)
        for k in ("ax", "ay", "az"):
            host[k] = np.full(st.n, a0, np.float32)
        ds = sx.DeviceState(ctx, host)
        tree, _ = gutil.device_tree(ctx, ds.dev["keys"], st.n, bucket, box)
        nn = tree.numNodes
        cen = ctx.alloc(4 * nn, np.float64)
        mp = ctx.alloc(8 * nn, np.float32)
        ctx.check(ctx.L.sx_gravity_upsweep(ctx.h, C.byref(ds.fields), C.byref(tree), theta, cen.ptr, mp.ptr), "upsweep")
        g = sx.SxGroups(firstBody=first, lastBody=last, numGroups=(last - first + 63) // 64)
        eg = C.c_double()
        if shells is None:
            ctx.check(ctx.L.sx_gravity_traverse(ctx.h, C.byref(g), C.byref(ds.fields), C.byref(tree), C.byref(box),
                                                cen.ptr, mp.ptr, 1.0, C.byref(eg)), "traverse")
        else:
            ctx.check(ctx.L.sx_gravity_traverse_pbc(ctx.h, C.byref(g), C.byref(ds.fields), C.byref(tree), C.byref(box),
                                                    cen.ptr, mp.ptr, 1.0, shells, C.byref(eg)), "traverse_pbc")
        a = np.column_stack([ds.get(k) for k in ("ax", "ay", "az")]).astype(np.float64)
        return a, eg.value, cen.get().reshape(-1, 4), mp.get().reshape(-1, 8)
    finally:
        ctx.set_exact(False)
        ctx.free_all()


def worst(err, bound):
    return float(np.max(err / (bound + 1e-300)))


def check_walk(tag, a, eg, ref, eg_ref, exact, rows=None):
    """the bounds of test_gpu_gravity.check_acc, on the rows where the oracle is finite"""
    rtol, atol, erel = WALK_BOUNDS[exact]
    rows = np.arange(ref.shape[0]) if rows is None else rows
    fin = rows[np.all(np.isfinite(ref[rows]), axis=1)]
    A = np.max(np.abs(ref[fin]))
    bound = rtol * np.abs(ref[fin]) + atol * A
    err = np.abs(a[fin] - ref[fin])
    print(tag, "exact" if exact else "production", "worst error / bound:", f"{worst(err, bound):.3g}",
          "egrav rel:", f"{abs(eg / eg_ref - 1):.3g}" if np.isfinite(eg_ref) else "oracle not finite")
    assert np.all(np.isfinite(a)) and np.isfinite(eg)
    assert np.all(err <= bound), (tag, worst(err, bound))
    if np.isfinite(eg_ref):
        assert eg == pytest.approx(eg_ref, rel=erel)


def all_open_bound(n, shells, S, ref, exact):
    if exact:
        return dr.reorder_bound(n, shells, S[:, 1:]) + 2.0 ** -24 * np.abs(ref[:, 1:])
    return FAST_CAP * S[:, 1:]


# ---- upsweep ---------------------------------------------------------------------------------------------------------

@VARIANTS
@pytest.mark.parametrize("name,bucket", CASE_BUCKETS)
def test_upsweep(ctx, ora, name, bucket, exact):
    st, obox = prepared(name, ora)
    _, _, cen_ref, mp_ref = oracle_walk(name, ora, 0.5, bucket)
    _, _, cen, mp = gpu_walk(ctx, st, obox, 0.5, bucket, exact, first=0, last=1)
    assert cen.shape == cen_ref.shape and mp.shape == mp_ref.shape
    if exact:
        assert np.array_equal(cen, cen_ref)
        assert np.array_equal(mp, mp_ref)
    else:
        check_upsweep_fast(cen, mp, cen_ref, mp_ref)


# ---- the walk against the oracle's walk --------------------------------------------------------------------------------

@VARIANTS
@pytest.mark.parametrize("theta", [0.5, 0.9])
@pytest.mark.parametrize("name,bucket", CASE_BUCKETS)
def test_walk_against_the_oracle(ctx, ora, name, bucket, theta, exact):
    st, obox = prepared(name, ora)
    ref, eg_ref, _, _ = oracle_walk(name, ora, theta, bucket)
    a, eg, _, _ = gpu_walk(ctx, st, obox, theta, bucket, exact)
    check_walk(f"{name} bucket {bucket} theta {theta}", a, eg, ref, eg_ref, exact)


@VARIANTS
@pytest.mark.parametrize("first,cut", [(100, 77), (1, 64), (63, 1), (4096 - 33, 129)])
def test_walk_sub_ranges_with_ragged_ends(ctx, ora, first, cut, exact):
    """targets [first, n - cut) only, as test_gravity_sub_range: the others keep their acceleration"""
    name = "halo_clumps_1e-3"
    st, obox = prepared(name, ora)
    last = st.n - cut
    ref, eg_ref, _, _ = oracle_walk(name, ora, 0.5, 64, first, last)
    a, eg, _, _ = gpu_walk(ctx, st, obox, 0.5, 64, exact, first, last, a0=0.25)
    full = oracle_walk(name, ora, 0.5, 64)[0]  # the scale A of the whole case
    rtol, atol, erel = WALK_BOUNDS[exact]
    rows = np.arange(first, last)
    bound = rtol * np.abs(ref[rows]) + atol * np.max(np.abs(full))
    err = np.abs(a[rows] - 0.25 - ref[rows])
    # 0.25 + a rounded to float: one more rounding of the output
    bound = bound + 2.0 ** -24 * np.abs(0.25 + ref[rows])
    print("sub-range", first, last, "exact" if exact else "production", "worst error / bound:", worst(err, bound))
    assert np.all(err <= bound)
    assert np.all(a[:first] == 0.25) and np.all(a[last:] == 0.25)
    assert eg == pytest.approx(eg_ref, rel=erel)


@VARIANTS
@pytest.mark.parametrize("n", gc.PICKS)
def test_picks_as_full_ranges(ctx, ora, n, exact):
    """1 .. 129 bodies: quarter and wave edges, a root that is a leaf; against the oracle's walk (theta = 0.5) where it
    has a tree to walk, and with every node open against the direct sum"""
    name = f"picks{n}"
    st, obox = prepared(name, ora)
    ref4, S = direct_of(name, ora)
    a, eg, _, _ = gpu_walk(ctx, st, obox, ALL_OPEN, 64, exact)
    bound = all_open_bound(n, 0, S, ref4, exact)
    err = np.abs(a - ref4[:, 1:])
    print(name, "exact" if exact else "production", "all open, worst error / bound:", worst(err, bound))
    assert np.all(np.isfinite(a)) and np.all(err <= bound)
    if n > 1:
        assert eg == pytest.approx(0.5 * np.sum(ref4[:, 0]), rel=WALK_BOUNDS[exact][2])
    for bucket in (64, 16):
        ref, eg_ref, _, _ = oracle_walk(name, ora, 0.5, bucket)
        a, eg, _, _ = gpu_walk(ctx, st, obox, 0.5, bucket, exact)
        if n == 1:
            assert not np.any(a) and eg == eg_ref  # a body exerts no force on itself; its own potential term
        else:
            check_walk(f"{name} bucket {bucket} theta 0.5", a, eg, ref, eg_ref, exact)


# ---- the walk with every node open against the direct sum in float64 ---------------------------------------------------

@VARIANTS
@pytest.mark.parametrize("name,bucket", CASE_BUCKETS)
def test_all_open_walk_against_the_direct_sum(ctx, ora, name, bucket, exact):
    st, obox = prepared(name, ora)
    ref4, S = direct_of(name, ora)
    a, eg, _, _ = gpu_walk(ctx, st, obox, ALL_OPEN, bucket, exact)
    bound = all_open_bound(st.n, 0, S, ref4, exact)
    err = np.abs(a - ref4[:, 1:])
    ratio = err / (bound + 1e-300)
    print(name, "bucket", bucket, "exact" if exact else "production", "all open, worst error / bound:",
          f"{ratio.max():.3g}", "targets beyond the bound:", int((ratio.max(axis=1) > 1).sum()), "of", st.n,
          "worst error / S_i:", f"{np.max(err / S[:, 1:]):.3g}")
    assert np.all(np.isfinite(a)) and np.isfinite(eg)
    assert np.all(err <= bound), (name, bucket, ratio.max())
    assert eg == pytest.approx(0.5 * np.sum(ref4[:, 0]), rel=WALK_BOUNDS[exact][2])


@VARIANTS
@pytest.mark.parametrize("bucket", [64, 16])
def test_all_open_image_walk_against_the_direct_sum(ctx, ora, bucket, exact):
    """sx_gravity_traverse_pbc, one shell, without the Ewald term, against direct(..., shells = 1) on the clump bodies
    and every eighth of the others (the reference sum is 27 times the open one)"""
    name = "periodic"
    st, obox = prepared(name, ora)
    t = np.flatnonzero((st.order >= 4096) | (np.arange(st.n) % 8 == 0))
    ref4, S = direct_of(name, ora, shells=1, targets=t)
    a, eg, _, _ = gpu_walk(ctx, st, obox, ALL_OPEN, bucket, exact, shells=1)
    bound = all_open_bound(st.n, 1, S, ref4, exact)
    err = np.abs(a[t] - ref4[:, 1:])
    print(name, "bucket", bucket, "exact" if exact else "production", "one shell, worst error / bound:",
          worst(err, bound), "worst error / S_i:", np.max(err / S[:, 1:]))
    assert np.all(np.isfinite(a)) and np.isfinite(eg)
    assert np.all(err <= bound)


# ---- sx_gravity_direct -------------------------------------------------------------------------------------------------

DIRECT_CASES = ["halo_clumps_1e-2", "halo_clumps_1e-3", "halo_clumps_1e-4", "mass_ratio"]


def shuffled(name, ora):
    """(fields in a shuffled order, the permutation): a tile of 256 sources then spans the box"""
    st, _ = prepared(name, ora)
    p = np.random.default_rng(7500).permutation(st.n)
    return gc.take(gc.fields_of(st), p), p


@VARIANTS
@pytest.mark.parametrize("order", ["key_order", "shuffled"])
@pytest.mark.parametrize("name", DIRECT_CASES)
def test_direct_sum(ctx, ora, name, order, exact):
    st, _ = prepared(name, ora)
    ref4, S = direct_of(name, ora)
    f = gc.fields_of(st)
    if order == "shuffled":
        f, p = shuffled(name, ora)
        ref4, S = ref4[p], S[p]
    e, o4, acc = run_direct(ctx, f, 0, exact)
    bound = dr.reorder_bound(st.n, 0, S) if exact else FAST_CAP * S
    err = np.abs(o4 - ref4)
    ratio = err[:, 1:] / (bound[:, 1:] + 1e-300)
    print(name, order, "exact" if exact else "fast", "direct sum, worst error / bound:", f"{ratio.max():.3g}",
          "targets beyond the bound:", int((ratio.max(axis=1) > 1).sum()), "of", st.n, "potential:",
          f"{worst(err[:, 0], bound[:, 0]):.3g}")
    assert np.all(np.isfinite(o4))
    assert np.all(err <= bound), (name, order, ratio.max())
    want_e = 0.5 * np.sum(ref4[:, 0])
    assert abs(e - want_e) <= (1e-13 if exact else 1e-6) * abs(want_e)


@VARIANTS
def test_direct_views_and_repeat_runs(ctx, ora, exact):
    """as test_gpu_direct.test_views, on shuffled clumps: a view's targets get the full run's values bit for bit, and a
    second run repeats the first"""
    f, p = shuffled("halo_clumps_1e-3", ora)
    n = f["x"].size
    full = run_direct(ctx, f, 0, exact, splits=3)
    again = run_direct(ctx, f, 0, exact, splits=3)
    assert again[0] == full[0] and np.array_equal(bits(again[1]), bits(full[1]))
    assert all(np.array_equal(bits(again[2][k]), bits(full[2][k])) for k in full[2])
    act = np.zeros(n, bool)
    act[5:n - 3] = True
    rng_view = lambda c: sx.SxGroups(firstBody=5, lastBody=n - 3, numGroups=(n - 8 + 63) // 64)
    check_view(full, run_direct(ctx, f, 0, exact, splits=3, view=rng_view), act)
    gs, ge, act = make_view(n, 4)

    def groups(c):
        gsd, ged = c.upload(gs), c.upload(ge)
        return sx.SxGroups(firstBody=0, lastBody=0, numGroups=gs.size, groupStart=gsd.ptr, groupEnd=ged.ptr)

    check_view(full, run_direct(ctx, f, 0, exact, splits=3, view=groups), act)


# ---- through the driver --------------------------------------------------------------------------------------------------

def clump_arrays():
    """halo_clumps(1e-3) with the fields of the gravity-only propagator: the halo moves as ic.plummer set it, the clump
    bodies start at rest"""
    f, lim, bnd = gc.case("halo_clumps_1e-3")
    arr, _, _, dt0 = ic.plummer(4096, 1)
    n = f["x"].size
    out = {k: f[k].copy() for k in f}
    for k in ("vx", "vy", "vz", "x_m1", "y_m1", "z_m1"):
        out[k] = np.concatenate([arr[k], np.zeros(n - 4096, np.float32)])
    out["id"] = np.arange(n, dtype=np.uint64)
    return out, po.make_box6(lim, bnd), dt0


@VARIANTS
def test_shadowed_steps_on_the_clumps(ctx, ora, exact):
    """two steps of propagator 3, the CPU composition re-seeded from the sim's state before each"""
    arr, obox, dt0 = clump_arrays()
    ctx.set_exact(exact)
    sim = make_sim(ctx, arr, obox, dt0)
    params = ora.params(g=1.0, theta=0.5)
    try:
        for s in range(2):
            g0, sc0 = state_of(sim)
            ref = nr.host_state(g0, sc0["minDt"], sc0["minDt_m1"], sc0["ttot"])
            fig = nr.nbody_step(ora, ref, obox, params)
            sim.step()
            got = sim.get(nr.FIELDS + ["ax", "ay", "az"])
            w = check_shadow_step(got, sim.scalars(), ref, fig, sc0, exact)
            print("clumps, step", s, "exact" if exact else "production", "worst error / bound:",
                  {k: f"{v:.2g}" for k, v in w.items()})
    finally:
        sim.close()
        ctx.set_exact(False)


def test_armed_step_on_the_clumps(ctx):
    """the force-error check of the step at a theta that opens every node: the walk and the direct sum are the same sum,
    each within 1e-5 of it, so max <= 2e-5 (test_gpu_gravity_check.py)"""
    arr, obox, dt0 = clump_arrays()
    sim = make_sim(ctx, arr, obox, dt0, theta=0.01)
    try:
        n = sim.size()
        sim.set_gravity_check(n)
        sim.step()
        c = sim.gravity_check()
        print("clumps, theta 0.01:", c)
        assert c["targets"] == n
        assert c["max"] <= 2e-5
    finally:
        sim.close()
