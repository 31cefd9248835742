"""Direct-sum gravity on the GPU (sx_gravity_direct, exact and fast variants) against the committed output of the
reference's ryoanji::directSum (tests/golden/direct_ref.npz, pinned by tests/test_direct_ref.py).

Bounds, none of them from what the kernels give:
* exact, one split: bit for bit -- the additions per target are the reference loop's, IEEE double sqrt and division
  round correctly on both sides, neither side contracts to FMA;
* exact, any split count: the bound for a re-ordered sum, n (2 shells + 1)^3 2^-52 S_i (direct_ref.reorder_bound);
* fast: the acceptance cap 1e-5 max|a_ref| (a hundred times finer than the ~1e-3 force error the tool is to measure),
  or four times the worst value measured on the fixture cases where that is smaller.
"""
import ctypes as C

import numpy as np
import pytest

import direct_ref as dr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

MARK = np.float32(0.25)
FAST_CAP = 1e-5
#: worst max|a - a_ref| / max|a_ref| of the fast variant over the fixture cases (n300_s2; 3.4e-7 and 3.8e-7 on the
#: two n = 1000 cases), the same with one and with two targets per lane
FAST_MEASURED = 7.81e-7
FAST_BOUND = min(FAST_CAP, 4.0 * FAST_MEASURED)


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


FIX = dr.load_fixture()
_scale = {}


def scale_of(case):
    """the restatement's sums of absolute terms (the reorder bound's S), computed once"""
    if case not in _scale:
        f, shells, _ = FIX[case]
        _scale[case] = dr.direct(f, shells)[1]
    return _scale[case]


def full_view(n):
    return lambda ctx: sx.SxGroups(firstBody=0, lastBody=n, numGroups=(n + 63) // 64)


def run_direct(ctx, f, shells, exact, splits=0, view=None, per_lane=None, fields_edit=None, want_out4=True):
    """(egrav, out4, {ax, ay, az}) of one call; the accelerations start at MARK"""
    n = f["x"].size
    host = dict(f)
    for k in ("ax", "ay", "az"):
        host[k] = np.full(n, MARK, np.float32)
    ctx.set_exact(exact)
    ctx.set_direct_splits(splits)
    if per_lane:
        assert ctx.L.sx_ctx_direct_targets_per_lane_internal(ctx.h, per_lane) == sx.SX_OK
    ds = sx.DeviceState(ctx, host)
    try:
        g = (view or full_view(n))(ctx)
        if fields_edit:
            fields_edit(ds.fields)
        box = sx.make_box([-0.5 * dr.L, 0.5 * dr.L] * 3, [1, 1, 1])
        e, o4 = ctx.gravity_direct(ds.fields, g, box=box if shells else None, num_shells=shells, G=float(dr.G),
                                   out4=want_out4)
        return e, o4, {k: ds.get(k) for k in ("ax", "ay", "az")}
    finally:
        ctx.set_exact(False)
        ctx.set_direct_splits(0)
        ctx.L.sx_ctx_direct_targets_per_lane_internal(ctx.h, 0)
        ctx.free_all()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("case", list(dr.CASES))
def test_exact_one_split_is_the_reference_bit_for_bit(ctx, case):
    f, shells, ref = FIX[case]
    e, o4, acc = run_direct(ctx, f, shells, True, splits=1)
    diff = np.abs(o4 - ref)
    print(case, "exact, one split: entries that differ", int((bits(o4) != bits(ref)).sum()), "max |diff|", diff.max())
    assert np.array_equal(bits(o4), bits(ref))
    for c, k in enumerate(("ax", "ay", "az")):
        want = (np.float64(MARK) + ref[:, 1 + c]).astype(np.float32)
        assert np.array_equal(bits(acc[k]), bits(want)), k
    want_e = 0.5 * np.sum(ref[:, 0])
    assert abs(e - want_e) <= 1e-13 * abs(want_e)


@pytest.mark.parametrize("splits", [3, 0], ids=["splits3", "auto"])
@pytest.mark.parametrize("case", list(dr.CASES))
def test_exact_any_split_count_within_the_reorder_bound(ctx, case, splits):
    f, shells, ref = FIX[case]
    bound = dr.reorder_bound(f["x"].size, shells, scale_of(case))
    e, o4, acc = run_direct(ctx, f, shells, True, splits=splits)
    print(case, splits, "error / reorder bound:", np.max(np.abs(o4 - ref) / bound))
    assert np.all(np.abs(o4 - ref) <= bound)
    want_e = 0.5 * np.sum(ref[:, 0])
    assert abs(e - want_e) <= 1e-13 * abs(want_e)
    e2, o42, acc2 = run_direct(ctx, f, shells, True, splits=splits)
    assert e2 == e and np.array_equal(bits(o42), bits(o4))
    assert all(np.array_equal(bits(acc2[k]), bits(acc[k])) for k in acc)


@pytest.mark.parametrize("per_lane", [1, 2])
@pytest.mark.parametrize("case", list(dr.CASES))
def test_fast_variant_against_the_fixture(ctx, case, per_lane):
    """measured on the MI355X, max|a - a_ref| / max|a_ref|: 3.4e-7 (n1000_s0), 3.8e-7 (n1000_s1), 7.8e-7 (n300_s2);
    the potential 1.3e-7, 5.2e-8, 4.4e-8 of its maximum; egrav 2.1e-8, 2.2e-8, 2.3e-8 relative.  The
    asserted bound is min(1e-5, 4 x 7.81e-7) = 3.1e-6."""
    f, shells, ref = FIX[case]
    e, o4, acc = run_direct(ctx, f, shells, False, per_lane=per_lane)
    amax = np.max(np.abs(ref[:, 1:]))
    err = np.max(np.abs(o4[:, 1:] - ref[:, 1:])) / amax
    want_e = 0.5 * np.sum(ref[:, 0])
    print(case, "targets per lane", per_lane, "fast: max|a - ref| / max|a_ref| =", err, "egrav relative error",
          abs(e - want_e) / abs(want_e), "potential", np.max(np.abs(o4[:, 0] - ref[:, 0])) / np.max(np.abs(ref[:, 0])))
    assert err <= FAST_BOUND
    assert np.max(np.abs(o4[:, 0] - ref[:, 0])) <= FAST_BOUND * np.max(np.abs(ref[:, 0]))
    assert abs(e - want_e) <= 1e-6 * abs(want_e)
    for c, k in enumerate(("ax", "ay", "az")):  # the float outputs: one more rounding
        want = np.float64(MARK) + ref[:, 1 + c]
        assert np.max(np.abs(acc[k] - want)) <= FAST_BOUND * amax + 2.0 ** -24 * np.max(np.abs(want))
    ex = run_direct(ctx, f, shells, True)[1]
    assert not np.array_equal(bits(ex), bits(o4))  # the fast kernel is the one that ran
    e2, o42, _ = run_direct(ctx, f, shells, False, per_lane=per_lane)
    assert e2 == e and np.array_equal(bits(o42), bits(o4))


def make_view(n, seed):
    """random-size groups (1..64 targets) tiling [0, n); every third one, in shuffled order"""
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


def check_view(full, got, act):
    e, o4, acc = got
    assert np.array_equal(bits(o4[act]), bits(full[1][act]))
    assert not np.any(o4[~act])  # out4 outside the view: not written (the zeros it was allocated with)
    for k in acc:
        assert np.array_equal(bits(acc[k][act]), bits(full[2][k][act])), k
        assert np.array_equal(bits(acc[k][~act]), bits(np.full(int((~act).sum()), MARK, np.float32))), k
    want_e = 0.5 * np.sum(o4[act, 0])
    assert abs(e - want_e) <= 1e-13 * abs(want_e)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_views(ctx, exact):
    f, shells, ref = FIX["n1000_s1"]
    n = f["x"].size
    full = run_direct(ctx, f, shells, exact, splits=3)

    act = np.zeros(n, bool)
    act[5:n - 3] = True
    rng_view = lambda c: sx.SxGroups(firstBody=5, lastBody=n - 3, numGroups=(n - 8 + 63) // 64)
    check_view(full, run_direct(ctx, f, shells, exact, splits=3, view=rng_view), act)

    gs, ge, act = make_view(n, 4)
    assert gs.size >= 8 and 0.15 * n < act.sum() < 0.6 * n

    def groups(c):
        gsd, ged = c.upload(gs), c.upload(ge)
        return sx.SxGroups(firstBody=0, lastBody=0, numGroups=gs.size, groupStart=gsd.ptr, groupEnd=ged.ptr)

    check_view(full, run_direct(ctx, f, shells, exact, splits=3, view=groups), act)


def test_empty_views(ctx):
    f, shells, ref = FIX["n300_s2"]
    n = f["x"].size
    for view in (lambda c: sx.SxGroups(firstBody=7, lastBody=7, numGroups=0),
                 lambda c: sx.SxGroups(firstBody=9, lastBody=4, numGroups=0)):
        e, o4, acc = run_direct(ctx, f, shells, False, view=view)
        assert e == 0.0 and not np.any(o4)
        assert all(np.array_equal(bits(acc[k]), bits(np.full(n, MARK, np.float32))) for k in acc)

    z = np.array([3, 10, 10], np.uint32)  # explicit groups of size 0

    def groups(c):
        zs = c.upload(z)
        return sx.SxGroups(firstBody=0, lastBody=0, numGroups=z.size, groupStart=zs.ptr, groupEnd=zs.ptr)

    e, o4, acc = run_direct(ctx, f, shells, True, view=groups)
    assert e == 0.0 and not np.any(o4)


def test_split_edge_cases(ctx):
    """n = 1000 sources: four tiles of 256, the last one of 232.  64 targets are one target block, so the automatic rule
    asks for 4096 splits and is clamped to the four tiles, as is an explicit request beyond them."""
    f, shells, ref = FIX["n1000_s0"]
    n = f["x"].size
    bound = dr.reorder_bound(n, shells, scale_of("n1000_s0"))
    view = lambda c: sx.SxGroups(firstBody=0, lastBody=64, numGroups=1)
    auto = run_direct(ctx, f, shells, True, view=view)
    four = run_direct(ctx, f, shells, True, view=view, splits=4)
    many = run_direct(ctx, f, shells, True, view=view, splits=1000)
    one = run_direct(ctx, f, shells, True, view=view, splits=1)
    assert np.array_equal(bits(one[1][:64]), bits(ref[:64]))
    assert np.array_equal(bits(auto[1]), bits(four[1])) and auto[0] == four[0]
    assert np.array_equal(bits(many[1]), bits(four[1])) and many[0] == four[0]
    assert not np.array_equal(bits(auto[1]), bits(one[1]))  # the automatic rule did split
    assert np.all(np.abs(auto[1][:64] - ref[:64]) <= bound[:64]) and not np.any(auto[1][64:])
    for per_lane in (1, 2):
        fast = run_direct(ctx, f, shells, False, view=view, per_lane=per_lane)
        assert np.max(np.abs(fast[1][:64, 1:] - ref[:64, 1:])) <= FAST_BOUND * np.max(np.abs(ref[:, 1:]))


def test_refusals(ctx):
    f, shells, ref = FIX["n300_s2"]
    n = f["x"].size

    def refused(what, **kw):
        with pytest.raises(sx.SxError) as ei:
            run_direct(ctx, f, kw.pop("shells", 0), False, **kw)
        msg = str(ei.value)
        print(what, "->", msg)
        assert f"code {sx.SX_ERR_ARG}" in msg and "sx_gravity_direct: " in msg and what in msg

    refused("numShells", shells=5)

    def no_h(fields):
        fields.h = None
    refused("h are required", fields_edit=no_h)

    def no_acc(fields):
        fields.ax = fields.ay = fields.az = None
    refused("no output", fields_edit=no_acc, want_out4=False)
    refused("beyond f->n", view=lambda c: sx.SxGroups(firstBody=0, lastBody=n + 1, numGroups=(n + 64) // 64))

    def beyond(c):
        gs, ge = c.upload(np.array([0, n - 10], np.uint32)), c.upload(np.array([10, n + 1], np.uint32))
        return sx.SxGroups(firstBody=0, lastBody=0, numGroups=2, groupStart=gs.ptr, groupEnd=ge.ptr)
    refused("beyond f->n", view=beyond)

    # out4 alone is an output
    e, o4, acc = run_direct(ctx, f, shells, True, splits=1, fields_edit=no_acc)
    assert np.array_equal(bits(o4), bits(ref))
