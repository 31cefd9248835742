"""Friends-of-friends groups on the GPU at seam level (sx_fof_compute through Context.fof) on uploaded synthetic columns,
against tests/fof_ref.py.  The partition is a property of the particle set, so labels, group counts, catalogue labels and
member counts are compared with array_equal; every such comparison first asserts that the input has no pair on the
criterion (near ties == 0: a condition on the input, not a tolerance).  Masses are float32 in [0.5, 1.5) / n, whose double
sums are exact in any order at these sizes: bit for bit.  Centres and velocities: within the summation bound the oracle
computes per group."""
import functools

import numpy as np
import pytest

import fof_ref as fr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

N = 20000


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def run(ctx, f, box, ell, ids=None, first=0, last=None, min_members=20, max_groups=4096, labels=True):
    """(device result, stats) for the particles [first, last) of the host columns f"""
    lim, bnd = box
    ds = sx.DeviceState(ctx, {k: np.asarray(v) for k, v in f.items()})
    try:
        dev_id = ctx.upload(np.ascontiguousarray(ids, dtype=np.uint64)) if ids is not None else None
        got = ctx.fof(ds.fields, sx.make_box(lim, bnd), sx.SxFof(ell, min_members, max_groups), id=dev_id, first=first,
                      last=last, labels=labels)
        return got, ctx.fof_stats()
    finally:
        ctx.free_all()


assert_same = fr.assert_same


BOXES = {"periodic": (fr.PERIODIC, 0), "open": (fr.OPEN, 16), "mixed": (fr.MIXED, 16)}


@functools.lru_cache(maxsize=None)
def clustered_case(name):
    """the clustered columns in the box `name`, ids (a random permutation), the linking length, and the oracle's result
    by index and by id; computed once and left unchanged"""
    box, outside = BOXES[name]
    f = fr.clustered(N, box=box, seed=7, outside=outside)
    ell = fr.mean_spacing_length(N, box)
    ids = np.random.default_rng(99).permutation(N).astype(np.uint64)
    return f, ids, ell, fr.fof(f, *box, ell), fr.fof(f, *box, ell, ids=ids)


def test_clustered_by_index_and_by_id(ctx):
    f, ids, ell, by_index, by_id = clustered_case("periodic")
    assert by_index["num_groups"] >= 30 and by_index["count"][0] > 100 and by_index["num_all"] > 5000
    got, stats = run(ctx, f, fr.PERIODIC, ell)
    assert_same(got, by_index, fr.PERIODIC)
    assert stats["num_all"] == by_index["num_all"] and stats["num_groups"] == by_index["num_groups"]
    assert stats["pair_tests"] >= by_index["links"]
    got, _ = run(ctx, f, fr.PERIODIC, ell, ids=ids)
    assert_same(got, by_id, fr.PERIODIC)
    # the same partition under either naming: a group's id label is the smallest id among the members of its index label
    smallest = np.full(N, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(smallest, by_index["label"].astype(np.int64), ids)
    assert np.array_equal(got["label"], smallest[by_index["label"].astype(np.int64)])


@pytest.mark.parametrize("name", ["open", "mixed"])
def test_boxes_clamping_and_fixed_axis(ctx, name):
    box = BOXES[name][0]
    f, ids, ell, by_index, by_id = clustered_case(name)
    lim, bnd = box
    outside = sum(int(np.count_nonzero((f[k] < lim[2 * a]) | (f[k] >= lim[2 * a + 1]))) for a, k in enumerate("xyz") if bnd[a] != 1)
    assert outside >= 8, "some particles lie outside the open axes"
    got, _ = run(ctx, f, box, ell)
    assert_same(got, by_index, box)
    got, _ = run(ctx, f, box, ell, ids=ids)
    assert_same(got, by_id, box)


def test_chain_round_the_periodic_axis(ctx):
    f = fr.helix()
    ref = fr.fof(f, *fr.PERIODIC, 0.01, min_members=1)
    assert ref["links"] == 4096 and ref["num_all"] == 1
    got, stats = run(ctx, f, fr.PERIODIC, 0.01, min_members=1)
    # the chain spans the box: its centre of mass is outside the definition's guarantee, and both sides still follow the
    # same formula
    assert_same(got, ref, fr.PERIODIC)
    assert got["count"].tolist() == [4097] and np.all(got["label"] == got["label"].min())


def test_dense_cell_has_no_list_cap(ctx):
    n = 3000
    f = fr.dense_ball(n)
    got, stats = run(ctx, f, fr.OPEN, 0.05, min_members=1)
    assert got["num_all"] == 1 and got["count"].tolist() == [n] and np.all(got["label"] == 0)
    assert stats["pair_tests"] == n * (n - 1) // 2, "every unordered pair of the cell is tested once"
    ref = fr.fof(f, *fr.OPEN, 0.05, min_members=1)
    assert ref["links"] == n * (n - 1) // 2
    assert_same(got, ref, fr.OPEN)


def small(n, seed):
    """n + 6 points in a corner of the periodic unit box, dense enough to form several groups"""
    rng = np.random.default_rng(seed)
    p = np.mod(0.97 + 0.08 * rng.random((n + 6, 3)), 1.0)
    return fr.with_dynamics({"x": p[:, 0].copy(), "y": p[:, 1].copy(), "z": p[:, 2].copy()}, seed)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
@pytest.mark.parametrize("sub", [False, True])
def test_wave_boundaries_and_sub_ranges(ctx, n, sub):
    f = small(n, seed=n)
    first, last = (4, 4 + n) if sub else (0, n)
    ell = 0.012
    ref = fr.fof(f, *fr.PERIODIC, ell, first=first, last=last, min_members=2)
    got, stats = run(ctx, f, fr.PERIODIC, ell, first=first, last=last, min_members=2)
    assert_same(got, ref, fr.PERIODIC)
    assert len(got["label"]) == n and stats["num_all"] == ref["num_all"]
    if n >= 63:
        assert 1 < ref["num_all"] < n, "the case has links and more than one group"
    if n:
        assert got["label"].min() >= first and got["label"].max() < last, "index labels are indices of the columns"


def test_particles_outside_the_range_link_nothing(ctx):
    """two particles of the range, 1.6 l apart, and one outside it halfway between them"""
    ell = 0.05
    f = fr.with_dynamics({"x": np.array([0.5, 0.5 + 0.8 * ell, 0.5 + 1.6 * ell, 0.9]), "y": np.full(4, 0.5), "z": np.full(4, 0.5)})
    order = [1, 0, 2, 3]
    f = {k: v[order] for k, v in f.items()}  # the bridge first
    got, _ = run(ctx, f, fr.OPEN, ell, first=1, last=4, min_members=1)
    assert got["num_all"] == 3 and got["label"].tolist() == [1, 2, 3]
    got, _ = run(ctx, f, fr.OPEN, ell, min_members=1)
    assert got["num_all"] == 2 and got["label"].tolist() == [0, 0, 0, 3]


def test_strict_criterion_and_periodic_faces(ctx):
    ell = 0.05
    for factor, groups in ((0.999999, 1), (1.000001, 2)):
        for axis in range(3):
            p = [np.array([0.4, 0.4]), np.array([0.5, 0.5]), np.array([0.6, 0.6])]
            p[axis] = p[axis] + np.array([0.0, factor * ell])
            f = fr.with_dynamics({"x": p[0], "y": p[1], "z": p[2]})
            ref = fr.fof(f, *fr.OPEN, ell, min_members=1)
            got, _ = run(ctx, f, fr.OPEN, ell, min_members=1)
            assert ref["num_all"] == groups
            assert_same(got, ref, fr.OPEN)
    for axis in range(3):
        p = [np.array([0.4, 0.4]), np.array([0.5, 0.5]), np.array([0.6, 0.6])]
        p[axis] = np.array([0.3 * ell, 1.0 - 0.3 * ell])
        f = fr.with_dynamics({"x": p[0], "y": p[1], "z": p[2]})
        ref = fr.fof(f, *fr.PERIODIC, ell, min_members=2)
        got, _ = run(ctx, f, fr.PERIODIC, ell, min_members=2)
        assert ref["num_all"] == 1 and got["count"].tolist() == [2]
        assert_same(got, ref, fr.PERIODIC)
        assert 0.0 <= got["com"][0][axis] < 1.0
        got, _ = run(ctx, f, fr.OPEN, ell, min_members=2)
        assert got["num_all"] == 2 and got["num_groups"] == 0 and len(got["count"]) == 0


@pytest.mark.parametrize("min_members, max_groups", [(1, 20000), (20, 4096), (100000, 4096), (20, 7), (1, 50)])
def test_catalogue_filter_and_capacity(ctx, min_members, max_groups):
    f, ids, ell, _, _ = clustered_case("periodic")
    ref = fr.fof(f, *fr.PERIODIC, ell, ids=ids, min_members=min_members, max_groups=max_groups)
    got, _ = run(ctx, f, fr.PERIODIC, ell, ids=ids, min_members=min_members, max_groups=max_groups, labels=False)
    assert got["label"] is None
    assert_same(got, ref, fr.PERIODIC)
    assert len(got["count"]) == min(ref["num_groups"], max_groups)
    if min_members == 1:
        assert got["num_groups"] == got["num_all"]
    if min_members == 100000:
        assert got["num_groups"] == 0 and len(got["group_label"]) == 0
    if max_groups == 7:
        assert got["num_groups"] > 7, "the total is reported, the prefix written"
    c = got["count"].astype(np.int64)
    assert np.all((c[:-1] > c[1:]) | ((c[:-1] == c[1:]) & (got["group_label"][:-1] < got["group_label"][1:])))


def test_catalogue_refused_without_capacity(ctx):
    f = small(10, 1)
    with pytest.raises(sx.SxError, match="maxGroups is 0 with a catalogue array set"):
        run(ctx, f, fr.PERIODIC, 0.012, max_groups=0)
    with pytest.raises(sx.SxError, match="exceeds a third of the periodic x extent"):
        run(ctx, f, fr.PERIODIC, 0.4)


def bits(got):
    return [got[k].tobytes() for k in ("group_label", "count", "mass", "com", "vel")] + [got["num_groups"], got["num_all"]]


def test_same_bits_on_every_run_and_under_permutation(ctx):
    f, ids, ell, _, by_id = clustered_case("periodic")
    a, sa = run(ctx, f, fr.PERIODIC, ell, ids=ids)
    b, sb = run(ctx, f, fr.PERIODIC, ell, ids=ids)
    assert bits(a) == bits(b) and np.array_equal(a["label"], b["label"])
    assert sa["pair_tests"] == sb["pair_tests"]
    p = np.random.default_rng(5).permutation(N)
    c, _ = run(ctx, {k: v[p] for k, v in f.items()}, fr.PERIODIC, ell, ids=ids[p])
    assert bits(a) == bits(c), "with ids the catalogue has the same bits under any permutation of the input"
    assert np.array_equal(a["label"][p], c["label"]), "and every id keeps its label"


def test_render_profile_and_fof_on_one_context_keep_apart(ctx):
    """a map, a profile and a group search on one context each keep scratch and figures of their own"""
    f, ids, ell, by_index, _ = clustered_case("periodic")
    cols = dict(f, h=np.full(N, 0.02, np.float32))
    box = sx.make_box(*fr.PERIODIC)
    ds = sx.DeviceState(ctx, cols)
    try:
        mspec = sx.SxMap("column", 2, (0.5, 0.5, 0.5), (1.0, 1.0), 0.0, (32, 32))
        pspec = sx.SxProfile(edges=np.linspace(0.0, 0.5, 9), quantities=("vel",), center=(0.5, 0.5, 0.5))
        fspec = sx.SxFof(ell, 20, 4096)
        img = ctx.render_map(ds.fields, box, mspec)[0]
        mstats = ctx.map_stats()
        prof = ctx.profile(ds.fields, box, pspec)
        pstats = ctx.profile_stats()
        got = ctx.fof(ds.fields, box, fspec)
        fstats = ctx.fof_stats()
        assert ctx.map_stats() == mstats and ctx.profile_stats() == pstats
        assert np.array_equal(got["label"], by_index["label"]) and fstats["num_all"] == by_index["num_all"]
        img2 = ctx.render_map(ds.fields, box, mspec)[0]
        prof2 = ctx.profile(ds.fields, box, pspec)
        assert ctx.fof_stats() == fstats
        assert np.array_equal(img, img2) and all(np.array_equal(prof[k], prof2[k]) for k in prof)
        again = ctx.fof(ds.fields, box, fspec)
        assert bits(again) == bits(got) and ctx.map_stats() == mstats and ctx.profile_stats() == pstats
    finally:
        ctx.free_all()
