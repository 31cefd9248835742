"""Two-point statistics on the GPU at seam level (sx_twopoint_compute through Context.twopoint) on uploaded synthetic
columns, against tests/twopoint_ref.py.  Only integers are added on the device and the oracle repeats every rounded
operation, so every array is compared with array_equal: there is no tolerance in this file."""
import functools

import numpy as np
import pytest

import twopoint_ref as tr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

E3 = [0.0, 0.1, 0.2, 0.3]


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def run(ctx, f, box, edges, series=tr.ALL, stride=1, phase=0, ids=None, first=0, last=None):
    """(device result, stats) for the particles [first, last) of the host columns f"""
    lim, bnd = box
    ds = sx.DeviceState(ctx, {k: np.asarray(v) for k, v in f.items()})
    try:
        dev_id = ctx.upload(np.ascontiguousarray(ids, dtype=np.uint64)) if ids is not None else None
        got = ctx.twopoint(ds.fields, sx.make_box(lim, bnd), sx.SxTwoPoint(edges, series, stride, phase), id=dev_id,
                           first=first, last=last)
        return got, ctx.twopoint_stats()
    finally:
        ctx.free_all()


def check(ctx, f, box, edges, series=tr.ALL, **kw):
    """the device result of a case against the oracle; returns (device result, oracle result, stats)"""
    ref = tr.twopoint(f, *box, edges, series=series, **kw)
    got, stats = run(ctx, f, box, edges, series=series, **kw)
    tr.assert_same(got, ref, series)
    assert stats["pairs_binned"] == ref["pairs"] and stats["pairs_tested"] >= ref["pairs"] + ref["coincident"]
    assert (stats["targets"], stats["nonfinite"], stats["coincident"]) == (ref["targets"], ref["nonfinite"], ref["coincident"])
    return got, ref, stats


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_small_counts(ctx, n):
    f = tr.uniform(n, seed=n)
    got, ref, _ = check(ctx, f, tr.PERIODIC, E3)
    assert ref["targets"] == n and got["pairs_expected"] == n * (n - 1) // 2
    if n >= 63:
        assert ref["pairs"] > 100


@pytest.mark.parametrize("first, last", [(1, 200), (60, 70), (64, 128), (5, 5), (193, 257)])
def test_sub_ranges_cut_a_wave(ctx, first, last):
    f = tr.uniform(257, seed=257)
    ids = np.random.default_rng(1).permutation(257).astype(np.uint64)
    check(ctx, f, tr.PERIODIC, E3, first=first, last=last)
    # by index the key is the column index, first included: phase 1 of stride 2 is the odd columns
    _, ref, _ = check(ctx, f, tr.PERIODIC, E3, first=first, last=last, stride=2, phase=1)
    assert ref["targets"] == len([k for k in range(first, last) if k % 2 == 1])
    check(ctx, f, tr.PERIODIC, E3, first=first, last=last, stride=2, phase=1, ids=ids)


BOXES = {"periodic": (tr.PERIODIC, 0), "open": (tr.OPEN, 16), "mixed": (tr.MIXED, 16)}
CLUMP_EDGES = np.concatenate([[0.0], np.geomspace(0.002, 0.025, 12)])


@functools.lru_cache(maxsize=None)
def clumpy_case(name):
    """the clumpy columns in the box `name`, ids (a random permutation), and the oracle's results by index and by id;
    computed once and left unchanged"""
    box, outside = BOXES[name]
    f = tr.clumpy(3000, box=box, seed=5, outside=outside, mdecades=1.0)
    ids = np.random.default_rng(99).permutation(3000).astype(np.uint64)
    return f, ids, tr.twopoint(f, *box, CLUMP_EDGES), tr.twopoint(f, *box, CLUMP_EDGES, ids=ids, stride=3, phase=1)


@pytest.mark.parametrize("name", ["periodic", "open", "mixed"])
def test_clumpy_by_index_and_by_id(ctx, name):
    box = BOXES[name][0]
    f, ids, by_index, by_id = clumpy_case(name)
    assert 5e4 < by_index["pairs"] < 2e5, by_index["pairs"]
    assert by_index["count"].min() > 0 and by_index["count"].max() > 50 * by_index["count"].min(), "a clump in a background"
    got, _ = run(ctx, f, box, CLUMP_EDGES)
    tr.assert_same(got, by_index)
    got, _ = run(ctx, f, box, CLUMP_EDGES, ids=ids)
    tr.assert_same(got, by_index)  # stride 1: the ids do not matter
    got, _ = run(ctx, f, box, CLUMP_EDGES, ids=ids, stride=3, phase=1)
    tr.assert_same(got, by_id)
    assert by_id["targets"] == 1000 and 0 < by_id["pairs"] < by_index["pairs"]


def test_permutation_with_ids_gives_equal_bits(ctx):
    f, ids, _, by_id = clumpy_case("periodic")
    perm = np.random.default_rng(4).permutation(3000)
    g = {k: v[perm] for k, v in f.items()}
    got, _ = run(ctx, g, tr.PERIODIC, CLUMP_EDGES, ids=ids[perm], stride=3, phase=1)
    tr.assert_same(got, by_id)


def test_stride_three_each_phase_and_the_identity(ctx):
    f = tr.uniform(600, seed=31, vscale=3.0)
    ids = np.random.default_rng(32).permutation(600).astype(np.uint64)
    c1 = check(ctx, f, tr.PERIODIC, E3, ids=ids)[0]["count"].astype(np.int64)
    total, same = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for phase in range(3):
        got, _, _ = check(ctx, f, tr.PERIODIC, E3, ids=ids, stride=3, phase=phase)
        total += got["count"].astype(np.int64)
        sel = ids % 3 == phase
        same += run(ctx, {k: v[sel] for k, v in f.items()}, tr.PERIODIC, E3, series=0)[0]["count"].astype(np.int64)
    # tests/test_twopoint_ref.py::test_stride_identity, on the device's counts
    assert np.array_equal(total - c1, c1 - same)


def test_all_particles_in_one_cell(ctx):
    f = tr.uniform(500, box=tr.OPEN, seed=41)
    edges = np.linspace(0.0, 5.0, 26)
    assert sx.twopoint_grid(sx.SxTwoPoint(edges), sx.make_box(*tr.OPEN), 500) == (1, 1, 1)
    _, ref, stats = check(ctx, f, tr.OPEN, edges)
    assert ref["pairs"] == stats["pairs_tested"] == 124750, "every unordered pair once"


def test_rmax_at_a_third_of_the_box(ctx):
    f = tr.uniform(300, seed=43)
    edges = np.linspace(0.0, 1.0 / 3.0, 8)
    assert sx.twopoint_grid(sx.SxTwoPoint(edges), sx.make_box(*tr.PERIODIC), 300) == (3, 3, 3)
    _, ref, _ = check(ctx, f, tr.PERIODIC, edges)
    assert ref["pairs"] > 5000
    # three cells per axis and particles on the faces and outside the box: wrapped into the grid, one image taken
    f["x"][:6] = [0.0, 1.0, -0.01, 1.01, 1.0 / 3.0, 2.0 / 3.0]
    check(ctx, f, tr.PERIODIC, edges)


def test_pair_on_an_edge_and_coincident_pairs(ctx):
    pos = np.array([[0.0625, 0.5, 0.5], [0.3125, 0.5, 0.5], [0.9375, 0.5, 0.5], [0.0625, 0.5, 0.5]])
    f = tr.columns(pos, vscale=2.0)
    got, ref, _ = check(ctx, f, tr.PERIODIC, [0.0, 0.25, 0.3])
    assert got["count"].tolist() == [2, 2] and got["coincident"] == 1
    got, _, _ = check(ctx, f, tr.OPEN, [0.0, 0.25, 0.3])
    assert got["count"].tolist() == [0, 2]
    # many coincident pairs: 40 points, each stored three times; only pairs with a target member are counted
    f = tr.uniform(40, seed=47)
    f = {k: np.concatenate([v, v, v]) for k, v in f.items()}
    got, ref, _ = check(ctx, f, tr.PERIODIC, E3)
    assert got["coincident"] == 3 * 40
    got, ref, _ = check(ctx, f, tr.PERIODIC, E3, stride=3, phase=0)
    assert 0 < got["coincident"] < 120


def test_nan_coordinate_inf_velocity_nan_mass(ctx):
    f = tr.uniform(200, seed=53)
    f["x"][5], f["z"][190] = np.nan, np.inf
    f["vy"][9] = np.inf
    f["m"][11] = np.nan
    got, ref, _ = check(ctx, f, tr.PERIODIC, E3, series=tr.ALL)
    assert got["nonfinite"] == 4 and got["targets"] == 196 and got["pairs_expected"] == 196 * 195 // 2
    got, ref, _ = check(ctx, f, tr.PERIODIC, E3, series=tr.VEL)
    assert got["nonfinite"] == 3, "the mass is not read without the mass series"
    assert np.all(np.isfinite(got["U1"])) and np.all(np.isfinite(got["T2"]))
    # the largest velocity among the finite particles sets the windows: not the huge one of a particle that is out
    f["vx"][5] = 3e38
    check(ctx, f, tr.PERIODIC, E3)


@pytest.mark.parametrize("nbins", [1, 256])
def test_one_bin_and_256_bins(ctx, nbins):
    f = tr.uniform(500, seed=59)
    _, ref, _ = check(ctx, f, tr.PERIODIC, np.linspace(0.0, 0.3, nbins + 1))
    assert ref["pairs"] > 10000


def test_log_edges_above_zero(ctx):
    f = tr.uniform(800, seed=61)
    edges = np.geomspace(0.01, 0.3, 17)
    got, ref, _ = check(ctx, f, tr.PERIODIC, edges)
    closer = tr.twopoint(f, *tr.PERIODIC, [0.0, 0.01], series=0)["count"][0]
    assert closer > 0, "pairs below the first edge exist and enter nothing"
    assert np.all(np.isfinite(got["xi"])) and got["xi"].shape == (16,)


def test_carries_and_borrows(ctx):
    """velocity components of +-vmax: u reaches +-0.87 2^Eu, so the low words of U1 and U3 wrap upwards and downwards
    on most adds"""
    f = tr.uniform(700, seed=67)
    rng = np.random.default_rng(68)
    for k in ("vx", "vy", "vz"):
        f[k] = (1.999 * rng.choice([-1.0, 1.0], 700)).astype(np.float32)
    got, ref, _ = check(ctx, f, tr.PERIODIC, E3)
    assert ref["windows"]["U1"] == 3
    for k in ("U1", "U3"):
        ints = ref["integers"][k]
        assert any(v < 0 for v in ints) or any(abs(v) >> 64 for v in ints)
    assert np.all(np.asarray([abs(v) >> 64 for v in ref["integers"]["A3"]]) > 0), "the high word is in use"
    # tiny and zero velocities: subnormal windows, every power underflows
    for scale in (0.0, 1e-45):
        for k in ("vx", "vy", "vz"):
            f[k] = (scale * rng.choice([-1.0, 1.0], 700)).astype(np.float32)
        check(ctx, f, tr.PERIODIC, E3)


def test_masses_over_six_decades(ctx):
    f = tr.uniform(600, seed=71, mdecades=6.0)
    assert f["m"].max() / f["m"].min() > 1e5
    got, ref, _ = check(ctx, f, tr.PERIODIC, E3, series=tr.FLAGS["WW"])
    assert np.all(got["ww"] > 0) and got["U1"] is None
    check(ctx, f, tr.PERIODIC, E3, series=tr.FLAGS["WW"] | tr.FLAGS["U2"])


def test_counts_only_leaves_the_other_arrays_untouched(ctx):
    f = tr.uniform(500, seed=73)
    got, ref, _ = check(ctx, f, tr.PERIODIC, E3, series=0)
    for k in tr.SERIES:
        assert got[k] is None and np.all(np.isnan(got["raw"][k])), "the arrays keep what the caller put there"
    assert got["s1"] is None and got["ww"] is None
    got, _, _ = check(ctx, f, tr.PERIODIC, E3, series=tr.FLAGS["U3"])
    assert np.all(np.isnan(got["raw"]["U1"])) and not np.any(np.isnan(got["raw"]["U3"]))
    assert np.array_equal(got["s3"], got["U3"] / got["count"])


def test_repeats_and_a_second_context(ctx):
    f, ids, by_index, _ = clumpy_case("mixed")
    a, _ = run(ctx, f, tr.MIXED, CLUMP_EDGES)
    b, _ = run(ctx, f, tr.MIXED, CLUMP_EDGES)
    other = sx.Context(0)
    try:
        c, _ = run(other, f, tr.MIXED, CLUMP_EDGES)
    finally:
        other.close()
    for got in (a, b, c):
        tr.assert_same(got, by_index)


def test_fof_profile_twopoint_share_a_context(ctx):
    """a FoF call, a profile call and a two-point call on one context in turn, each equal to its own call on a fresh
    context"""
    f, ids, by_index, _ = clumpy_case("periodic")
    f = dict(f, h=np.full(3000, 0.02, np.float32))
    box = sx.make_box(*tr.PERIODIC)
    prof = sx.SxProfile(np.linspace(0.0, 0.8, 9), ("vel",), center=(0.3, 0.3, 0.3))

    def calls(c, which):
        ds = sx.DeviceState(c, f)
        try:
            out = {}
            if "fof" in which:
                out["fof"] = c.fof(ds.fields, box, sx.SxFof(0.01, 5, 256))
            if "profile" in which:
                out["profile"] = c.profile(ds.fields, box, prof)
            if "twopoint" in which:
                out["twopoint"] = c.twopoint(ds.fields, box, sx.SxTwoPoint(CLUMP_EDGES, tr.ALL))
            return out
        finally:
            c.free_all()

    together = calls(ctx, ("fof", "profile", "twopoint"))
    tr.assert_same(together["twopoint"], by_index)
    for which in ("fof", "profile", "twopoint"):
        fresh = sx.Context(0)
        try:
            alone = calls(fresh, (which,))[which]
        finally:
            fresh.close()
        for k, v in alone.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, together[which][k], equal_nan=True), (which, k)


def same_bits(a, b):
    """two results of a Context call (dicts and sequences of arrays, scalars and None) equal bit for bit"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_timed_calls_give_the_same_bits(ctx):
    """each of fof, twopoint and profile untimed, timed and untimed again on one context: the same results and stats,
    figures after the timed call, and zeros in every _ms after an untimed one (the times are "of the last call")"""
    f = dict(tr.uniform(257, seed=257), h=np.full(257, 0.05, np.float32))
    box = sx.make_box(*tr.PERIODIC)
    edges = np.linspace(0.0, 0.3, 9)
    prof = sx.SxProfile(np.linspace(0.0, 0.8, 9), ("vel",), center=(0.5, 0.5, 0.5))
    passes = {
        "fof": (lambda d: ctx.fof(d.fields, box, sx.SxFof(0.1, 2, 256)), ctx.fof_stats, ctx.set_fof_timing,
                ctx.fof_times, 4),
        "twopoint": (lambda d: ctx.twopoint(d.fields, box, sx.SxTwoPoint(edges, tr.ALL)), ctx.twopoint_stats,
                     ctx.set_twopoint_timing, ctx.twopoint_times, 4),
        "profile": (lambda d: ctx.profile(d.fields, box, prof), ctx.profile_stats, ctx.set_profile_timing,
                    ctx.profile_times, 3),
    }
    ds = sx.DeviceState(ctx, f)
    try:
        for name, (call, stats, set_timing, times, stages) in passes.items():
            got, figures = [], []
            for timed in (False, True, False):
                set_timing(timed)
                try:
                    got.append((call(ds), stats()))
                finally:
                    set_timing(False)
                figures.append(times())
            assert same_bits(got[0], got[1]) and same_bits(got[0], got[2]), name
            for fig in figures:
                ms = [v for k, v in fig.items() if k.endswith("_ms")]
                assert len(ms) == stages and len(fig) == (4 if name != "profile" else stages + 1), (name, fig)
                assert all(np.isfinite(v) and v >= 0.0 for v in fig.values()), (name, fig)
            # kernels ran between the first and the last boundary of the timed call
            assert sum(v for k, v in figures[1].items() if k.endswith("_ms")) > 0.0, (name, figures[1])
            assert all(v == 0.0 for k, v in figures[2].items() if k.endswith("_ms")), (name, figures[2])
            if name == "profile":
                assert figures[0]["pass_bytes"] == figures[1]["pass_bytes"] == figures[2]["pass_bytes"] > 0
    finally:
        ctx.free_all()
