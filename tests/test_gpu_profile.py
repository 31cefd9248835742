"""Binned profiles on the GPU at seam level (sx_profile_compute through Context.profile) on uploaded synthetic columns,
against tests/profile_ref.py.  The sums are exact integers rounded once, so every array of the result -- counts, W, S1,
S2, D -- is compared bit for bit, and min and max by value: there is no tolerance anywhere in this file."""
import numpy as np
import pytest

import profile_ref as pr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

PERIODIC = ([-0.5, 0.5, -0.5, 0.5, -0.5, 0.5], [1, 1, 1])
OPEN = ([-0.5, 0.5, -0.5, 0.5, -0.5, 0.5], [0, 0, 0])
MIXED = ([-0.5, 0.5, 0.0, 2.0, -1.0, 0.5], [1, 0, 2])
FOUR = ("rho", "p", "vel", "u")
COLUMNS = ["x", "y", "z", "vx", "vy", "vz", "h", "m", "temp", "kx", "xm", "rho", "c", "divv", "curlv", "alpha"]


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def particles(n, seed=0, lim=PERIODIC[0]):
    rng = np.random.default_rng(seed)
    f = {k: (lim[2 * a] + (lim[2 * a + 1] - lim[2 * a]) * rng.random(n)) for a, k in enumerate("xyz")}
    for k in ("vx", "vy", "vz", "divv"):
        f[k] = rng.standard_normal(n).astype(np.float32)
    for k in ("h", "c", "curlv", "alpha", "kx", "rho"):
        f[k] = rng.uniform(0.05, 2.0, n).astype(np.float32)
    f["m"] = rng.uniform(0.5, 1.5, n).astype(np.float32) / np.float32(max(n, 1))
    f["xm"] = (f["m"] * rng.uniform(0.8, 1.25, n)).astype(np.float32)
    f["temp"] = rng.uniform(0.5, 2.0, n) * 1e-15
    return f


def run(ctx, f, box, first=0, last=None, std=False, lds=True, **kw):
    """(device result, oracle result, stats) for the particles [first, last) of the host columns f"""
    n = len(f["x"])
    last = n if last is None else last
    lim, bnd = box
    ds = sx.DeviceState(ctx, {k: np.asarray(f[k]) for k in COLUMNS}, std=True)
    try:
        ctx.set_profile_lds(lds)
        spec = sx.SxProfile(**kw)
        got = ctx.profile(ds.fields, sx.make_box(lim, bnd), spec, first, last, std=std)
        stats = ctx.profile_stats()
    finally:
        ctx.set_profile_lds(True)
        ctx.free_all()
    kw = dict(kw)
    edges, quantities = kw.pop("edges"), kw.pop("quantities")
    ref = pr.profile({k: np.asarray(v)[first:last] for k, v in f.items()}, lim, bnd, edges, quantities, std=std, **kw)
    return got, ref, stats


def assert_same(got, ref):
    assert np.array_equal(got["count"], ref["count"]), (got["count"], ref["count"])
    assert got["nonfinite"][0] == ref["nonfinite"][0]
    for k in ("W", "S1", "S2", "D"):
        a, b = got[k].view(np.uint64), ref[k].view(np.uint64)
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:4], got[k][a != b][:4], ref[k][a != b][:4])
    for k in ("min", "max"):
        assert np.array_equal(got[k], ref[k]), k


def sedov_like_table():
    r = np.linspace(0.0, 0.9, 40)
    return ("table", r, 1.0 + 3.0 * np.exp(-((r - 0.3) / 0.05) ** 2))


@pytest.mark.parametrize("n, sub", [(0, False), (1, False), (63, False), (65, False), (65, True), (4097, False), (4097, True)])
def test_sizes_and_sub_ranges(ctx, n, sub):
    f = particles(max(n, 8), seed=n)
    first, last = (5, n - 3) if sub else (0, n)
    got, ref, stats = run(ctx, f, PERIODIC, first, last, edges=np.linspace(0.0, 0.5, 8), quantities=FOUR,
                          solutions={"rho": sedov_like_table()})
    assert_same(got, ref)
    assert int(got["count"].sum()) == last - first and stats["particles"] == last - first
    assert stats["lds"] == (1 if last > first else 0) and stats["passes"] == (2 if last > first else 0)
    if n == 0:
        assert not got["W"].any() and np.all(got["min"] == np.inf) and np.all(got["max"] == -np.inf)


def test_all_particles_in_one_bin_and_one_particle_per_bin(ctx):
    f = particles(300, seed=1)
    got, ref, _ = run(ctx, f, OPEN, edges=[0.0, 0.25, 0.5, 1.0, 2.0], quantities=("vel",), coord="h",
                      center=(0.0, 0.0, 0.0))
    assert_same(got, ref)
    f["h"][:] = np.float32(0.3)
    got, ref, _ = run(ctx, f, OPEN, edges=[0.0, 0.25, 0.5, 1.0, 2.0], quantities=("vel",), coord="h")
    assert_same(got, ref)
    assert got["count"].tolist() == [0, 300, 0, 0, 0, 0]
    nb = 37
    edges = np.linspace(-0.5, 0.5, nb + 1)
    g = particles(nb, seed=2)
    g["x"] = 0.5 * (edges[1:] + edges[:-1])
    got, ref, _ = run(ctx, g, OPEN, edges=edges, quantities=("vel", "vrad"), coord="x")
    assert_same(got, ref)
    assert got["count"].tolist() == [1] * nb + [0, 0]
    assert np.array_equal(got["min"][:, :nb], got["max"][:, :nb])


@pytest.mark.parametrize("edges", [np.linspace(-0.3, 0.4, 15), -0.3 + 0.7 * np.linspace(0.0, 1.0, 12) ** 2],
                         ids=["uniform", "uneven"])
def test_coordinates_exactly_on_edges(ctx, edges):
    """edges[b] <= c < edges[b + 1]: a particle on an edge belongs to the bin above it, one on edges[nbins] overflows"""
    nb = len(edges) - 1
    x = np.concatenate([edges, np.nextafter(edges, -1.0), np.nextafter(edges, 1.0)])
    f = particles(x.size, seed=3)
    f["x"] = x
    got, ref, _ = run(ctx, f, OPEN, edges=edges, quantities=("c",), coord="x")
    assert_same(got, ref)
    assert got["count"][nb] == 1 and got["count"][nb + 1] == 2  # below edges[0]; on and above edges[nbins]
    assert got["count"][:nb].tolist() == [3] * nb


def test_minimum_image_near_a_face(ctx):
    f = particles(2000, seed=4)
    kw = dict(edges=np.linspace(0.0, 0.6, 13), quantities=("vrad", "vel", "h"), center=(0.45, -0.48, 0.1))
    per, ref, _ = run(ctx, f, PERIODIC, **kw)
    assert_same(per, ref)
    opn, ref, _ = run(ctx, f, OPEN, **kw)
    assert_same(opn, ref)
    assert not np.array_equal(per["count"], opn["count"])  # the images moved particles between the shells
    for coord in ("x", "y", "z"):
        got, ref, _ = run(ctx, particles(500, seed=5, lim=MIXED[0]), MIXED, edges=np.linspace(-1.0, 1.0, 9),
                          quantities=("vrad",), coord=coord, center=(0.4, 1.9, 0.4))
        assert_same(got, ref)


@pytest.mark.parametrize("nq", [1, 4])
@pytest.mark.parametrize("where", ["one", "lds", "lds+1", "most"])
def test_lds_and_global_paths_agree(ctx, nq, where):
    """nbins on either side of the capacity of one LDS tile (above it pass 2 runs once per tile), and the global path
    forced at the same nbins: the same bits"""
    cap = sx.profile_lds_bins(nq)
    nbins = {"one": 1, "lds": cap, "lds+1": cap + 1, "most": 4096}[where]
    f = particles(3000, seed=6)
    kw = dict(edges=np.linspace(0.0, 0.9, nbins + 1), quantities=FOUR[:nq], solutions={"rho": sedov_like_table()})
    got, ref, stats = run(ctx, f, PERIODIC, **kw)
    tiles = -(-(nbins + 2) // (cap + 2))
    assert stats["lds"] == 1 and stats["passes"] == 1 + tiles and (tiles > 1) == (nbins > cap)
    assert_same(got, ref)
    other, _, stats = run(ctx, f, PERIODIC, lds=False, **kw)
    assert stats["lds"] == 0 and stats["passes"] == 2
    for k in got:
        assert got[k].tobytes() == other[k].tobytes(), k


def test_carries_and_a_wide_range(ctx):
    n = 5000
    f = particles(n, seed=7)
    M = 3.7e11
    f["temp"] = np.where(np.arange(n) % 2 == 0, M, -M)
    f["temp"][-1] = M  # the pairs cancel exactly, one is left
    got, ref, _ = run(ctx, f, OPEN, edges=[0.0, 1.0], quantities=("temp",), center=(0.0, 0.0, 0.0))
    assert_same(got, ref)
    assert got["S1"][0].sum() == 2 * M  # 2501 of +M, 2499 of -M; every partial sum is a small multiple of M
    f["temp"] = np.full(n, M)
    got, ref, _ = run(ctx, f, OPEN, edges=[0.0, 1.0], quantities=("temp",))
    assert_same(got, ref)
    assert got["S1"][0].sum() == n * M
    rng = np.random.default_rng(8)
    f["temp"] = 10.0 ** rng.uniform(-30, 30, n) * rng.choice([-1.0, 1.0], n)
    got, ref, _ = run(ctx, f, OPEN, edges=np.linspace(0.0, 0.9, 4), quantities=("temp", "u"), weight="mass")
    assert_same(got, ref)


def test_one_nan_goes_to_nonfinite(ctx):
    f = particles(200, seed=9)
    f["temp"][17] = np.nan
    f["temp"][18] = np.inf
    got, ref, stats = run(ctx, f, PERIODIC, edges=np.linspace(0.0, 0.5, 6), quantities=("vel", "u"))
    assert_same(got, ref)
    assert got["nonfinite"][0] == 2 == stats["nonfinite"] and got["count"].sum() == 198
    assert np.isfinite(got["S1"]).all() and np.isfinite(got["max"][1][got["count"] > 0]).all()
    # a quantity that does not read temp sees all of them
    got, ref, _ = run(ctx, f, PERIODIC, edges=np.linspace(0.0, 0.5, 6), quantities=("vel",))
    assert_same(got, ref)
    assert got["nonfinite"][0] == 0


@pytest.mark.parametrize("std", [False, True])
def test_density_pdf_with_log_spaced_edges(ctx, std):
    f = particles(3000, seed=10)
    got, ref, _ = run(ctx, f, PERIODIC, std=std, edges=np.logspace(-1.0, 0.0, 24), quantities=("rho", "p"), coord="rho",
                      weight="mass")
    assert_same(got, ref)
    assert got["count"][:23].sum() > 1000 and got["count"][23] > 0 and got["count"][24] > 0


def test_mass_weight_with_unequal_masses(ctx):
    f = particles(1000, seed=11)
    f["m"] = (f["m"] * np.random.default_rng(1).uniform(0.01, 100.0, 1000)).astype(np.float32)
    got, ref, _ = run(ctx, f, PERIODIC, edges=np.linspace(0.0, 0.5, 6), quantities=("vel", "alpha", "divv", "curlv"),
                      weight="mass", solutions={"vel": sedov_like_table()})
    assert_same(got, ref)


def test_tables(ctx):
    """two knots; knots on particle radii (the value there is y[j] itself); clamping on both sides; rscale"""
    f = particles(600, seed=12)
    r = np.sort(pr.evaluate(f, *OPEN, ())[0])
    kw = dict(edges=np.linspace(0.0, 0.9, 10), quantities=("rho", "vel"))
    for table in (("table", [0.2, 0.6], [1.0, 2.0]), ("table", r[50:550:5], np.cos(7.0 * r[50:550:5])),
                  ("table", [0.1, 0.3, 0.3, 0.5], [1.0, 2.0, 4.0, 3.0]), sedov_like_table() + (0.37,),
                  ("table", r[100:200], r[100:200] ** 2, 1.0 / 3.0)):
        got, ref, _ = run(ctx, f, OPEN, solutions={"rho": table, "vel": ("table", [0.0, 2.0], [0.0, 2.0])}, **kw)
        assert_same(got, ref)
        assert got["D"].any()


@pytest.mark.parametrize("xgeom", [1, 2, 3])
def test_noh_closed_form(ctx, xgeom):
    f = particles(800, seed=13)
    f["x"][0] = f["y"][0] = f["z"][0] = 0.0  # r = 0: behind the front
    time = 0.9
    r = pr.evaluate(f, *OPEN, ())[0]
    r2 = 0.5 * (5.0 / 3.0 - 1) * time
    assert (r > r2).sum() > 100 and (r <= r2).sum() > 10 and r[0] == 0.0
    got, ref, _ = run(ctx, f, OPEN, edges=np.linspace(0.0, 0.9, 10), quantities=("rho",),
                      solutions={"rho": ("noh", dict(time=time, rho0=1.9, xgeom=xgeom))})
    assert_same(got, ref)


def test_repeats_and_another_context_give_the_same_bits(ctx):
    f = particles(4097, seed=14)
    kw = dict(edges=np.linspace(0.0, 0.5, 51), quantities=FOUR, solutions={"rho": sedov_like_table()})
    first, ref, _ = run(ctx, f, PERIODIC, **kw)
    assert_same(first, ref)
    again, _, _ = run(ctx, f, PERIODIC, **kw)
    other = sx.Context(0)
    try:
        third, _, _ = run(other, f, PERIODIC, **kw)
    finally:
        other.close()
    for k in first:
        assert first[k].tobytes() == again[k].tobytes() == third[k].tobytes(), k


def test_refusals(ctx):
    f = particles(16, seed=15)
    ds = sx.DeviceState(ctx, {k: f[k] for k in COLUMNS})  # no rho column
    try:
        box = sx.make_box(*PERIODIC)
        with pytest.raises(sx.SxError, match="rho needs the rho column"):
            ctx.profile(ds.fields, box, sx.SxProfile([0.0, 1.0], ("rho",)), std=True)
        with pytest.raises(sx.SxError, match="strictly ascending"):
            ctx.profile(ds.fields, box, sx.SxProfile([0.0, 0.0], ("vel",)))
        with pytest.raises(sx.SxError, match="not a range"):
            ctx.profile(ds.fields, box, sx.SxProfile([0.0, 1.0], ("vel",)), first=3, last=17)
        ds.fields.temp = None
        with pytest.raises(sx.SxError, match="p needs temp"):
            ctx.profile(ds.fields, box, sx.SxProfile([0.0, 1.0], ("vel", "p")))
    finally:
        ctx.free_all()
