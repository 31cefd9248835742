"""Column-density and slice maps on the GPU (sx_map_render) at seam level, uploaded arrays against tests/map_ref.py.

Bounds, per pixel and scale-aware (the scales are sums of magnitudes of the terms, as StepChecker's):

    |S0 - S0_ref| <= r S0_ref,    |S1 - S1_ref| <= r sum_j |w_j a_j|,    r = FIT + (n + c) 2^-24

with n the pixel's contributions and FIT the relative kernel-fit error pinned by tests/test_map_capi_cpu.py (4 x 8.8e-7;
the slice's kernelW is pinned at 3.1e-7 by tests/test_capi_cpu.py, below it).  None of it comes from what the kernel gives.

Derivation of c, to first order, with u = 2^-24 the largest relative error of one float rounding:
* accumulation: n fused multiply-adds in list order, n u S0 (the n of the formula);
* values: the weight w is rounded once, and so is the product w a: 2 u S0;
* the kernel's argument t = (dx^2 du^2 + dy^2 dv^2) / he^2: the three stored factors, the two squares, two products and
  one FMA make 8 roundings, at most 6 u of t after the weights of the two squared terms, i.e. 3 u of q = sqrt(t) < 2:
  6 u D with D = sum_j |dw_j / dq_j| the pixel's sensitivity to the distances (the oracle's dq0, dq1);
* geometry: a record's position is a float in pixels relative to its tile's origin, of magnitude up to 16 + ru (its
  reach ru = 2 he in pixels: it touches the tile), and the difference to the pixel centre is rounded again (up to ru):
  u (16 + 2 ru) pixels per axis, sqrt(2) times that for the distance, sqrt(2) u (32 / ru + 4) in units of he = ru / 2.
So  c = 2 + (6 + sqrt(2) (32 / ru_min + 4)) D / S0  per pixel, ru_min = 2 min(he) / max(du, dv) per case (he >= half a
pixel: ru_min >= 1).  Over a whole disc D / S0 = int |Y'| 2 pi q dq / int Y 2 pi q dq = 2.95 (slices: 3.76), which makes c
about 70 at ru = 4; a pixel that holds only the outer edges of supports has D / S0 = 13 / (2 - q) and a c to match: the
check stays relative to the pixel's own sum, and says what float geometry can deliver there.

Measured on an MI355X, worst use of a bound over the pixels of a case (S0 / S1): periodic 0.041 / 0.030, zoom 0.114 /
0.113, chunks 0.272 / 0.272, clamp 0.402 / 0.394, slices 0.085 / 0.103, periodic images narrower than a tile (32 x 4 ...
1 x 1) 0.212 / 0.213.  The worst is above a quarter, so the bound stands as derived (it would have been cut to four times the measured use otherwise).
"""
import numpy as np
import pytest

import map_ref as mr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FIT = 4 * 8.8e-7
UNIT = [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]
K = mr.kernel_constant()


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def geometry_factor(h, spec, clamp=True):
    """6 + sqrt(2) (32 / ru_min + 4) of the derivation above"""
    ny, nx = spec.shape
    pix = max(spec.width[0] / nx, spec.width[1] / ny)
    he = max(float(np.min(h)), 0.5 * pix) if clamp else float(np.min(h))
    return 6.0 + np.sqrt(2.0) * (32.0 / (2.0 * he / pix) + 4.0)


class Case:
    """particles, box and an SxMap; the oracle's images are computed once and shared"""

    def __init__(self, pos, h, m, lim, bnd, spec, a=None):
        self.pos, self.h, self.m, self.lim, self.bnd, self.spec, self.a = pos, h, m, lim, bnd, spec, a
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            s = self.spec
            self._ref = mr.render(self.pos, self.h, self.m, self.lim, self.bnd, s.kind, s.axis, list(s.center),
                                  list(s.width), list(s.npix), depth=s.depth, K=K, a=self.a, scales=True)
        return self._ref

    def gpu(self, ctx, a_dtype=np.float32, first=0, last=None, with_a=True, cap=0):
        host = {"x": self.pos[:, 0], "y": self.pos[:, 1], "z": self.pos[:, 2], "h": self.h, "m": self.m}
        ds = sx.DeviceState(ctx, host)
        try:
            da = ctx.upload(np.asarray(self.a, a_dtype)) if (with_a and self.a is not None) else None
            ctx.set_map_pair_cap(cap)
            box = sx.make_box(self.lim, self.bnd)
            s0, s1 = ctx.render_map(ds.fields, box, self.spec, a=da, first=first, last=last, K=K)
            return s0, s1, ctx.map_stats()
        finally:
            ctx.set_map_pair_cap(0)
            ctx.free_all()

    def footprints(self):
        """particles whose bounding square of the reach (2 he; slice: sqrt(4 h^2 - dn^2)) holds a pixel centre: what the
        binning counts.  The square may hold a centre that the disc misses, so this is at least the particles that
        contribute."""
        s = self.spec
        au, av, an = (s.axis + 1) % 3, (s.axis + 2) % 3, s.axis
        L = [self.lim[2 * k + 1] - self.lim[2 * k] if self.bnd[k] == 1 else 0.0 for k in range(3)]
        ny, nx = s.shape
        du, dv = s.width[0] / nx, s.width[1] / ny
        h = self.h.astype(np.float64)
        dn = mr._min_image(self.pos[:, an] - s.center[an], L[an])
        if s.kind == mr.COLUMN:
            reach = 2.0 * np.maximum(h, 0.5 * max(du, dv))
            keep = (np.abs(dn) <= 0.5 * s.depth) if s.depth > 0 else np.ones(h.size, bool)
        else:
            keep = 4.0 * h * h - dn * dn > 0
            reach = np.sqrt(np.maximum(4.0 * h * h - dn * dn, 0.0))
        pu = s.center[au] - 0.5 * s.width[0] + (np.arange(nx) + 0.5) * du
        pv = s.center[av] - 0.5 * s.width[1] + (np.arange(ny) + 0.5) * dv
        inu = (np.abs(mr._min_image(self.pos[:, au][:, None] - pu[None, :], L[au])) <= reach[:, None]).any(axis=1)
        inv = (np.abs(mr._min_image(self.pos[:, av][:, None] - pv[None, :], L[av])) <= reach[:, None]).any(axis=1)
        return int((keep & inu & inv).sum())

    def check(self, s0, s1, name):
        r = self.ref
        g = geometry_factor(self.h, self.spec, clamp=self.spec.kind == mr.COLUMN)
        empty = r["count"] == 0
        # where the oracle has no contribution the image is exactly zero
        assert not s0[empty].any(), name
        line = f"{name}: max n = {r['count'].max()}"
        for tag, got, want, scale, dq in (("S0", s0, r["sum0"], r["sum0"], r["dq0"]), ("S1", s1, r["sum1"], r["abs1"], r["dq1"])):
            if got is None:
                continue
            assert not got[empty].any(), name
            ok = scale > 0
            c = 2.0 + g * dq[ok] / scale[ok]
            bound = (FIT + (r["count"][ok] + c) * U) * scale[ok]
            use = np.abs(got - want)[ok] / bound
            line += f", {tag}: median c = {np.median(c):.0f}, worst use of the bound {use.max():.3f}"
            assert not (np.abs(got - want)[~ok]).any(), (name, tag)
            if use.max() > 1.0:
                print(line)
            assert use.max() <= 1.0, (name, tag, use.max(), c[use.argmax()], r["count"][ok][use.argmax()])
        print(line)


def periodic_case(axis, kind=mr.COLUMN, center=(0.5, 0.5, 0.5), seed=7):
    rng = np.random.default_rng(seed)
    n = 2000
    pos = rng.random((n, 3))
    h = rng.uniform(0.06, 0.078, n).astype(np.float32)
    m = (rng.uniform(0.5, 1.5, n) / n).astype(np.float32)
    a = rng.normal(size=n).astype(np.float32)  # signed
    spec = sx.SxMap(kind, axis, center, (1.0, 1.0), 0.0, (32, 32))
    return Case(pos, h, m, UNIT, [1, 1, 1], spec, a)


_cases = {}


def case(name):
    if name not in _cases:
        if name.startswith("periodic"):
            _cases[name] = periodic_case(int(name[-1]))
        elif name == "zoom":
            rng = np.random.default_rng(11)
            n = 1500
            pos = rng.random((n, 3))
            h = rng.uniform(0.03, 0.04, n).astype(np.float32)
            m = (rng.uniform(0.5, 1.5, n) / n).astype(np.float32)
            a = rng.normal(size=n).astype(np.float32)
            # axis 1: u = z, v = x.  The window leaves the cloud along u ([0.6, 1.1]), pixels 0.0125 x 0.015, 40 x 24:
            # 3 x 2 tiles with partial ones in both directions; the slab y in [0.25, 0.75] keeps about half the particles
            spec = sx.SxMap("column", 1, (0.41, 0.5, 0.85), (0.5, 0.36), 0.5, (40, 24))
            _cases[name] = Case(pos, h, m, UNIT, [0, 0, 0], spec, a)
        elif name == "clamp":
            c = periodic_case(2, seed=13)
            c.h = np.full(c.h.size, 0.2 / 32, np.float32)
            _cases[name] = c
        elif name == "slice":
            c = periodic_case(2, kind=mr.SLICE, center=(0.5, 0.5, 0.01), seed=17)
            c.pos[0] = (0.31, 0.64, 0.98)  # reaches the plane z = 0.01 through the periodic face
            c.h[0] = 0.07
            _cases[name] = c
    return _cases[name]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_periodic_column_map(ctx, axis):
    """2 x 2 tiles, footprints that wrap in u and in v, a signed float column"""
    c = case(f"periodic{axis}")
    s0, s1, st = c.gpu(ctx)
    c.check(s0, s1, f"periodic axis {axis}")
    assert st["footprints"] == 2000 and st["bands"] == 1
    # wrapped footprints exist: some particle within its reach of the box edge contributes on the far side
    assert abs(s0.sum() / 32 ** 2 - float(c.m.astype(np.float64).sum())) < 1e-5 * float(c.m.sum())


@pytest.mark.parametrize("npix", [(32, 4), (4, 32), (40, 1), (1, 1), (4, 4), (32, 7)])
def test_periodic_image_narrower_than_a_tile(ctx, npix):
    """a periodic axis that spans fewer pixels than half a tile: a pixel is further from its tile's centre than half the
    period, so its distance to a record folds by more than one image; 40 x 1 is a 1-D profile, 1 x 1 the whole box"""
    rng = np.random.default_rng(23)
    n = 300
    pos = rng.random((n, 3))
    h = rng.uniform(0.06, 0.078, n).astype(np.float32)
    m = (rng.uniform(0.5, 1.5, n) / n).astype(np.float32)
    a = rng.normal(size=n).astype(np.float32)
    for kind in ("column", "slice"):
        c = Case(pos, h, m, UNIT, [1, 1, 1], sx.SxMap(kind, 2, (0.5, 0.5, 0.3), (1.0, 1.0), 0.0, npix), a)
        s0, s1, st = c.gpu(ctx)
        assert s0.shape == (npix[1], npix[0]) and st["footprints"] == c.footprints()
        c.check(s0, s1, f"{kind} {npix[0]} x {npix[1]}")


def test_double_column(ctx):
    c = case("periodic2")
    s0, s1, _ = c.gpu(ctx, a_dtype=np.float64)
    c.check(s0, s1, "periodic axis 2, double a")
    f0, f1, _ = c.gpu(ctx, a_dtype=np.float32)
    assert np.array_equal(s0, f0) and np.array_equal(s1, f1)  # a float column holds the same values


def test_open_zoom_window_with_slab(ctx):
    c = case("zoom")
    s0, s1, st = c.gpu(ctx)
    cut = np.abs(c.pos[:, 1] - 0.5) > 0.25
    assert 0.4 < cut.mean() < 0.6
    assert (c.ref["count"] == 0).any() and (c.ref["count"] > 0).any()
    assert st["footprints"] == c.footprints() >= int((c.ref["hits"] > 0).sum())
    c.check(s0, s1, "zoom")


def test_chunk_boundaries(ctx):
    """C - 1, C, C + 1 and 2 C + 1 particles in one tile's list, a handful in another"""
    C = sx.map_chunk_records()
    for n in (C - 1, C, C + 1, 2 * C + 1):
        rng = np.random.default_rng(n)
        pos = np.empty((n + 5, 3))
        pos[:n, :2] = rng.uniform(0.15, 0.35, (n, 2))  # reach 0.06: stays inside tile (0, 0) = [0, 0.5)^2
        pos[n:, :2] = rng.uniform(0.70, 0.80, (5, 2))
        pos[:, 2] = rng.random(n + 5)
        h = np.full(n + 5, 0.03, np.float32)
        m = rng.uniform(0.5, 1.5, n + 5).astype(np.float32)
        a = rng.normal(size=n + 5).astype(np.float32)
        c = Case(pos, h, m, UNIT, [0, 0, 0], sx.SxMap("column", 2, (0.5, 0.5, 0.5), (1.0, 1.0), 0.0, (32, 32)), a)
        s0, s1, st = c.gpu(ctx)
        assert st["longest"] == n and st["pairs"] == n + 5 and st["footprints"] == n + 5, st
        c.check(s0, s1, f"chunk {n}")


def test_bands(ctx):
    c = case("periodic2")
    s0, s1, st = c.gpu(ctx)
    # the two tile rows hold about half the pairs each: a cap of 0.6 of the total makes each its own band
    b0, b1, stb = c.gpu(ctx, cap=int(0.6 * st["pairs"]))
    assert stb["bands"] == 2 and stb["pairs"] == st["pairs"] and stb["longest"] == st["longest"]
    assert np.array_equal(s0, b0) and np.array_equal(s1, b1)
    with pytest.raises(sx.SxError, match="code 4.*pair cap"):
        c.gpu(ctx, cap=st["pairs"] // 4)


def test_h_clamp(ctx):
    """all h at 0.2 pixel: the result is the oracle's with the same clamp, and no particle is lost"""
    c = case("clamp")
    s0, s1, st = c.gpu(ctx)
    c.check(s0, s1, "clamp")
    assert (c.ref["hits"] >= 1).all() and st["footprints"] == c.h.size
    unclamped = mr.render(c.pos[:50], c.h[:50], c.m[:50], UNIT, [1, 1, 1], mr.COLUMN, 2, [0.5] * 3, [1.0, 1.0], [32, 32],
                          K=K, clamp=False)
    assert (unclamped["hits"] == 0).any()  # without the clamp particles fall between the pixel centres


def test_slices(ctx):
    c = case("slice")
    assert c.ref["hits"][0] > 0
    s0, s1, st = c.gpu(ctx)
    c.check(s0, s1, "slice")
    assert st["footprints"] == c.footprints() >= int((c.ref["hits"] > 0).sum())
    # without the particle behind the periodic face the image differs where it contributes
    s0b, _, _ = c.gpu(ctx, first=1)
    assert 0 < (s0b != s0).sum() <= c.ref["hits"][0]
    # open box, plane beyond every support: zeros
    o = Case(c.pos, c.h, c.m, UNIT, [0, 0, 0], sx.SxMap("slice", 2, (0.5, 0.5, 1.2), (1.0, 1.0), 0.0, (32, 32)), c.a)
    z0, z1, st = o.gpu(ctx)
    assert not z0.any() and not z1.any() and st["pairs"] == 0 and st["footprints"] == 0


def test_empty_cases(ctx):
    c = case("periodic2")
    s0, s1, st = c.gpu(ctx, first=100, last=100)
    assert not s0.any() and not s1.any() and st["pairs"] == 0
    w = Case(c.pos * 0.2, c.h * 0.2, c.m, UNIT, [0, 0, 0],
             sx.SxMap("column", 2, (0.7, 0.7, 0.5), (0.3, 0.3), 0.0, (40, 24)), c.a)  # the cloud is in [0, 0.2]^3
    s0, s1, st = w.gpu(ctx)
    assert not s0.any() and not s1.any() and st["footprints"] == 0
    # a = NULL: sum1 is not touched
    ds = sx.DeviceState(ctx, {"x": c.pos[:, 0], "y": c.pos[:, 1], "z": c.pos[:, 2], "h": c.h, "m": c.m})
    try:
        d0 = ctx.upload(np.full(32 * 32, -7.0))
        d1 = ctx.upload(np.full(32 * 32, -7.0))
        ctx.render_map(ds.fields, sx.make_box(UNIT, [1, 1, 1]), c.spec, a=None, K=K, sum0=d0, sum1=d1)
        assert (d0.get() > 0).all() and np.array_equal(d1.get(), np.full(32 * 32, -7.0))
    finally:
        ctx.free_all()


def test_deterministic(ctx):
    c = case("periodic2")
    s0, s1, _ = c.gpu(ctx)
    keys = ctx.alloc(2000, np.uint64)
    ds = sx.DeviceState(ctx, {"x": c.pos[:, 0], "y": c.pos[:, 1], "z": c.pos[:, 2], "h": c.h, "m": c.m})
    box = sx.make_box(UNIT, [1, 1, 1])
    ctx.check(ctx.L.sx_sfc_keys(ctx.h, ds.fields.x, ds.fields.y, ds.fields.z, keys.ptr, 2000, sx.C.byref(box)), "keys")
    ctx.sync()
    ctx.free_all()
    t0, t1, _ = c.gpu(ctx)
    assert np.array_equal(s0, t0) and np.array_equal(s1, t1)
