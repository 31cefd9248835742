"""Power spectra on the GPU at seam level, uploaded arrays against tests/spectrum_ref.py: the mesh deposit
(sx_mesh_deposit), the transform (sx_fft3d), the shell sums (sx_shell_sums) and the chain (sx_spectrum_compute).

Deposit.  Per cell and scale-aware, the form of tests/test_gpu_map.py:

    |S0 - S0_ref| <= r S0_ref,    |S1_a - S1_ref| <= r sum_j |w_j a_j|,    r = FIT + (n_c + c) 2^-24

with n_c the cell's contributions and FIT = 4 x 3.1e-7, four times the fit error of kernelWt pinned by
tests/test_capi_cpu.py.  Derivation of c, to first order, u = 2^-24 the largest relative error of one float rounding;
nothing in it is taken from the kernel's output:
* accumulation: n_c fused multiply-adds in list order, n_c u S0 (the n_c of the formula);
* values: the weight w is rounded once, and so is the product w a: 2 u S0;
* the kernel's argument t = (dx^2 + dy^2 + dz^2) D^2 / he^2: the stored factor, one square and two FMAs (each at most u of
  the whole sum, its terms being positive) and the product make 5 roundings, at most 5 u of t, i.e. 2.5 u of
  q = sqrt(t) < 2: 5 u G with G = sum_j |dw_j / dq_j| the cell's sensitivity to the distances (the oracle's dq0, dq1);
* geometry: a record's coordinate is a float in cells relative to its block's origin.  A record that reaches a cell of
  the block lies within ru + 3.5 of the block's centre (ru = 2 he / D its reach in cells; the minimum image about the
  centre is no further than the image that reaches the cell), so its magnitude is at most 8 + ru; the difference to the
  cell centre and its fold by whole periods round once more (at most ru for a cell inside the support):
  u (8 + 2 ru) cells per axis, sqrt(3) times that for the distance over three axes (the maps' slices have two in-plane
  axes and a tile of 16: sqrt(2) u (16 + 2 ru)), sqrt(3) u (16 / ru + 4) in units of he = ru D / 2.
So  c = 2 + (5 + sqrt(3) (16 / ru_min + 4)) G / S0  per cell, ru_min = 2 max(min h, D / 2) / D >= 1 per case.

Transform.  Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2, for radix-2 / radix-4 Cooley-Tukey:
|y^ - y|_2 / |y|_2 <= t eta / (1 - t eta), t = 3 log2 n stages over the three axes, eta = mu + gamma_4 (sqrt 2 + mu),
mu = 2^-52 the twiddle error, gamma_4 = 4 x 2^-53 / (1 - 4 x 2^-53); twice that against np.fft.fftn, for numpy's own error.

Shell sums.  All terms are non-negative: |P - P_ref| <= modes[s] 2^-52 P_ref per shell, against np.bincount.

Chain.  By Parseval the error vector of a shell has norm at most E = sqrt(prefactor mean_c sum_a e_ac^2), e_ac the
first-order propagation of the deposit bounds through W_a = S0^(p-1) S1_a:

    e_ac = S0^(p-1) (r1_a sum_j |w_j a_j| + |1 - p| |S1_a| r0)      (density itself: e_c = r0 S0)

and | sqrt P_gpu(s) - sqrt P_ref(s) | <= E + (transform bound + modes[s] 2^-52) sqrt P_total for every shell.

Measured on an MI355X, worst use of a bound over the cells of a case (S0 / S1): random n = 16 0.216 / 0.230, n = 32 0.204 /
0.206, support wider than half the box 0.233 / 0.234, clamp 0.479 / 0.480, offset box 0.201 / 0.212, block lists of 255,
256, 257, 513: 0.190 / 0.190, 0.178 / 0.182, 0.173 / 0.177, 0.228 / 0.229, sub-range 0.228 / 0.236.  The worst is above a
quarter, so the deposit bound stands as derived (the maps' rule: it would have been cut to four times the measured use
otherwise).  Transform: relative l2 error 2.6e-16 (n = 16) .. 4.3e-16 (n = 256) against bounds of 2.0e-14 .. 4.1e-14, which
are a theorem's and stay.  Shell sums: worst use 0.080 / 0.052 / 0.030 at n = 16 / 32 / 64.  Chain: E is 1.1e-5 .. 2.5e-5 of
sqrt(P_total); worst use of E per kind at n = 16 / 32: velocity p = 0 0.0009 / 0.0016, p = 1/2 0.0005 / 0.0004, p = 1/3
0.0002 / 0.0008, density 0.0057 / 0.0071, scalar column 0.0003 / 0.0001 (the per-cell errors are far from all at their
bounds with one sign, which is what E allows for).  The worst, 0.0071, is below a quarter: E is cut to four times the
measured use, E_CUT = 0.0284.  Parseval on the device's own mesh holds to 6e-16.
"""
import numpy as np
import pytest

import map_ref as mr
import spectrum_ref as sr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FIT = 4 * 3.1e-7
UNIT = [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]
K = mr.kernel_constant()

# the quarter rule of the header: the deposit bound stands as derived, the chain's E is cut to 4 x 0.0071
CUT = 1.0
E_CUT = 0.0284


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


def geometry_factor(h, n, L=1.0):
    """5 + sqrt(3) (16 / ru_min + 4) of the derivation above"""
    D = L / n
    ru = 2.0 * max(float(np.min(h)), 0.5 * D) / D
    return 5.0 + np.sqrt(3.0) * (16.0 / ru + 4.0)


def cell_bounds(ref, g, ranks=0):
    """(r0, r1[a]) of the derivation per cell, 0 where the scale is 0; ranks: further roundings of regrouped sums"""
    with np.errstate(divide="ignore", invalid="ignore"):
        c0 = 2.0 + g * np.where(ref["sum0"] > 0, ref["dq0"] / ref["sum0"], 0.0)
        c1 = 2.0 + g * np.where(ref["abs1"] > 0, ref["dq1"] / ref["abs1"], 0.0)
    return FIT + (ref["count"] + ranks + c0) * U, FIT + (ref["count"][None] + ranks + c1) * U


class Case:
    """particles in the unit periodic box, three signed columns, a mesh size; the oracle's meshes are computed once"""

    def __init__(self, name, pos, h, m, n, seed=1, lim=UNIT):
        self.name, self.pos, self.h, self.m, self.n, self.lim = name, pos, h, m, n, lim
        self.a = np.random.default_rng(seed).normal(size=(len(h), 3)).astype(np.float32)
        self._ref = {}

    def ref(self, first=0, last=None):
        key = (first, last)
        if key not in self._ref:
            s = slice(first, last)
            self._ref[key] = sr.mesh(self.pos[s], self.h[s], self.m[s], self.lim, self.n, K=K, a=self.a[s], scales=True)
        return self._ref[key]

    def gpu(self, ctx, a_dtype=np.float32, first=0, last=None, cap=0, between=False):
        host = {"x": self.pos[:, 0], "y": self.pos[:, 1], "z": self.pos[:, 2], "h": self.h, "m": self.m}
        ds = sx.DeviceState(ctx, host)
        try:
            cols = [ctx.upload(np.ascontiguousarray(self.a[:, k], a_dtype)) for k in range(3)]
            ctx.set_spectrum_pair_cap(cap)
            box = sx.make_box(self.lim, [1, 1, 1])
            if between:  # another kernel between two runs
                keys = ctx.alloc(len(self.h), np.uint64)
                ctx.check(ctx.L.sx_sfc_keys(ctx.h, ds.fields.x, ds.fields.y, ds.fields.z, keys.ptr, len(self.h),
                                            sx.C.byref(box)), "keys")
                ctx.sync()
            s0, s1 = ctx.mesh_deposit(ds.fields, box, self.n, a=cols, first=first, last=last, K=K)
            return s0, s1, ctx.spectrum_stats()
        finally:
            ctx.set_spectrum_pair_cap(0)
            ctx.free_all()

    def check(self, s0, s1, first=0, last=None):
        r = self.ref(first, last)
        r0, r1 = cell_bounds(r, geometry_factor(self.h[first:last], self.n, self.lim[1] - self.lim[0]))
        cut = CUT
        empty = r["count"] == 0
        # a cell is exactly 0 where no support contains its centre
        assert not s0[empty].any() and not s1[:, empty].any(), self.name
        uses = []
        for tag, got, want, scale, rr in (("S0", s0, r["sum0"], r["sum0"], r0), ("S1", s1, r["sum1"], r["abs1"], r1)):
            ok = scale > 0
            assert not np.abs(got - want)[~ok].any(), (self.name, tag)
            use = (np.abs(got - want)[ok] / (rr[ok] * scale[ok])).max()
            uses.append(use)
        print(f"{self.name}: max n_c = {r['count'].max()}, worst use of the derived bound S0 {uses[0]:.3f} / S1 {uses[1]:.3f}"
              f" (cut {cut:.3f})")
        assert max(uses) <= cut, (self.name, uses, cut)


def cloud(seed, npart, hlo, hhi):
    rng = np.random.default_rng(seed)
    pos = rng.random((npart, 3))
    h = rng.uniform(hlo, hhi, npart).astype(np.float32)
    m = (rng.uniform(0.5, 1.5, npart) / npart).astype(np.float32)
    return pos, h, m


_cases = {}


def case(name):
    if name not in _cases:
        if name.startswith("random"):
            n = int(name[6:])
            # mixed h: from below half a cell of the coarser mesh (clamped there) to six cells of the finer
            _cases[name] = Case(name, *cloud(7, 2000, 0.02, 0.09), n, seed=8)
        elif name == "fold":
            pos, h, m = cloud(11, 300, 0.05, 0.08)
            h[17] = 0.3  # support 2 h = 0.6 > L / 2: cells see it through the nearest image on every axis
            h[201] = 0.26
            _cases[name] = Case(name, pos, h, m, 16, seed=12)
        elif name == "clamp":
            pos, h, m = cloud(13, 2000, 0.1 / 32, 0.4 / 32)  # all below D / 2 = 0.5 / 32
            _cases[name] = Case(name, pos, h, m, 32, seed=14)
        elif name == "offset":
            # a cubic box away from the origin with an edge that is no power of two
            pos, h, m = cloud(19, 800, 0.02, 0.09)
            lim = [-1.3, 1.7, 0.4, 3.4, -3.0, 0.0]
            _cases[name] = Case(name, pos * 3.0 + np.array([lim[0], lim[2], lim[4]]), h * 3.0, m, 16, seed=20, lim=lim)
    return _cases[name]


@pytest.mark.parametrize("n", [16, 32])
def test_deposit_random(ctx, n):
    """2000 particles, mixed h, three signed columns; float and double columns give the same bits"""
    c = case(f"random{n}")
    s0, s1, st = c.gpu(ctx)
    c.check(s0, s1)
    d0, d1, _ = c.gpu(ctx, a_dtype=np.float64)
    assert np.array_equal(s0, d0) and np.array_equal(s1, d1)
    assert st["clamped"] == int((c.h < 0.5 / n).sum()) and st["bands"] == 1
    assert (c.ref()["hits"] >= 1).all()  # the clamp leaves no particle between the centres


def test_deposit_support_wider_than_half_the_box(ctx):
    c = case("fold")
    assert 2.0 * c.h[17] > 0.5 and c.ref()["hits"][17] > 16 ** 3 // 2
    s0, s1, _ = c.gpu(ctx)
    c.check(s0, s1)
    d0, d1, _ = c.gpu(ctx, a_dtype=np.float64)
    assert np.array_equal(s0, d0) and np.array_equal(s1, d1)


def test_deposit_clamp(ctx):
    """all h below D / 2: the oracle's result with the same clamp, no particle is lost, stats counts them"""
    c = case("clamp")
    s0, s1, st = c.gpu(ctx)
    c.check(s0, s1)
    assert st["clamped"] == c.h.size and (c.ref()["hits"] >= 1).all()
    d0, d1, _ = c.gpu(ctx, a_dtype=np.float64)
    assert np.array_equal(s0, d0) and np.array_equal(s1, d1)
    unclamped = sr.mesh(c.pos[:50], c.h[:50], c.m[:50], UNIT, 32, K=K, clamp=False)
    assert (unclamped["hits"] == 0).any()  # without the clamp particles fall between the cell centres


def test_deposit_offset_box(ctx):
    c = case("offset")
    s0, s1, _ = c.gpu(ctx)
    c.check(s0, s1)


@pytest.mark.parametrize("npart", [255, 256, 257, 513])
def test_deposit_chunk_boundaries(ctx, npart):
    """C - 1, C, C + 1 and 2 C + 1 particles in one block's list, a handful in another"""
    assert sx.spectrum_chunk_records() == 256
    n = 32
    rng = np.random.default_rng(npart)
    pos = np.empty((npart + 5, 3))
    # block (0, 0, 0) is [0, 8) x [0, 8) x [0, 4) cells; a clamped reach of one cell stays inside from 1.2 .. 6.8 / 2.8
    pos[:npart, :2] = rng.uniform(1.2, 6.8, (npart, 2)) / n
    pos[:npart, 2] = rng.uniform(1.2, 2.8, npart) / n
    pos[npart:] = (rng.uniform(1.2, 2.8, (5, 3)) + np.array([16.0, 8.0, 12.0])) / n
    h = np.full(npart + 5, 0.3 / n, np.float32)
    m = rng.uniform(0.5, 1.5, npart + 5).astype(np.float32)
    c = Case(f"chunk{npart}", pos, h, m, n, seed=npart + 1)
    s0, s1, st = c.gpu(ctx)
    assert st["longest"] == npart and st["pairs"] == npart + 5 and st["clamped"] == npart + 5, st
    c.check(s0, s1)
    d0, d1, _ = c.gpu(ctx, a_dtype=np.float64)
    assert np.array_equal(s0, d0) and np.array_equal(s1, d1)


def test_deposit_sub_range(ctx):
    c = case("random16")
    s0, s1, _ = c.gpu(ctx, first=100, last=1500)
    c.check(s0, s1, first=100, last=1500)
    e0, e1, st = c.gpu(ctx, first=700, last=700)
    assert not e0.any() and not e1.any() and st["pairs"] == 0


def test_deposit_pair_caps(ctx):
    c = case("random32")
    s0, s1, st = c.gpu(ctx)
    # eight block layers of about an eighth of the pairs each: a cap of 0.3 of the total makes bands of two
    b0, b1, stb = c.gpu(ctx, cap=int(0.3 * st["pairs"]))
    assert stb["bands"] >= 4 and stb["pairs"] == st["pairs"] and stb["longest"] == st["longest"]
    assert np.array_equal(s0, b0) and np.array_equal(s1, b1)
    with pytest.raises(sx.SxError, match="code 4.*pair cap"):
        c.gpu(ctx, cap=st["pairs"] // 40)


def test_deposit_deterministic(ctx):
    c = case("random16")
    s0, s1, _ = c.gpu(ctx)
    t0, t1, _ = c.gpu(ctx, between=True)
    assert np.array_equal(s0, t0) and np.array_equal(s1, t1)


def test_render_and_deposit_on_one_context_keep_apart(ctx):
    """the maps and the deposit run the same pair-binning engine, each with scratch and figures of its own: a banded
    deposit between two renders changes neither the map's stats nor its image, and is itself what it is alone"""
    c = case("random16")
    fresh = sx.Context(0)
    try:
        pairs = c.gpu(fresh)[2]["pairs"]
        # four block layers of about a quarter of the pairs each: no two fit under 0.3 of the total
        cap = int(0.3 * pairs)
        f0, f1, fst = c.gpu(fresh, cap=cap)
    finally:
        fresh.close()
    assert fst["bands"] >= 2
    spec = sx.SxMap("column", 2, (0.5, 0.5, 0.5), (1.0, 1.0), 0.0, (32, 32))
    box = sx.make_box(UNIT, [1, 1, 1])
    ds = sx.DeviceState(ctx, {"x": c.pos[:, 0], "y": c.pos[:, 1], "z": c.pos[:, 2], "h": c.h, "m": c.m})
    try:
        cols = [ctx.upload(np.ascontiguousarray(c.a[:, k])) for k in range(3)]
        r0, r1 = ctx.render_map(ds.fields, box, spec, a=cols[0], K=K)
        alone = ctx.map_stats()
        assert alone["footprints"] == 2000 and alone["pairs"] > 0
        ctx.set_spectrum_pair_cap(cap)
        s0, s1 = ctx.mesh_deposit(ds.fields, box, c.n, a=cols, K=K)
        assert ctx.map_stats() == alone
        t0, t1 = ctx.render_map(ds.fields, box, spec, a=cols[0], K=K)
        assert np.array_equal(r0, t0) and np.array_equal(r1, t1) and ctx.map_stats() == alone
        assert ctx.spectrum_stats() == fst
        assert np.array_equal(s0, f0) and np.array_equal(s1, f1)
    finally:
        ctx.set_spectrum_pair_cap(0)
        ctx.free_all()


# ---- transform ---------------------------------------------------------------------------------------------------

def fft_bound(n):
    mu = 2.0 ** -52
    g4 = 4 * 2.0 ** -53 / (1 - 4 * 2.0 ** -53)
    eta = mu + g4 * (np.sqrt(2.0) + mu)
    t = 3 * np.log2(n)
    return t * eta / (1 - t * eta)


def rel2(got, want):
    return float(np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel()))


@pytest.mark.parametrize("n", [16, 32, 64, 128, 256])
def test_fft_random(ctx, n):
    rng = np.random.default_rng(100 + n)
    w = rng.normal(size=(n, n, n)) + 1j * rng.normal(size=(n, n, n))
    got = ctx.fft3d(w)
    want = np.fft.fftn(w) / float(n) ** 3
    err = rel2(got, want)
    print("n = %d: relative l2 error %.3e, bound %.3e" % (n, err, 2 * fft_bound(n)))
    assert err <= 2 * fft_bound(n)


@pytest.mark.parametrize("n", [16, 32, 64])
def test_fft_closed_forms(ctx, n):
    rng = np.random.default_rng(n)
    # a real input: the transform is Hermitian, and numpy's within the bound
    w = rng.normal(size=(n, n, n))
    got = ctx.fft3d(w)
    assert rel2(got, np.fft.fftn(w) / float(n) ** 3) <= 2 * fft_bound(n)
    idx = (-np.arange(n)) % n
    assert rel2(got[np.ix_(idx, idx, idx)], np.conj(got)) <= 2 * fft_bound(n)
    # an impulse at the origin: all modes equal n^-3; elsewhere a phase ramp
    w = np.zeros((n, n, n), complex)
    w[0, 0, 0] = 1.0
    assert np.array_equal(ctx.fft3d(w), np.full((n, n, n), float(n) ** -3, complex))
    cz, cy, cx = 3, n - 2, n // 2 + 1
    w = np.zeros((n, n, n), complex)
    w[cz, cy, cx] = 2.5
    k = np.arange(n)

    def phase(az, ay, ax):  # exp(2 pi i (a . k) / n) with the argument reduced in integers
        return np.exp(2j * np.pi * ((k[:, None, None] * az + k[None, :, None] * ay + k[None, None, :] * ax) % n) / n)

    assert rel2(ctx.fft3d(w), 2.5 * np.conj(phase(cz, cy, cx)) / float(n) ** 3) <= 2 * fft_bound(n)
    # a single plane wave: one non-zero mode
    mz, my, mx = 2, n - 3, n // 2
    w = phase(mz, my, mx)
    want = np.zeros((n, n, n), complex)
    want[mz, my, mx] = 1.0
    got = ctx.fft3d(w)
    assert np.linalg.norm((got - want).ravel()) <= 2 * fft_bound(n)  # the input's own rounding: numpy's exp
    assert abs(got[mz, my, mx] - 1.0) <= 2 * fft_bound(n)


# ---- shell sums --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [16, 32, 64])
def test_shell_sums(ctx, n):
    rng = np.random.default_rng(200 + n)
    w = (rng.normal(size=(n, n, n)) + 1j * rng.normal(size=(n, n, n))) * rng.uniform(0.1, 10.0, (n, n, n))
    s, modes = sr.shells(n)
    want = np.bincount(s.ravel(), weights=(w.real ** 2 + w.imag ** 2).ravel(), minlength=modes.size)
    p, md = ctx.shell_sums(w, prefactor=1.0)
    assert md.dtype == np.uint64 and np.array_equal(md, modes)
    use = np.abs(p - want) / (modes.astype(np.float64) * 2.0 ** -52 * want)
    print("n = %d: worst use of modes 2^-52 P: %.3f (shell %d)" % (n, use.max(), use.argmax()))
    assert use.max() <= 1.0
    p2, _ = ctx.shell_sums(w, prefactor=1.0)
    assert np.array_equal(p, p2)
    # accumulate = 1 adds: half of another mesh's sums on top
    w2 = rng.normal(size=(n, n, n)) + 1j * rng.normal(size=(n, n, n))
    q, _ = ctx.shell_sums(w2, prefactor=0.5)
    acc, md = ctx.shell_sums(w2, prefactor=0.5, power=p)
    assert np.array_equal(acc, p + q) and np.array_equal(md, modes)


# ---- the chain ---------------------------------------------------------------------------------------------------

class Chain:
    """the 16^3 jittered lattice with the sheared velocity field plus noise, its oracle meshes per n"""

    def __init__(self):
        self.pos, self.h, self.m = sr.lattice(16)
        rng = np.random.default_rng(5)
        self.v = (sr.shear_velocity(self.pos) + 0.05 * rng.normal(size=self.pos.shape)).astype(np.float32)
        self.temp = rng.uniform(1.0, 2.0, len(self.h))  # a double column
        self._ref = {}

    def ref(self, n):
        if n not in self._ref:
            a = np.column_stack([self.v.astype(np.float64), self.temp])
            self._ref[n] = sr.mesh(self.pos, self.h, self.m, UNIT, n, K=K, a=a, scales=True)
        return self._ref[n]


_chain = []


def chain():
    if not _chain:
        _chain.append(Chain())
    return _chain[0]


def chain_reference(r, kind, weight, column, n, ranks=0):
    """(power_ref, E) of the header for the oracle meshes r"""
    g = geometry_factor(chain().h, n)
    r0, r1 = cell_bounds(r, g, ranks)
    s0 = r["sum0"]
    if kind == "velocity":
        p, pre, cols = sr.POWERS[weight], 0.5, [0, 1, 2]
    elif column:
        p, pre, cols = 0.0, 1.0, [3]
    else:
        power, _ = sr.spectrum(s0, n, 1.0)
        return power, float(np.sqrt(np.mean((r0 * s0) ** 2)))
    ok = s0 > 0
    f = np.zeros_like(s0)
    f[ok] = s0[ok] ** (p - 1.0)
    e2 = np.zeros_like(s0)
    for a in cols:
        e2 += (f * (r1[a] * r["abs1"][a] + abs(1.0 - p) * np.abs(r["sum1"][a]) * r0)) ** 2
    power, _ = sr.spectrum(sr.field(s0, r["sum1"][cols], weight if kind == "velocity" else 0), n, pre)
    return power, float(np.sqrt(pre * np.mean(e2)))


@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("kind, weight, column", [("velocity", 0, False), ("velocity", 1, False), ("velocity", 2, False),
                                                  ("scalar", 0, False), ("scalar", 0, True)])
def test_chain(ctx, n, kind, weight, column):
    c = chain()
    r = c.ref(n)
    want, E = chain_reference(r, kind, weight, column, n)
    _, modes = sr.shells(n)
    host = {"x": c.pos[:, 0], "y": c.pos[:, 1], "z": c.pos[:, 2], "h": c.h, "m": c.m,
            "vx": c.v[:, 0], "vy": c.v[:, 1], "vz": c.v[:, 2]}
    ds = sx.DeviceState(ctx, host)
    try:
        box = sx.make_box(UNIT, [1, 1, 1])
        spec = sx.SxSpectrum(kind, weight, n)
        cols = [ctx.upload(c.temp)] if column else None
        power, md = ctx.spectrum(ds.fields, box, spec, a=cols, K=K)
        if kind == "velocity":  # the columns passed explicitly give the same bits as f->vx, vy, vz
            again, _ = ctx.spectrum(ds.fields, box, spec, a=[ds.dev["vx"], ds.dev["vy"], ds.dev["vz"]], K=K)
            assert np.array_equal(power, again)
        s0, s1 = ctx.mesh_deposit(ds.fields, box, n, a=cols if column else [ds.dev["vx"], ds.dev["vy"], ds.dev["vz"]], K=K)
    finally:
        ctx.free_all()
    assert np.array_equal(md, modes) and np.isfinite(power).all()
    key = (kind, weight, column, n)
    total = np.sqrt(want.sum())
    slack = (2 * fft_bound(n) + modes.astype(np.float64) * 2.0 ** -52) * total
    diff = np.abs(np.sqrt(power) - np.sqrt(want))
    use = float((np.maximum(diff - slack, 0.0) / E).max())
    cut = E_CUT
    print(f"{key}: E / sqrt(P_total) = {E / total:.3e}, worst use of E {use:.4f} (cut {cut:.4f})")
    assert use <= cut
    # Parseval on the device's own mesh
    if kind == "velocity":
        W, pre = sr.field(s0, s1, weight), 0.5
    else:
        W, pre = (sr.field(s0, s1, 0) if column else s0), 1.0
    mean = pre * float((W ** 2).sum()) / n ** 3
    print(f"{key}: Parseval to {abs(power.sum() - mean) / mean:.2e}")
    assert abs(power.sum() - mean) <= 1e-12 * mean
