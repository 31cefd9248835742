"""Non-cubic, off-origin and mixed-boundary boxes shared by the box tests (test_boxes_oracle.py, test_gpu_boxes.py,
test_gpu_timestep.py, dist_worker.py --ic box:<name>).  Importable without a GPU.

The cases separate what a cube [-0.5, 0.5]^3 with one boundary type cannot: per-axis lengths and inverse lengths that
are not exact in binary, limits far from the origin, and periodic (1), open (0) and fixed (2) axes in one box.

  case        box                                  bnd    lattice    what it exercises
  thin_z      1 x 1 x 0.125                        1,1,1  56x56x7    the cluster kernels' applyPBC rule path on z only
  gresho      1 x 1 x 0.111 around the origin      1,1,1  63x63x7    the same, with a length that is no power of two
  windshock   0.5 x 0.125 x 0.125                  1,1,1  64x16x16   the folded fast path everywhere, wraps on a long axis
  mixed       1.4 x 0.7 x 0.35 off the origin      1,0,2  32x16x8    both paths in one run, an open and a fixed axis
  far_mixed   mixed at x + 1000, z - 38.35         1,0,2  32x16x8    absolute coordinates that a float cannot hold
  far_pbc     windshock's shape at (-513, 200, .7) 1,1,1  64x16x16   the same in a fully periodic box
  open_grav   2 x 1 x 0.5, lattice shrunk by 0.8   0,0,0  32x16x8    open-box self-gravity (g = 1) in a non-cubic box

Parity with the reference is claimed while 2 h_max < L_d / 2 on every periodic axis d: beyond it the reference's
single-shift applyPBC is no longer the minimum image (check_regime asserts this precondition on the oracle's h).
"""
import math

import numpy as np

import pyoracle as po

make_box6 = po.make_box6

CASES = {
    "thin_z": dict(lim=(0.0, 1.0, 0.0, 1.0, 0.0, 0.125), bnd=(1, 1, 1), dims=(56, 56, 7), g=0.0, shrink=1.0),
    "gresho": dict(lim=(-0.5, 0.5, -0.5, 0.5, -0.0555, 0.0555), bnd=(1, 1, 1), dims=(63, 63, 7), g=0.0, shrink=1.0),
    "windshock": dict(lim=(0.0, 0.5, 0.0, 0.125, 0.0, 0.125), bnd=(1, 1, 1), dims=(64, 16, 16), g=0.0, shrink=1.0),
    "mixed": dict(lim=(0.3, 1.7, -0.25, 0.45, 1.0, 1.35), bnd=(1, 0, 2), dims=(32, 16, 8), g=0.0, shrink=1.0),
    "far_mixed": dict(lim=(1000.3, 1001.7, -0.25, 0.45, -37.35, -37.0), bnd=(1, 0, 2), dims=(32, 16, 8), g=0.0,
                      shrink=1.0),
    "far_pbc": dict(lim=(-513.1, -512.6, 200.0, 200.125, 0.7, 0.825), bnd=(1, 1, 1), dims=(64, 16, 16), g=0.0,
                    shrink=1.0),
    "open_grav": dict(lim=(-1.0, 1.0, -0.5, 0.5, -0.25, 0.25), bnd=(0, 0, 0), dims=(32, 16, 8), g=1.0, shrink=0.8),
}
NG0 = 100
DT0 = 1e-5


def box_of(name):
    c = CASES[name]
    return make_box6(c["lim"], c["bnd"])


def lengths(box):
    lim = list(box.lim)
    return np.array([lim[1] - lim[0], lim[3] - lim[2], lim[5] - lim[4]])


def state(name, seed=1, dims=None, dt0=DT0):
    """the cell-centred lattice of the case (x fastest), every coordinate jittered by 0.2 spacing U(-1, 1);
    returns (HostState, OxBox).  dims overrides the lattice (the small golden variants), dt0 the first time-step
    (1e-3, near the Courant step, makes the particles move by a few per cent of h per step: the skin run)"""
    c = CASES[name]
    box = box_of(name)
    lim = np.array(c["lim"])
    lo, L = lim[0::2], lim[1::2] - lim[0::2]
    nx, ny, nz = dims or c["dims"]
    n = nx * ny * nz
    rng = np.random.default_rng(seed)
    t = []  # normalised coordinates in (0, 1)
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for idx, m in ((ii, nx), (jj, ny), (kk, nz)):
        t.append((idx.ravel() + 0.5 + 0.2 * rng.uniform(-1.0, 1.0, n)) / m)
    s = c["shrink"]
    t = [0.5 + s * (v - 0.5) for v in t]
    st = po.HostState(n)
    st.x[:], st.y[:], st.z[:] = lo[0] + L[0] * t[0], lo[1] + L[1] * t[1], lo[2] + L[2] * t[2]
    vol = float(np.prod(L)) * s ** 3
    st.h[:] = np.float32(0.5 * np.cbrt(3.0 / (4.0 * math.pi) * NG0 * vol / n))
    st.m[:] = np.float32(1.0 / n)
    st.alpha[:] = np.float32(0.05)
    # internal energy u = 1 + 0.5 sin along x (sound speed ~1, like the velocities); as a temperature of 1 it would be
    # u = cv ~ 1.2e7, and with dt0 = 1e-5 the first step throws particles out of the open and fixed axes
    st.temp[:] = (1.0 + 0.5 * np.sin(2.0 * math.pi * t[0])) / np.float64(po.ideal_gas_cv())
    st.vx[:] = (0.3 * np.sin(2.0 * math.pi * t[1])).astype(np.float32)
    st.vy[:] = (0.2 * np.sin(2.0 * math.pi * t[2])).astype(np.float32)
    st.vz[:] = (0.1 * np.sin(2.0 * math.pi * t[0])).astype(np.float32)
    for d in "xyz":
        st.arrays[d + "_m1"][:] = (st.arrays["v" + d].astype(np.float64) * dt0).astype(np.float32)
    st.id[:] = np.arange(n, dtype=np.uint64)
    st.minDt = st.minDt_m1 = dt0
    return st, box


# the boxes of the position-update tests: `mixed`, and its limits rotated with bnd (0, 2, 1): open x (0.35), fixed y
# (1.4), periodic z (0.7), so that every axis has another role and the periodic length is another one
POSITION_BOXES = {
    "mixed": (CASES["mixed"]["lim"], (1, 0, 2)),
    "mixed_perm": ((1.0, 1.35, 0.3, 1.7, -0.25, 0.45), (0, 2, 1)),
}


def positions_state(boxname, n=4096, seed=5):
    """a state for the position kernels in a mixed-boundary box, random a, x_m1, du, four classes of particles:
      0  at rest (v == 0) within 2h of a fixed wall: positions.hpp's fixed-boundary skip, must not move
      1  at rest at least 3h from the fixed walls: must move
      2  moving (v != 0) within 2h of a fixed wall: must move; half of them within 1e-6 of the wall and heading out:
         they leave the box and must not be wrapped
      3  moving, half of them within 1e-6 of a periodic limit and heading out: must wrap; a quarter within 1e-6 of an
         open limit and heading out: must not be wrapped
    returns (HostState, OxBox, class per particle); the caller sorts it if it needs SFC order"""
    lim, bnd = POSITION_BOXES[boxname]
    box = make_box6(lim, bnd)
    lim = np.array(lim)
    lo, L = lim[0::2], lim[1::2] - lim[0::2]
    rng = np.random.default_rng(seed)
    st = po.HostState(n)
    h = (0.01 * (1.0 + 0.3 * rng.uniform(-1, 1, n))).astype(np.float32)
    st.h[:] = h
    cls = rng.integers(0, 4, n)
    X = lo[None, :] + L[None, :] * rng.uniform(0.02, 0.98, (n, 3))
    fix, per = bnd.index(2), bnd.index(1)
    side = rng.integers(0, 2, n)
    depth = rng.uniform(0.05, 0.95, n) * 2.0 * h  # strictly inside 2h
    near = np.where(side == 0, lo[fix] + depth, lo[fix] + L[fix] - depth)
    far = lo[fix] + 3.0 * 0.013 + (L[fix] - 6.0 * 0.013) * rng.uniform(0, 1, n)
    X[:, fix] = np.where((cls == 0) | (cls == 2), near, np.where(cls == 1, far, X[:, fix]))
    for k in ("ax", "ay", "az", "divv"):
        st.arrays[k][:] = rng.standard_normal(n).astype(np.float32) * 20.0
    V = rng.standard_normal((n, 3)).astype(np.float32) * np.float32(0.3)
    V[V == 0] = np.float32(0.1)
    dXm1 = rng.standard_normal((n, 3)).astype(np.float32) * np.float32(1e-6)
    out = (cls == 3) & (rng.integers(0, 2, n) == 1)
    X[out, per] = np.where(side[out] == 0, lo[per] + 1e-6 * rng.uniform(0, 1, out.sum()),
                           lo[per] + L[per] - 1e-6 * rng.uniform(0, 1, out.sum()))
    dXm1[out, per] = np.where(side[out] == 0, -3e-5, 3e-5).astype(np.float32)
    opn = bnd.index(0)
    for sel, d in (((cls == 2) & (rng.integers(0, 2, n) == 1), fix), ((cls == 3) & ~out & (rng.integers(0, 2, n) == 1), opn)):
        X[sel, d] = np.where(side[sel] == 0, lo[d] + 1e-6 * rng.uniform(0, 1, sel.sum()),
                             lo[d] + L[d] - 1e-6 * rng.uniform(0, 1, sel.sum()))
        dXm1[sel, d] = np.where(side[sel] == 0, -3e-5, 3e-5).astype(np.float32)
    V[cls < 2] = 0.0
    st.x[:], st.y[:], st.z[:] = X[:, 0], X[:, 1], X[:, 2]
    for d, c in enumerate("xyz"):
        st.arrays["v" + c][:] = V[:, d]
        st.arrays[c + "_m1"][:] = dXm1[:, d]
    st.temp[:] = 1.0 + 0.5 * rng.uniform(0, 1, n)
    u = st.temp * po.ideal_gas_cv()
    st.du[:] = rng.standard_normal(n) * 0.1 * u / 1e-3  # |du dt| < u / 10: u stays positive
    st.du_m1[:] = (rng.standard_normal(n) * 0.1 * u / 1e-3).astype(np.float32)
    st.m[:] = np.float32(1.0 / n)
    st.alpha[:] = np.float32(0.05)
    st.id[:] = np.arange(n, dtype=np.uint64)
    st.nc[:] = cls.astype(np.uint32)  # the class travels with the particle through a sort of all fields
    return st, box, cls


def sort_all(st, box, ora):
    """Hilbert-sort every field of st in place (positions_state's a, du and class included); returns the order"""
    keys = ora.sfc_keys(st, box).copy()
    o = np.argsort(keys, kind="stable")
    for k in st.arrays:
        st.arrays[k][:] = st.arrays[k][o]
    st.keys[:] = keys[o]
    return o


def check_position_classes(before, after, cls, box):
    """what the classes of positions_state must show between two states in the same order: class 0 unchanged in x, v
    and x_m1, every other particle moved, wraps (a jump of more than L/2) on the periodic axis only, in both
    directions"""
    L = lengths(box)
    moved = np.zeros(before.n, bool)
    for d, c in enumerate("xyz"):
        dx = after.arrays[c] - before.arrays[c]
        moved |= dx != 0
        wraps = np.abs(dx) > 0.5 * L[d]
        if box.bnd[d] == 1:
            assert np.any(dx[wraps] > 0) and np.any(dx[wraps] < 0), c
            assert np.all((after.arrays[c] >= box.lim[2 * d]) & (after.arrays[c] <= box.lim[2 * d + 1])), c
        else:  # particles cross the open and the fixed limits on both sides and stay outside
            assert not wraps.any(), c
            assert np.any(after.arrays[c] < box.lim[2 * d]) and np.any(after.arrays[c] > box.lim[2 * d + 1]), c
    assert (cls == 0).sum() > 100 and not moved[cls == 0].any()
    for k in ("vx", "vy", "vz", "x_m1", "y_m1", "z_m1"):  # (the energy update is not part of the skip on the CPU path)
        assert np.array_equal(after.arrays[k][cls == 0], before.arrays[k][cls == 0]), k
    for c in (1, 2, 3):
        assert (cls == c).sum() > 100 and moved[cls == c].all(), c


def edge_particles(box):
    """key edge cases of a box: a particle exactly on each lower limit, one exactly on each upper limit (it clamps to
    the last cell) and one a nextafter below each upper limit, the other two coordinates at an uneven interior point;
    returns x, y, z"""
    lim = np.array(list(box.lim))
    lo, hi = lim[0::2], lim[1::2]
    mid = lo + (hi - lo) * np.array([0.37, 0.61, 0.23])
    pts = []
    for d in range(3):
        for v in (lo[d], hi[d], np.nextafter(hi[d], lo[d])):
            p = mid.copy()
            p[d] = v
            pts.append(p)
    pts += [lo.copy(), hi.copy(), np.nextafter(hi, lo)]
    pts = np.array(pts)
    return pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()


def with_edges(st, box):
    """st with edge_particles(box) appended (positions only matter: keys, sort and tree)"""
    ex, ey, ez = edge_particles(box)
    out = po.HostState(st.n + ex.size)
    for k in ("x", "y", "z"):
        out.arrays[k][:st.n] = st.arrays[k]
    out.x[st.n:], out.y[st.n:], out.z[st.n:] = ex, ey, ez
    return out


def sort_by_key(st, box, ora):
    """Hilbert-sort the conserved fields of st in place (the reference's sync); returns st"""
    keys = ora.sfc_keys(st, box).copy()
    o = np.argsort(keys, kind="stable")
    for k in po.CONSERVED:
        st.arrays[k][:] = st.arrays[k][o]
    st.keys[:] = keys[o]
    return st


def check_regime(st, box, ora=None):
    """precondition of the parity claim, on the oracle alone: after the h iteration 2 h_max < L_d / 2 on every
    periodic axis.  Returns (rule, waves), computed as the kernels decide them:
      rule   share of the clusters (256 SFC-consecutive particles, origin at the first) whose largest
             (|fold(x_i - o)| + 2 h_i) / L_d over the periodic axes reaches 0.49: the cluster kernels' applyPBC path
      waves  share of the waves of 64 with a lane at |fold(x_i - o)| + 2.05 h_i >= 0.49 L_d on a periodic axis: the
             search waves that leave the float prefilter"""
    ora = ora or po.load_oracle()
    s = sort_by_key(st.copy(), box, ora)
    ora.find_neighbors(s, box, iterate_h=True)
    L = lengths(box)
    pbc = [box.bnd[d] == 1 for d in range(3)]
    for d in range(3):
        if pbc[d]:
            assert 2.0 * float(s.h.max()) < 0.5 * L[d], (d, float(s.h.max()), L[d])
    n = s.n
    origin = (np.arange(n) // 256) * 256
    h = s.h.astype(np.float32)
    ext = np.zeros(n, np.float32)
    unsafe = np.zeros(n, bool)
    for d, c in enumerate("xyz"):
        if not pbc[d]:
            continue
        x = s.arrays[c]
        r = x - x[origin]
        r = (r - L[d] * np.rint(r * (1.0 / L[d]))).astype(np.float32)
        ext = np.maximum(ext, (np.abs(r) + np.float32(2.0) * h) * np.float32(1.0 / L[d]))
        unsafe |= (np.abs(r) + np.float32(2.05) * h) >= np.float32(0.49) * np.float32(L[d])
    ncl = (n + 255) // 256
    rule = np.array([ext[c * 256:(c + 1) * 256].max() >= np.float32(0.49) for c in range(ncl)])
    nw = (n + 63) // 64
    waves = np.array([unsafe[w * 64:(w + 1) * 64].any() for w in range(nw)])
    return float(rule.mean()), float(waves.mean())
