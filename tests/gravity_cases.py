"""Seeded inputs for the gravity tests that the smooth fixtures (Evrard sphere, mass-wave lattice, uniform random
bodies) do not reach: clumps inside a sparse halo, unequal masses, massless bodies, coincident bodies, bodies on node
boundaries, a box far from the origin, deep trees, tiny views, a periodic box.  numpy only: the GPU tests import this
module and need neither the reference nor a compiler (like direct_ref.py).

Every case returns (f, lim, bnd): f = {x, y, z: float64; m, h: float32}, the box limits (xmin, xmax, ymin, ...) and the
boundary per axis (0 open, 1 periodic).  All cases hold about 4k bodies.

Two models of the production arithmetic, both evaluated in float64 from float32 displacements so that only the
rounding of the displacement is in them:
* displacement_rounded_once: x_j - x_i formed in double, rounded to float once -- what an honest float P2P sees;
* origin_rounded: both coordinates rounded to float relative to a far origin (the first body of each run of 64
  consecutive bodies in Morton order), then subtracted.  A pair's displacement then carries an absolute error of about
  2^-24 W, W the extent of the run, i.e. a relative error 2^-24 W / r.
"""
import numpy as np

import direct_ref as dr
from sphexa_amd import ic

PICKS = (1, 2, 15, 16, 17, 63, 64, 65, 129)
OFFSET = (1024.0, -2048.0, 512.0)
CLUMPS, CLUMP_SIZE, OUTER = 24, 8, 200


def _fields(arr):
    return {"x": np.array(arr["x"], np.float64), "y": np.array(arr["y"], np.float64),
            "z": np.array(arr["z"], np.float64), "m": np.array(arr["m"], np.float32),
            "h": np.array(arr["h"], np.float32)}


def _append(f, x, y, z, m, h):
    add = {"x": x, "y": y, "z": z, "m": m, "h": h}
    return {k: np.concatenate([f[k], np.asarray(add[k], f[k].dtype)]) for k in f}


def halo_clumps(sigma, seed=1):
    """ic.plummer(4096, 1) plus 24 clumps of 8 bodies (normal, standard deviation sigma) around 24 of its 200 outermost
    bodies; a clump body has the halo's mass and h = sigma / 8.  The clump bodies are the last 192."""
    arr, lim, bnd, _ = ic.plummer(4096, 1)
    f = _fields(arr)
    rng = np.random.default_rng(7000 + seed)
    r = np.sqrt(f["x"] ** 2 + f["y"] ** 2 + f["z"] ** 2)
    hosts = rng.choice(np.argsort(r)[-OUTER:], CLUMPS, replace=False)
    k = CLUMPS * CLUMP_SIZE
    d = rng.normal(0.0, sigma, (3, CLUMPS, CLUMP_SIZE))
    x, y, z = (f[c][hosts][:, None] + d[a] for a, c in enumerate("xyz"))
    f = _append(f, x.ravel(), y.ravel(), z.ravel(), np.full(k, f["m"][0]), np.full(k, np.float32(sigma / 8.0)))
    return f, list(lim), list(bnd)


def mass_ratio():
    """Plummer positions, masses log-uniform over six decades, one body off centre with 90 % of the total mass 1"""
    arr, lim, bnd, _ = ic.plummer(4096, 2)
    f = _fields(arr)
    rng = np.random.default_rng(7100)
    m = 10.0 ** rng.uniform(-6.0, 0.0, f["x"].size)
    r = np.sqrt(f["x"] ** 2 + f["y"] ** 2 + f["z"] ** 2)
    big = int(np.argmin(np.abs(r - 1.0)))  # one scale radius off the centre
    m[big] = 0.0
    m *= 0.1 / m.sum()
    m[big] = 0.9
    f["m"] = m.astype(np.float32)
    return f, list(lim), list(bnd)


MASSLESS_GROUP = 70


def massless():
    """halo_clumps(1e-3), a tight group of 70 bodies with m = 0 (more than one leaf at every bucket size in use: a
    massless internal node, whose expansion centre is (0, 0, 0)) and, last, one body with mass at exactly (0, 0, 0)"""
    f, lim, bnd = halo_clumps(1e-3)
    rng = np.random.default_rng(7200)
    c = np.array([5.0, -3.0, 4.0])
    p = c[:, None] + rng.normal(0.0, 1e-3, (3, MASSLESS_GROUP))
    f = _append(f, p[0], p[1], p[2], np.zeros(MASSLESS_GROUP), np.full(MASSLESS_GROUP, np.float32(1e-3 / 8.0)))
    f = _append(f, [0.0], [0.0], [0.0], [f["m"][0]], [f["h"][0]])
    return f, lim, bnd


def coincident():
    """a Plummer halo in which two pairs of bodies have identical coordinates (r = 0, softened), sixteen bodies sit
    exactly on octree node boundaries lo + k 2^-p L (none at the box centre, which `massless` covers) and three on the
    lower box faces"""
    arr, lim, bnd, _ = ic.plummer(4096, 3)
    f = _fields(arr)
    for a, b in ((10, 11), (2000, 3000)):
        for c in "xyz":
            f[c][b] = f[c][a]
    lo, L = lim[0], lim[1] - lim[0]
    rng = np.random.default_rng(7300)
    for i in range(16):
        p = int(rng.integers(2, 8))
        k = rng.integers(1, 2 ** p, 3)
        k[0] += k[0] == 2 ** (p - 1)  # not the box centre: (0, 0, 0) is the expansion centre of every empty node
        for a, c in enumerate("xyz"):
            f[c][100 + i] = lo + int(k[a]) * 2.0 ** -p * L
    for i, c in enumerate("xyz"):
        f[c][200 + i] = lo
    return f, list(lim), list(bnd)


def off_origin():
    """halo_clumps(1e-3) translated by OFFSET, the box with it"""
    f, lim, bnd = halo_clumps(1e-3)
    for a, c in enumerate("xyz"):
        f[c] = f[c] + OFFSET[a]
        lim[2 * a] += OFFSET[a]
        lim[2 * a + 1] += OFFSET[a]
    return f, lim, bnd


def deep_uniform():
    """a jittered 16^3 lattice in the open unit cube: at one body per leaf the tree has four fully opened internal
    levels under a tiny opening angle"""
    s = 16
    rng = np.random.default_rng(7400)
    g = (np.arange(s) + 0.5) / s
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    n = s ** 3
    f = {c: v.ravel() + rng.uniform(-0.3, 0.3, n) / s for c, v in zip("xyz", (xx, yy, zz))}
    f["m"] = np.full(n, np.float32(1.0 / n))
    f["h"] = np.full(n, np.float32(0.5 / s))
    return f, [0.0, 1.0, 0.0, 1.0, 0.0, 1.0], [0, 0, 0]


def morton_order(f, lim, bits=21):
    """stable order of the bodies along the Morton curve of the box"""
    key = np.zeros(f["x"].size, np.uint64)
    q = []
    for a, c in enumerate("xyz"):
        u = (f[c] - lim[2 * a]) / (lim[2 * a + 1] - lim[2 * a])
        q.append(np.clip((u * 2.0 ** bits).astype(np.int64), 0, 2 ** bits - 1).astype(np.uint64))
    for b in range(bits):
        for a in range(3):
            key |= ((q[a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return np.argsort(key, kind="stable")


def take(f, idx):
    return {k: v[idx].copy() for k, v in f.items()}


def picks(n):
    """the first n bodies of halo_clumps(1e-3) along the Morton curve, in its box"""
    f, lim, bnd = halo_clumps(1e-3)
    return take(f, morton_order(f, lim)[:n]), lim, bnd


def periodic():
    """halo_clumps(1e-3) scaled into the periodic unit cube (lengths, h included, divided by the box length)"""
    f, lim, bnd = halo_clumps(1e-3)
    L = lim[1] - lim[0]
    for a, c in enumerate("xyz"):
        f[c] = (f[c] - lim[2 * a]) / L
    f["h"] = (f["h"].astype(np.float64) / L).astype(np.float32)
    return f, [0.0, 1.0, 0.0, 1.0, 0.0, 1.0], [1, 1, 1]


#: name -> (constructor, number of bodies the case adds at the end of its halo)
CASES = {
    "halo_clumps_1e-2": (lambda: halo_clumps(1e-2), CLUMPS * CLUMP_SIZE),
    "halo_clumps_1e-3": (lambda: halo_clumps(1e-3), CLUMPS * CLUMP_SIZE),
    "halo_clumps_1e-4": (lambda: halo_clumps(1e-4), CLUMPS * CLUMP_SIZE),
    "mass_ratio": (mass_ratio, 0),
    "massless": (massless, CLUMPS * CLUMP_SIZE + MASSLESS_GROUP + 1),
    "coincident": (coincident, 0),
    "off_origin": (off_origin, CLUMPS * CLUMP_SIZE),
    "deep_uniform": (deep_uniform, 0),
}
_cache = {}


def case(name):
    """(f, lim, bnd) of a named case, built once; callers must not modify the arrays"""
    if name not in _cache:
        _cache[name] = CASES[name][0]()
    return _cache[name]


def direct(f, shells=0, L=1.0, targets=None, block=256):
    """direct_ref.direct over blocks of targets (its temporaries are targets x n)"""
    t = np.arange(f["x"].size) if targets is None else np.asarray(targets)
    parts = [dr.direct(f, shells, L=L, targets=t[b:b + block]) for b in range(0, t.size, block)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _p2p_from(d32, f, t):
    """accelerations of the targets t in float64 from float32 displacements d32 = (dx, dy, dz), each targets x n"""
    dx, dy, dz = (d.astype(np.float64) for d in d32)
    hij = f["h"][t, None] + f["h"][None, :]
    hij2 = (hij * hij).astype(np.float64)
    r2 = dx * dx + (dy * dy + dz * dz)
    inv_r = 1.0 / np.sqrt(np.maximum(r2, hij2))
    w = f["m"].astype(np.float64)[None, :] * inv_r * (inv_r * inv_r)
    return np.column_stack([np.sum(dx * w, axis=1), np.sum(dy * w, axis=1), np.sum(dz * w, axis=1)])


def displacement_rounded_once(f, targets, block=256):
    t = np.asarray(targets)
    out = []
    for b in range(0, t.size, block):
        tb = t[b:b + block]
        out.append(_p2p_from([(f[c][None, :] - f[c][tb, None]).astype(np.float32) for c in "xyz"], f, tb))
    return np.concatenate(out)


def origin_rounded(f, order, runs=None, run=64):
    """(targets, accelerations): bodies taken in `order`, `run` consecutive ones share the first one's position as
    origin; source and target are rounded to float relative to it, then subtracted in float.  runs: which runs"""
    n = order.size
    nruns = (n + run - 1) // run
    tt, out = [], []
    for k in (range(nruns) if runs is None else runs):
        tb = order[k * run:(k + 1) * run]
        d = []
        for c in "xyz":
            o = f[c][tb[0]]
            s, g = (f[c] - o).astype(np.float32), (f[c][tb] - o).astype(np.float32)
            d.append(s[None, :] - g[:, None])
        tt.append(tb)
        out.append(_p2p_from(d, f, tb))
    return np.concatenate(tt), np.concatenate(out)


def oracle_state(f, lim, bnd, ora):
    """(state, box) for the CPU oracle, the bodies sorted by its SFC keys; state.order[k] is the index in f of the
    k-th sorted body"""
    import pyoracle as po

    n = f["x"].size
    st = po.HostState(n)
    for k in f:
        st.arrays[k][:] = f[k]
    st.id[:] = np.arange(n, dtype=np.uint64)
    box = po.make_box6(lim, bnd)
    keys = ora.sfc_keys(st, box).copy()
    o = np.argsort(keys, kind="stable")
    for k in po.CONSERVED:
        st.arrays[k][:] = st.arrays[k][o]
    st.keys[:] = keys[o]
    st.order = o
    return st, box


def fields_of(st):
    return {k: st.arrays[k].copy() for k in ("x", "y", "z", "m", "h")}
