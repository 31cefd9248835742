"""The oracle of the two-point statistics (include/sphexa_hip.h, "two-point statistics: pair counts and velocity structure
functions"; TEST INFRASTRUCTURE ONLY).  It restates the section from its header comment alone:

  * every unordered pair of the range in numpy, O(n^2), one rounded operation at a time, in the header's order and
    bracketing; no grid, no cut-off other than the bins;
  * bins by np.searchsorted(edges, r, side="right") - 1;
  * the exact sum of a series in Python integers: the windows from vmax and mmax, fixed(t) = sign(t) floor(|t| 2^(64 - E)),
    an integer sum per bin, and one final rounding through fractions.Fraction (float(Fraction) is correctly rounded, ties
    to even).

The result has the keys of sphexa_amd.Context.twopoint's raw arrays: count (uint64), U1 U2 U3 A3 T2 WW (float64, None where
the series is off), targets, nonfinite, coincident, and pairs, the number of binned pairs.
"""
import math
from fractions import Fraction

import numpy as np

ZERO_WINDOW = -1074
SERIES = ("U1", "U2", "U3", "A3", "T2", "WW")
FLAGS = {k: 1 << i for i, k in enumerate(SERIES)}
VEL, ALL = 31, 63


# ---- the number format ---------------------------------------------------------------------------------------------
def window(terms):
    """the smallest integer E with max |t| < 2^E; ZERO_WINDOW where every term is 0"""
    m = max((abs(float(t)) for t in terms), default=0.0)
    return math.frexp(m)[1] if m > 0.0 else ZERO_WINDOW  # m = f 2^e with 1/2 <= f < 1


def to_fixed(t, E):
    """sign(t) floor(|t| 2^(64 - E)) as a Python integer"""
    n, d = abs(float(t)).as_integer_ratio()
    sh = 64 - E
    v = (n << sh) // d if sh >= 0 else n // (d << -sh)
    return -v if t < 0 else v


def from_fixed(total, E):
    """the double nearest (ties to even) to total 2^(E - 64)"""
    return float(Fraction(total) * Fraction(2) ** (E - 64))


def words(v):
    """a Python integer as the (low, high) words of its 128-bit two's complement"""
    v &= (1 << 128) - 1
    return v & ((1 << 64) - 1), v >> 64


def windows(vmax, mmax):
    """the windows of the six series from the largest |velocity component| and |mass| of the finite particles"""
    eu = window([vmax]) + 2
    em = window([mmax])
    return {"U1": eu, "U2": 2 * eu, "U3": 3 * eu, "A3": 3 * eu, "T2": 2 * eu, "WW": 2 * em}


def bin_sums(t, bins, nb, E):
    """the exact sums of the terms t per bin, rounded once: the same integers as sum(to_fixed(t, E)), with the mantissas
    and exponents taken apart by numpy (frexp is exact) and the shifts and sums done on Python integers"""
    t = np.asarray(t, np.float64)
    frac, ex = np.frexp(np.abs(t))
    mant = (frac * 2.0 ** 53).astype(np.int64).tolist()  # exact: |t| = mant 2^(ex - 53)
    shift = (ex.astype(np.int64) - 53 + 64 - E).tolist()
    neg = (t < 0).tolist()
    acc = [0] * nb
    for mk, sk, ng, b in zip(mant, shift, neg, np.asarray(bins).tolist()):
        v = mk << sk if sk >= 0 else mk >> -sk
        acc[b] += -v if ng else v
    return np.array([from_fixed(a, E) for a in acc], np.float64), acc


# ---- the pairs ---------------------------------------------------------------------------------------------------
def min_image(d, L, periodic):
    """L added or subtracted once where |d| > L / 2 on a periodic axis"""
    if not periodic:
        return d
    half = 0.5 * L
    return np.where(d > half, d - L, np.where(d < -half, d + L, d))


def pairs(f, lim, bnd, edges, stride=1, phase=0, ids=None, first=0, last=None, mass=False):
    """every pair of the definition that falls into a bin: dict of i, j (indices into the range), bin, r, dx, dy, dz; and
    the totals"""
    n_all = len(f["x"])
    last = n_all if last is None else last
    sl = slice(first, last)
    pos = [np.asarray(f[k], np.float64)[sl] for k in "xyz"]
    vel = [np.asarray(f[k], np.float32)[sl].astype(np.float64) for k in ("vx", "vy", "vz")]
    fin = np.ones(last - first, bool)
    for a in pos + vel:
        fin &= np.isfinite(a)
    if mass:
        fin &= np.isfinite(np.asarray(f["m"], np.float32)[sl].astype(np.float64))
    key = np.asarray(ids, np.uint64)[sl] if ids is not None else np.arange(first, last, dtype=np.uint64)
    tgt = (key % np.uint64(stride)) == np.uint64(phase)
    idx = np.flatnonzero(fin)
    edges = np.asarray(edges, np.float64)
    nb = len(edges) - 1
    L = [lim[2 * a + 1] - lim[2 * a] for a in range(3)]
    out = {k: [] for k in ("i", "j", "bin", "r", "dx", "dy", "dz")}
    coincident = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for q, i in enumerate(idx[:-1]):
            j = idx[q + 1:]
            d = [min_image(pos[a][j] - pos[a][i], L[a], bnd[a] == 1) for a in range(3)]
            r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            take = tgt[j] | tgt[i]
            coincident += int(np.count_nonzero(take & (r2 == 0.0)))
            r = np.sqrt(r2)
            ok = take & (r2 != 0.0) & (r >= edges[0]) & (r < edges[nb])
            if not ok.any():
                continue
            out["i"].append(np.full(int(ok.sum()), i))
            out["j"].append(j[ok])
            out["bin"].append(np.searchsorted(edges, r[ok], side="right") - 1)
            out["r"].append(r[ok])
            for a, k in enumerate(("dx", "dy", "dz")):
                out[k].append(d[a][ok])
    out = {k: (np.concatenate(v) if v else np.zeros(0, np.int64 if k in ("i", "j", "bin") else np.float64))
           for k, v in out.items()}
    totals = {"targets": int(np.count_nonzero(fin & tgt)), "nonfinite": int(np.count_nonzero(~fin)),
              "coincident": coincident, "finite": fin, "target": tgt}
    return out, totals, vel


def twopoint(f, lim, bnd, edges, series=ALL, stride=1, phase=0, ids=None, first=0, last=None):
    """the series of the header comment for the particles [first, last) of the host columns f"""
    mass = bool(series & FLAGS["WW"])
    pr, tot, vel = pairs(f, lim, bnd, edges, stride, phase, ids, first, last, mass)
    nb = len(edges) - 1
    i, j, b = pr["i"], pr["j"], pr["bin"]
    res = {"count": np.bincount(b, minlength=nb).astype(np.uint64), "targets": tot["targets"],
           "nonfinite": tot["nonfinite"], "coincident": tot["coincident"], "pairs": int(len(b))}
    fin = tot["finite"]
    vmax = max((float(np.max(np.abs(v[fin]))) for v in vel), default=0.0) if fin.any() else 0.0
    mmax = 0.0
    if mass:
        m = np.asarray(f["m"], np.float32)[first:last if last is not None else len(f["x"])].astype(np.float64)
        mmax = float(np.max(np.abs(m[fin]))) if fin.any() else 0.0
    E = windows(vmax, mmax)
    res["windows"] = E
    terms = {}
    if series & VEL:
        dv = [v[j] - v[i] for v in vel]
        u = ((dv[0] * pr["dx"] + dv[1] * pr["dy"]) + dv[2] * pr["dz"]) / pr["r"]
        u2 = u * u
        u3 = u2 * u
        terms.update(U1=u, U2=u2, U3=u3, A3=np.abs(u3), T2=(dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
        res["u"] = u
    if mass:
        terms["WW"] = m[i] * m[j]
    res["integers"] = {}
    for k in SERIES:
        if series & FLAGS[k]:
            res[k], res["integers"][k] = bin_sums(terms[k], b, nb, E[k])
        else:
            res[k] = None
    res["r"], res["bin"] = pr["r"], b
    return res


def assert_same(got, ref, series=ALL):
    """every array and total of a device result (the dict of Context.twopoint) equal to the oracle's, bit for bit"""
    assert np.array_equal(got["count"], ref["count"]), (got["count"], ref["count"])
    for k in ("targets", "nonfinite", "coincident"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in SERIES:
        if series & FLAGS[k]:
            assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
        else:
            assert got[k] is None


# ---- inputs ------------------------------------------------------------------------------------------------------
PERIODIC = ([0.0, 1.0, 0.0, 1.0, 0.0, 1.0], [1, 1, 1])
OPEN = ([0.0, 1.0, 0.0, 1.0, 0.0, 1.0], [0, 0, 0])
MIXED = ([-0.5, 0.5, 0.0, 2.0, -1.0, 0.5], [1, 0, 2])


def columns(pos, seed=0, vscale=1.0, mdecades=0.0):
    """host columns x y z (float64) vx vy vz m (float32) for the positions pos (n, 3)"""
    rng = np.random.default_rng(seed)
    n = len(pos)
    f = {k: np.ascontiguousarray(pos[:, a], np.float64) for a, k in enumerate("xyz")}
    for k in ("vx", "vy", "vz"):
        f[k] = (vscale * rng.standard_normal(n)).astype(np.float32)
    f["m"] = (10.0 ** (mdecades * rng.random(n)) / max(1, n)).astype(np.float32)
    return f


def uniform(n, box=PERIODIC, seed=0, **kw):
    lim = box[0]
    rng = np.random.default_rng(seed)
    pos = np.stack([lim[2 * a] + (lim[2 * a + 1] - lim[2 * a]) * rng.random(n) for a in range(3)], axis=1)
    return columns(pos, seed + 1, **kw)


def clumpy(n=3000, box=PERIODIC, seed=5, clump=0.4, sigma=0.02, outside=0, **kw):
    """a clump of clump n particles (a Gaussian of width sigma of the shortest extent) in a sparse uniform background;
    `outside` background particles are pushed beyond the faces of the open axes"""
    lim, bnd = box
    rng = np.random.default_rng(seed)
    ext = np.array([lim[2 * a + 1] - lim[2 * a] for a in range(3)])
    lo = np.array([lim[2 * a] for a in range(3)])
    nc = int(clump * n)
    pos = lo + ext * rng.random((n, 3))
    pos[:nc] = lo + 0.3 * ext + sigma * ext.min() * rng.standard_normal((nc, 3))
    for a in range(3):
        if bnd[a] == 1:
            pos[:, a] = lo[a] + np.mod(pos[:, a] - lo[a], ext[a])
    for k in range(outside):
        a = [q for q in range(3) if bnd[q] != 1][k % max(1, sum(1 for q in range(3) if bnd[q] != 1))]
        pos[nc + k, a] = lo[a] - 0.01 * ext[a] * (1 + k) if k % 2 else lo[a] + ext[a] * (1 + 0.01 * (1 + k))
    return columns(pos, seed + 1, **kw)


def lattice(k=8, a=1.0 / 8):
    """a simple cubic lattice of k^3 points with spacing a, at the cell centres of the box [0, k a)^3"""
    g = (np.arange(k) + 0.5) * a
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return pos
