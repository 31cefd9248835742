"""The oracle of the binned profiles (include/sphexa_hip.h, "binned profiles and analytic L1 with exact sums"; TEST
INFRASTRUCTURE ONLY).  It restates the section from its header comment alone:

  * per-particle arithmetic in numpy, one rounded operation at a time, in the header's order and bracketing;
  * bins by np.searchsorted(edges, c, side="right") - 1, underflow in entry nbins, overflow in entry nbins + 1;
  * the exact sum of a series in Python integers: window E, fixed(t) = sign(t) floor(|t| 2^(96 - E)), an integer sum, and
    one final rounding through fractions.Fraction (float(Fraction) is correctly rounded, ties to even).

The result has the layout of sphexa_amd.Context.profile: count (uint64), nonfinite, W, and S1, S2, D, min, max of shape
(nq, nbins + 2).
"""
import math
from fractions import Fraction

import numpy as np

import pyoracle as po

ZERO_WINDOW = -1074


# ---- the number format --------------------------------------------------------------------------------------------
def window(terms):
    """the smallest E with max |t| < 2^E; ZERO_WINDOW where every term is 0"""
    m = max((abs(float(t)) for t in terms), default=0.0)
    return math.frexp(m)[1] if m > 0.0 else ZERO_WINDOW  # m = f 2^e with 1/2 <= f < 1


def to_fixed(t, E):
    """sign(t) floor(|t| 2^(96 - E)) as a Python integer"""
    n, d = abs(float(t)).as_integer_ratio()
    sh = 96 - E
    v = (n << sh) // d if sh >= 0 else n // (d << -sh)
    return -v if t < 0 else v


def from_fixed(total, E):
    """the double nearest (ties to even) to total 2^(E - 96)"""
    return float(Fraction(total) * Fraction(2) ** (E - 96))


def exact_sum(terms):
    E = window(terms)
    return from_fixed(sum(to_fixed(t, E) for t in terms), E)


def words(v):
    """a Python integer as the (low, high) words of its 128-bit two's complement"""
    v &= (1 << 128) - 1
    return v & ((1 << 64) - 1), v >> 64


def exact_bin_sums(t, bins, nb2):
    """the exact sums of the terms t per bin (nb2 bins): the same integers as sum(to_fixed), gathered by shift in int64
    halves so that numpy does the per-particle work"""
    t = np.asarray(t, np.float64)
    E = window([np.max(np.abs(t))]) if t.size else ZERO_WINDOW
    out = np.zeros(nb2)
    if E == ZERO_WINDOW:
        return out
    f, e = np.frexp(np.abs(t))
    mant = np.ldexp(f, 53).astype(np.int64)           # |t| = mant 2^(e - 53), exactly
    s = e.astype(np.int64) - 53 + 96 - E              # fixed = mant 2^s, s <= 43
    down = s < 0
    mant = np.where(down, mant >> np.minimum(np.where(down, -s, 0), 63), mant)
    s = np.where(down, 0, s)
    mant = np.where(t < 0, -mant, mant)
    hi, lo = mant >> 26, mant & ((1 << 26) - 1)       # mant = hi 2^26 + lo for either sign
    key = np.asarray(bins, np.int64) * 64 + s
    H, L = np.zeros(nb2 * 64, np.int64), np.zeros(nb2 * 64, np.int64)
    np.add.at(H, key, hi)
    np.add.at(L, key, lo)
    totals = [0] * nb2
    for k in np.flatnonzero((H != 0) | (L != 0)):
        totals[k // 64] += ((int(H[k]) << 26) + int(L[k])) << int(k % 64)
    for b in range(nb2):
        out[b] = from_fixed(totals[b], E)
    return out


# ---- per-particle arithmetic --------------------------------------------------------------------------------------
def displacement(f, lim, bnd, center):
    d = []
    for a, k in enumerate("xyz"):
        da = np.asarray(f[k], np.float64) - np.float64(center[a])
        L = np.float64(lim[2 * a + 1]) - np.float64(lim[2 * a])
        if bnd[a] == 1 and L > 0.0:
            da = da - L * np.rint(da / L)
        d.append(da)
    return d


def quantity(name, f, d, r, std, mui, gamma):
    cv = np.float64(po.ideal_gas_cv(np.float32(mui), gamma))
    gm1 = np.float64(gamma) - 1.0
    if name in ("rho", "p"):
        if std:
            rho = np.asarray(f["rho"], np.float32)
        else:
            rho = (np.asarray(f["kx"], np.float32) * np.asarray(f["m"], np.float32)) / np.asarray(f["xm"], np.float32)
        if name == "rho":
            return rho.astype(np.float64)
        return (rho.astype(np.float64) * ((cv * np.asarray(f["temp"], np.float64)) * gm1)).astype(np.float32).astype(np.float64)
    if name == "u":
        return cv * np.asarray(f["temp"], np.float64)
    if name == "temp":
        return np.asarray(f["temp"], np.float64).copy()
    if name in ("vel", "vrad"):
        vx, vy, vz = (np.asarray(f[k], np.float32).astype(np.float64) for k in ("vx", "vy", "vz"))
        if name == "vel":
            return np.sqrt((vx * vx + vy * vy) + vz * vz)
        num = (d[0] * vx + d[1] * vy) + d[2] * vz
        return np.where(r == 0.0, 0.0, num / np.where(r == 0.0, 1.0, r))
    return np.asarray(f[name], np.float32).astype(np.float64)


def solution(sol, c):
    """sol: ("table", r, y[, rscale]) or ("noh", dict); c finite"""
    if sol[0] == "table":
        r, y = np.asarray(sol[1], np.float64), np.asarray(sol[2], np.float64)
        xi = c * np.float64(sol[3] if len(sol) > 3 else 1.0)
        j = np.clip(np.searchsorted(r, xi, side="right") - 1, 0, r.size - 2)  # the last index with r[j] <= xi
        rj, yj = r[j], y[j]
        with np.errstate(all="ignore"):
            s = ((y[j + 1] - yj) / (r[j + 1] - rj)) * (xi - rj) + yj
        s = np.where(xi == rj, yj, s)
        return np.where(xi < r[0], y[0], np.where(xi >= r[-1], y[-1], s))
    kw = dict(gamma=5.0 / 3.0, rho0=1.0, vel0=-1.0, xgeom=3, rscale=1.0)
    kw.update(sol[1])
    g, rho0, vel0, t, xg = kw["gamma"], kw["rho0"], kw["vel0"], kw["time"], kw["xgeom"]
    xi = c * np.float64(kw["rscale"])
    r2 = 0.5 * (g - 1) * abs(vel0) * t
    behind = rho0 * ((g + 1) / (g - 1)) ** float(xg)
    with np.errstate(all="ignore"):
        b = 1.0 - np.float64(vel0 * t) / np.maximum(xi, 1e-300)
        pw = np.ones_like(b) if xg == 1 else (b if xg == 2 else b * b)
        ahead = np.float64(rho0) * pw
    return np.where(xi > r2, ahead, behind)


def evaluate(f, lim, bnd, quantities, coord="radius", center=(0.0, 0.0, 0.0), weight="number", solutions=None,
             std=False, mui=10.0, gamma=5.0 / 3.0):
    """(c, w, [q], [s or None], finite mask, terms (1 + 3 nq rows)) of every particle"""
    solutions = solutions or {}
    with np.errstate(all="ignore"):
        d = displacement(f, lim, bnd, center)
        r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        c = {"radius": r, "x": d[0], "y": d[1], "z": d[2]}[coord] if coord in ("radius", "x", "y", "z") else \
            quantity(coord, f, d, r, std, mui, gamma)
        w = np.asarray(f["m"], np.float32).astype(np.float64) if weight == "mass" else np.ones(c.size)
        ok = np.isfinite(c) & np.isfinite(w)
        qs, ss, terms = [], [], [w]
        for name in quantities:
            q = quantity(name, f, d, r, std, mui, gamma)
            wq = w * q
            s2 = wq * q
            dev = np.zeros(c.size)
            s = None
            if solutions.get(name) is not None:
                s = solution(solutions[name], np.where(ok, c, 0.0))
                dev = w * np.abs(q - s)
                ok = ok & np.isfinite(s)
            ok = ok & np.isfinite(q) & np.isfinite(wq) & np.isfinite(s2) & np.isfinite(dev)
            qs.append(q), ss.append(s), terms.extend([wq, s2, dev])
    return c, w, qs, ss, ok, terms


def bin_index(edges, c):
    edges = np.asarray(edges, np.float64)
    nb = edges.size - 1
    b = np.searchsorted(edges, c, side="right") - 1
    return np.where(b < 0, nb, np.where(b >= nb, nb + 1, b))


def profile(f, lim, bnd, edges, quantities, **kw):
    """the whole result, the layout of Context.profile"""
    c, w, qs, ss, ok, terms = evaluate(f, lim, bnd, quantities, **kw)
    nb2, nq = len(edges) + 1, len(quantities)
    b = bin_index(edges, c[ok])
    out = {"count": np.bincount(b, minlength=nb2).astype(np.uint64), "nonfinite": np.array([np.sum(~ok)], np.uint64),
           "W": exact_bin_sums(terms[0][ok], b, nb2)}
    for k, key in enumerate(("S1", "S2", "D")):
        out[key] = np.array([exact_bin_sums(terms[1 + 3 * q + k][ok], b, nb2) for q in range(nq)]).reshape(nq, nb2)
    out["min"], out["max"] = np.full((nq, nb2), np.inf), np.full((nq, nb2), -np.inf)
    for q in range(nq):
        np.minimum.at(out["min"][q], b, qs[q][ok])
        np.maximum.at(out["max"][q], b, qs[q][ok])
    return out


def l1(res, k=0):
    """(sum over all entries of D_k) / (sum of W), both in ascending index"""
    d = wsum = 0.0
    for v in res["D"][k]:
        d += float(v)
    for v in res["W"]:
        wsum += float(v)
    return d / wsum
