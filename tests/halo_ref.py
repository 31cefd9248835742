"""The oracle of the group properties (sx_halo): numpy only, on top of fof_ref.fof, written from the definitions in
include/sphexa_hip.h and not from the device code.

Selection: rho >= rho_min with rho the float (kx * m) / xm, or the float column rho (std); a NaN is not selected; the
unselected particles are taken out before fof_ref.fof sees the columns, and get the label 2^64 - 1.
Moments about (X, V, M) = (com, vel, mass) -- the oracle's own, or `about`, the device's returned ones: these are held to
the bound of the group search already, so a comparison about the device's values is a pure summation bound,
4 N_g 2^-53 sum |term| (/ M) plus 2^-51 of the magnitude for the final division.  The terms themselves are written with
the brackets of the header, so both sides round every term alike.
Potential: O(c^2) per group in float64, W = sum_{i<j} m_i m_j r^2 / r_eff^3 with r_eff^2 = max(r^2, (h_i + h_j)^2) and
h_i + h_j a float sum; epot = -G W; a pair with r^2 = 0 contributes 0.  The contract is |epot - (-G W)| <= 2^-15 G W.
"""
import numpy as np

import fof_ref as fr

EPS = 2.0 ** -53
NONE = np.uint64(np.iinfo(np.uint64).max)
CONTRACT = 2.0 ** -15
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx xy xz yy yz zz


def density(f, std):
    if std:
        return np.asarray(f["rho"], np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.asarray(f["kx"], np.float32) * np.asarray(f["m"], np.float32)) / np.asarray(f["xm"], np.float32)


def selected(f, rho_min, std, n):
    if not rho_min > 0.0:
        return np.ones(n, bool)
    return density(f, std).astype(np.float64) >= rho_min  # a NaN compares false


def pair_energy(x, y, z, m, h, lim, bnd, block=1024):
    """W and the numbers of softened and unsoftened pairs (r > 0) of the members given in float64 (h, m: float32)"""
    c = len(x)
    m64 = m.astype(np.float64)
    W, soft, hard = 0.0, 0, 0
    for lo in range(0, c, block):
        hi = min(c, lo + block)
        r2 = np.zeros((hi - lo, c))
        for a, p in enumerate((x, y, z)):
            d = fr.min_image(p[None, :] - p[lo:hi, None], lim[2 * a + 1] - lim[2 * a], bnd[a] == 1)
            r2 += d * d
        hij = h[lo:hi, None] + h[None, :]  # float32
        h2 = (hij * hij).astype(np.float64)
        upper = np.arange(c)[None, :] > np.arange(lo, hi)[:, None]
        use = upper & (r2 > 0.0)
        re2 = np.where(use, np.maximum(r2, h2), 1.0)
        term = np.where(use, m64[lo:hi, None] * m64[None, :] * r2 / (re2 * np.sqrt(re2)), 0.0)
        W += float(np.sum(term))
        soft += int(np.count_nonzero(use & (r2 < h2)))
        hard += int(np.count_nonzero(use & (r2 >= h2)))
    return W, soft, hard


def moments(x, y, z, m, v, X, V, M, lim, bnd):
    """sigma, shape (6), angmom (3), rmax and their tolerances for members in ascending id about (X, V, M)"""
    n = len(x)
    d = [fr.min_image(p - X[a], lim[2 * a + 1] - lim[2 * a], bnd[a] == 1) for a, p in enumerate((x, y, z))]
    w = [v[a].astype(np.float64) - V[a] for a in range(3)]
    m = m.astype(np.float64)
    bound = 4.0 * n * EPS
    sigma, shape, sig_tol, shp_tol = np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6)
    for k, (a, b) in enumerate(PAIRS):
        t = (m * w[a]) * w[b]
        sigma[k] = t.sum() / M
        sig_tol[k] = bound * np.abs(t).sum() / M + 4 * EPS * abs(sigma[k])
        t = (m * d[a]) * d[b]
        shape[k] = t.sum() / M
        shp_tol[k] = bound * np.abs(t).sum() / M + 4 * EPS * abs(shape[k])
    ang, ang_tol = np.zeros(3), np.zeros(3)
    for k, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
        t = m * ((d[a] * w[b]) - (d[b] * w[a]))
        ang[k] = t.sum()
        ang_tol[k] = bound * np.abs(t).sum() + 4 * EPS * abs(ang[k])
    rmax = np.sqrt(np.max((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return sigma, shape, ang, rmax, sig_tol, shp_tol, ang_tol


def halo(f, lim, bnd, ell, ids=None, first=0, last=None, min_members=20, max_groups=4096, rho_min=0.0, std=False,
         G=1.0, cv=None, max_pair_members=0, about=None, potential=True):
    """the dict of Context.halos for the particles [first, last) of the columns f, plus per entry the tolerances
    sigma_tol, shape_tol, angmom_tol, eint_tol, W (the exact pair sum), soft and hard (pairs per branch), and what
    fof_ref.fof adds.  about: a dict with the device's mass, com, vel to take the moments about."""
    n_all = len(f["x"])
    last = n_all if last is None else last
    n = last - first
    sl = slice(first, last)
    cols = {k: np.asarray(v)[sl] for k, v in f.items()}
    idv = np.asarray(ids, np.uint64)[sl] if ids is not None else np.arange(first, last, dtype=np.uint64)
    sel = selected(cols, rho_min, std, n)
    sub = {k: v[sel] for k, v in cols.items()}
    out = fr.fof(sub, lim, bnd, ell, ids=idv[sel], min_members=min_members, max_groups=max_groups)
    label = np.full(n, NONE, np.uint64)
    label[sel] = out["label"]
    sub_label = out["label"]
    out["label"] = label
    out["selected"] = sel
    k = len(out["count"])
    cap = max_pair_members if max_pair_members else 1 << 20
    res = {key: np.zeros((k,) + tail) for key, tail in (("sigma", (6,)), ("shape", (6,)), ("angmom", (3,)), ("rmax", ()),
                                                         ("eint", ()), ("epot", ()), ("W", ()), ("sigma_tol", (6,)),
                                                         ("shape_tol", (6,)), ("angmom_tol", (3,)), ("eint_tol", ()))}
    res["soft"], res["hard"] = np.zeros(k, np.int64), np.zeros(k, np.int64)
    sid = idv[sel]
    order = np.lexsort((sid, sub_label))  # by group, then by id
    starts = np.searchsorted(sub_label[order], out["group_label"])
    for g in range(k):
        mem = order[starts[g]:starts[g] + int(out["count"][g])]
        x, y, z = (np.asarray(sub[c], np.float64)[mem] for c in "xyz")
        m = np.asarray(sub["m"], np.float32)[mem]
        v = [np.asarray(sub[c], np.float32)[mem] for c in ("vx", "vy", "vz")]
        src = about if about is not None else out
        M, X, V = src["mass"][g], src["com"][g], src["vel"][g]
        (res["sigma"][g], res["shape"][g], res["angmom"][g], res["rmax"][g], res["sigma_tol"][g], res["shape_tol"][g],
         res["angmom_tol"][g]) = moments(x, y, z, m, v, X, V, M, lim, bnd)
        if cv is not None:
            t = m.astype(np.float64) * (cv * np.asarray(sub["temp"], np.float64)[mem])
            res["eint"][g] = t.sum()
            res["eint_tol"][g] = 4.0 * len(mem) * EPS * np.abs(t).sum() + 4 * EPS * abs(res["eint"][g])
        if potential and "h" in sub:
            if len(mem) > cap:
                res["epot"][g] = res["W"][g] = np.nan
            else:
                W, soft, hard = pair_energy(x, y, z, m, np.asarray(sub["h"], np.float32)[mem], lim, bnd)
                res["W"][g], res["soft"][g], res["hard"][g] = W, soft, hard
                res["epot"][g] = -(float(np.float32(G)) * W)
    out.update(res)
    c = out["count"].astype(np.int64)
    out["pair_terms"] = int(np.sum(np.where(c <= cap, c * (c - 1) // 2, 0)))
    return out


def assert_properties(got, ref, thermal=False, potential=True):
    """the comparison the GPU tests share: ref is halo(..., about=got)"""
    for key in ("sigma", "shape", "angmom"):
        err = np.abs(got[key] - ref[key])
        print(key, "max err / tol", float(np.max(err / np.maximum(ref[key + "_tol"], 1e-300), initial=0.0)))
        assert np.all(err <= ref[key + "_tol"]), (key, err.max())
    assert np.all(np.abs(got["rmax"] - ref["rmax"]) <= 2.0 ** -52 * ref["rmax"]), "rmax: the exact maximum, one sqrt"
    if thermal:
        assert np.all(np.abs(got["eint"] - ref["eint"]) <= ref["eint_tol"])
    if potential:
        ok = np.isfinite(ref["epot"])
        assert np.array_equal(np.isnan(got["epot"]), ~ok)
        rel = np.abs(got["epot"][ok] - ref["epot"][ok]) / np.maximum(np.abs(ref["epot"][ok]), 1e-300)
        print("epot: max relative error", float(np.max(rel, initial=0.0)), "contract", CONTRACT)
        assert np.all(np.abs(got["epot"][ok] - ref["epot"][ok]) <= CONTRACT * np.abs(ref["epot"][ok]))


# ---- the inputs the tests share ------------------------------------------------------------------------------------

def ball(rng, n, centre, radius):
    v = rng.standard_normal((n, 3))
    v *= (radius * rng.random(n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return np.asarray(centre)[None, :] + v


def tile_edge_state(seed=11, radius=0.004):
    """groups of 513, 257, 256, 255, 2 and 1 members as tight balls far apart in the periodic unit box, and one of 40
    astride the corner (0, 0, 0); h such that both branches occur; shuffled.  Returns (columns, linking length, the
    counts in catalogue order)"""
    rng = np.random.default_rng(seed)
    sizes = [513, 257, 256, 255, 2, 1, 40]
    centres = [(0.2, 0.2, 0.2), (0.7, 0.2, 0.3), (0.2, 0.7, 0.4), (0.7, 0.7, 0.6), (0.45, 0.45, 0.8), (0.5, 0.1, 0.9),
               (0.0, 0.0, 0.0)]
    p = np.concatenate([ball(rng, c, ctr, radius) for c, ctr in zip(sizes, centres)])
    p = np.mod(p, 1.0)
    n = len(p)
    f = {"x": p[:, 0].copy(), "y": p[:, 1].copy(), "z": p[:, 2].copy()}
    fr.with_dynamics(f, seed)
    f["h"] = (rng.integers(1, 64, n).astype(np.float64) * 2.0 ** -14).astype(np.float32)  # 6e-5 .. 3.8e-3
    perm = rng.permutation(n)
    return {k: v[perm] for k, v in f.items()}, 2.0 * radius, sorted(sizes, reverse=True)


def bridge_state(seed=12, std=False):
    """two dense balls of 60 joined by a chain of 21 particles 0.8 l apart; the density columns put the balls at 10 and
    the chain at 1 (one chain particle: NaN).  Returns (columns, linking length, chain mask)"""
    rng = np.random.default_rng(seed)
    ell = 0.01
    a, b = np.array([0.3, 0.5, 0.5]), np.array([0.3 + 22 * 0.8 * ell, 0.5, 0.5])
    chain = a[None, :] + np.outer(np.arange(1, 22) * 0.8 * ell, [1.0, 0.0, 0.0])
    p = np.concatenate([ball(rng, 60, a, 0.6 * ell), ball(rng, 60, b, 0.6 * ell), chain])
    n = len(p)
    is_chain = np.arange(n) >= 120
    f = {"x": p[:, 0].copy(), "y": p[:, 1].copy(), "z": p[:, 2].copy()}
    fr.with_dynamics(f, seed)
    f["h"] = np.full(n, 0.002, np.float32)
    rho = np.where(is_chain, 1.0, 10.0).astype(np.float32)
    rho[125] = np.nan
    if std:
        f["rho"] = rho
    else:
        f["kx"] = np.full(n, 2.0, np.float32)
        f["xm"] = (f["kx"] * f["m"] / rho).astype(np.float32)
    perm = rng.permutation(n)
    return {k: v[perm] for k, v in f.items()}, ell, is_chain[perm]
