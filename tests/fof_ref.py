"""The friends-of-friends oracle: numpy only, written from the definition in include/sphexa_hip.h and not from the device
code (its own cell list, min-label hooking with pointer jumping, plain numpy sums).

Link: i != j are friends iff dx^2 + dy^2 + dz^2 < l^2 (strict), d_a the minimum image on axes with bnd == 1 and the plain
difference on open (0) and fixed (2) axes.  Groups: connected components.  Label: the smallest id (or index) of a group.
Catalogue: groups of min_members or more by count descending, label ascending; mass, centre of mass relative to the label
particle, mass-weighted velocity.

The partition is a property of the particle set as long as no pair sits on the criterion: near_ties() counts the pairs
with |d^2 / l^2 - 1| < 1e-9, and every comparison of labels first asserts that it is 0 -- a condition on the inputs, not
a tolerance.
"""
import numpy as np

EPS = 2.0 ** -53


def min_image(d, L, periodic):
    if not periodic:
        return d
    return np.where(d > 0.5 * L, d - L, np.where(d < -0.5 * L, d + L, d))


def _cells(pos, lim, bnd, ell, cap=48):
    """cell coordinates (n, 3) and cells per axis: edge >= ell, particles outside an open box in the edge cells"""
    n = len(pos[0])
    dims, c = [], np.zeros((n, 3), np.int64)
    for a in range(3):
        lo, L = lim[2 * a], lim[2 * a + 1] - lim[2 * a]
        d = int(min(cap, max(3 if bnd[a] == 1 else 1, np.floor(L / ell * (1 - 1e-6)) if L > 0 else 1)))
        t = np.floor((pos[a] - lo) / L * d).astype(np.int64) if L > 0 else np.zeros(n, np.int64)
        c[:, a] = np.mod(t, d) if bnd[a] == 1 else np.clip(t, 0, d - 1)
        dims.append(d)
    return c, dims


def candidate_pairs(pos, lim, bnd, ell, block=1 << 22):
    """yields (i, j, d2) with i < j for every pair of particles in the same or in adjacent cells, in blocks"""
    n = len(pos[0])
    if n < 2:
        return
    c, dims = _cells(pos, lim, bnd, ell)
    key = c[:, 0] + dims[0] * (c[:, 1] + dims[1] * c[:, 2])
    order = np.argsort(key, kind="stable")
    skey = key[order]
    ncell = dims[0] * dims[1] * dims[2]
    start = np.searchsorted(skey, np.arange(ncell + 1))
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                nb, ok = np.zeros((n, 3), np.int64), np.ones(n, bool)
                for a, o in enumerate((ox, oy, oz)):
                    t = c[:, a] + o
                    if bnd[a] == 1:
                        t = np.mod(t, dims[a])
                    else:
                        ok &= (t >= 0) & (t < dims[a])
                        t = np.clip(t, 0, dims[a] - 1)
                    nb[:, a] = t
                nkey = nb[:, 0] + dims[0] * (nb[:, 1] + dims[1] * nb[:, 2])
                cnt = np.where(ok, start[nkey + 1] - start[nkey], 0)
                who = np.flatnonzero(cnt)
                lo = 0
                while lo < len(who):
                    hi = lo + max(1, int(np.searchsorted(np.cumsum(cnt[who[lo:]]), block)))
                    sel = who[lo:hi]
                    k = cnt[sel]
                    i = np.repeat(sel, k)
                    off = np.arange(k.sum()) - np.repeat(np.cumsum(k) - k, k)
                    j = order[np.repeat(start[nkey[sel]], k) + off]
                    keep = i < j
                    i, j = i[keep], j[keep]
                    d2 = np.zeros(len(i))
                    for a in range(3):
                        d = min_image(pos[a][i] - pos[a][j], lim[2 * a + 1] - lim[2 * a], bnd[a] == 1)
                        d2 = d2 + d * d if a else d * d
                    yield i, j, d2
                    lo = hi


def links(pos, lim, bnd, ell):
    """(i, j) of every friend pair, i < j, and the number of near ties among the candidates"""
    li, lj, ties = [], [], 0
    for i, j, d2 in candidate_pairs(pos, lim, bnd, ell):
        ties += int(np.count_nonzero(np.abs(d2 / (ell * ell) - 1.0) < 1e-9))
        f = d2 < ell * ell
        li.append(i[f])
        lj.append(j[f])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return cat(li), cat(lj), ties


def near_ties(pos, lim, bnd, ell):
    """pairs with |d^2 / l^2 - 1| < 1e-9: the partition of such an input may depend on how d^2 is rounded"""
    return links(pos, lim, bnd, ell)[2]


def components(n, i, j):
    """root[k] = the smallest index of k's component: hook the larger root under the smaller, jump, repeat"""
    lab = np.arange(n, dtype=np.int64)
    while True:
        a, b = lab[i], lab[j]
        if np.array_equal(a, b):
            return lab
        np.minimum.at(lab, np.maximum(a, b), np.minimum(a, b))
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def fof(f, lim, bnd, ell, ids=None, first=0, last=None, min_members=20, max_groups=4096):
    """the groups of the particles [first, last) of the columns f (x, y, z; m, vx, vy, vz for the catalogue).  Returns the
    dict of Context.fof plus links, ties and, per catalogue entry, com_tol and vel_tol (k, 3): the summation bound
    4 N_g 2^-53 sum |term| of both sides' orders divided by M, and 2^-51 of the magnitudes that the division, the addition
    of the reference point and the fold round once more on either side."""
    n_all = len(f["x"])
    last = n_all if last is None else last
    sl = slice(first, last)
    pos = [np.asarray(f[k], np.float64)[sl] for k in "xyz"]
    n = last - first
    idv = (np.asarray(ids, np.uint64)[sl] if ids is not None else np.arange(first, last, dtype=np.uint64))
    li, lj, ties = links(pos, lim, bnd, ell)
    root = components(n, li, lj)
    minid = np.full(n, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(minid, root, idv)
    label = minid[root]
    roots, counts = np.unique(root, return_counts=True)
    out = {"label": label, "num_all": len(roots), "links": len(li), "ties": ties}
    sel = counts >= max(1, min_members)
    out["num_groups"] = int(sel.sum())
    roots, counts = roots[sel], counts[sel]
    glabel = minid[roots]
    o = np.lexsort((glabel, -counts.astype(np.int64)))[:max_groups]
    roots, counts, glabel = roots[o], counts[o], glabel[o]
    out["group_label"], out["count"] = glabel, counts.astype(np.uint32)
    k = len(roots)
    mass, com, vel = np.zeros(k), np.zeros((k, 3)), np.zeros((k, 3))
    com_tol, vel_tol = np.zeros((k, 3)), np.zeros((k, 3))
    if k and "m" in f:
        m_all = np.asarray(f["m"])[sl].astype(np.float64)
        v_all = [np.asarray(f[c])[sl].astype(np.float64) for c in ("vx", "vy", "vz")]
        by_root = np.argsort(root, kind="stable")
        rstart = np.searchsorted(root[by_root], roots)
        for g in range(k):
            mem = by_root[rstart[g]:rstart[g] + counts[g]]
            mem = mem[np.argsort(idv[mem], kind="stable")]
            m = m_all[mem]
            M = m.sum()
            mass[g] = M
            bound = 4.0 * len(mem) * EPS
            for a in range(3):
                L, per = lim[2 * a + 1] - lim[2 * a], bnd[a] == 1
                ref = pos[a][mem[0]]
                term = m * min_image(pos[a][mem] - ref, L, per)
                c = ref + term.sum() / M
                if per:
                    c = c + L if c < lim[2 * a] else c - L if c >= lim[2 * a + 1] else c
                com[g, a] = c
                com_tol[g, a] = bound * np.abs(term).sum() / M + 4 * EPS * (abs(ref) + abs(term.sum() / M) + (abs(L) if per else 0))
                tv = m * v_all[a][mem]
                vel[g, a] = tv.sum() / M
                vel_tol[g, a] = bound * np.abs(tv).sum() / M + 4 * EPS * abs(vel[g, a])
    out.update(mass=mass, com=com, vel=vel, com_tol=com_tol, vel_tol=vel_tol)
    return out


# ---- the comparison the GPU tests share ------------------------------------------------------------------------

def assert_same(got, ref, box, exact_mass=True):
    assert ref["ties"] == 0, "the input has pairs on the criterion: the partition may depend on rounding"
    assert got["num_all"] == ref["num_all"] and got["num_groups"] == ref["num_groups"]
    if got["label"] is not None:
        assert np.array_equal(got["label"], ref["label"]), np.flatnonzero(got["label"] != ref["label"])[:8]
    assert np.array_equal(got["group_label"], ref["group_label"])
    assert np.array_equal(got["count"], ref["count"])
    if exact_mass:
        assert np.array_equal(got["mass"].view(np.uint64), ref["mass"].view(np.uint64))
    lim, bnd = box
    d = got["com"] - ref["com"]
    for a in range(3):  # positions on a periodic axis are equal modulo the period
        d[:, a] = min_image(d[:, a], lim[2 * a + 1] - lim[2 * a], bnd[a] == 1)
    print("com: max |d| / tol", float(np.max(np.abs(d) / ref["com_tol"], initial=0.0)),
          "vel:", float(np.max(np.abs(got["vel"] - ref["vel"]) / ref["vel_tol"], initial=0.0)))
    assert np.all(np.abs(d) <= ref["com_tol"]), (np.abs(d).max(), ref["com_tol"].min())
    assert np.all(np.abs(got["vel"] - ref["vel"]) <= ref["vel_tol"])


# ---- the inputs the tests share ------------------------------------------------------------------------------------

PERIODIC = ([0.0, 1.0, 0.0, 1.0, 0.0, 1.0], [1, 1, 1])
OPEN = ([0.0, 1.0, 0.0, 1.0, 0.0, 1.0], [0, 0, 0])
MIXED = ([-0.5, 0.5, 0.0, 2.0, -1.0, 0.5], [1, 0, 2])


def clustered(n=20000, blobs=40, sigma=0.01, box=PERIODIC, seed=7, outside=0):
    """half the particles in Gaussian blobs of width sigma (times the box's shortest side), half uniform, shuffled;
    `outside` of them moved beyond the faces of the open axes.  Columns x, y, z (float64), m in [0.5, 1.5) / n and
    vx, vy, vz (float32)."""
    rng = np.random.default_rng(seed)
    lim, bnd = box
    lo, L = np.array(lim[0::2]), np.array(lim[1::2]) - np.array(lim[0::2])
    nb = n // 2
    centres = rng.random((blobs, 3))
    u = np.concatenate([centres[rng.integers(0, blobs, nb)] + sigma * L.min() / L * rng.standard_normal((nb, 3)),
                        rng.random((n - nb, 3))])
    u = u[rng.permutation(n)]
    for a in range(3):
        if bnd[a] == 1:
            u[:, a] = np.mod(u[:, a], 1.0)
    x = lo + L * u
    for a in range(3):
        if bnd[a] == 1:
            x[:, a] = np.where(x[:, a] >= lim[2 * a + 1], lim[2 * a], x[:, a])  # the rounding of lo + L u
    open_axes = [a for a in range(3) if bnd[a] != 1]
    if outside and open_axes:
        who = rng.choice(n, outside, replace=False)
        for k, p in enumerate(who):
            a = open_axes[k % len(open_axes)]
            x[p, a] = lim[2 * a + (k // len(open_axes)) % 2] + (0.3 * L[a] * rng.random() + 1e-3) * (1 if (k // len(open_axes)) % 2 else -1)
    f = {"x": x[:, 0].copy(), "y": x[:, 1].copy(), "z": x[:, 2].copy()}
    f["m"] = (rng.uniform(0.5, 1.5, n).astype(np.float32) / np.float32(n)).astype(np.float32)
    for c in ("vx", "vy", "vz"):
        f[c] = rng.standard_normal(n).astype(np.float32)
    return f


def mean_spacing_length(n, box, linking=0.2):
    lim = box[0]
    vol = (lim[1] - lim[0]) * (lim[3] - lim[2]) * (lim[5] - lim[4])
    return linking * (vol / n) ** (1.0 / 3.0)


def with_dynamics(f, seed=1):
    """m, vx, vy, vz for columns that have positions only"""
    n, rng = len(f["x"]), np.random.default_rng(seed)
    f["m"] = (rng.uniform(0.5, 1.5, n).astype(np.float32) / np.float32(max(n, 1))).astype(np.float32)
    for c in ("vx", "vy", "vz"):
        f[c] = rng.standard_normal(n).astype(np.float32)
    return f


def helix(n=4097, ell=0.01, spacing=0.9, seed=3):
    """n points along a helix that winds round the periodic x axis of the unit box, `spacing` l apart, shuffled: one
    group with n - 1 links (the ends do not meet)"""
    s = spacing * ell * np.arange(n)
    # turns are 6 l apart along x; after the wrap (16.7 turns per box length) they fall 2 l and 4 l from earlier ones
    radius, pitch = 0.2, 0.06
    w = 1.0 / np.hypot(2 * np.pi * radius, pitch)
    t = s * w
    x = np.mod(0.3 + pitch * t, 1.0)
    y = 0.5 + radius * np.cos(2 * np.pi * t)
    z = 0.5 + radius * np.sin(2 * np.pi * t)
    p = np.random.default_rng(seed).permutation(n)
    return with_dynamics({"x": x[p], "y": y[p], "z": z[p]})


def dense_ball(n=3000, ell=0.05, seed=4):
    """n points in a ball of radius l / 8 inside one cell: one group, n (n - 1) / 2 friend pairs"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v *= (ell / 8 * rng.random(n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return with_dynamics({"x": 0.55 + v[:, 0], "y": 0.5 + v[:, 1], "z": 0.61 + v[:, 2]})
