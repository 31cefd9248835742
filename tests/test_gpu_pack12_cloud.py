"""packed12 cluster neighbor lists (sx_pack12.hpp) on a random cloud: the search's writer, every reader.

600 particles (two full 256-particle clusters and one of 88 targets) in an open and in a periodic box, placed in
well-separated random clumps of k + 1 particles with 2h between a clump's diameter and the gap to the next clump, so
that every member has exactly k neighbors, all well inside its kernel (a well-conditioned IAD matrix even for k = 7).
k takes 7, 8, 9, counts that are no multiple of 8 and the ngmax cap (150; one case with ngmax = 256), a pair (k = 1)
and a single particle (k = 0).  In the periodic box clumps wrap around the faces.

  * the neighbor sets from sx_export_neighbors and nc equal a brute-force search on the CPU;
  * XMass, VeDefGradh, IAD + divv/curlv, AV switches and momentum, each in isolation on the oracle's inputs, match
    the oracle within the tolerance of test_gpu_cluster_kernels.py (RTOL * per-particle scale), for the fast
    (cluster) kernels and for the exact (gather) kernels reading the same lists;
  * once with the default packed12 threshold (every cluster packed) and once with the threshold lowered between the
    cloud's smallest and largest union count, so that one run holds packed clusters and u16 clusters (which take the
    chunked loop).  The CPU test checks that the cloud's union counts really lie on both sides of that threshold.

One particle has no neighbor and two have a single one.  Their IAD matrix is singular (rank <= 1: the determinant is
rounding noise or zero, c_ij huge or non-finite in the oracle as on the GPU), so what follows from a target's own c_ij
(c_ij, divv, curlv, alpha, du, a) is not compared for these three targets; their xm, kx, gradh, prho and c are, and so is
every other target.  The
test asserts that the oracle's values are finite for most targets, so the comparison is not vacuous.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_util as gutil
import pyoracle as po
import sphexa_amd as sx
from test_gpu_cluster_kernels import check_all, reference_chain

N = 600
# neighbor counts of the clumps (a clump of k + 1 particles gives each of them k neighbors); 600 particles in all
CLUMPS = {150: [150, 99, 65, 64, 37, 31, 23, 17, 16, 15, 12, 11, 9, 9, 8, 7, 7, 1, 0],
          256: [256, 200, 99, 17, 12, 7, 1, 0]}
FROM_OWN_C = ["c11", "c12", "c13", "c22", "c23", "c33", "divv", "curlv", "alpha", "du", "ax", "ay", "az"]
CASES = [("open", 150), ("periodic", 150), ("open", 256)]


@functools.lru_cache(maxsize=None)
def cloud(kind, ngmax):
    """(state sorted by SFC key with h, nc set; box; reference neighbor list (n, ngmax); neighbor sets; cluster
    union counts)"""
    ora = po.load_oracle()
    rng = np.random.default_rng(7 + ngmax + (kind == "periodic"))
    periodic = kind == "periodic"
    sizes = [k + 1 for k in CLUMPS[ngmax]]
    assert sum(sizes) == N
    # clump radii at one density; every member's 2h = 2.4 rho covers its clump (diameter 2 rho) and stays 0.4 rho
    # and more short of every other clump
    rho = [0.0224 * max(s, 3) ** (1.0 / 3.0) for s in sizes]
    centers = []
    for a, ra in enumerate(rho):
        for _ in range(100000):
            c = rng.uniform(-0.5, 0.5, 3) if periodic else rng.uniform(-0.5 + ra, 0.5 - ra, 3)
            ok = True
            for cb, rb in zip(centers, rho):
                d = c - cb
                if periodic:
                    d -= np.rint(d)
                if np.sqrt(d @ d) < ra + rb + 2.4 * max(ra, rb) + 0.01:
                    ok = False
                    break
            if ok:
                break
        assert ok, "no room for the clumps"
        centers.append(c)
    pos, hh = [], []
    for c, r, s in zip(centers, rho, sizes):
        v = rng.standard_normal((s, 3))
        v *= (r * rng.random(s) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
        q = c + v
        if periodic:
            q -= np.rint(q)  # clumps near a face wrap around
        pos.append(q)
        hh.append(np.full(s, 1.2 * r))
    pos, hh = np.concatenate(pos), np.concatenate(hh)
    st = po.HostState(N)
    st.x[:], st.y[:], st.z[:] = pos[:, 0], pos[:, 1], pos[:, 2]
    box = po.make_box(-0.5, 0.5, periodic)
    st.h[:] = hh
    st.m[:] = (1.0 + 0.2 * rng.random(N)) / N
    st.temp[:] = 1.0 + rng.random(N)
    for k in ("vx", "vy", "vz"):
        st.arrays[k][:] = 0.1 * rng.standard_normal(N)
    st.alpha[:] = 0.05 + 0.5 * rng.random(N)
    st.id[:] = np.arange(N, dtype=np.uint64)
    gutil.sorted_state(st, box, ora)
    p = np.stack([st.x, st.y, st.z], axis=1)
    d = p[:, None, :] - p[None, :, :]
    if periodic:
        d -= np.rint(d)
    dist = np.sqrt(np.sum(d * d, axis=2))
    nbr = np.zeros((N, ngmax), np.uint32)
    sets = []
    for i in range(N):
        two_h = 2.0 * float(st.h[i])
        js = np.nonzero(dist[i] < two_h)[0]
        js = js[js != i]
        assert js.size <= ngmax and (not periodic or two_h < 0.49)
        assert not np.any(np.abs(dist[i] - two_h) < 1e-3 * two_h)  # no pair near the criterion's rounding
        st.nc[i] = js.size + 1
        nbr[i, :js.size] = js
        sets.append(js)
    ucounts = [np.unique(np.concatenate(sets[c:c + 256] + [np.zeros(0, np.int64)])).size for c in range(0, N, 256)]
    return st, box, nbr, sets, ucounts


def lowered(ucounts):
    return (min(ucounts) + max(ucounts)) // 2


@pytest.mark.parametrize("kind,ngmax", CASES)
def test_cloud_counts_and_unions(kind, ngmax):
    """CPU: the cloud has the counts the format's edges need, and union counts on both sides of the lowered threshold"""
    st, _, _, _, ucounts = cloud(kind, ngmax)
    cnt = st.nc.astype(np.int64) - 1
    assert sorted(set(cnt.tolist())) == sorted(set(CLUMPS[ngmax]))  # every clump's members have its count
    assert np.sum(cnt == 0) == 1 and np.sum(cnt == 1) == 2 and np.any(cnt == ngmax)
    assert {0, 1, 7} <= set((cnt % 8).tolist())
    assert len(ucounts) == 3 and max(ucounts) <= 4095
    thr = lowered(ucounts)
    assert min(ucounts) <= thr < max(ucounts), ucounts


@pytest.fixture(scope="module")
def ctx():
    c = sx.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ora():
    return po.load_oracle()


@functools.lru_cache(maxsize=None)
def reference(kind, ngmax):
    ora = po.load_oracle()
    st, box, nbr, _, _ = cloud(kind, ngmax)
    params = ora.params()
    params.ngmax = ngmax
    chk = st.copy()
    with np.errstate(all="ignore"):
        ref, sc = reference_chain(ora, chk, box, nbr.ravel(), params, st.minDt)
    return ref, sc


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("threshold", ["default", "lowered"])
@pytest.mark.parametrize("kind,ngmax", CASES)
def test_cloud_sets_and_kernels(ctx, kind, ngmax, threshold, exact):
    st, obox, nbr, sets, ucounts = cloud(kind, ngmax)
    ref, sc = reference(kind, ngmax)
    box = gutil.box_to_sx(obox)
    thr = 4095 if threshold == "default" else lowered(ucounts)
    L, h, n = ctx.L, ctx.h, N
    ctx.set_pack12_max(thr)
    ctx.set_exact(exact)
    try:
        ds = sx.DeviceState(ctx, gutil.host_dict(st))
        tree, _ = gutil.device_tree(ctx, ds.dev["keys"], n, 64, box)
        p = sx.default_params(ngmax=ngmax)
        stats = sx.SxNbStats()
        ctx.check(L.sx_find_neighbors(h, C.byref(ds.fields), C.byref(tree), C.byref(box), C.byref(p), 0, n, 0,
                                      C.byref(stats)), "search")
        # ---- the search's lists, read back through exportNeighbors
        assert np.array_equal(ds.get("nc"), st.nc)
        assert np.array_equal(ds.get("h"), st.h)
        assert stats.maxUnion == max(ucounts) and stats.sumUnion == sum(ucounts), (stats.maxUnion, ucounts)
        out = ctx.alloc(n * ngmax, np.uint32)
        ctx.check(L.sx_export_neighbors(h, ds.dev["nc"].ptr, 0, n, ngmax, out.ptr), "export")
        rows = out.get().reshape(n, ngmax)
        for i in range(n):
            assert np.array_equal(np.sort(rows[i, :sets[i].size]), sets[i]), i
            assert not rows[i, sets[i].size:].any(), i
        # ---- every pair kernel in isolation on the oracle's inputs
        g = sx.SxGroups(firstBody=0, lastBody=n, numGroups=(n + 63) // 64)
        f = ds.fields
        worst = {}

        singular = st.nc <= 2

        def check(names):
            for k in names:
                got = ds.get(k)
                if k in FROM_OWN_C:
                    got[singular] = ref[k][singular]
                worst[k] = check_all(k, got, ref, sc)
                fin = np.isfinite(ref[k])
                assert fin.mean() > 0.5, (k, float(fin.mean()))  # the comparison is not vacuous
                ds.set(k, ref[k])

        with np.errstate(all="ignore"):
            ctx.check(L.sx_xmass_only(h, C.byref(g), C.byref(f), C.byref(p), C.byref(box)), "xmass")
            check(["xm"])
            ctx.check(L.sx_ve_def_gradh(h, C.byref(g), C.byref(f), C.byref(p), C.byref(box)), "gradh")
            check(["kx", "gradh"])
            ctx.check(L.sx_eos(h, 0, n, 10.0, 5.0 / 3.0, f.temp, f.m, f.kx, f.xm, f.gradh, f.prho, f.c, None, None),
                      "eos")
            check(["prho", "c"])
            ctx.check(L.sx_iad_divv_curlv(h, C.byref(g), C.byref(f), C.byref(p), C.byref(box)), "iad")
            check(["c11", "c12", "c13", "c22", "c23", "c33", "divv", "curlv"])
            ctx.check(L.sx_av_switches(h, C.byref(g), C.byref(f), C.byref(p), C.byref(box), float(st.minDt)), "av")
            check(["alpha"])
            mdt = C.c_float()
            ctx.check(L.sx_momentum_energy(h, C.byref(g), None, C.byref(f), C.byref(p), C.byref(box), C.byref(mdt)),
                      "momentum")
            check(["du", "ax", "ay", "az"])
        print(kind, ngmax, threshold, "exact" if exact else "fast", ucounts, {k: f"{v:.1e}" for k, v in worst.items()})
    finally:
        ctx.set_exact(False)
        ctx.set_pack12_max(None)
        ctx.free_all()
