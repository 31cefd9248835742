"""Skin lists with several ranks: filter-served steps between full builds on an SFC decomposition.

A full build requests its halos within the skin radius 2 h (1 + s); a reuse step keeps the decomposition, refreshes
the halos' x, y, z, h, m over the build's send lists and reduces the displacement grid over all ranks; the decision to
rebuild, and to redo a step whose re-searched spheres left the build's halo region, is taken by every rank together.
The step's neighbor search result must not change: after every step the nc and h of each particle (by id, merged over
the ranks) equal those of a fresh distributed sync + search of the same state (tests/dist_skin_worker.py: a second
simulation with the skin off, handed the state before every step).  nc counts every neighbor within 2h, and the filter
only ever tests candidates with the reference's exact criterion, so equal nc means equal neighbor sets.  The fields the
pair kernels produce agree within float summation order (the two unions order the neighbors differently), and every
rank takes the same build decisions (identical skin statistics).  Host-staged transport, every rank on the one GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIN = ["builds", "reuse_steps", "stale_clusters", "exact_clusters", "plain_steps", "resyncs"]


def run(tmp_path, nproc, port, ic, side, steps, skin=0.08, max_reuse=24, g=0.0, extra=()):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_skin_worker.py"), "--out",
           str(tmp_path), "--ic", ic, "--side", str(side), "--steps", str(steps), "--skin", str(skin),
           "--max-reuse", str(max_reuse), "--g", str(g), *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{q}.npz"))) for q in range(nproc)]


def merged(ranks, s, tag, keys):
    out = {k: np.concatenate([d[f"s{s}_{tag}_{k}"] for d in ranks]) for k in keys}
    o = np.argsort(out["id"])
    return {k: v[o] for k, v in out.items()}


def check_equals_fresh_search(ranks, ic, nproc, steps):
    """after every step, by id over all ranks: nc and h of the skin run equal those of the fresh distributed search of
    the same state, the fields agree to float summation order, one dt, the same build decisions on every rank"""
    keys = ["id", "nc", "h", "xm", "kx", "divv", "alpha", "ax", "ay", "az", "du", "x", "vx"]
    n = None
    for s in range(steps):
        ga, gb = merged(ranks, s, "a", keys), merged(ranks, s, "b", keys)
        n = ga["id"].size
        assert np.array_equal(ga["id"], gb["id"]) and np.array_equal(ga["id"], np.arange(n))
        bad = np.nonzero(ga["nc"] != gb["nc"])[0]
        assert bad.size == 0, (ic, nproc, s, bad.size, ga["nc"][bad[:8]], gb["nc"][bad[:8]])
        assert np.array_equal(ga["h"], gb["h"]), (ic, nproc, s)
        for k in ("xm", "kx", "divv", "alpha", "ax", "ay", "az", "du", "x", "vx"):
            x, y = ga[k].astype(np.float64), gb[k].astype(np.float64)
            tol = 2e-4 * np.abs(y) + 2e-5 * np.max(np.abs(y))
            assert np.all(np.abs(x - y) <= tol), (ic, nproc, s, k, float(np.max(np.abs(x - y) / (np.abs(y) + 1e-30))))
        dts = {float(d[f"s{s}_a_dt"][0]) for d in ranks}
        assert len(dts) == 1
        # every rank takes the same build decisions
        sk = np.array([d[f"s{s}_skin"] for d in ranks])
        for col in (0, 1, 4, 5, 6, 7):  # builds, reuse steps, plain steps, resyncs, skin factor, next factor
            assert np.all(sk[:, col] == sk[0, col]), (s, col, sk[:, col])


@pytest.mark.parametrize("nproc,port,ic,side,steps,skin", [(2, 29651, "sedov", 20, 10, 0.08),
                                                           (3, 29652, "sedov", 20, 8, 0.08),
                                                           (2, 29653, "noh", 20, 8, 0.08),
                                                           (3, 29654, "noh", 22, 8, 0.3),
                                                           (8, 29655, "sedov", 24, 6, 0.08)])
def test_distributed_skin_equals_fresh_search(tmp_path, nproc, port, ic, side, steps, skin):
    ranks = run(tmp_path, nproc, port, ic, side, steps, skin)
    check_equals_fresh_search(ranks, ic, nproc, steps)
    last = np.array([d[f"s{steps - 1}_skin"] for d in ranks])
    kept, frozen = int(last[:, 8].sum()), int(last[:, 9].sum())  # clusters whose lists were kept (of them frozen)
    print(ic, nproc, side, skin, dict(zip(SKIN, last[0][:6])), "stale per rank", last[:, 2], "kept", kept,
          "frozen", frozen)
    assert last[0][SKIN.index("reuse_steps")] > 0, last[0]
    if ic == "sedov":
        # the lattice outside the blast: steps whose hits match a recorded list set keep it on every rank's clusters
        assert kept > 0, last


@pytest.mark.parametrize("nproc,port,skin", [(2, 29660, 0.05), (2, 29661, 0.08), (3, 29662, 0.05), (3, 29663, 0.08)])
def test_distributed_skin_converging_patch(tmp_path, nproc, port, skin):
    """clusters searched again on a reuse step at a rank boundary while the peer's particles close in
    (tests/dist_skin_worker.py --ic converge): a cold lattice at rest but for a patch of one rank, a ball of 4
    spacings on its boundary with a resting rank, which moves towards that rank, 0.02 spacings in the step before the
    first and up to 1.1 times more with every step.  The re-search of a stale cluster only sees the halos of the last
    full build; a particle that was outside the request box then is no halo however close it has come
    (sx_sim_skin.cpp coverListKernel: the sphere grown by a bound of the motion since the build must fit the box, or
    every rank redoes the step from a full sync).  Same assertions as test_distributed_skin_equals_fresh_search after
    every step.  And the path was taken: the patch's mean drift passes the box's slack over the search sphere plus the
    skin, (kHaloMargin - 1) (1 + s) 2 h + s 2 h; some reuse step served stale clusters (searched them again) with
    neither a full build nor a resync on that step.  Side 40: 64000 particles, 250 clusters of 256 -- the clusters
    around the patch stay below the share of 1/8 that makes the next step a full build"""
    side, steps = 40, 16
    ranks = run(tmp_path, nproc, port, "converge", side, steps, skin, extra=("--ball", "4", "--patch-step", "0.02"))
    # per step, summed over the ranks: stale, exact-search and early exact clusters; of rank 0: builds, reuse steps,
    # resyncs (the same on every rank); the patch's mean drift in units of h
    sk = np.array([[d[f"s{s}_skin"] for d in ranks] for s in range(steps)])  # [step, rank, column]
    cum = np.concatenate([np.zeros((1,) + sk.shape[1:]), sk])
    per = np.diff(cum, axis=0)
    spacing, h = ranks[0]["spacing"]
    drift = np.array([sum(d[f"s{s}_drift"][0] for d in ranks) / sum(d[f"s{s}_drift"][1] for d in ranks)
                      for s in range(steps)])
    wrong = []
    for s in range(steps):
        ga, gb = merged(ranks, s, "a", ["id", "nc"]), merged(ranks, s, "b", ["id", "nc"])
        wrong.append(int(np.sum(ga["nc"] != gb["nc"])))
    print("converge", nproc, "ranks, s =", skin, "patch (particles, resting rank, moving rank)", ranks[0]["patch"])
    served = []
    for s in range(steps):
        stale, exact, early = (int(per[s, :, c].sum()) for c in (2, 3, 10))
        build, reuse, resync = (int(per[s, 0, c]) for c in (0, 1, 5))
        print(f"  step {s}: stale {stale} exact {exact} (early exact {early}) build {build} reuse {reuse} "
              f"resync {resync} drift {drift[s] / h:.3f} h = {drift[s] / spacing:.3f} spacings, wrong nc {wrong[s]}")
        if reuse and stale > 0 and build == 0 and resync == 0:
            served.append(s)
    check_equals_fresh_search(ranks, "converge", nproc, steps)
    assert drift[-1] >= ((1.05 - 1.0) * (1.0 + skin) + skin) * 2.0 * h, (drift[-1] / h, skin)
    assert served, per[:, 0, :6]


@pytest.mark.parametrize("nproc,port,side", [(2, 29656, 20), (3, 29657, 22)])
def test_distributed_skin_with_gravity(tmp_path, nproc, port, side):
    """Evrard with self-gravity (G = 1) on 2-3 ranks with skin lists: on reuse steps the near/far split takes request
    boxes of the current positions and every MAC box holds its cell (node) and its drifted particles.  Against the
    same ranks syncing every step: nc and h by id exactly; the accelerations within the Barnes-Hut error of two
    different decompositions (the multi-rank field itself is within median 1e-3 / max 1e-2 of |a| of a direct sum,
    tests/test_gpu_distributed.py): |a - a_fresh| / rms(a) median <= 5e-4, max <= 5e-3 (measured 4e-5 / 2.2e-4);
    egrav within 1e-3"""
    steps = 6
    ranks = run(tmp_path, nproc, port, "evrard", side, steps, 0.05, g=1.0)
    keys = ["id", "nc", "h", "ax", "ay", "az", "xm", "kx", "du"]
    worst = (0.0, 0.0)
    for s in range(steps):
        ga, gb = merged(ranks, s, "a", keys), merged(ranks, s, "b", keys)
        assert np.array_equal(ga["id"], gb["id"])
        assert np.array_equal(ga["nc"], gb["nc"]), (s, int(np.sum(ga["nc"] != gb["nc"])))
        assert np.array_equal(ga["h"], gb["h"]), s
        A = np.stack([ga[k] for k in ("ax", "ay", "az")]).astype(np.float64)
        B = np.stack([gb[k] for k in ("ax", "ay", "az")]).astype(np.float64)
        rms = np.sqrt(np.mean(np.sum(B * B, axis=0)))
        err = np.sqrt(np.sum((A - B) ** 2, axis=0)) / rms
        worst = (max(worst[0], float(np.median(err))), max(worst[1], float(err.max())))
        assert np.median(err) <= 5e-4 and err.max() <= 5e-3, (s, float(np.median(err)), float(err.max()))
        ea, eb = ranks[0][f"s{s}_a_egrav"][0], ranks[0][f"s{s}_b_egrav"][0]
        assert abs(ea / eb - 1) <= 1e-3, (s, ea, eb)
    last = np.array([d[f"s{steps - 1}_skin"] for d in ranks])
    print("evrard", nproc, side, "gravity |da|/rms median, max", worst, dict(zip(SKIN, last[0][:6])))
    assert last[0][SKIN.index("reuse_steps")] > 0, last[0]


@pytest.mark.parametrize("opts,port", [(("--std",), 29658), (("--av-clean",), 29659)])
def test_distributed_skin_std_and_avclean(tmp_path, opts, port):
    """the std propagator (HydroProp: the filter's fused XMass writes rho) and VE with avClean (the dV halos) on skin
    lists with 2 ranks, against the same ranks syncing every step: nc and h by id exactly, rates to float summation
    order"""
    steps = 8
    ranks = run(tmp_path, 2, port, "sedov", 20, steps, 0.05, extra=opts)
    fields = ["ax", "ay", "az", "du", "x", "vx"] + (["rho"] if "--std" in opts else ["xm", "kx", "divv", "alpha"])
    for s in range(steps):
        ga, gb = merged(ranks, s, "a", ["id", "nc", "h"] + fields), merged(ranks, s, "b", ["id", "nc", "h"] + fields)
        assert np.array_equal(ga["id"], gb["id"])
        assert np.array_equal(ga["nc"], gb["nc"]) and np.array_equal(ga["h"], gb["h"]), (opts, s)
        for k in fields:
            x, y = ga[k].astype(np.float64), gb[k].astype(np.float64)
            tol = 2e-4 * np.abs(y) + 2e-5 * np.max(np.abs(y))
            assert np.all(np.abs(x - y) <= tol), (opts, s, k)
    last = np.array([d[f"s{steps - 1}_skin"] for d in ranks])
    assert last[0][SKIN.index("reuse_steps")] > 0, last[0]
