"""Sim.render over two and three ranks on one GPU (host-staged transport, gloo control plane, launched as
test_gpu_distributed_observables.py launches its worker): every rank receives the same image, and it is the one-rank
image of the same particles up to the regrouping of the float partial sums.

Bound: a pixel's n contributions are added in float in ascending index on every rank (n u S0 on each side, u = 2^-24), and
the ranks' partial sums, exact doubles of floats, are then added in double; the one-rank image adds the same terms in one
float chain.  The two differ by at most (n + ranks) u S0 per pixel (S1: the same with sum |w_j a_j|); n and the scales
come from the oracle tests/map_ref.py over the merged particles.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dist_map_worker as worker
import map_ref as mr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, STEPS = 10, 2
PORTS = {2: 29701, 3: 29702}
U = 2.0 ** -24
BOX = ([-0.5, 0.5] * 3, [1, 1, 1])


def run_ranks(nproc, out):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(PORTS[nproc]), os.path.join(ROOT, "tests", "dist_map_worker.py"), "--out",
           str(out), "--side", str(SIDE), "--steps", str(STEPS)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(out, f"rank{q}.npz"))) for q in range(nproc)]


@pytest.fixture(scope="module", params=[2, 3])
def ranks(request, tmp_path_factory):
    return run_ranks(request.param, tmp_path_factory.mktemp(f"dist_map{request.param}"))


@pytest.fixture(scope="module")
def one_rank(ranks):
    """the merged particles rendered on one rank at seam level, and the oracle's counts and scales for them"""
    m = {k: np.concatenate([d[k] for d in ranks]) for k in worker.FIELDS}
    assert np.array_equal(np.sort(m["id"]), np.arange(SIDE ** 3))  # every particle on exactly one rank
    assert all(0 < d["id"].size < SIDE ** 3 for d in ranks)
    ctx = sx.Context(0)
    sim = sx.Sim(ctx, 64, sx.make_box(*BOX))  # for map_spec's defaults only
    out = {}
    try:
        ds = sx.DeviceState(ctx, {k: m[k] for k in ("x", "y", "z", "h", "m", "temp")})
        a = sx.DeviceArray(ctx, ds.fields.temp, SIDE ** 3, np.float64)
        for name, kw in worker.MAPS:
            spec = sim.map_spec(**kw)
            s0, s1 = ctx.render_map(ds.fields, sim.box, spec, a=a, K=sim.params.K)
            ref = mr.render(np.stack([m["x"], m["y"], m["z"]], axis=1), m["h"], m["m"], BOX[0], BOX[1], spec.kind,
                            spec.axis, list(spec.center), list(spec.width), list(spec.npix), K=sim.params.K, a=m["temp"])
            out[name] = (s0, s1, ctx.map_stats(), ref)
    finally:
        sim.close()
        ctx.close()
    return out


@pytest.mark.parametrize("name", ["column", "slice"])
def test_every_rank_has_the_same_image(ranks, name):
    for d in ranks[1:]:
        for k in ("_sum0", "_sum1"):
            assert np.array_equal(d[name + k].view(np.uint64), ranks[0][name + k].view(np.uint64))
    assert ranks[0][name + "_sum0"].shape == (24, 40) and (ranks[0][name + "_sum0"] > 0).any()


def test_refusal_on_one_rank_reaches_every_rank(ranks):
    """rank 0's pair cap refuses its render; the others learn of it through the reduction instead of waiting in it, and
    the next render is whole again"""
    assert "pair cap" in str(ranks[0]["refusal"]) and "code 4" in str(ranks[0]["refusal"])
    for d in ranks[1:]:
        assert "refused on another rank" in str(d["refusal"]) and "code 4" in str(d["refusal"])
    for d in ranks:
        assert np.array_equal(d["after_refusal_sum0"], ranks[0]["column_sum0"])


@pytest.mark.parametrize("name", ["column", "slice"])
def test_image_agrees_with_one_rank(ranks, one_rank, name):
    s0, s1, stats, ref = one_rank[name]
    bound = (ref["count"] + len(ranks)) * U
    e0 = np.abs(ranks[0][name + "_sum0"] - s0)
    e1 = np.abs(ranks[0][name + "_sum1"] - s1)
    use0 = (e0 / np.where(ref["sum0"] > 0, bound * ref["sum0"], 1.0)).max()
    use1 = (e1 / np.where(ref["abs1"] > 0, bound * ref["abs1"], 1.0)).max()
    print(f"{len(ranks)} ranks, {name}: worst use of the regrouping bound S0 {use0:.3f}, S1 {use1:.3f}")
    assert use0 <= 1.0 and use1 <= 1.0
    assert not ranks[0][name + "_sum0"][ref["count"] == 0].any()
    # in-window particles: each is local to one rank
    assert sum(int(d[name + "_stats"][3]) for d in ranks) == stats["footprints"]
    assert sum(int(d[name + "_stats"][0]) for d in ranks) == stats["pairs"]
