"""Sim.profile over two and three ranks on one GPU (host-staged transport, gloo control plane, launched as
test_gpu_distributed_spectrum.py launches its worker): every rank receives the same arrays, and they are, bit for bit,
Context.profile of the merged particles on one rank and the oracle's (tests/profile_ref.py).  The sums are integers, so
there is no bound: the regrouping over the ranks changes nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dist_profile_worker as worker
import profile_ref as pr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, STEPS = 10, 2
PORTS = {2: 29721, 3: 29722}
BOX = ([-0.5, 0.5] * 3, [1, 1, 1])


def run_ranks(nproc, out):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(PORTS[nproc]), os.path.join(ROOT, "tests", "dist_profile_worker.py"),
           "--out", str(out), "--side", str(SIDE), "--steps", str(STEPS)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(out, f"rank{q}.npz"))) for q in range(nproc)]


@pytest.fixture(scope="module", params=[2, 3])
def ranks(request, tmp_path_factory):
    return run_ranks(request.param, tmp_path_factory.mktemp(f"dist_profile{request.param}"))


@pytest.fixture(scope="module")
def merged(ranks):
    m = {k: np.concatenate([d[k] for d in ranks]) for k in worker.FIELDS}
    assert np.array_equal(np.sort(m["id"]), np.arange(SIDE ** 3))  # every particle on exactly one rank
    assert all(0 < d["id"].size < SIDE ** 3 for d in ranks)
    return m


def bits(a):
    return a.tobytes()


@pytest.mark.parametrize("name", [p[0] for p in worker.PROFILES])
def test_every_rank_has_the_same_arrays(ranks, name):
    for d in ranks[1:]:
        for k in worker.ARRAYS:
            assert bits(d[f"{name}_{k}"]) == bits(ranks[0][f"{name}_{k}"]), k
    assert sum(int(d[f"{name}_particles"]) for d in ranks) == SIDE ** 3  # each read its own locals only
    assert int(ranks[0][f"{name}_count"].sum()) + int(ranks[0][f"{name}_nonfinite"][0]) == SIDE ** 3


@pytest.mark.parametrize("name", [p[0] for p in worker.PROFILES])
def test_equal_to_one_rank_and_to_the_oracle(ranks, merged, name):
    kw = dict(dict(worker.PROFILES)[name])
    ctx = sx.Context(0)
    try:
        ds = sx.DeviceState(ctx, {k: merged[k] for k in worker.FIELDS if k != "id"})
        one = ctx.profile(ds.fields, sx.make_box(*BOX), sx.SxProfile(**kw))
    finally:
        ctx.close()
    edges, quantities = kw.pop("edges"), kw.pop("quantities")
    ref = pr.profile(merged, BOX[0], BOX[1], edges, quantities, **kw)
    got = {k: ranks[0][f"{name}_{k}"] for k in worker.ARRAYS}
    for k in ("count", "nonfinite", "W", "S1", "S2", "D"):
        assert bits(got[k]) == bits(one[k]), k
        assert bits(got[k]) == bits(ref[k].astype(got[k].dtype)), k
    for k in ("min", "max"):
        assert np.array_equal(got[k], one[k]) and np.array_equal(got[k], ref[k]), k
    assert got["count"][:-2].sum() > 0


def test_refusal_on_one_rank_reaches_every_rank(ranks):
    """rank 0's edges descend; the others learn of it through the first reduction instead of waiting in the next, and
    the next profile is whole again"""
    assert "strictly ascending" in str(ranks[0]["refusal"]) and "code 4" in str(ranks[0]["refusal"])
    for d in ranks[1:]:
        assert "refused on another rank" in str(d["refusal"]) and "code 4" in str(d["refusal"])
    for d in ranks:
        for k in worker.ARRAYS:
            assert bits(d[f"after_refusal_{k}"]) == bits(ranks[0][f"radial_{k}"]), k
