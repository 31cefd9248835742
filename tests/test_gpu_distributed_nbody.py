"""The gravity-only propagator (propagator 3) on several ranks: sx_sim_set_comm on an nbody sim runs the existing
distributedSync and distributedGravity.  2 and 3 ranks over the host-staged transport on one GPU, po.evrard_state(20)
(~3.9k bodies), 3 steps, against the 1-rank run per particle by id:

* a within median 1e-3 and max 1e-2 of |a|, egrav within 1e-3: the bounds DESIGN section 8 and
  tests/test_gpu_distributed.py hold multi-rank gravity to (the near / far split changes which cells are opened);
* dt identical on all ranks; the particle count conserved; every rank used both source paths.

Each run is a fresh child (one process per rank, at most 3 at once) under its own time limit; the first non-zero exit
fails the test."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, STEPS = 20, 3
_one_rank = {}


def run(tmp_path, nproc, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_nbody_worker.py"), "--out",
           str(tmp_path), "--side", str(SIDE), "--steps", str(STEPS)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{q}.npz"))) for q in range(nproc)]


def merged(ranks):
    got = {k: np.concatenate([d[k] for d in ranks]) for k in ("id", "x", "ax", "ay", "az", "h", "m")}
    o = np.argsort(got["id"])
    return {k: v[o] for k, v in got.items()}


def one_rank(tmp_path):
    if not _one_rank:
        d = tmp_path / "one"
        d.mkdir()
        ranks = run(str(d), 1, 29690)
        _one_rank.update(merged(ranks), egrav=float(ranks[0]["conserved"][2]), dts=ranks[0]["dts"])
    return _one_rank


@pytest.mark.parametrize("nproc,port", [(2, 29691), (3, 29692)])
def test_nbody_ranks(tmp_path, nproc, port):
    ref = one_rank(tmp_path)
    ranks = run(str(tmp_path), nproc, port)
    got = merged(ranks)
    # the particle count is conserved and every particle is owned once
    assert np.array_equal(got["id"], ref["id"])
    for k in ("h", "m"):
        assert np.array_equal(got[k], ref[k]), k
    # dt is identical on all ranks, at every step
    for d in ranks[1:]:
        assert np.array_equal(d["dts"], ranks[0]["dts"]) and np.array_equal(d["scalars"], ranks[0]["scalars"])
    a = np.stack([got[k] for k in ("ax", "ay", "az")], 1).astype(np.float64)
    a1 = np.stack([ref[k] for k in ("ax", "ay", "az")], 1).astype(np.float64)
    err = np.linalg.norm(a - a1, axis=1) / np.linalg.norm(a1, axis=1)
    egrav = float(ranks[0]["conserved"][2])
    print(f"{nproc} ranks against 1: a median {np.median(err):.2g}, max {err.max():.2g} of |a|; egrav "
          f"{egrav / ref['egrav'] - 1:.2g}; dt {ranks[0]['dts']} vs {ref['dts']}; (halos, far, remote cells) "
          f"{[tuple(int(v) for v in d['gravity']) for d in ranks]}")
    assert np.median(err) < 1e-3 and err.max() < 1e-2
    assert abs(egrav / ref["egrav"] - 1) < 1e-3
    assert ranks[0]["conserved"][1] == 0.0
    for d in ranks:
        halos, far_cells, remote_cells = d["gravity"]
        assert 0 < far_cells < remote_cells and halos > 0
