"""Sim.observe() over two ranks on one GPU (host-staged transport, gloo control plane, launched as
test_gpu_distributed.py launches its worker): the row is the same on every rank, its sums are those of the restatement
(tests/obs_ref.py) over the merged ranks' particles to 1e-12 sum|term|, and the Mach RMS divides by the global count.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import obs_ref
import sphexa_amd as sx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, STEPS, NPROC, PORT = 16, 2, 2, 29671
REL = 1e-12


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out = tmp_path_factory.mktemp("dist_obs")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(NPROC), "--master-addr",
           "127.0.0.1", "--master-port", str(PORT), os.path.join(ROOT, "tests", "dist_obs_worker.py"), "--out",
           str(out), "--side", str(SIDE), "--steps", str(STEPS)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(out, f"rank{q}.npz"))) for q in range(NPROC)]


@pytest.fixture(scope="module")
def merged(ranks):
    names = [k for k in ranks[0] if not k.startswith("row_")]
    m = {k: np.concatenate([d[k] for d in ranks]) for k in names}
    assert np.array_equal(np.sort(m["id"]), np.arange(SIDE ** 3))  # every particle on exactly one rank
    assert all(0 < d["id"].size < SIDE ** 3 for d in ranks)
    return m


@pytest.mark.parametrize("kind", ["mach_rms", "grav_waves"])
def test_rows_identical_on_every_rank(ranks, kind):
    rows = [d["row_" + kind] for d in ranks]
    for r in rows[1:]:
        assert np.array_equal(r.view(np.uint64), rows[0].view(np.uint64))
    assert rows[0][0] == STEPS and len(rows[0]) == len(sx.OBS_COLUMNS[kind])


def test_mach_rms_divides_by_the_global_count(ranks, merged):
    row = dict(zip(sx.OBS_COLUMNS["mach_rms"], ranks[0]["row_mach_rms"]))
    want, mag = obs_ref.sums("mach_rms", merged)
    n = SIDE ** 3
    got_sum = row["machRms"] ** 2 * n
    assert abs(got_sum - want["machSquareSum"]) <= REL * mag["machSquareSum"]
    assert row["machRms"] == pytest.approx(np.sqrt(want["machSquareSum"] / n), rel=1e-12) and row["machRms"] > 0
    # a local count in the quotient would be off by about sqrt(2)
    assert abs(row["machRms"] / np.sqrt(want["machSquareSum"] / ranks[0]["id"].size) - 1) > 0.2
    # the conserved columns are the sums over both ranks
    for k in ("ecin", "eint"):
        assert abs(row[k] - want[k]) <= REL * mag[k], k
    lin = np.sqrt(want["px"] ** 2 + want["py"] ** 2 + want["pz"] ** 2)
    ang = np.sqrt(want["Lx"] ** 2 + want["Ly"] ** 2 + want["Lz"] ** 2)
    # |(a, b, c)| moves by at most the length of the error vector: sqrt(3) times the largest component bound
    assert abs(row["linmom"] - lin) <= 2 * REL * max(mag[k] for k in ("px", "py", "pz"))
    assert abs(row["angmom"] - ang) <= 2 * REL * max(mag[k] for k in ("Lx", "Ly", "Lz"))
    assert row["etot"] == row["ecin"] + row["eint"] + row["egrav"] and row["egrav"] == 0.0


def test_grav_wave_row_equals_the_restatement(ranks, merged):
    row = dict(zip(sx.OBS_COLUMNS["grav_waves"], ranks[0]["row_grav_waves"]))
    want, mag = obs_ref.sums("grav_waves", merged)
    names = obs_ref.EXTRA["grav_waves"]
    for name in names:
        assert abs(row[name] - want[name]) <= REL * mag[name], (name, row[name], want[name])
    h = obs_ref.htt([want[k] for k in names], 0.3, 0.4)
    bound = obs_ref.htt_bound([2 * REL * mag[k] for k in names], 0.3, 0.4)
    assert abs(row["httplus"] - h[0]) <= bound[0] and abs(row["httcross"] - h[1]) <= bound[1]
    for k in ("ecin", "eint"):
        assert abs(row[k] - want[k]) <= REL * mag[k], k
