"""Sim.set_cooling over two ranks on one GPU (host-staged transport, gloo control plane, launched as
test_gpu_distributed_profile.py launches its worker): the lattice at rest for four steps with the limiter on.  The
cooling-time criterion joins each rank's candidate before the minimum over the ranks, so both take the same steps;
every particle follows the cooling curve of its own rho; the ranks' radiated energies add up to the one-rank total.

Each run is held to the oracle applied step by step with its own rho (as test_gpu_cooling_sim.py does on one rank), and
the two runs to each other: temp by id within the single-rank allowance, the radiated energies within the summation
bound and that allowance in energy."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cooling_ref as cr
import dist_cooling_worker as worker
import sphexa_amd as sx
from sphexa_amd import ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, STEPS, PORT = 16, 4, 29731
MARGIN = 16.0


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out = tmp_path_factory.mktemp("dist_cooling")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(PORT), os.path.join(ROOT, "tests", "dist_cooling_worker.py"), "--out", str(out),
           "--side", str(SIDE), "--steps", str(STEPS)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(out, f"rank{q}.npz"))) for q in range(2)]


@pytest.fixture(scope="module")
def one_rank():
    ctx = sx.Context(0)
    try:
        return worker.run(sx, ctx, SIDE, STEPS, True), worker.run(sx, ctx, SIDE, STEPS, False)
    finally:
        ctx.close()


def merged(parts, prefix=""):
    m = {k: np.concatenate([d[prefix + k] for d in parts]) for k in (("id", "temp") if prefix else worker.FIELDS)}
    assert np.array_equal(np.sort(m["id"]), np.arange(SIDE ** 3))  # every particle on exactly one rank
    return cr.by_id(m)


def test_both_ranks_take_the_same_steps(ranks):
    assert all(0 < d["id"].size < SIDE ** 3 for d in ranks)
    assert np.array_equal(ranks[0]["minDt"], ranks[1]["minDt"])
    # each rank's own criterion is never below the step taken, and the smaller of the two is honoured
    for d in ranks:
        assert np.all(d["minDt"] <= d["minDtCool"])
    print("minDt", ranks[0]["minDt"], "minDtCool", ranks[0]["minDtCool"], ranks[1]["minDtCool"])


def test_temp_and_energy_against_one_rank(ranks, one_rank):
    eps = max(cr.gpu_reference(0)["eps_ref"], cr.eps_floor())
    f = ic.turbulence(SIDE)[0]
    tab = cr.Table(*cr.scaled_table(f["temp"][0], worker.STRENGTH))
    cv = float(ic.ideal_gas_cv(np.float32(ic.TURBULENCE_CONSTANTS["muiConst"]), ic.TURBULENCE_CONSTANTS["gamma"]))
    T0 = f["temp"]  # ids are the lattice's indices
    two, one = merged(ranks), cr.by_id({k: one_rank[0][k] for k in worker.FIELDS})
    want = {}
    for name, run, parts, twin in (("two", two, ranks, merged(ranks, "twin_")),
                                   ("one", one, [one_rank[0]], cr.by_id({k: one_rank[1][k] for k in ("id", "temp")}))):
        # the oracle step by step, with the step's dt and every particle's rho of that step, whichever rank had it
        want[name] = T0
        for k, dt in enumerate(parts[0]["minDt"]):
            step = cr.by_id({"id": np.concatenate([d[f"id_step{k}"] for d in parts]),
                             "rho": np.concatenate([d[f"rho_step{k}"] for d in parts])})
            assert np.array_equal(step["id"], np.arange(SIDE ** 3))
            want[name] = cr.integrate64(tab, want[name], (step["rho"].astype(np.float64) * float(dt)) / cv)
        drift = np.max(np.abs(twin["temp"] - T0))
        allow = STEPS * MARGIN * eps * T0 + drift
        err = np.abs(run["temp"] - want[name])
        print("%s rank(s): cooled to %.4f of T_0, max error %.3e, allowance %.3e (twin drift %.3e)"
              % (name, np.mean(run["temp"] / T0), err.max(), allow.min(), drift))
        assert np.all(run["temp"] < 0.95 * T0)
        assert np.all(err <= allow), name
    # the two runs against each other: the single-rank allowance (on the MI355X the two come out equal bit for bit;
    # the difference of the two oracle results, what the decompositions' own rho would explain, is printed only)
    print("two against one: max |dT| %.3e (the oracle with either run's rho differs by %.3e)"
          % (np.max(np.abs(two["temp"] - one["temp"])), np.max(np.abs(want["two"] - want["one"]))))
    assert np.all(np.abs(two["temp"] - one["temp"]) <= allow)
    # the ranks' energies add up to the one-rank total: the summation bound of the folds (one rounding per term and a
    # double sum in a fixed order: (n + 1) 2^-53 of the terms' sum, on either side) and the allowance in energy
    m = one["m"].astype(np.float64)
    total_two = float(ranks[0]["radiated_total"]) + float(ranks[1]["radiated_total"])
    total_one = float(one_rank[0]["radiated_total"])
    eint0 = math.fsum(m * cv * T0)
    bound = (SIDE ** 3 + 1) * 2.0 ** -53 * (total_two + total_one) + math.fsum(m * cv * allow)
    print("radiated: two ranks %.12g, one rank %.12g, difference %.3e, bound %.3e"
          % (total_two, total_one, total_two - total_one, bound))
    assert total_one > 0.02 * eint0
    assert abs(total_two - total_one) <= bound
    for d in ranks:
        assert float(d["radiated_total"]) == pytest.approx(math.fsum(d["radiated"]), rel=1e-14)
