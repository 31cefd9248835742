"""Sim.spectrum over two and three ranks on one GPU (host-staged transport, gloo control plane, launched as
test_gpu_distributed_map.py launches its worker): every rank receives the same spectrum, bit for bit, and it is the
one-rank spectrum of the same particles up to the regrouping of the float partial sums.

Bound.  A cell's n_c contributions are added in float in ascending index on every rank, and the ranks' partial sums, exact
doubles of floats, are then added in double; the one-rank mesh adds the same terms (the records do not depend on the rank)
in one float chain.  The two differ by at most r = (n_c + ranks) 2^-24 of S0 per cell (S1: of sum |w_j a_j|).  Through
W_a = S0^(p-1) S1_a that is e_ac = S0^(p-1) r (sum_j |w_j a_j| + |1 - p| |S1_a|) (the density itself: r S0), and by Parseval
| sqrt P_ranks(s) - sqrt P_one(s) | <= E + (2 x transform bound + modes[s] 2^-52) sqrt P_total, E = sqrt(prefactor mean_c
sum_a e_ac^2), as in tests/test_gpu_spectrum.py; n_c and the scales come from tests/spectrum_ref.py over the merged
particles.  Measured on an MI355X: E is 0.6e-5 .. 1.4e-5 of sqrt(P_total), worst use of it 0.005 with two ranks and 0.008
with three (the density spectrum both times).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dist_spectrum_worker as worker
import spectrum_ref as sr
import sphexa_amd as sx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, STEPS = 10, 2
PORTS = {2: 29711, 3: 29712}
U = 2.0 ** -24
BOX = ([-0.5, 0.5] * 3, [1, 1, 1])
N = worker.N


def run_ranks(nproc, out):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(PORTS[nproc]), os.path.join(ROOT, "tests", "dist_spectrum_worker.py"),
           "--out", str(out), "--side", str(SIDE), "--steps", str(STEPS)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(out, f"rank{q}.npz"))) for q in range(nproc)]


@pytest.fixture(scope="module", params=[2, 3])
def ranks(request, tmp_path_factory):
    return run_ranks(request.param, tmp_path_factory.mktemp(f"dist_spectrum{request.param}"))


@pytest.fixture(scope="module")
def one_rank(ranks):
    """the merged particles through Context.spectrum on one rank, and the oracle's counts and scales for them"""
    m = {k: np.concatenate([d[k] for d in ranks]) for k in worker.FIELDS}
    assert np.array_equal(np.sort(m["id"]), np.arange(SIDE ** 3))  # every particle on exactly one rank
    assert all(0 < d["id"].size < SIDE ** 3 for d in ranks)
    ctx = sx.Context(0)
    out = {}
    try:
        box = sx.make_box(*BOX)
        ds = sx.DeviceState(ctx, {k: m[k] for k in worker.FIELDS if k != "id"})
        temp = sx.DeviceArray(ctx, ds.fields.temp, SIDE ** 3, np.float64)
        for name, kw in worker.SPECTRA:
            spec = sx.SxSpectrum(kw["kind"], kw.get("weight"), kw["n"])
            out[name] = ctx.spectrum(ds.fields, box, spec, a=[temp] if kw.get("field") else None) + (ctx.spectrum_stats(),)
    finally:
        ctx.close()
    a = np.column_stack([m["vx"], m["vy"], m["vz"], m["temp"]]).astype(np.float64)
    out["ref"] = sr.mesh(np.stack([m["x"], m["y"], m["z"]], axis=1), m["h"], m["m"], BOX[0], N, a=a)
    return out


@pytest.mark.parametrize("name", [s[0] for s in worker.SPECTRA])
def test_every_rank_has_the_same_spectrum(ranks, name):
    for d in ranks[1:]:
        assert np.array_equal(d[name + "_power"].view(np.uint64), ranks[0][name + "_power"].view(np.uint64))
        assert np.array_equal(d[name + "_modes"], ranks[0][name + "_modes"])
    assert np.array_equal(ranks[0][name + "_modes"], sx.spectrum_modes(N)) and (ranks[0][name + "_power"] >= 0).all()


def test_refusal_on_one_rank_reaches_every_rank(ranks):
    """rank 0's pair cap refuses its deposit; the others learn of it through the reduction instead of waiting in it, and
    the next spectrum is whole again"""
    assert "pair cap" in str(ranks[0]["refusal"]) and "code 4" in str(ranks[0]["refusal"])
    for d in ranks[1:]:
        assert "refused on another rank" in str(d["refusal"]) and "code 4" in str(d["refusal"])
    for d in ranks:
        assert np.array_equal(d["after_refusal_power"], ranks[0]["energy_power"])


def fft_bound(n):
    mu = 2.0 ** -52
    g4 = 4 * 2.0 ** -53 / (1 - 4 * 2.0 ** -53)
    eta = mu + g4 * (np.sqrt(2.0) + mu)
    t = 3 * np.log2(n)
    return t * eta / (1 - t * eta)


@pytest.mark.parametrize("name", [s[0] for s in worker.SPECTRA])
def test_spectrum_agrees_with_one_rank(ranks, one_rank, name):
    power, modes, stats = one_rank[name]
    ref = one_rank["ref"]
    r = (ref["count"] + len(ranks)) * U
    s0 = ref["sum0"]
    if name == "density":
        pre, e2 = 1.0, (r * s0) ** 2
    else:
        p, pre, cols = {"energy": (0.5, 0.5, [0, 1, 2]), "mean": (0.0, 0.5, [0, 1, 2]), "temp": (0.0, 1.0, [3])}[name]
        f = np.zeros_like(s0)
        f[s0 > 0] = s0[s0 > 0] ** (p - 1.0)
        e2 = sum((f * r * (ref["abs1"][a] + abs(1.0 - p) * np.abs(ref["sum1"][a]))) ** 2 for a in cols)
    E = float(np.sqrt(pre * np.mean(e2)))
    got = ranks[0][name + "_power"]
    total = np.sqrt(power.sum())
    slack = (2 * fft_bound(N) + modes.astype(np.float64) * 2.0 ** -52) * total
    use = float((np.maximum(np.abs(np.sqrt(got) - np.sqrt(power)) - slack, 0.0) / E).max())
    print(f"{len(ranks)} ranks, {name}: E / sqrt(P_total) = {E / total:.2e}, worst use of the regrouping bound {use:.3f}")
    assert use <= 1.0
    # each particle is local to one rank
    assert sum(int(d[name + "_stats"][0]) for d in ranks) == stats["pairs"]
    assert sum(int(d[name + "_stats"][3]) for d in ranks) == stats["clamped"]
