"""Multi-rank VE steps on one GPU (host-staged transport, gloo control plane) against the single-domain oracle.

The SFC decomposition, particle exchange, halo discovery and the five halo exchanges per step must not change
the physics: after step 1 (identical inputs) every particle's nc and h equal the oracle's and the float fields
agree within the full-step tolerance of test_gpu_parity.py; the global time-step is identical on all ranks.
(On the Sedov lattice the h-nc iteration does not trigger, so the reference's stale-halo-h convention does not
come into play.)  RCCL with several ranks needs one GPU per rank (bench.py --gpus N on a full node); the RCCL
transport's own calls run here on a one-rank communicator (test_rccl_one_rank_transport).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import pyoracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["x", "y", "z", "vx", "vy", "vz", "temp", "x_m1", "y_m1", "z_m1", "du_m1", "alpha", "xm", "kx", "prho", "c",
          "divv", "c11", "c22", "c33", "du", "ax", "ay", "az"]


def run_ranks(tmp_path, nproc, side, steps, port, ic="sedov"):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker.py"), "--out",
           str(tmp_path), "--side", str(side), "--steps", str(steps), "--ic", ic]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{q}.npz"))) for q in range(nproc)]


def merged(ranks, s):
    out = {}
    for k in ["id", "nc", "h"] + FIELDS:
        out[k] = np.concatenate([d[f"s{s}_{k}"] for d in ranks])
    o = np.argsort(out["id"])
    return {k: v[o] for k, v in out.items()}


@pytest.mark.parametrize("nproc,port,side", [(2, 29641, 16), (3, 29642, 16), (8, 29644, 24)])
def test_distributed_steps_match_oracle(tmp_path, nproc, port, side):
    """8 ranks = one node's GPUs (seven peers per rank), all on the one GPU of the test box"""
    steps = 2
    ranks = run_ranks(tmp_path, nproc, side, steps, port)
    st, obox = po.sedov_state(side)
    ora = po.load_oracle()
    ref = st.copy()
    for s in range(steps):
        ora.step(ref, obox)
        got = merged(ranks, s)
        assert got["id"].size == st.n and np.array_equal(got["id"], np.arange(st.n))
        o = np.argsort(ref.id)
        if s == 0:
            assert np.array_equal(got["nc"], ref.nc[o])
            assert np.array_equal(got["h"], ref.h[o])
        for k in FIELDS:
            a = got[k].astype(np.float64)
            b = ref.arrays[k][o].astype(np.float64)
            tol = 1e-4 * np.abs(b) + 1e-5 * np.max(np.abs(b))
            assert np.all(np.abs(a - b) <= tol), (s, k, np.max(np.abs(a - b) / (np.abs(b) + 1e-300)))
        dts = {tuple(d[f"s{s}_scalars"]) for d in ranks}
        assert len(dts) == 1  # identical global time-step on every rank
        # conserved quantities summed over ranks (computeConservedQuantities' MPI_Reduce): same on every rank and
        # equal to the sums over the merged state
        cqs = np.array([d[f"s{s}_conserved"] for d in ranks])
        assert np.allclose(cqs, cqs[0], rtol=1e-12, atol=0)
        hs = po.HostState(st.n)
        for k in ("x", "y", "z", "vx", "vy", "vz", "temp"):
            hs.arrays[k][:] = got[k]
        hs.m[:] = st.m[0]
        hs.nc[:] = got["nc"]
        ek, ei, _, _, nc = po.conserved_quantities(hs)
        assert cqs[0][0] == pytest.approx(ek, rel=1e-10) and cqs[0][1] == pytest.approx(ei, rel=1e-10)
        assert cqs[0][4] == nc
        assert list(dts)[0][0] == pytest.approx(ref.minDt, rel=1e-5)
        # every rank holds halos and a non-empty local range
        for d in ranks:
            first, last, n, _ = d[f"s{s}_layout"]
            assert last > first and n > last - first


def test_distributed_box_steps_match_oracle(tmp_path):
    """2 ranks, 3 steps in `windshock` (0.5 x 0.125 x 0.125 periodic: the longest axis 4 times the others, which the
    halo margin and the halo layout see in no cube), then in `mixed` (a periodic, an open and a fixed axis off the
    origin), against the single-domain oracle from the same converged h: nc and h exact on every step, the float
    fields within compare_state's bounds"""
    import box_cases as bc
    from test_gpu_parity import compare_state

    ora = po.load_oracle()
    for name, port in (("windshock", 29645), ("mixed", 29646)):
        out = tmp_path / name
        out.mkdir()
        steps = 3
        ranks = run_ranks(out, 2, 0, steps, port, ic="box:" + name)
        st, obox = bc.state(name)
        po.converge_h(ora, st, obox)  # as the worker: halos keep the pre-iteration h, so start from the converged one
        ref = st.copy()
        for s in range(steps):
            ora.step(ref, obox)
            got = merged(ranks, s)
            assert got["id"].size == st.n and np.array_equal(got["id"], np.arange(st.n)), (name, s)
            compare_state(got, ref, strict_discrete=True)
            dts = {tuple(d[f"s{s}_scalars"]) for d in ranks}
            assert len(dts) == 1 and list(dts)[0][0] == pytest.approx(ref.minDt, rel=1e-5), (name, s)
            for d in ranks:
                first, last, n, _ = d[f"s{s}_layout"]
                assert last > first and n > last - first, (name, s)


def test_distributed_device_ic_conserves(tmp_path):
    """slab IC generated on the device per rank, first sync redistributes by SFC; energy conserved"""
    ranks = run_ranks(tmp_path, 2, 20, 3, 29643, ic="sedov_dev")
    got = merged(ranks, 2)
    assert got["id"].size == 20 ** 3 and np.array_equal(got["id"], np.arange(20 ** 3))
    st, _ = po.sedov_state(20)
    e0 = po.total_energy(st)
    hs = po.HostState(st.n)
    for k in ("vx", "vy", "vz", "temp"):
        hs.arrays[k][:] = got[k]
    hs.m[:] = st.m
    assert abs(po.total_energy(hs) / e0 - 1) < 1e-6


def run_ranks_opts(tmp_path, nproc, side, steps, port, ic, extra=()):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker.py"), "--out",
           str(tmp_path), "--side", str(side), "--steps", str(steps), "--ic", ic, *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [dict(np.load(os.path.join(tmp_path, f"rank{q}.npz"))) for q in range(nproc)]


def direct_gravity(x, y, z, m, h, G=1.0):
    """softened direct sum (P2P of kernel.hpp:514-535 over all pairs, R^2 >= (h_i + h_j)^2), in float64"""
    n = x.size
    a = np.zeros((n, 3))
    P = np.stack([x, y, z], 1)
    for i0 in range(0, n, 512):
        i1 = min(n, i0 + 512)
        d = P[None, :, :] - P[i0:i1, None, :]
        R2 = np.sum(d * d, axis=2)
        hij = (h[i0:i1, None].astype(np.float64) + h[None, :])
        R2e = np.maximum(R2, hij * hij)
        w = m[None, :] / (R2e * np.sqrt(R2e))
        a[i0:i1] = G * np.einsum("ij,ijk->ik", w, d)
    return a


@pytest.mark.parametrize("nproc,port", [(2, 29651), (3, 29652)])
def test_distributed_gravity_matches_direct_sum(tmp_path, nproc, port):
    """multi-rank self-gravity (near halos + far level-6 cell multipoles) on the Evrard substitute: the gravity part
    of the GPU acceleration (total minus the oracle's hydro-only acceleration) against a softened direct sum, within
    the Barnes-Hut error of theta = 0.5 with quadrupoles (median 1e-3, max 1e-2 of |a|; the single-rank oracle
    shows 1e-4 / 1.8e-3 on this IC); the hydro part and every
    other field of step 1 against the single-rank oracle with gravity"""
    side = 20
    ranks = run_ranks_opts(tmp_path, nproc, side, 1, port, "evrard")
    got = {}
    for k in ["id", "h", "nc", "ax", "ay", "az", "x", "y", "z", "temp"]:
        got[k] = np.concatenate([d[f"s0_{k}"] for d in ranks])
    o = np.argsort(got["id"])
    got = {k: v[o] for k, v in got.items()}
    ora = po.load_oracle()
    st, obox = po.evrard_state(side)
    po.converge_h(ora, st, obox)  # as the worker: no h iteration left in the step (halos keep pre-iteration h)
    assert np.array_equal(got["id"], np.arange(st.n))
    # hydro-only forces from the oracle on the same IC
    hydro = st.copy()
    ora.step(hydro, obox, params=ora.params(g=0.0))
    oh = np.argsort(hydro.id)
    hu = st.h.copy()
    ag = direct_gravity(st.x, st.y, st.z, st.m.astype(np.float64), hu)
    a_gpu = np.stack([got["ax"], got["ay"], got["az"]], 1).astype(np.float64)
    a_h = np.stack([hydro.ax[oh], hydro.ay[oh], hydro.az[oh]], 1).astype(np.float64)
    err = np.linalg.norm(a_gpu - a_h - ag, axis=1) / np.linalg.norm(ag, axis=1)
    assert np.median(err) < 1e-3 and np.max(err) < 1e-2, (np.median(err), np.max(err))
    # the reference's own multi-rank gravity on the same IC (Domain::syncGrav + computeGlobalMultipoles +
    # computeGravity under MPICH with 2 ranks, oracle/gen_grav_mpi.py): two Barnes-Hut trees of theta = 0.5 (the
    # reference's focus tree vs this library's local + level-6 far tree), so within the opening-angle error
    fx = gu.load("evrard20_grav_mpi.npz")
    assert np.array_equal(fx["x"], st.x) and np.array_equal(fx["h"], st.h)
    a_ref = fx["acc_p2"].astype(np.float64)
    err_ref = np.linalg.norm(a_gpu - a_h - a_ref, axis=1) / np.linalg.norm(a_ref, axis=1)
    egrav_gpu = ranks[0]["s0_conserved"][2]
    print(f"{nproc} ranks vs the reference's 2-rank gravity: median {np.median(err_ref):.2g}, max {err_ref.max():.2g}; "
          f"egrav {egrav_gpu:.8g} vs {fx['egrav_p2'][0]:.8g}")
    assert np.median(err_ref) < 1e-3 and np.max(err_ref) < 1e-2, (np.median(err_ref), err_ref.max())
    assert abs(egrav_gpu / fx["egrav_p2"][0] - 1) < 1e-3
    # both source paths were exercised: some remote cells far (multipoles), some near (gravity halos)
    for d in ranks:
        halos, far_cells, remote_cells = d["s0_gravity"]
        assert 0 < far_cells < remote_cells and halos > 0, d["s0_gravity"]
    # the full step with gravity: nc exact, everything else within the BH error of the accelerations
    full = st.copy()
    ora.step(full, obox, params=ora.params(g=1.0))
    of = np.argsort(full.id)
    assert np.array_equal(got["nc"], full.nc[of])
    for k in ["x", "y", "z", "temp"]:
        a, b = got[k].astype(np.float64), full.arrays[k][of].astype(np.float64)
        assert np.all(np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-5 * np.max(np.abs(b))), k


@pytest.mark.parametrize("nproc,port", [(2, 29661)])
def test_distributed_std_steps_match_oracle(tmp_path, nproc, port):
    """std propagator with the SFC decomposition: halos of v, rho, p, c then c_ij (std_hydro.hpp:150-158)"""
    side, steps = 16, 2
    ranks = run_ranks_opts(tmp_path, nproc, side, steps, port, "sedov", ("--std",))
    st, obox = po.sedov_state(side)
    ora = po.load_oracle()
    ref = st.copy()
    p = ora.params(std=True)
    fields = ["x", "y", "z", "vx", "vy", "vz", "temp", "rho", "p", "c", "c11", "c22", "c33", "du", "ax", "ay", "az"]
    for s in range(steps):
        ora.step(ref, obox, params=p)
        got = {k: np.concatenate([d[f"s{s}_{k}"] for d in ranks]) for k in ["id", "nc", "h"] + fields}
        og = np.argsort(got["id"])
        o = np.argsort(ref.id)
        if s == 0:
            assert np.array_equal(got["nc"][og], ref.nc[o]) and np.array_equal(got["h"][og], ref.h[o])
        for k in fields:
            a = got[k][og].astype(np.float64)
            b = ref.arrays[k][o].astype(np.float64)
            tol = 1e-4 * np.abs(b) + 1e-5 * np.max(np.abs(b))
            assert np.all(np.abs(a - b) <= tol), (s, k, np.max(np.abs(a - b) / (np.abs(b) + 1e-300)))


@pytest.mark.parametrize("opts,port", [((), 29661), (("--std",), 29662), (("--av-clean",), 29663)])
def test_overlapped_exchanges_bitwise_equal_serial(tmp_path, opts, port):
    """halo exchanges overlapped with the interior clusters (communication stream, interior/boundary cluster lists,
    ve_hydro.hpp:150-186 exchange points) give bitwise the same state as the serial exchanges, for the VE, avClean
    and std propagators; the split is real (both lists non-empty) and covers every cluster"""
    side, steps, nproc = 32, 2, 2
    a_dir, b_dir = tmp_path / "ovl", tmp_path / "ser"
    a_dir.mkdir()
    b_dir.mkdir()
    ovl = run_ranks_opts(a_dir, nproc, side, steps, port, "sedov", opts)
    ser = run_ranks_opts(b_dir, nproc, side, steps, port + 100, "sedov", opts + ("--no-overlap",))
    keys = [k for k in ovl[0] if not k.endswith("_overlap")]
    for q in range(nproc):
        for k in keys:
            assert np.array_equal(ovl[q][k], ser[q][k], equal_nan=True), (q, k)
        for s in range(steps):
            first, last, _, _ = ovl[q][f"s{s}_layout"]
            ncl = (last - first + 255) // 256
            inner, bound = ovl[q][f"s{s}_overlap"]
            assert inner + bound == ncl and inner > 0 and bound > 0, (q, s, inner, bound, ncl)
            assert tuple(ser[q][f"s{s}_overlap"]) == (0, 0)


def test_rccl_one_rank_transport():
    """the RCCL transport (sx_comm.cpp RcclTransport) executes on the device: a one-rank communicator from a real
    ncclGetUniqueId / ncclCommInitRank, the self segment of alltoallv (device copy + an empty ncclGroupStart/End),
    and ncclAllReduce sum-u32 / min-f64 / sum-f64 in place on device buffers, each checked against the host values"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29671", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_worker.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "RCCL one-rank OK" in r.stdout, r.stdout[-2000:]
