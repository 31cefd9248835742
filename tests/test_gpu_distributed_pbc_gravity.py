"""Periodic self-gravity with several ranks (the reference composes it in gravity_wrapper.hpp:133-157:
the Barnes-Hut walk over one shell of periodic images, then the Ewald correction from the global root multipole).

sx_sim's multi-rank gravity (sx_sim_gravity.cpp distributedGravity) walks its near tree (locals + gravity halos) and its far
tree (level-6 cell multipoles) over the images; the near/far split tests the cells' images; the Ewald correction takes
the two trees' combined root.  On the periodic density-wave IC (oracle/pyoracle.py pbc_wave_state, 16^3 particles,
G = 1), one step on 1 rank (the single-rank image walk) and on 2 and 3 ranks (host-staged transport on one GPU):
* gravity part of a (total minus the oracle's hydro-only step) against the 27-image softened direct sum + the oracle's
  Ewald correction (tests/pbc_gravity_ref.py): median 4e-3, max 1e-2 of the largest |a| (the Barnes-Hut error of
  theta = 0.5 with quadrupoles; the walk's error is relative to the images' whole field, most of which the Ewald term
  cancels -- one rank, i.e. the image walk pinned to the reference's own in tests/test_gpu_ewald.py: 1.6e-3 / 3.2e-3);
* several ranks against one: median 1e-3, max 1e-2 of the largest |a| (measured 6e-4 / 3e-3); egrav within 2e-3 of
  the one-rank value (measured 8e-4: egrav is the small remainder of the images' energy and the Ewald term's);
* nc exact against the oracle; both source paths used (far cells and gravity halos on every rank)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pbc_gravity_ref as pr
import pyoracle as po

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = 16


def run(tmp_path, nproc, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker.py"), "--out",
           str(tmp_path), "--side", str(SIDE), "--steps", "1", "--ic", "pbc_wave"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ranks = [dict(np.load(os.path.join(tmp_path, f"rank{q}.npz"))) for q in range(nproc)]
    got = {k: np.concatenate([d[f"s0_{k}"] for d in ranks]) for k in ("id", "nc", "ax", "ay", "az")}
    o = np.argsort(got["id"])
    got = {k: v[o] for k, v in got.items()}
    got["egrav"] = float(ranks[0]["s0_conserved"][2])
    got["gravity"] = [d["s0_gravity"] for d in ranks]
    return got


@pytest.fixture(scope="module")
def reference():
    st, obox = po.pbc_wave_state(SIDE)
    ora = po.load_oracle()
    hydro = st.copy()
    ora.step(hydro, obox, params=ora.params(g=0.0))
    oh = np.argsort(hydro.id)
    a_h = np.stack([hydro.ax[oh], hydro.ay[oh], hydro.az[oh]], 1).astype(np.float64)
    a_g, eg = pr.periodic_field(st.x, st.y, st.z, st.m, st.h, 1.0)
    return {"n": st.n, "nc": hydro.nc[oh], "a_h": a_h, "a_g": a_g, "egrav": eg, "runs": {}}


@pytest.mark.parametrize("nproc,port", [(1, 29681), (2, 29682), (3, 29683)])
def test_periodic_gravity_ranks(tmp_path, reference, nproc, port):
    got = run(tmp_path, nproc, port)
    ref = reference
    assert np.array_equal(got["id"], np.arange(ref["n"]))
    assert np.array_equal(got["nc"], ref["nc"])
    a = np.stack([got["ax"], got["ay"], got["az"]], 1).astype(np.float64) - ref["a_h"]
    scale = np.abs(ref["a_g"]).max()
    err = np.linalg.norm(a - ref["a_g"], axis=1) / scale
    print(f"{nproc} rank(s): gravity vs 27-image direct sum + Ewald: median {np.median(err):.2g}, max {err.max():.2g} "
          f"of max|a| {scale:.3g}; egrav {got['egrav']:.8g} vs {ref['egrav']:.8g}; (halos, far, remote cells) "
          f"{[tuple(int(v) for v in g) for g in got['gravity']]}")
    assert np.median(err) < 4e-3 and err.max() < 1e-2, (np.median(err), err.max())
    ref["runs"][nproc] = (a, got["egrav"])
    if nproc > 1:
        for halos, far_cells, remote_cells in got["gravity"]:
            assert 0 < far_cells < remote_cells and halos > 0
        if 1 in ref["runs"]:
            a1, e1 = ref["runs"][1]
            d = np.linalg.norm(a - a1, axis=1) / scale
            print(f"  against 1 rank: median {np.median(d):.2g}, max {d.max():.2g}; egrav {got['egrav'] / e1 - 1:.2g}")
            assert np.median(d) < 1e-3 and d.max() < 1e-2
            assert abs(got["egrav"] / e1 - 1) < 2e-3
