"""Worker of tests/test_gpu_distributed_observables.py (launched by torch.distributed.run with the gloo control plane,
as tests/dist_worker.py):

  python -m torch.distributed.run --nproc-per-node P --master-addr 127.0.0.1 --master-port X \
      tests/dist_obs_worker.py --out DIR [--side S] [--steps K]

Each rank owns an index slice of the Sedov IC, runs K distributed VE steps over the host transport and, after the last
one, writes the row of Sim.observe() for the Mach RMS and for the gravitational waves and its local particles' fields
to DIR/rank<r>.npz.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sph-exa_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

FIELDS = ["id", "x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az", "m", "c", "temp", "nc"]
THETA, PHI = 0.3, 0.4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--side", type=int, default=16)
    ap.add_argument("--steps", type=int, default=2)
    args = ap.parse_args()

    import torch.distributed as dist

    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    import pyoracle as po
    import sphexa_amd as sx

    ctx = sx.Context(0)
    comm = sx.Comm("host")
    st, obox = po.sedov_state(args.side)
    sim = sx.Sim(ctx, 2 * st.n // size + 4096, sx.make_box(list(obox.lim), list(obox.bnd)))
    sim.set_comm(comm)
    f, l = st.n * rank // size, st.n * (rank + 1) // size
    sim.set_state({k: v[f:l] for k, v in st.arrays.items()}, st.minDt, st.minDt_m1)
    for _ in range(args.steps):
        sim.step()
    out = {}
    for kind in ("mach_rms", "grav_waves"):
        sim.set_observable(kind, **(dict(gravWaveTheta=THETA, gravWavePhi=PHI) if kind == "grav_waves" else {}))
        row = sim.observe()
        assert list(row) == sx.OBS_COLUMNS[kind]
        out["row_" + kind] = np.array(list(row.values()), dtype=np.float64)
    out.update(sim.get(FIELDS))
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **out)
    sim.close()
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
