"""Worker of tests/test_gpu_distributed_nbody.py (launched by torch.distributed.run with the gloo control plane).

  python -m torch.distributed.run --nproc-per-node P --master-addr 127.0.0.1 --master-port X \
      tests/dist_nbody_worker.py --out DIR [--side S] [--steps K]

Each rank owns an index slice of po.evrard_state(S), runs K gravity-only steps (propagator 3) over the host-staged
transport and writes its local particles and scalars after the last step to DIR/rank<r>.npz.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sph-exa_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

FIELDS = ["id", "x", "y", "z", "h", "m", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "ax", "ay", "az"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--side", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()

    import torch.distributed as dist

    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    import pyoracle as po
    import sphexa_amd as sx

    ctx = sx.Context(0)
    comm = sx.Comm("host")
    st, obox = po.evrard_state(args.side)
    box = sx.make_box(list(obox.lim), list(obox.bnd))
    sim = sx.Sim(ctx, 2 * st.n // size + 4096, box, params=sx.default_params(g=1.0, theta=0.5), propagator=3)
    if size > 1:
        sim.set_comm(comm)
    f, l = st.n * rank // size, st.n * (rank + 1) // size
    keep = ("x", "y", "z", "h", "m", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "id")
    sim.set_state({k: st.arrays[k][f:l] for k in keep}, st.minDt, st.minDt_m1)
    dts = []
    for _ in range(args.steps):
        sim.step()
        dts.append(sim.scalars()["minDt"])
    out = sim.get(FIELDS)
    sc = sim.scalars()
    out["dts"] = np.array(dts)
    out["scalars"] = np.array([sc["minDt"], sc["minDt_m1"], sc["ttot"]])
    cq = sim.conserved()
    out["conserved"] = np.array([cq[k] for k in ("ecin", "eint", "egrav", "etot")])
    gs = sim.gravity_stats()
    out["gravity"] = np.array([gs["halos"], gs["far_cells"], gs["remote_cells"]])
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **out)
    sim.close()
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
