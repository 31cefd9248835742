"""Worker of tests/test_gpu_distributed_cooling.py (launched by torch.distributed.run with the gloo control plane, as
tests/dist_profile_worker.py):

  python -m torch.distributed.run --nproc-per-node P --master-addr 127.0.0.1 --master-port X \
      tests/dist_cooling_worker.py --out DIR [--side S] [--steps K]

Each rank owns an index slice of the lattice at rest (ic.turbulence), runs K distributed VE steps over the host
transport twice -- first without cooling (the twin that measures the hydrodynamic rounding drift), then with the table
and the limiter of run() -- and writes its local particles, every step's time-step and rho, and its cooling figures to
DIR/rank<r>.npz.
The test calls run() itself for the one-rank figures.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sph-exa_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ["id", "temp", "m", "kx", "xm"]
STRENGTH, CT_CRIT = 6e5, 0.1


def run(sx, ctx, side, steps, cool, comm=None, rank=0, size=1):
    """K steps of this rank's slice of the lattice; dict of the locals, the steps' minDt and the cooling figures"""
    import cooling_ref as cr
    from sphexa_amd import cooling, ic

    f, lim, bnd, dt0 = ic.turbulence(side)
    n = len(f["x"])
    sim = sx.Sim(ctx, 2 * n // size + 4096, sx.make_box(lim, bnd), ic.turbulence_params(sx.default_params()))
    if comm is not None:
        sim.set_comm(comm)
    a, b = n * rank // size, n * (rank + 1) // size
    sim.set_state({k: v[a:b] for k, v in f.items()}, dt0, dt0)
    table = cooling.Cooling(*cr.scaled_table(f["temp"][0], STRENGTH)) if cool else None
    if cool:
        sim.set_cooling(table, ct_crit=CT_CRIT)
    out = {"minDt": [], "minDtCool": [], "radiated": []}
    for k in range(steps):
        sim.step()
        out["minDt"].append(sim.scalars()["minDt"])
        # the step's rho by id (particles change their place, and their rank, from step to step)
        g = sim.get(["id", "kx", "m", "xm"])
        out[f"id_step{k}"], out[f"rho_step{k}"] = g["id"], cr.sim_rho(g, False)
        if cool:
            st = sim.cooling_stats()
            out["minDtCool"].append(st["minDtCool"])
            out["radiated"].append(st["radiated"])
    if cool:
        out["radiated_total"] = sim.cooling_stats()["radiated_total"]
    out.update(sim.get(FIELDS))
    sim.close()
    if table is not None:
        table.close()
    return {k: np.asarray(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--side", type=int, default=16)
    ap.add_argument("--steps", type=int, default=4)
    args = ap.parse_args()

    import torch.distributed as dist

    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    import sphexa_amd as sx

    ctx = sx.Context(0)
    comm = sx.Comm("host")
    twin = run(sx, ctx, args.side, args.steps, False, comm, rank, size)
    cooled = run(sx, ctx, args.side, args.steps, True, comm, rank, size)
    out = dict(cooled)
    out.update({"twin_" + k: twin[k] for k in ("id", "temp", "minDt")})
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **out)
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
