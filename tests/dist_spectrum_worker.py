"""Worker of tests/test_gpu_distributed_spectrum.py (launched by torch.distributed.run with the gloo control plane, as
tests/dist_map_worker.py):

  python -m torch.distributed.run --nproc-per-node P --master-addr 127.0.0.1 --master-port X \
      tests/dist_spectrum_worker.py --out DIR [--side S] [--steps K]

Each rank owns an index slice of the Sedov IC, runs K distributed VE steps over the host transport, takes the spectra of
SPECTRA with Sim.spectrum and writes them, its deposit statistics and its local particles to DIR/rank<r>.npz; in between,
rank 0 alone sets a pair cap that refuses its deposit.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sph-exa_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

FIELDS = ["id", "x", "y", "z", "h", "m", "vx", "vy", "vz", "temp"]
N = 16
#: (name, keywords of Sim.spectrum)
SPECTRA = [("energy", dict(n=N, kind="velocity", weight="energy")), ("mean", dict(n=N, kind="velocity")),
           ("temp", dict(n=N, kind="scalar", field="temp")), ("density", dict(n=N, kind="scalar"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--side", type=int, default=10)
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
    for name, kw in SPECTRA:
        _, power, modes = sim.spectrum(**kw)
        out[name + "_power"], out[name + "_modes"] = power, modes
        out[name + "_stats"] = np.array(list(sim.spectrum_stats().values()), dtype=np.uint64)
    # a refusal only rank 0 meets (its pair cap): every rank must come back with an error, none may wait in the reduction
    if rank == 0:
        sim.set_spectrum_pair_cap(1)
    try:
        sim.spectrum(**SPECTRA[0][1])
        out["refusal"] = np.array("")
    except sx.SxError as e:
        out["refusal"] = np.array(str(e))
    sim.set_spectrum_pair_cap(0)
    _, again, _ = sim.spectrum(**SPECTRA[0][1])
    out["after_refusal_power"] = again
    out.update(sim.get(FIELDS))
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **out)
    sim.close()
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
