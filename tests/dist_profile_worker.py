"""Worker of tests/test_gpu_distributed_profile.py (launched by torch.distributed.run with the gloo control plane, as
tests/dist_spectrum_worker.py):

  python -m torch.distributed.run --nproc-per-node P --master-addr 127.0.0.1 --master-port X \
      tests/dist_profile_worker.py --out DIR [--side S] [--steps K]

Each rank owns an index slice of the Sedov IC, runs K distributed VE steps over the host transport, takes the profiles of
PROFILES with Sim.profile and writes their arrays and its local particles to DIR/rank<r>.npz; in between, rank 0 alone
asks for edges that are not ascending.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sph-exa_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

FIELDS = ["id", "x", "y", "z", "h", "m", "vx", "vy", "vz", "temp", "kx", "xm", "c", "divv", "curlv", "alpha"]
ARRAYS = ["count", "nonfinite", "W", "S1", "S2", "D", "min", "max"]
_R = np.linspace(0.0, 0.9, 30)
TABLE = ("table", _R, 1.0 + 3.0 * np.exp(-((_R - 0.2) / 0.05) ** 2))
#: (name, keywords of Sim.profile); the centre near a face: the minimum image crosses the rank boundaries
PROFILES = [
    ("radial", dict(edges=np.linspace(0.0, 0.6, 13), quantities=("rho", "p", "vel", "u"), solutions={"rho": TABLE})),
    ("face", dict(edges=np.linspace(0.0, 0.8, 300), quantities=("vrad", "c", "divv", "temp"), weight="mass",
                  center=(0.45, -0.48, 0.1), solutions={"temp": ("table", [0.0, 1.0], [0.0, 1e-15])})),
    ("axis", dict(edges=np.linspace(-0.5, 0.5, 5), quantities=("curlv",), coord="z", center=(0.0, 0.0, 0.0))),
    ("pdf", dict(edges=np.logspace(-0.2, 0.2, 9), quantities=("h", "alpha"), coord="rho", weight="mass",
                 solutions={"h": ("noh", dict(time=0.1))})),
]


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
    for name, kw in PROFILES:
        res = sim.profile(**kw)
        for k in ARRAYS:
            out[f"{name}_{k}"] = res["raw"][k]
        out[f"{name}_particles"] = np.array(sim.profile_stats()["particles"])
    # a specification only rank 0 makes unacceptable: every rank must come back with an error, none may wait
    kw = dict(PROFILES[0][1])
    if rank == 0:
        kw["edges"] = kw["edges"][::-1].copy()
    try:
        sim.profile(**kw)
        out["refusal"] = np.array("")
    except sx.SxError as e:
        out["refusal"] = np.array(str(e))
    again = sim.profile(**PROFILES[0][1])
    for k in ARRAYS:
        out[f"after_refusal_{k}"] = again["raw"][k]
    out.update(sim.get(FIELDS))
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **out)
    sim.close()
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
