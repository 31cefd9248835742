"""Worker of the multi-rank skin-list test (tests/test_gpu_distributed_skin.py), launched by torch.distributed.run.

  python -m torch.distributed.run --nproc-per-node P ... tests/dist_skin_worker.py --out DIR
      --ic sedov|noh|evrard|converge [--side S] [--steps K] [--skin 0.08] [--max-reuse 24]

Every rank runs two simulations over the host-staged transport: `a` with skin lists (filter-served steps between
full builds), `b` with the skin off (a fresh distributed sync + search every step).  Before each step b is handed a's
state of this rank, so both step from the same global state; the rank writes, per step, ids / nc / h and the compared
fields of both, and a's skin statistics, to DIR/rank<r>.npz.

--ic converge: the cold uniform lattice (Sedov's, its energy spike replaced by the background value, h converged) at
rest, but for a patch of one rank inside a ball on its boundary with another rank, which moves towards that resting
rank (dist_oracle.converging_patch on the owners of the first sync): the clusters around the patch go stale and are
searched again at a rank boundary while particles of the peer close in.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sph-exa_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

STATE = ["x", "y", "z", "h", "m", "temp", "vx", "vy", "vz", "x_m1", "y_m1", "z_m1", "du_m1", "alpha", "id"]
FIELDS = ["id", "nc", "h", "ax", "ay", "az", "du", "x", "vx"]
SKIN = ["builds", "reuse_steps", "stale_clusters", "exact_clusters", "plain_steps", "resyncs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--ic", default="sedov")
    ap.add_argument("--side", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--skin", type=float, default=0.08)
    ap.add_argument("--max-reuse", type=int, default=24)
    ap.add_argument("--g", type=float, default=0.0, help="gravitational constant (self-gravity; evrard: 1)")
    ap.add_argument("--std", action="store_true", help="std propagator (HydroProp)")
    ap.add_argument("--av-clean", action="store_true", help="HydroVeProp<avClean=true>")
    ap.add_argument("--ball", type=float, default=3.0, help="converge: radius of the patch in lattice spacings")
    ap.add_argument("--patch-step", type=float, default=0.04,
                    help="converge: the patch's move in the step before the first, in lattice spacings (dt0 = this / "
                         "speed; dt may grow by 1.1 per step)")
    args = ap.parse_args()

    import torch.distributed as dist

    dist.init_process_group("gloo")
    rank, size = dist.get_rank(), dist.get_world_size()
    import pyoracle as po
    import sphexa_amd as sx

    ctx = sx.Context(0)
    comm = sx.Comm("host")
    st, obox = {"noh": po.noh_state, "evrard": po.evrard_state}.get(args.ic, po.sedov_state)(args.side)
    if args.ic == "converge":
        import dist_oracle as do

        ora = po.load_oracle()
        st.temp[:] = np.float64(st.temp.min())
        po.converge_h(ora, st, obox)
        # owners as the first sync assigns them, computed on the host from the whole IC
        owner = do.sfc_owners(ora, st, obox, size)
        pos = np.stack([st.x, st.y, st.z], axis=1).astype(np.float64)
        reach = 2.0 * float(st.h.max()) * do.HALO_MARGIN * (1.0 + args.skin) * args.side  # request box, in spacings
        # tilted off the lattice axes: with the velocity along an axis, a resting particle whose only moving neighbours
        # lie in its own lattice plane has divv = 0 up to rounding, and the AV switch's test divv < 0 then puts alpha
        # at alphamin or near alphamax with the order of the neighbour sum (no lattice vector up to 3 spacings is
        # perpendicular to the tilted direction)
        patch, direction, _, pair = do.converging_patch(pos, owner, obox, 1.0 / args.side, args.ball, reach,
                                                        tilt=(0.113, 0.171, 0.067))
        dt0 = args.patch_step / args.side  # unit speed
        for k, d in enumerate(("x", "y", "z")):
            st.arrays["v" + d][patch] = np.float32(direction[k])
            # the integrator's previous displacement, as pyoracle.noh_state sets it
            st.arrays[d + "_m1"][:] = (st.arrays["v" + d].astype(np.float64) * dt0).astype(np.float32)
        st.minDt = st.minDt_m1 = dt0
    if args.ic in ("evrard", "noh"):
        po.converge_h(po.load_oracle(), st, obox)  # the IC's h would iterate in the first search
    box = sx.make_box(list(obox.lim), list(obox.bnd))
    cap = 2 * st.n // size + 4096
    prm = sx.default_params(g=args.g, std=args.std, av_clean=args.av_clean)
    a, b = sx.Sim(ctx, cap, box, params=prm), sx.Sim(ctx, cap, box, params=prm)
    for sim, f in ((a, args.skin), (b, 0.0)):
        sim.set_comm(comm)
        sim.set_skin(f, args.max_reuse if f > 0 else 1)
    f0, l0 = st.n * rank // size, st.n * (rank + 1) // size
    a.set_state({k: v[f0:l0] for k, v in st.arrays.items()}, st.minDt, st.minDt_m1)
    out = {}
    for s in range(args.steps):
        g = a.get(STATE)
        sc = a.scalars()
        b.set_state(g, sc["minDt"], sc["minDt_m1"])
        a.step()
        b.step()
        fields = FIELDS + (["rho"] if args.std else ["xm", "kx", "divv", "alpha"])
        for tag, sim in (("a", a), ("b", b)):
            for k, v in sim.get(fields).items():
                out[f"s{s}_{tag}_{k}"] = v
            out[f"s{s}_{tag}_dt"] = np.array([sim.scalars()["minDt"]])
            out[f"s{s}_{tag}_egrav"] = np.array([sim.conserved()["egrav"]])
        ks = a.skin_stats()
        out[f"s{s}_skin"] = np.array([ks[k] for k in SKIN] + [ks["factor"], ks["next_factor"], ks["kept_clusters"],
                                                             ks["frozen_clusters"], ks["early_exact"]], np.float64)
        out[f"s{s}_layout"] = np.array(list(a.layout().values()), np.int64)
        if args.ic == "converge":
            # how far this rank's patch particles are from where they started (minimum image): sum, count
            g = a.get(["id", "x", "y", "z"])
            sel = patch[g["id"].astype(np.int64)]
            d = np.stack([g[k][sel] for k in ("x", "y", "z")], axis=1) - pos[g["id"].astype(np.int64)[sel]]
            d -= np.rint(d)  # the unit periodic box
            out[f"s{s}_drift"] = np.array([np.sqrt(np.sum(d * d, axis=1)).sum(), sel.sum()], np.float64)
    if args.ic == "converge":
        out["patch"] = np.array([int(patch.sum()), *pair], np.int64)
        out["spacing"] = np.array([1.0 / args.side, float(st.h.max())])
        out["patch_ids"] = st.id[patch].astype(np.int64)
    np.savez(os.path.join(args.out, f"rank{rank}.npz"), **out)
    a.close()
    b.close()
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
