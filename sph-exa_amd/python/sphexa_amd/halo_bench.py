"""Cost of the group properties (sx_sim_halos, Sim.halos): the search of fof_bench plus the moments and the segmented
all-pairs kernel of the self-energy.

    python -m sphexa_amd.halo_bench [--plummer 1048576] [--side 100] [--steps 20] --out profiles/halo_mi355x.json

One process, one MI355X, the two states of fof_bench: ic.plummer(n) under the gravity-only propagator after one step (a
core of most of the bodies in one group: the pair kernel's large case), and ic.evrard(side) under VE with self-gravity
after `steps` steps, behind a density cut at `--rho-min` (the sphere's initial density at r = 0.3 by default) with the
thermal energy.  Linking length `--linking` (0.2) mean interparticle spacings, min_members 20.  Reported per state: the
median of `reps` host-clock times of Sim.halos (it ends with the results on the host) with all flags and with the search
alone; the HIP-event times of the four stages (group search, moments, pair kernel with its scan and the host's read of the
item count, combination and copies); the pair terms, the work items and the pair rate terms / pair-kernel time; the
device bytes the first call adds to the sim's arena; the largest groups with their virial parameter.  Prints one JSON
line and writes it to --out; needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def measure(ctx, sim, a, name, rho_min, flags):
    n = sim.size()
    spec = sim.halos_spec(a.linking, None, a.min_members, a.max_groups, rho_min, flags)
    search = sim.halos_spec(a.linking, None, a.min_members, a.max_groups, rho_min, ())
    before = sim.memory()
    cat = sim.halos(spec=spec)
    added = sim.memory()["device"] - before["device"]
    out = dict(state=name, particles=n, linking_length=spec.linking, rho_min=rho_min, flags=list(flags),
               num_groups=cat["num_groups"], num_all=cat["num_all"], largest=[int(c) for c in cat["count"][:3]],
               epot=[float(v) for v in cat["epot"][:3]], ekin=[float(v) for v in cat["ekin"][:3]],
               alpha_vir=[float(v) for v in cat["alpha_vir"][:3]], scratch_bytes=added, scratch_bytes_per_particle=added / n)
    out["halos_ms"], out["halos_ms_min"] = timed(lambda: sim.halos(spec=spec), a.reps)
    out["search_only_ms"], out["search_only_ms_min"] = timed(lambda: sim.halos(spec=search), a.reps)
    ctx.set_halo_timing(True)
    stages = []
    for _ in range(a.reps):
        sim.halos(spec=spec)
        stages.append(ctx.halo_times())
    ctx.set_halo_timing(False)
    out.update({k: float(np.median([s[k] for s in stages])) for k in stages[0]})
    stats = sim.halos_stats()
    out.update(stats)
    out["pairs_per_s"] = stats["pair_terms"] / (out["pairs_ms"] * 1e-3) if out["pairs_ms"] > 0 else 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plummer", type=int, default=1 << 20, help="bodies of the Plummer sphere (0: skip)")
    ap.add_argument("--side", type=int, default=100, help="lattice side of the Evrard sphere (0: skip)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--linking", type=float, default=0.2)
    ap.add_argument("--min-members", type=int, default=20)
    ap.add_argument("--max-groups", type=int, default=4096)
    ap.add_argument("--rho-min", type=float, default=1.0 / (2.0 * np.pi * 0.3))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import sphexa_amd as sx
    from sphexa_amd import ic

    res = dict(linking=a.linking, min_members=a.min_members, reps=a.reps, states=[])
    ctx = sx.Context(0)
    if a.plummer:
        f, lim, bnd, dt0 = ic.plummer(a.plummer)
        sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), sx.default_params(g=1.0, theta=0.5, nbody=True))
        try:
            sim.set_state(f, dt0, dt0)
            sim.step()
            res["states"].append(measure(ctx, sim, a, f"ic.plummer({a.plummer}), gravity only, 1 step", 0.0,
                                         ("moments", "potential")))
        finally:
            sim.close()
    if a.side:
        f, lim, bnd, dt0 = ic.evrard(a.side)
        sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), sx.default_params(g=1.0, theta=0.5))
        try:
            sim.set_state(f, dt0, dt0)
            for _ in range(a.steps):
                sim.step()
            ctx.sync()
            res["states"].append(measure(ctx, sim, a, f"ic.evrard({a.side}), VE + self-gravity, {a.steps} steps",
                                         a.rho_min, ("moments", "thermal", "potential")))
        finally:
            sim.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
