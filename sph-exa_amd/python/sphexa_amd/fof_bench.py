"""Cost of the friends-of-friends group finder (sx_sim_fof, Sim.fof) next to the first step of the route it replaces:
copying the seven columns a host group finder needs (x, y, z, m, vx, vy, vz: 40 B per particle) to the host.

    python -m sphexa_amd.fof_bench [--plummer 1048576] [--side 100] [--steps 20] --out profiles/fof_mi355x.json

One process, one MI355X, two states: ic.plummer(n) under the gravity-only propagator (a halo core with thousands of
particles inside a linking length: the dense-cell case), and ic.evrard(side) under VE with self-gravity after `steps`
steps (a collapsing clump in an open box).  Linking length: `--linking` (0.2) mean interparticle spacings
(V_box / N)^(1/3), min_members 20.  Reported per state: the median of `reps` host-clock times of Sim.fof (it ends with
the catalogue on the host), without and with the per-particle labels; the HIP-event times of the four stages (grid, link,
compress, catalogue: a call with sx_set_fof_timing; the catalogue's interval includes the host's read of the group
count); pair tests per particle and union retries; the cell grid; the device bytes the first call adds to the sim's
arena; the host-clock time of Sim.get of the seven columns.  Prints one JSON line and writes it to --out; needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COLUMNS = ["x", "y", "z", "m", "vx", "vy", "vz"]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def measure(sx, ctx, sim, a, name):
    n = sim.size()
    spec = sim.fof_spec(a.linking, None, a.min_members, a.max_groups)
    before = sim.memory()
    cat = sim.fof(spec=spec)
    added = sim.memory()["device"] - before["device"]
    out = dict(state=name, particles=n, linking_length=spec.linking, grid=sx.fof_grid(spec, sim.box, n),
               num_groups=cat["num_groups"], num_all=cat["num_all"],
               largest=[int(c) for c in cat["count"][:3]], largest_mass=[float(m) for m in cat["mass"][:3]],
               scratch_bytes=added, scratch_bytes_per_particle=added / n)
    out["fof_ms"], out["fof_ms_min"] = timed(lambda: sim.fof(spec=spec), a.reps)
    out["fof_labels_ms"], out["fof_labels_ms_min"] = timed(lambda: sim.fof(spec=spec, labels=True), a.reps)
    ctx.set_fof_timing(True)
    stages = []
    for _ in range(a.reps):
        sim.fof(spec=spec)
        stages.append(ctx.fof_times())
    ctx.set_fof_timing(False)
    out.update({k: float(np.median([s[k] for s in stages])) for k in stages[0]})
    stats = sim.fof_stats()
    out.update(pair_tests=stats["pair_tests"], pair_tests_per_particle=stats["pair_tests"] / n,
               union_retries=stats["union_retries"])
    sim.get(COLUMNS)
    out["host_copy_ms"], out["host_copy_ms_min"] = timed(lambda: sim.get(COLUMNS), a.reps)
    out["host_copy_bytes"] = 40 * n
    out["fof_over_host_copy"] = out["fof_ms"] / out["host_copy_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plummer", type=int, default=1 << 20, help="bodies of the Plummer sphere (0: skip)")
    ap.add_argument("--side", type=int, default=100, help="lattice side of the Evrard sphere (0: skip)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--linking", type=float, default=0.2)
    ap.add_argument("--min-members", type=int, default=20)
    ap.add_argument("--max-groups", type=int, default=4096)
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
            res["states"].append(measure(sx, ctx, sim, a, f"ic.plummer({a.plummer}), gravity only, 1 step"))
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
            res["states"].append(measure(sx, ctx, sim, a, f"ic.evrard({a.side}), VE + self-gravity, {a.steps} steps"))
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
