"""Cost of the two-point statistics (sx_sim_twopoint, Sim.twopoint) next to the first step of the route they replace
(copying x, y, z, m, vx, vy, vz to the host: 40 B per particle) and next to the pair search they share a grid with (the
link stage of Sim.fof at linking = r_max: the same cells, the same pair tests, a union in the place of the bins).

    python -m sphexa_amd.twopoint_bench [--plummer 1048576] [--side 100] [--steps 20] --out profiles/twopoint_mi355x.json

One process, one MI355X, two states: ic.turbulence(side) stirred for `steps` VE steps in its periodic box, and
ic.plummer(n) under the gravity-only propagator.  Bins: `--bins` (32) log-spaced from r_max / 100 to r_max = `--rmax` (4)
mean interparticle spacings (V_box / N)^(1/3); on the Plummer sphere, whose box is mostly empty, the spacing is that of the
half-mass sphere.  Per state, for stride 1 and `--stride` (8) and for counts only and all series: the median of `reps`
host-clock times of Sim.twopoint, the HIP-event times of the four stages, pairs tested and binned per second of the pair
stage; then the stage times of Sim.fof at linking = r_max and the ratio pair stage / link stage; the host-clock time of
Sim.get of the seven columns.  Prints one JSON line and writes it to --out; needs a GPU.
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


def measure(sx, ctx, sim, a, name, spacing):
    n = sim.size()
    rmax = a.rmax * spacing
    edges = np.geomspace(rmax / 100.0, rmax, a.bins + 1)
    before = sim.memory()
    sim.twopoint(edges, series=("count",))
    added = sim.memory()["device"] - before["device"]
    out = dict(state=name, particles=n, mean_spacing=spacing, r_max=rmax, bins=a.bins,
               grid=sx.twopoint_grid(sx.SxTwoPoint(edges), sim.box, n), scratch_bytes=added,
               scratch_bytes_per_particle=added / n, runs=[])
    for stride in (1, a.stride):
        for label, series, mass in (("counts", ("count",), False), ("all", ("count", "vel"), True)):
            spec = sim.twopoint_spec(edges, series, stride, 0, mass)
            run = dict(stride=stride, series=label)
            run["call_ms"], run["call_ms_min"] = timed(lambda: sim.twopoint(spec=spec), a.reps)
            ctx.set_twopoint_timing(True)
            stages = []
            for _ in range(a.reps):
                sim.twopoint(spec=spec)
                stages.append(ctx.twopoint_times())
            ctx.set_twopoint_timing(False)
            run.update({k: float(np.median([s[k] for s in stages])) for k in stages[0]})
            stats = sim.twopoint_stats()
            run.update(stats)
            run["accepted_fraction"] = stats["pairs_binned"] / max(1, stats["pairs_tested"])
            run["pairs_tested_per_s"] = stats["pairs_tested"] / (run["pairs_ms"] * 1e-3) if run["pairs_ms"] else None
            run["pairs_binned_per_s"] = stats["pairs_binned"] / (run["pairs_ms"] * 1e-3) if run["pairs_ms"] else None
            out["runs"].append(run)
    # the yardstick: the group finder's link stage on the same grid
    fof = sx.SxFof(rmax, 20, 4096)
    sim.fof(spec=fof)
    ctx.set_fof_timing(True)
    stages = []
    for _ in range(a.reps):
        sim.fof(spec=fof)
        stages.append(ctx.fof_times())
    ctx.set_fof_timing(False)
    link = float(np.median([s["link_ms"] for s in stages]))
    tests = sim.fof_stats()["pair_tests"]
    out.update(fof_link_ms=link, fof_pair_tests=tests, fof_tests_per_s=tests / (link * 1e-3) if link else None)
    for run in out["runs"]:
        run["pairs_over_fof_link"] = run["pairs_ms"] / link if link else None
    sim.get(COLUMNS)
    out["host_copy_ms"], out["host_copy_ms_min"] = timed(lambda: sim.get(COLUMNS), a.reps)
    out["host_copy_bytes"] = 40 * n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plummer", type=int, default=1 << 20, help="bodies of the Plummer sphere (0: skip)")
    ap.add_argument("--side", type=int, default=100, help="lattice side of the turbulence box (0: skip)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rmax", type=float, default=4.0, help="r_max in mean interparticle spacings")
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import sphexa_amd as sx
    from sphexa_amd import ic

    res = dict(rmax_spacings=a.rmax, bins=a.bins, reps=a.reps, states=[])
    ctx = sx.Context(0)
    if a.side:
        f, lim, bnd, dt0 = ic.turbulence(a.side)
        sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), ic.turbulence_params(sx.default_params()))
        try:
            sim.set_state(f, dt0, dt0)
            sim.set_turbulence(Lbox=lim[1] - lim[0])
            for _ in range(a.steps):
                sim.step()
            ctx.sync()
            vol = (lim[1] - lim[0]) * (lim[3] - lim[2]) * (lim[5] - lim[4])
            res["states"].append(measure(sx, ctx, sim, a, f"ic.turbulence({a.side}), stirred VE, {a.steps} steps",
                                         (vol / sim.size()) ** (1.0 / 3.0)))
        finally:
            sim.close()
    if a.plummer:
        f, lim, bnd, dt0 = ic.plummer(a.plummer)
        sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), sx.default_params(g=1.0, theta=0.5, nbody=True))
        try:
            sim.set_state(f, dt0, dt0)
            sim.step()
            # half of the mass lies within 1.305 a: the spacing of that sphere
            spacing = (4.0 * np.pi / 3.0 * 1.305 ** 3 / (0.5 * sim.size())) ** (1.0 / 3.0)
            res["states"].append(measure(sx, ctx, sim, a, f"ic.plummer({a.plummer}), gravity only, 1 step", spacing))
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
