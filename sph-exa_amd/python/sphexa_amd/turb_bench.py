"""Cost of the turbulence stirring inside the VE step: the periodic-box lattice of ic.turbulence(side), timed without
stirring (the unchanged VE path), with the fast stirring kernel and with the exact one.

    python sph-exa_amd/python/sphexa_amd/turb_bench.py --side 200 --steps 20 --warmup 5 --out profiles/turb_n200.json

Each mode runs in its own Sim from the same state; `off` runs again at the end to show the spread.  ms/step is a host
clock around sx_sim_step calls (each ends in a stream synchronise); the noise-advance and stirring times are the HIP
events of sx_sim_turbulence_times, averaged over the timed steps.  The fast kernel's shares of peak come from a model
kept here, evaluated on the mode table (not read from the ISA or from hardware counters): 48 B per particle (x, y, z
read; ax, ay, az read and written) against the measured HBM copy rate, and the model's float multiply/add/FMA
operations per particle against the FP32 vector rate (packed; the FP64 vector rate is half of it).
Prints one JSON line; needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sphexa_amd as sx  # noqa: E402
from sphexa_amd import ic  # noqa: E402

HBM_BYTES_PER_S = 6.29e12        # measured float4 copy rate of the MI355X
FP32_OPS_PER_S = 157.3e12 / 2    # FP32 vector peak (FLOP/s, packed), one FMA = 2 FLOP: multiply/add/FMA per second


def fast_kernel_instructions(turb, lbox):
    """a model of the float multiply / add / FMA operations per particle of the lattice kernel, from the table: per
    lattice row (i, j) with modes 4 products and 4 sums for e^{i(ix +- jy)}; per point 8 products and 8 sums for the
    four sign variants and 6 multiply-adds for each of them; 3 x 2 x 4 for the harmonics' recurrence and 3 for the
    angles; 3 for the final sums.  (The three angle reductions in double and the sincosf calls are not counted.)"""
    idx = np.rint(np.abs(turb.arrays()["modes"].reshape(-1, 3)) * lbox / (2.0 * np.pi)).astype(int)
    points = {tuple(r) for r in idx}
    rows = {(r[0], r[1]) for r in points}
    return 8 * len(rows) + (16 + 24) * len(points) + 24 + 3 + 3, len(points)


def run(ctx, state, mode, steps, warmup, lbox):
    f, lim, bnd, dt0 = state
    ctx.set_exact(False)
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), ic.turbulence_params(sx.default_params()))
    try:
        sim.set_state(f, dt0, dt0)
        if mode != "off":
            sim.set_turbulence(Lbox=lbox)
        # only the stirring kernel switches with the variant: the hydro kernels stay the production ones
        # (sx_set_exact would switch both), so the exact stirring kernel is timed through a table off the fast path
        if mode == "exact":
            st = sim.turbulence_state()
            modes = st["turbulence::modes"].copy()
            modes[np.flatnonzero(modes)[0]] *= 1.0 + 1e-6  # one component off the lattice: the exact loop
            st["turbulence::modes"] = modes
            sim.set_turbulence_state(st)
        for _ in range(warmup):
            sim.step()
        noise, stir = [], []
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            sim.step()
            if mode != "off":
                t = sim.turbulence_times()
                noise.append(t["noise"])
                stir.append(t["stirring"])
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        out = dict(mode=mode, ms_per_step=ms, stage_ms=sim.stage_times())
        if mode != "off":
            out.update(noise_ms=float(np.mean(noise)), stirring_ms=float(np.mean(stir)),
                       stirring_ms_min=float(np.min(stir)), ecin=sim.conserved()["ecin"])
            if mode == "fast":
                instr, points = fast_kernel_instructions(sim.turbulence(), lbox)
                n = len(f["x"])
                out.update(fp32_operations_per_particle=instr, lattice_points=points,
                           traffic_floor_fraction=48.0 * n / HBM_BYTES_PER_S / (out["stirring_ms"] * 1e-3),
                           fp32_rate_fraction=instr * n / FP32_OPS_PER_S / (out["stirring_ms"] * 1e-3))
        return out
    finally:
        sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lbox", type=float, default=1.0)
    ap.add_argument("--modes", default="off,fast,exact,off", help="comma-separated runs: off, fast, exact")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sx.Context(0)
    state = ic.turbulence(a.side, a.lbox)
    res = dict(workload=f"ic.turbulence({a.side})", particles=a.side ** 3, steps=a.steps, warmup=a.warmup,
               hbm_bytes_per_s=HBM_BYTES_PER_S, fp32_ops_per_s=FP32_OPS_PER_S,
               runs=[run(ctx, state, m, a.steps, a.warmup, a.lbox) for m in a.modes.split(",")])
    by = {r["mode"]: r for r in res["runs"]}
    if "fast" in by and "exact" in by:
        res["fast_over_exact_stirring"] = by["fast"]["stirring_ms"] / by["exact"]["stirring_ms"]
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
