"""Cost of the power spectra (sx_spectrum_compute, Sim.spectrum) next to the route they replace, copying the columns to
the host.

    python -m sphexa_amd.spectrum_bench [--side 200] [--warmup 5] [--n 128,256] [--turbulence] \
        --out profiles/spectrum_sedov_n200.json

One process, one MI355X: Sim.init_sedov(side) in its periodic box (or, with --turbulence, ic.turbulence(side) stirred),
`warmup` steps, then for every mesh size the kinetic-energy spectrum (kind "velocity", weight "energy": four
accumulators in the gather, two transforms).  Per size: the median of `reps` host-clock times of Sim.spectrum (it ends
with the shells on the host) and of the seam call Context.spectrum on the sim's fields, the HIP-event times of its stages
(binning = counting + emitting the pairs, sort = radix sort + list offsets, gather, fft = both transforms, shells) from a
call with sx_set_spectrum_timing, the pairs, bands, the longest block list, the clamped particles and the bytes the first
call of that size added to the sim's memory (the sizes run in ascending order and buffers only grow, so the sum over
the sizes is what the largest keeps).  In the same process the yardstick: Sim.get of the eight columns x y z h m vx vy vz to host memory, 44 B per
particle, which is where a host-side spectrum would only begin.  Prints one JSON line and writes it to --out; needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COLUMNS = ["x", "y", "z", "h", "m", "vx", "vy", "vz"]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def spectrum_case(ctx, sim, n, reps):
    import sphexa_amd as sx

    f, _ = sim.fields()
    spec = sx.SxSpectrum("velocity", "energy", n)
    before = sim.memory()["device"]
    k, power, modes = sim.spectrum(n, "velocity", "energy")  # allocates the meshes and builds the tables of n
    held = sim.memory()["device"] - before
    med, best = timed(lambda: sim.spectrum(n, "velocity", "energy"), reps)
    ctx.spectrum(f, sim.box, spec, K=sim.params.K)
    seam, seam_best = timed(lambda: ctx.spectrum(f, sim.box, spec, K=sim.params.K), reps)
    ctx.set_spectrum_timing(True)
    ctx.spectrum(f, sim.box, spec, K=sim.params.K)
    stages = ctx.spectrum_times()
    ctx.set_spectrum_timing(False)
    return dict(n=n, sim_spectrum_ms=med, sim_spectrum_ms_min=best, seam_ms=seam, seam_ms_min=seam_best, stages=stages,
                sim_bytes_added=held, power_total=float(power.sum()), power_peak_shell=int(np.argmax(power[1:]) + 1),
                **sim.spectrum_stats())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", default="128,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--turbulence", action="store_true", help="ic.turbulence(side), stirred, instead of the Sedov box")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import sphexa_amd as sx
    from sphexa_amd import ic

    ctx = sx.Context(0)
    n = a.side ** 3
    if a.turbulence:
        f, lim, bnd, dt0 = ic.turbulence(a.side, 1.0)
        sim = sx.Sim(ctx, n, sx.make_box(lim, bnd), ic.turbulence_params(sx.default_params()))
        sim.set_state(f, dt0, dt0)
        sim.set_turbulence(Lbox=1.0)
        workload = f"ic.turbulence({a.side}), stirred"
    else:
        sim = sx.Sim(ctx, n, sx.make_box([-0.5, 0.5] * 3, [1, 1, 1]))
        sim.init_sedov(a.side)
        workload = f"Sim.init_sedov({a.side})"
    res = dict(workload=workload, particles=n, warmup=a.warmup, reps=a.reps, cases=[])
    try:
        for _ in range(a.warmup):
            sim.step()
        ctx.sync()
        sim.get(COLUMNS)
        res["host_copy_ms"], res["host_copy_ms_min"] = timed(lambda: sim.get(COLUMNS), a.reps)
        res["host_copy_bytes"] = 44 * n
        for size in [int(v) for v in a.n.split(",")]:
            res["cases"].append(spectrum_case(ctx, sim, size, a.reps))
        res["sim_device_bytes"] = sim.memory()["device"]
        last = res["cases"][-1]
        res[f"spectrum_{last['n']}_over_host_copy"] = last["sim_spectrum_ms"] / res["host_copy_ms"]
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
