"""Cost of the radiative cooling: the two kernels on columns of their own, and inside the Sedov step.

    python -m sphexa_amd.cooling_bench --side 200 --steps 20 --warmup 5 --repeats 3 --out profiles/cooling_mi355x.json

Kernels: sx_cool and sx_cooling_time on side^3 particles, all above the floor, whose temperatures are log-spaced over a
five-segment schematic table (the lanes of a wave on different segments: the worst case for the alpha == 1 select).
kernel_ms: HIP events round the kernels of a call (sx_cooling_times; the table is uploaded once, before them);
call_ms: a host clock round the whole call, which also copies the result back and synchronises.  Step: the Sedov blast of side^3 particles with cooling off and on, in alternating blocks of
`steps` steps on two sims of one process and one device, `repeats` times; ms/step is a host clock around sx_sim_step
calls, the kernels' own times are the HIP events of sx_sim_cooling_times averaged over the timed steps.

Yardstick: one pass of sx_cool moves 24 B per particle (temp 8 B read and 8 B written, rho and m 4 B each read), one of
sx_cooling_time 12 B; inside a VE step rho is formed from kx, xm and m, which makes it 28 B and 20 B.  The fractions
reported are those bytes over the kernel's time over the measured HBM copy rate.  Prints one JSON line; needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sphexa_amd as sx  # noqa: E402
from sphexa_amd import cooling, ic  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X

#: a schematic curve, not an astrophysical one: five power-law segments with exponents above, at and below 1
SCHEMATIC_T = np.array([1.0, 3.0, 6.0, 50.0, 400.0, 5000.0])
SCHEMATIC_L = np.array([0.5, 2.0, 4.0, 1.0, 3.0, 40.0])


def time_calls(ctx, fn, which, calls, warmup):
    """(whole calls by the host clock, their kernels by device events), ms each"""
    for _ in range(warmup):
        fn()
    ctx.sync()
    call, kernel = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t0) * 1e3)
        kernel.append(cooling.kernel_times(ctx)[which])
    return call, kernel


def bench_kernels(ctx, n, calls, warmup):
    """every particle above the floor and cooling, the lanes of a wave on different segments"""
    table = cooling.Cooling(SCHEMATIC_T, SCHEMATIC_L)
    rng = np.random.default_rng(0)
    temp0 = rng.permutation(np.geomspace(1.5, 15000.0, n))
    rho = ctx.upload((10.0 ** rng.uniform(-1.0, 1.0, n)).astype(np.float32))
    m = ctx.upload(np.full(n, 1.0 / n, np.float32))
    temp = ctx.upload(temp0)
    cooling.set_timing(ctx, True)
    out = {}
    try:
        # dt small enough that the temperatures keep their spread over the timed calls
        runs = (("cool", 24.0, lambda: cooling.cool(ctx, table, rho, m, temp, 1.25, 1e-6)),
                ("coolingTime", 12.0, lambda: cooling.cooling_time(ctx, table, rho, temp, 1.25)))
        for which, nbytes, fn in runs:
            call, kernel = time_calls(ctx, fn, which, calls, warmup)
            out[which] = dict(kernel_ms_min=float(np.min(kernel)), kernel_ms_mean=float(np.mean(kernel)),
                              call_ms_min=float(np.min(call)), call_ms_mean=float(np.mean(call)),
                              bytes_per_particle=nbytes,
                              kernel_hbm_fraction=nbytes * n / HBM_BYTES_PER_S / (float(np.mean(kernel)) * 1e-3))
    finally:
        cooling.set_timing(ctx, False)
        for d in (rho, m, temp):
            ctx.free(d)
        table.close()
    return out


def sedov_table():
    """the schematic curve over u = 0.2 .. 1000 of the blast (cv of the default parameters), strong enough that the
    core cools in some 1e-4"""
    cv = float(ic.ideal_gas_cv())
    return cooling.Cooling(SCHEMATIC_T * 0.2 / cv, SCHEMATIC_L * 3e5)


def bench_step(ctx, side, steps, warmup, repeats, ct_crit):
    n = side ** 3
    table = sedov_table()
    sims = {}
    for mode in ("off", "on"):
        sim = sx.Sim(ctx, n, sx.make_box([-0.5, 0.5] * 3, [1, 1, 1]))
        sim.init_sedov(side)
        if mode == "on":
            sim.set_cooling(table, ct_crit=ct_crit)
        for _ in range(warmup):
            sim.step()
        sims[mode] = sim
    blocks = {"off": [], "on": []}
    kernels = {"coolingTime": [], "cool": []}
    try:
        for _ in range(repeats):
            for mode in ("off", "on"):
                sim = sims[mode]
                ctx.sync()
                t0 = time.perf_counter()
                for _ in range(steps):
                    sim.step()
                    if mode == "on":
                        for k, v in sim.cooling_times().items():
                            kernels[k].append(v)
                ctx.sync()
                blocks[mode].append((time.perf_counter() - t0) * 1e3 / steps)
        stats = sims["on"].cooling_stats()
        out = dict(ms_per_step_off=blocks["off"], ms_per_step_on=blocks["on"],
                   added_ms=float(np.mean(blocks["on"]) - np.mean(blocks["off"])),
                   on_floor=stats["on_floor"], radiated_total=stats["radiated_total"], ct_crit=ct_crit)
        for k, b in (("cool", 28.0), ("coolingTime", 20.0)):
            ms = float(np.mean(kernels[k]))
            out[k] = dict(ms_mean=ms, ms_min=float(np.min(kernels[k])), bytes_per_particle=b,
                          hbm_fraction=b * n / HBM_BYTES_PER_S / (ms * 1e-3) if ms > 0 else None,
                          hbm_fraction_of_24_or_12=(24.0 if k == "cool" else 12.0) * n / HBM_BYTES_PER_S / (ms * 1e-3)
                          if ms > 0 else None)
        return out
    finally:
        for sim in sims.values():
            sim.close()
        table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--ct-crit", type=float, default=0.1)
    ap.add_argument("--parent-step-ms", type=float, default=7.66, help="the parent commit's Sedov step at 8M particles")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sx.Context(0)
    n = a.side ** 3
    res = dict(workload=f"sedov -n {a.side}", particles=n, steps=a.steps, warmup=a.warmup, repeats=a.repeats,
               hbm_bytes_per_s=HBM_BYTES_PER_S, kernels=bench_kernels(ctx, n, a.calls, a.warmup),
               step=bench_step(ctx, a.side, a.steps, a.warmup, a.repeats, a.ct_crit))
    res["step"]["added_fraction_of_parent_step"] = res["step"]["added_ms"] / a.parent_step_ms
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
