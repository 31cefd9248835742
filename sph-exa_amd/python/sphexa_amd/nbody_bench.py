"""Cost of the gravity-only step (propagator 3) next to the VE + self-gravity step on the same bodies: ic.evrard(side),
G = 1, theta = 0.5.

    python sph-exa_amd/python/sphexa_amd/nbody_bench.py --side 300 --steps 20 --warmup 5 \
        --runs nbody,ve,ve,nbody [--ve-lib PATH] --out profiles/nbody_evrard_n300.json

Each run is a fresh child process with its own Sim from the same state, in the order given (ABBA by default, so a
drift of the device shows as a difference between the two runs of one kind); `ve_noskin` is the VE step without skin
lists, which like the nbody step syncs and walks a fresh tree every step; `nbody_idle` leaves the device idle for
17 ms after every step, the time the VE step spends outside the walk.  --ve-lib names another in-tree build of
the library for the `ve` runs (SPHEXA_AMD_LIB: an A/B against the parent commit's build).  ms/step is a host clock
around sx_sim_step calls (each ends in a stream synchronise); the stage and kernel times are the HIP events of
sx_sim_stage_times and sx_sim_kernel_times, averaged over the timed steps.  The integrate kernel's share of the
streaming rate is 104 B per body (x y z x_m1 a read; x y z v x_m1 keys written) over its event time against the
measured HBM copy rate.  Bytes per body are the sim's arenas (sx_sim_memory) after the timed steps; the body count for
a 288 GB device is computed from them, not run.  Prints one JSON line; needs a GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of the MI355X
HBM_CAPACITY = 288e9
INTEGRATE_BYTES = 104


def single(kind, side, steps, warmup):
    import sphexa_amd as sx
    from sphexa_amd import ic

    f, lim, bnd, dt0 = ic.evrard(side)
    n = len(f["x"])
    ctx = sx.Context(0)
    ctx.set_exact(False)
    sim = sx.Sim(ctx, n, sx.make_box(lim, bnd), sx.default_params(g=1.0, theta=0.5, nbody=kind.startswith("nbody")))
    try:
        sim.set_state(f, dt0, dt0)
        if kind == "ve_noskin":  # sync + search every step: the walk on a fresh tree, as in the nbody step
            sim.set_skin(0.0)
        for _ in range(warmup):
            sim.step()
        stages, kernels = [], []
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            sim.step()
            if kind == "nbody_idle":  # the device idles as long as the VE step's hydro stages take: the walk's duty cycle
                time.sleep(0.017)
            stages.append(sim.stage_times())
            kernels.append(sim.kernel_times())
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        out = dict(kind=kind, lib=os.path.relpath(sx.LIB_PATH, sx.ROOT), particles=n, ms_per_step=ms,
                   stage_ms={k: float(np.mean([s[k] for s in stages])) for k in stages[0]},
                   kernel_ms={k: float(np.mean([s[k] for s in kernels])) for k in kernels[0]},
                   kernel_ms_min={k: float(np.min([s[k] for s in kernels])) for k in kernels[0]},
                   egrav=sim.scalars()["egrav"], ttot=sim.scalars()["ttot"])
        if hasattr(sim.L, "sx_sim_memory"):
            mem = sim.memory()
            out.update(device_bytes=mem["device"], bytes_per_body=mem["device"] / n,
                       bodies_in_288GB_computed=int(HBM_CAPACITY / (mem["device"] / n)))
        if kind.startswith("nbody"):
            t = out["kernel_ms"]["nbodyIntegrate"] * 1e-3
            out.update(integrate_ms=out["kernel_ms"]["nbodyIntegrate"],
                       integrate_bytes_per_s=INTEGRATE_BYTES * n / t,
                       integrate_fraction_of_hbm_copy_rate=INTEGRATE_BYTES * n / t / HBM_BYTES_PER_S)
        return out
    finally:
        sim.close()
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=300)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", default="nbody,ve,ve,nbody",
                    help="comma-separated runs in order: nbody, ve, ve_noskin (VE without skin lists), nbody_idle (the "
                         "host sleeps 17 ms after every step; its ms/step includes the sleep)")
    ap.add_argument("--ve-lib", default=None, help="library of the ve runs (default: this build)")
    ap.add_argument("--single", default=None, help="(child) one run of this kind, its JSON on the last line")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.single:
        print(json.dumps(single(a.single, a.side, a.steps, a.warmup)))
        return
    runs = []
    for kind in a.runs.split(","):
        env = dict(os.environ)
        if kind.startswith("ve") and a.ve_lib:
            env["SPHEXA_AMD_LIB"] = os.path.abspath(a.ve_lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--single", kind, "--side", str(a.side), "--steps",
               str(a.steps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if r.returncode != 0:  # no further run on a device a child has left in an unknown state
            sys.exit(f"run {kind} failed with code {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = dict(workload=f"ic.evrard({a.side})", particles=runs[0]["particles"], steps=a.steps, warmup=a.warmup,
               hbm_bytes_per_s=HBM_BYTES_PER_S, runs=runs)
    by = {}
    for r in runs:
        by.setdefault(r["kind"], []).append(r)
    for kind, rs in by.items():
        res[kind + "_ms_per_step"] = [r["ms_per_step"] for r in rs]
        res[kind + "_gravity_stage_ms"] = [r["stage_ms"]["Gravity"] for r in rs]
        res[kind + "_walk_kernel_ms"] = [r["kernel_ms"]["gravity"] for r in rs]
    if "nbody" in by and "ve" in by:
        res["nbody_over_ve_step"] = float(np.mean(res["nbody_ms_per_step"]) / np.mean(res["ve_ms_per_step"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
