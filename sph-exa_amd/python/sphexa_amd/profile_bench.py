"""Cost of the binned profiles (sx_profile_compute, Sim.profile) next to the route they replace: copying the columns to
the host and reducing them with the numpy of oracle/trajectory.py.

    python -m sphexa_amd.profile_bench [--side 200] [--steps 20] [--nbins 50] --out profiles/profile_sedov_n200.json

One process, one MI355X: Sim.init_sedov(side), `steps` steps, then the radial profile of rho, p, |v| and u in `nbins`
shells of [0, 0.5) with the reference's Sedov table on rho (tests/golden/traj_sedov50.npz, rescaled to the run's time by
rscale = (t_sol / t)^0.4).  Reported: the median of `reps` host-clock times of Sim.profile (it ends with the result on
the host) and of the seam call Context.profile on the sim's fields; the HIP-event times of pass 1 (windows), pass 2
(integer sums) and the conversion from a call with sx_set_profile_timing, the bytes a pass reads and the fraction of
the HBM peak (--peak-tbs, 8 TB/s) that is; the same call with the bins in global memory instead of LDS
(sx_set_profile_lds 0), and both paths again with more bins (`--nbins-wide`, 1000: above the 231 of one LDS tile for four
quantities, so pass 2 runs once per tile); and the yardstick in the same process: Sim.get of the ten columns
(trajectory.FIELDS, 60 B per particle) alone, and followed by trajectory.profiles and trajectory.analytic_l1.  The two
routes' L1 are printed side by side.  Prints one JSON line and writes it to --out; needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def seam_case(ctx, sim, spec, reps, lds, peak):
    f, _ = sim.fields()
    ctx.set_profile_lds(lds)
    call = lambda: ctx.profile(f, sim.box, spec, params=sim.params)  # noqa: E731
    call()
    med, best = timed(call, reps)
    ctx.set_profile_timing(True)
    stages = []
    for _ in range(reps):
        call()
        stages.append(ctx.profile_times())
    ctx.set_profile_timing(False)
    stats = ctx.profile_stats()
    ctx.set_profile_lds(True)
    out = {k: float(np.median([s[k] for s in stages])) for k in ("pass1_ms", "pass2_ms", "final_ms")}
    out.update(nbins=int(spec.nbins), lds=stats["lds"], seam_ms=med, seam_ms_min=best,
               pass_bytes=stages[0]["pass_bytes"])
    for k in ("pass1", "pass2"):
        out[k + "_hbm_fraction"] = out["pass_bytes"] / (out[k + "_ms"] * 1e-3) / peak if out[k + "_ms"] > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--nbins", type=int, default=50)
    ap.add_argument("--nbins-wide", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import sphexa_amd as sx
    import trajectory as tj

    sol = np.load(os.path.join(ROOT, "tests", "golden", "traj_sedov50.npz"))
    table, t_sol = sol["sol"], float(sol["sol_time"][0])
    ctx = sx.Context(0)
    n = a.side ** 3
    sim = sx.Sim(ctx, n, sx.make_box([-0.5, 0.5] * 3, [1, 1, 1]))
    res = dict(workload=f"Sim.init_sedov({a.side}), {a.steps} steps", particles=n, reps=a.reps, nbins=a.nbins, cases=[])
    try:
        sim.init_sedov(a.side)
        for _ in range(a.steps):
            sim.step()
        ctx.sync()
        t = sim.scalars()["ttot"]
        rscale = (t_sol / t) ** 0.4
        kw = dict(quantities=("rho", "p", "vel", "u"), solutions={"rho": ("table", table[:, 0], table[:, 1], rscale)})
        edges = np.linspace(0.0, 0.5, a.nbins + 1)

        before = sim.memory()
        prof = sim.profile(edges, **kw)
        after = sim.memory()
        res["sim_bytes_added"] = after["device"] - before["device"]
        res["sim_profile_ms"], res["sim_profile_ms_min"] = timed(lambda: sim.profile(edges, **kw), a.reps)
        res["l1_rho_device"] = prof["l1"]["rho"]
        res["nonfinite"] = prof["nonfinite"]

        def host_route():
            f = sim.get(tj.FIELDS)
            _, means, cnt = tj.profiles(f, 0.5, a.nbins)
            rho, _ = tj.eos_rho_p(f)
            return means, tj.analytic_l1(tj.radii(f) * rscale, rho.astype(np.float64), table[:, 0], table[:, 1])

        sim.get(tj.FIELDS)
        res["host_copy_ms"], res["host_copy_ms_min"] = timed(lambda: sim.get(tj.FIELDS), a.reps)
        res["host_copy_bytes"] = 60 * n
        means, res["l1_rho_host"] = host_route()
        res["host_route_ms"], res["host_route_ms_min"] = timed(host_route, max(2, a.reps // 2))
        res["means_max_rel_diff"] = {k: float(np.max(np.abs(prof["mean"][k] / means[k] - 1.0))) for k in means}
        peak = a.peak_tbs * 1e12
        for nbins in (a.nbins, a.nbins_wide):
            spec = sim.profile_spec(np.linspace(0.0, 0.5, nbins + 1), **kw)
            for lds in (True, False):
                res["cases"].append(seam_case(ctx, sim, spec, a.reps, lds, peak))
        res["lds_bins_nq4"] = sx.profile_lds_bins(4)
        res["profile_over_host_copy"] = res["sim_profile_ms"] / res["host_copy_ms"]
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
