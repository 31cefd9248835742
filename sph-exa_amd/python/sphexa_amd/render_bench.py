"""Cost of the maps (sx_map_render) next to the route they replace, copying the columns to the host.

    python -m sphexa_amd.render_bench [--side 200] [--warmup 5] [--npix 512,1024,2048] [--evrard 100] \
        --out profiles/render_sedov_n200.json

One process, one MI355X: Sim.init_sedov(side), `warmup` steps, then for every size and for "column" and "slice" (axis 2,
the whole box, temp as the column a) `reps` renders into device images.  Per case: the median host-clock time of a render
(it ends in a stream synchronise), the HIP-event times of its stages (binning = counting + emitting the pairs, sort =
radix sort + list offsets, render = the tile gather) from a render with sx_set_map_timing, the pairs, bands, the longest
tile list and the scratch bytes; and the time of Sim.render, which adds the copy of the two images to the host.  In the
same process the yardstick: Sim.get(["x", "y", "z", "h", "m", "temp"]) to host memory, 28 B per particle.
--evrard S adds one column map through the centre of ic.evrard(S), the worst case for the list length.  Prints one JSON
line and writes it to --out; needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COLUMNS = ["x", "y", "z", "h", "m", "temp"]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def render_case(ctx, sim, kind, npix, reps, field="temp", **kw):
    import sphexa_amd as sx

    spec = sim.map_spec(kind, npix=npix, **kw)
    f, _ = sim.fields()
    a = sx.DeviceArray(ctx, getattr(f, field), int(f.n), sx.DTYPES[field]) if field else None
    d0, d1 = ctx.alloc(npix * npix, np.float64), ctx.alloc(npix * npix, np.float64)

    def seam():
        ctx.render_map(f, sim.box, spec, a=a, K=sim.params.K, sum0=d0, sum1=d1)
        ctx.sync()

    try:
        seam()  # allocates the scratch
        med, best = timed(seam, reps)
        ctx.set_map_timing(True)
        seam()
        stages = ctx.map_times()
        ctx.set_map_timing(False)
        out = dict(kind=kind, npix=npix, render_ms=med, render_ms_min=best, stages=stages, **ctx.map_stats())
        if field is None or field in sx.MAP_FIELDS:
            sim.render(spec=spec, field=field)
            out["sim_render_ms"], _ = timed(lambda: sim.render(spec=spec, field=field), max(1, reps // 2))
        return out
    finally:
        ctx.free(d0)
        ctx.free(d1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--npix", default="512,1024,2048")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--evrard", type=int, default=0, help="side of an Evrard sphere for the longest-list case (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import sphexa_amd as sx
    from sphexa_amd import ic

    ctx = sx.Context(0)
    n = a.side ** 3
    res = dict(workload=f"Sim.init_sedov({a.side})", particles=n, warmup=a.warmup, reps=a.reps, cases=[])
    sim = sx.Sim(ctx, n, sx.make_box([-0.5, 0.5] * 3, [1, 1, 1]))
    try:
        sim.init_sedov(a.side)
        for _ in range(a.warmup):
            sim.step()
        ctx.sync()
        sim.get(COLUMNS)
        res["host_copy_ms"], res["host_copy_ms_min"] = timed(lambda: sim.get(COLUMNS), a.reps)
        res["host_copy_bytes"] = 28 * n
        for npix in [int(v) for v in a.npix.split(",")]:
            for kind in ("column", "slice"):
                res["cases"].append(render_case(ctx, sim, kind, npix, a.reps, axis=2))
        res["sim_device_bytes"] = sim.memory()["device"]
        c1024 = [c for c in res["cases"] if c["npix"] == 1024 and c["kind"] == "column"]
        if c1024:
            res["column_1024_over_host_copy"] = c1024[0]["render_ms"] / res["host_copy_ms"]
    finally:
        sim.close()
    if a.evrard:
        f, lim, bnd, dt0 = ic.evrard(a.evrard)
        sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), sx.default_params(g=1.0, nbody=True))
        try:
            sim.set_state(f, dt0, dt0)
            ev = render_case(ctx, sim, "column", 1024, a.reps, field=None, axis=2, center=(0.0, 0.0, 0.0),
                             width=(2.0, 2.0))
            ev.update(workload=f"ic.evrard({a.evrard})", particles=len(f["x"]))
            res["evrard"] = ev
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
