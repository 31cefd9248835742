"""Cost of the direct gravity sum (sx_gravity_direct) and the walk's force error at a production size.

    python sph-exa_amd/python/sphexa_amd/direct_bench.py --out profiles/direct_bench.json

* ic.evrard(100), all targets against all sources, fast and exact;
* 4096 sampled targets (every s-th 64-particle block) against ic.evrard(300), with the source splits automatic, 1 and
  four times automatic, one and two targets per lane (fast), and exact;
* the walk's force error at theta 0.3 / 0.5 / 0.7 on ic.evrard(300) from the sampled check of one Sim step each
  (Sim.set_gravity_check).

ms is a host clock around the call, which ends in a stream synchronise (it returns egrav); the best and the mean of
--repeat calls after one warm-up call.  The shares of peak use flops per pair counted from the source
(sx_direct.hip), an FMA as two, rsqrt, sqrt and the division as one each, the comparisons and conversions not counted:
  fast   3 (dX) + 5 (R2: mul, 2 fma) + 1 (h_i + h_j) + 1 (its square) + 1 (max) + 1 (rsq) + 3 (m invR^3) + 8 (4 fma) = 23
         FP32, against the packed FP32 vector peak;
  exact  3 + 5 + 1 (sqrt) + 1 (1/x) + 1 (invR^2) + 2 (m invR invR^2) + 8 (4 mul, 4 add) = 21 FP64 (h_i + h_j and its
         square are FP32), against the FP64 vector peak, half the FP32 one.
Prints one JSON line; needs a GPU.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sphexa_amd as sx  # noqa: E402
from sphexa_amd import ic  # noqa: E402

FP32_FLOPS = 157.3e12       # FP32 vector peak of the MI355X (packed)
FP64_FLOPS = FP32_FLOPS / 2
FLOPS_PER_PAIR = {"fast": 23, "exact": 21}


class Particles:
    """x, y, z, m, h of an IC on the device, and zeroed ax, ay, az"""

    def __init__(self, ctx, f):
        self.ctx, self.n = ctx, len(f["x"])
        self.fields = sx.SxFields()
        self.fields.n = self.n
        self.dev = {}
        for k in ("x", "y", "z", "m", "h"):
            self.dev[k] = ctx.upload(np.asarray(f[k], dtype=sx.DTYPES[k]))
        for k in ("ax", "ay", "az"):
            self.dev[k] = ctx.alloc(self.n, np.float32)
        for k, d in self.dev.items():
            setattr(self.fields, k, d.ptr)

    def zero(self):
        for k in ("ax", "ay", "az"):
            self.ctx.L.sx_memset(self.ctx.h, self.dev[k].ptr, 0, 4 * self.n)

    def acc(self, idx):
        return np.stack([self.dev[k].get()[idx] for k in ("ax", "ay", "az")], axis=1).astype(np.float64)


def sampled_groups(ctx, n, targets):
    blocks = (n + 63) // 64
    want = max(1, (targets + 63) // 64)
    stride = max(1, (blocks + want // 2) // want)
    gs = np.arange(0, blocks, stride, dtype=np.uint32) * 64
    ge = np.minimum(gs + 64, n).astype(np.uint32)
    idx = np.concatenate([np.arange(s, e) for s, e in zip(gs, ge)])
    gsd, ged = ctx.upload(gs), ctx.upload(ge)
    return sx.SxGroups(firstBody=0, lastBody=0, numGroups=gs.size, groupStart=gsd.ptr, groupEnd=ged.ptr), idx


def timed(ctx, p, groups, num_targets, variant, splits, per_lane, repeat):
    ctx.set_exact(variant == "exact")
    ctx.set_direct_splits(splits)
    ctx.L.sx_ctx_direct_targets_per_lane_internal(ctx.h, per_lane)
    ms = []
    if variant == "exact":
        repeat = 1  # seconds per call
    for k in range(repeat + 1):
        p.zero()
        ctx.sync()
        t0 = time.perf_counter()
        ctx.gravity_direct(p.fields, groups, G=1.0)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = ms[1:]
    pairs = float(num_targets) * p.n
    peak = FP64_FLOPS if variant == "exact" else FP32_FLOPS
    best = min(ms)
    out = dict(variant=variant, splits="auto" if splits == 0 else splits, targets=int(num_targets), sources=p.n,
               ms=best, ms_mean=float(np.mean(ms)), pairs_per_s=pairs / (best * 1e-3),
               peak_fraction=FLOPS_PER_PAIR[variant] * pairs / (best * 1e-3) / peak)
    if variant == "fast":
        out["targets_per_lane"] = per_lane
    ctx.set_exact(False)
    ctx.set_direct_splits(0)
    ctx.L.sx_ctx_direct_targets_per_lane_internal(ctx.h, 0)
    print(out, file=sys.stderr, flush=True)
    return out


def auto_splits(num_targets, n, per_lane):
    tb = max(1, -(-num_targets // (256 * per_lane)))
    return min(max(-(-4096 // tb), 1), -(-n // 256))


def force_error(ctx, state, theta, targets):
    f, lim, bnd, dt0 = state
    sim = sx.Sim(ctx, len(f["x"]), sx.make_box(lim, bnd), params=sx.default_params(g=1.0, theta=theta))
    try:
        sim.set_state(f, dt0, dt0)
        sim.set_gravity_check(targets)
        sim.step()
        out = sim.gravity_check()
        out["theta"] = theta
        print(out, file=sys.stderr, flush=True)
        return out
    finally:
        sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all-side", type=int, default=100)
    ap.add_argument("--sample-side", type=int, default=300)
    ap.add_argument("--targets", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--thetas", default="0.3,0.5,0.7")
    ap.add_argument("--no-exact", action="store_true", help="skip the exact (FP64) runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sx.Context(0)
    res = dict(fp32_flops=FP32_FLOPS, fp64_flops=FP64_FLOPS, flops_per_pair=FLOPS_PER_PAIR, repeat=a.repeat, runs=[])

    # all targets against all sources
    p = Particles(ctx, ic.evrard(a.all_side)[0])
    g = sx.SxGroups(firstBody=0, lastBody=p.n, numGroups=(p.n + 63) // 64)
    for variant, per_lane in [("fast", 1), ("fast", 2)] + ([] if a.no_exact else [("exact", 1)]):
        r = timed(ctx, p, g, p.n, variant, 0, per_lane, a.repeat)
        r["workload"] = f"ic.evrard({a.all_side}) all pairs"
        res["runs"].append(r)
    ctx.free_all()

    # a sample of targets against a production-size source set
    state = ic.evrard(a.sample_side)
    p = Particles(ctx, state[0])
    g, idx = sampled_groups(ctx, p.n, a.targets)
    for per_lane in (1, 2):
        k = auto_splits(idx.size, p.n, per_lane)
        for splits in (0, 1, 4 * k):
            r = timed(ctx, p, g, idx.size, "fast", splits, per_lane, a.repeat)
            r.update(workload=f"ic.evrard({a.sample_side}) sampled", automatic_splits=k)
            res["runs"].append(r)
    fast = p.acc(idx)
    if not a.no_exact:
        r = timed(ctx, p, g, idx.size, "exact", 0, 1, a.repeat)
        r["workload"] = f"ic.evrard({a.sample_side}) sampled"
        res["runs"].append(r)
        exact = p.acc(idx)
        res["fast_vs_exact_sampled_max"] = float(np.max(np.abs(fast - exact)) / np.max(np.abs(exact)))
    ctx.free_all()

    res["walk_force_error"] = [force_error(ctx, state, float(t), a.targets) for t in a.thetas.split(",") if t]
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
