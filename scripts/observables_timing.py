"""Device time of the observables reductions on one 8M-particle state (the Sedov -n 200 size):

  (a) sx_conserved_quantities: one particle per thread, ten block barriers per 256 particles;
  (b) sx_observables, the fused grid-stride pass, for time_energy, mach_rms and grav_waves.

Each call is bracketed by HIP events on the context's stream (the call synchronises, so the bracket holds the two
kernels and the copy of the sums); the variants alternate within every round so that they see the same machine state,
and the median over the rounds after a warm-up is reported, with the bytes each pass has to read.

    python scripts/observables_timing.py [--n 8000000] [--rounds 30] [--out profiles/observables_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sph-exa_amd", "python"))

import sphexa_amd as sx  # noqa: E402

# bytes per particle: x y z (24) + vx vy vz m (16) + temp (8) + nc (4), then the kind's fields
BYTES = {"conserved": 52, "time_energy": 52, "mach_rms": 56, "grav_waves": 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200 ** 3)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("observables_timing: no GPU (a timing is a GPU measurement)")
    n = args.n
    rng = np.random.default_rng(0)
    ctx = sx.Context(0)
    f = sx.SxFields()
    f.n = n
    for k in ("x", "y", "z", "temp"):
        setattr(f, k, ctx.upload(rng.uniform(0.0, 1.0, n)).ptr)
    for k in ("vx", "vy", "vz", "ax", "ay", "az"):
        setattr(f, k, ctx.upload(rng.normal(0.0, 1.0, n).astype(np.float32)).ptr)
    for k in ("m", "c"):
        setattr(f, k, ctx.upload(rng.uniform(0.5, 1.5, n).astype(np.float32)).ptr)
    f.nc = ctx.upload(rng.integers(50, 150, n).astype(np.uint32)).ptr
    stream = torch.cuda.ExternalStream(ctx.L.sx_get_stream(ctx.h))
    out9 = (C.c_double * 9)()

    def conserved():
        ctx.check(ctx.L.sx_conserved_quantities(ctx.h, C.byref(f), 0, n, 10.0, 5.0 / 3.0, out9), "conserved")
        return list(out9)

    variants = {"conserved": conserved}
    for kind in ("time_energy", "mach_rms", "grav_waves"):
        variants[kind] = (lambda kind=kind: list(ctx.observables(f, kind, 0, n).values()))
    ms = {k: [] for k in variants}
    values = {}
    for r in range(args.warmup + args.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            values[name] = fn()
            e1.record(stream)
            e1.synchronize()
            if r >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    res = {"n": n, "rounds": args.rounds, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name, t in ms.items():
        med = float(np.median(t))
        res[name] = {"median_ms": med, "min_ms": float(np.min(t)), "max_ms": float(np.max(t)),
                     "bytes_per_particle": BYTES[name], "GB_per_s": BYTES[name] * n / med * 1e-6}
    res["mach_rms_over_conserved"] = res["mach_rms"]["median_ms"] / res["conserved"]["median_ms"]
    # the fused pass forms the same nine sums: relative difference of the two kernels' energies
    res["ecin_rel_diff"] = abs(values["time_energy"][0] - values["conserved"][0]) / abs(values["conserved"][0])
    res["eint_rel_diff"] = abs(values["time_energy"][1] - values["conserved"][1]) / abs(values["conserved"][1])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
