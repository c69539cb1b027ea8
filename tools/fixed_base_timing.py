"""Timing of the fixed-base multiplication (ecg_fixed_base_mul_dev) over the
candidate windows, on device-resident scalars, both curves.

Per curve and size the tables of the candidates are built once and the scalars
uploaded once; per round the candidates are interleaved call by call after
three warm-up calls each.  Host clock around each call, which ends in a stream
synchronise (stream = NULL).  One JSON line per window and round, then per
window the round medians, their spread and the rate in point additions per
second (n W / median): the figure to set beside the MSM's.

Usage: python tools/fixed_base_timing.py [--log-n 20 24] [--windows 8 12 16] [--reps 20] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "0g-ec-gpu_amd"))
import ecgpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--windows", type=int, nargs="+", default=[8, 12, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    prog = ecgpu.program(ecgpu.Device(0))
    for curve in ("bls12_381", "bn254"):
        tables = {c: ecgpu.fixed_base_table(prog, curve, window=c) for c in args.windows}
        for log_n in args.log_n:
            n = 1 << log_n
            s = np.random.default_rng(1).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
            s[:, 3] &= np.uint64((1 << 60) - 1)  # < r on both curves
            d_s = ecgpu.DeviceBuffer.upload(prog, s)
            d_out = ecgpu.DeviceBuffer(prog, n * 2 * ecgpu.CURVE_FQ_LIMBS[ecgpu.CURVE_NAMES[curve]] * 8)
            legs = {c: (lambda t=t: ecgpu.fixed_base_mul_dev(prog, curve, t, d_s, n, d_out)) for c, t in tables.items()}
            medians = {c: [] for c in legs}
            for rnd in range(args.rounds):
                ms = {c: [] for c in legs}
                for f in legs.values():
                    for _ in range(3):
                        f()
                for _ in range(args.reps):
                    for c, f in legs.items():
                        t0 = time.perf_counter()
                        f()
                        ms[c].append((time.perf_counter() - t0) * 1e3)
                for c, v in ms.items():
                    medians[c].append(statistics.median(v))
                    print(json.dumps({"curve": curve, "log_n": log_n, "round": rnd, "window": c,
                                      "min_ms": round(min(v), 3), "median_ms": round(medians[c][-1], 3),
                                      "max_ms": round(max(v), 3), "reps": len(v)}), flush=True)
            for c, v in medians.items():
                W, rows, nbytes = ecgpu.fixed_base_plan_info(curve, c)
                med = statistics.median(v)
                print(json.dumps({"curve": curve, "log_n": log_n, "window": c, "windows": W, "table_bytes": nbytes,
                                  "round_medians_ms": [round(x, 3) for x in v], "spread_ms": round(max(v) - min(v), 3),
                                  "point_adds_per_s": round(n * W / (med * 1e-3), 0),
                                  "outputs_per_s": round(n / (med * 1e-3), 0)}), flush=True)
            d_s.free()
            d_out.free()
        for t in tables.values():
            t.free()
    prog.close()


if __name__ == "__main__":
    main()
