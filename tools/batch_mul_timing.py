"""Timing of the variable-base batch multiplication (ecg_batch_mul_dev) on
device-resident points and scalars, both curves, beside two existing paths:
  fixed_base  ecg_fixed_base_mul_dev at the same n (16 gathered mixed additions
              per output: the rate of chained additions on the card);
  mexp        ecg_multiple_multiexp with one line and num_chunks = line_len, the
              only earlier device route to the same values (sizes up to --mexp-max).

Per curve and size the points are generated on the device and the scalars
uploaded once; per round the legs are interleaved call by call after three
warm-up calls each.  Host clock around each call, which ends in a stream
synchronise (stream = NULL).  One JSON line per leg and round, then per leg the
round medians, their spread and the ratios to the batch multiplication.

Usage: python tools/batch_mul_timing.py [--log-n 16 20 24] [--reps 10] [--rounds 3] [--mexp-max 16]"""
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
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mexp-max", type=int, default=16)
    args = ap.parse_args()
    prog = ecgpu.program(ecgpu.Device(0))
    for curve in ("bls12_381", "bn254"):
        table = ecgpu.fixed_base_table(prog, curve)
        for log_n in args.log_n:
            n = 1 << log_n
            s = np.random.default_rng(1).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
            s[:, 3] &= np.uint64((1 << 60) - 1)  # < r on both curves
            d_s = ecgpu.DeviceBuffer.upload(prog, s)
            d_p = ecgpu.gen_bases_dev(prog, curve, 12345, 6789, n)
            d_out = ecgpu.DeviceBuffer(prog, d_p.nbytes)
            legs = {"batch_mul": lambda: ecgpu.batch_mul_dev(prog, curve, d_p, d_s, n, d_out),
                    "batch_mul_one_scalar": lambda: ecgpu.batch_mul_dev(prog, curve, d_p, d_s, n, d_out, one_scalar=True),
                    "fixed_base": lambda: ecgpu.fixed_base_mul_dev(prog, curve, table, d_s, n, d_out)}
            if log_n <= args.mexp_max:
                legs["mexp"] = lambda: ecgpu.multiple_multiexp(prog, d_p, (d_s, n), n, curve=curve)
            medians = {k: [] for k in legs}
            for rnd in range(args.rounds):
                ms = {k: [] for k in legs}
                for f in legs.values():
                    for _ in range(3):
                        f()
                for _ in range(args.reps):
                    for k, f in legs.items():
                        t0 = time.perf_counter()
                        f()
                        ms[k].append((time.perf_counter() - t0) * 1e3)
                for k, v in ms.items():
                    medians[k].append(statistics.median(v))
                    print(json.dumps({"curve": curve, "log_n": log_n, "round": rnd, "leg": k,
                                      "min_ms": round(min(v), 3), "median_ms": round(medians[k][-1], 3),
                                      "max_ms": round(max(v), 3), "reps": len(v)}), flush=True)
            bm = statistics.median(medians["batch_mul"])
            for k, v in medians.items():
                med = statistics.median(v)
                print(json.dumps({"curve": curve, "log_n": log_n, "leg": k,
                                  "round_medians_ms": [round(x, 3) for x in v], "spread_ms": round(max(v) - min(v), 3),
                                  "outputs_per_s": round(n / (med * 1e-3), 0),
                                  "ratio_to_batch_mul": round(med / bm, 3)}), flush=True)
            for d in (d_s, d_p, d_out):
                d.free()
        table.free()
    prog.close()


if __name__ == "__main__":
    main()
