"""Timing of the division by X^m - c (ecg_poly_div_binomial_dev) over log_m, next
to the division by X - z (ecg_poly_div_linear_dev) at the same size, on
device-resident 2^log_n data, both fields.

The method of fr_scan_timing.py: per field and round every leg is warmed by three
calls, then the legs are interleaved call by call; host clock around each call,
which ends in a stream synchronise (Program.synchronize; neither call waits by
itself here, the linear one is asked for no value).  All legs are out of place.
One JSON line per leg and round, then the round medians, their spread and the
ratio to the linear call, with the path and split the plan query reports.

Usage: python tools/fr_binomial_timing.py [--log-n 24] [--reps 30] [--rounds 3] [--log-m 0 1 3 ...]"""
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

PATH_NAMES = {ecgpu.DIVB_PATH_LINEAR: "linear", ecgpu.DIVB_PATH_STRIDED: "strided", ecgpu.DIVB_PATH_COLUMNS: "columns"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log-m", type=int, nargs="*", default=None)
    args = ap.parse_args()
    n = 1 << args.log_n
    strided = [lm for lm in range(32) if ecgpu.poly_div_binomial_plan(n, lm)[0] == ecgpu.DIVB_PATH_STRIDED]
    log_ms = args.log_m or sorted({0, 1, 3, 5, max(strided), max(strided) + 1, 12, 16, 20, 23})
    print(json.dumps({"log_n": args.log_n, "reps": args.reps, "rounds": args.rounds, "log_m": log_ms}), flush=True)
    prog = ecgpu.program(ecgpu.Device(0))
    for fname in ("bls12_381_fr", "bn254_fr"):
        c = ecgpu.fr_mont_from_int(fname, 0x123456789ABCDEF)
        a = np.random.default_rng(1).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)  # < r: any such value is a valid Montgomery form
        d_in = ecgpu.DeviceBuffer.upload(prog, a)
        d_out = ecgpu.DeviceBuffer(prog, a.nbytes)

        def linear():
            ecgpu.poly_div_linear_dev(prog, fname, d_in, n, c, d_out, want_value=False)
            prog.synchronize()

        def binomial(lm):
            def f():
                ecgpu.poly_div_binomial_dev(prog, fname, d_in, n, lm, c, d_out)
                prog.synchronize()
            return f

        legs = {"linear": linear, **{"log_m=%d" % lm: binomial(lm) for lm in log_ms}}
        medians = {k: [] for k in legs}
        for rnd in range(args.rounds):
            ms = {k: [] for k in legs}
            for f in legs.values():
                for _ in range(3):
                    f()
            for _ in range(args.reps):
                for k, f in legs.items():
                    t = time.perf_counter()
                    f()
                    ms[k].append((time.perf_counter() - t) * 1e3)
            for k, v in ms.items():
                medians[k].append(statistics.median(v))
                print(json.dumps({"field": fname, "log_n": args.log_n, "round": rnd, "leg": k, "min_ms": round(min(v), 3),
                                  "median_ms": round(medians[k][-1], 3), "max_ms": round(max(v), 3), "reps": len(v)}),
                      flush=True)
        lin = statistics.median(medians["linear"])
        for k, v in medians.items():
            row = {"field": fname, "leg": k, "round_medians_ms": [round(x, 3) for x in v],
                   "spread_ms": round(max(v) - min(v), 3), "vs_linear": round(statistics.median(v) / lin, 3)}
            if k != "linear":
                path, segments, rows = ecgpu.poly_div_binomial_plan(n, int(k.split("=")[1]))
                row.update(path=PATH_NAMES[path], segments=segments, rows_per_segment=rows)
            print(json.dumps(row), flush=True)
        d_in.free()
        d_out.free()
    prog.close()


if __name__ == "__main__":
    main()
