"""Timing of the Fr scans (ecg_poly_div_linear_dev, ecg_batch_inverse_dev) next
to the plain NTT, on device-resident 2^log_n data, both fields.

Per field and round the four legs are interleaved call by call after three
warm-up calls each: the plain transform (ecg_fft_dev), the division with its
quotient (out of place), the evaluation only, and the batch inversion (out of
place).  Host clock around each call; every leg ends in a stream synchronise
(ecg_fft_dev does itself, the division through value_out, the inversion through
Program.synchronize).  One JSON line per leg and round, then the spread of the
round medians.

Usage: python tools/fr_scan_timing.py [--log-n 24] [--reps 30] [--rounds 3]"""
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

GEN = {"bls12_381_fr": 7, "bn254_fr": 5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    n = 1 << args.log_n
    prog = ecgpu.program(ecgpu.Device(0))
    for fname, g in GEN.items():
        r = ecgpu.FR_MODULUS[ecgpu.FIELD_NAMES[fname]]
        om = ecgpu.fr_mont_from_int(fname, pow(g, (r - 1) >> args.log_n, r))
        z = ecgpu.fr_mont_from_int(fname, 0x123456789ABCDEF)
        a = np.random.default_rng(1).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)  # < r: any such value is a valid Montgomery form
        d_ntt, d_in = ecgpu.DeviceBuffer.upload(prog, a), ecgpu.DeviceBuffer.upload(prog, a)
        d_out = ecgpu.DeviceBuffer(prog, a.nbytes)

        def inverse():
            ecgpu.batch_inverse_dev(prog, fname, d_in, n, d_out)
            prog.synchronize()

        legs = {"ntt_plain": lambda: ecgpu.fft_dev(prog, fname, d_ntt, om, args.log_n),
                "div_quotient": lambda: ecgpu.poly_div_linear_dev(prog, fname, d_in, n, z, d_out),
                "div_eval_only": lambda: ecgpu.poly_div_linear_dev(prog, fname, d_in, n, z),
                "batch_inverse": inverse}
        medians = {k: [] for k in legs}
        for rnd in range(args.rounds):
            ms = {k: [] for k in legs}
            for k, f in legs.items():
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
        ntt = statistics.median(medians["ntt_plain"])
        for k, v in medians.items():
            print(json.dumps({"field": fname, "leg": k, "round_medians_ms": [round(x, 3) for x in v],
                              "spread_ms": round(max(v) - min(v), 3),
                              "vs_ntt": round(statistics.median(v) / ntt, 3)}), flush=True)
        for b in (d_ntt, d_in, d_out):
            b.free()
    prog.close()


if __name__ == "__main__":
    main()
