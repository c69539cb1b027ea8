"""Timing of the Fr grand product (ecg_fr_grand_product_dev) next to the batch
inversion and the plain NTT, on device-resident 2^log_n data, both fields.

Per field and round the legs are interleaved call by call after three warm-up
calls each: the plain transform (ecg_fft_dev), the batch inversion (out of
place) and the grand product at (k_num, k_den) = (1, 0), (1, 1), (3, 3), (4, 4),
out of place over distinct columns.  Host clock around each call; every leg
ends in a stream synchronise (ecg_fft_dev does itself, the others through
Program.synchronize).  One JSON line per leg and round, then the spread of the
round medians with the ratio to the same run's batch inversion and the
algorithmic bandwidth, (2 (k_num + k_den) + 1) x 32 x n bytes per call.

Usage: python tools/fr_grand_product_timing.py [--log-n 24] [--reps 30] [--rounds 3]"""
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
SHAPES = [(1, 0), (1, 1), (3, 3), (4, 4)]


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
        rng = np.random.default_rng(1)
        cols = []
        for _ in range(8):
            a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
            a[:, 3] &= np.uint64((1 << 60) - 1)  # < r: any such value is a valid Montgomery form
            cols.append(ecgpu.DeviceBuffer.upload(prog, a))
        d_ntt = ecgpu.DeviceBuffer.upload(prog, a)
        d_out = ecgpu.DeviceBuffer(prog, a.nbytes)

        def inverse():
            ecgpu.batch_inverse_dev(prog, fname, cols[0], n, d_out)
            prog.synchronize()

        def product(kn, kd):
            def leg():
                ecgpu.fr_grand_product_dev(prog, fname, n, cols[:kn], cols[4:4 + kd], d_out)
                prog.synchronize()
            return leg

        legs = {"ntt_plain": lambda: ecgpu.fft_dev(prog, fname, d_ntt, om, args.log_n), "batch_inverse": inverse}
        legs.update({"grand_product_%d_%d" % s: product(*s) for s in SHAPES})
        gbytes = {"grand_product_%d_%d" % s: (2 * sum(s) + 1) * 32 * n / 1e9 for s in SHAPES}
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
        inv = statistics.median(medians["batch_inverse"])
        for k, v in medians.items():
            line = {"field": fname, "leg": k, "round_medians_ms": [round(x, 3) for x in v],
                    "spread_ms": round(max(v) - min(v), 3), "vs_batch_inverse": round(statistics.median(v) / inv, 3)}
            if k in gbytes:
                line["algorithmic_GB_per_s"] = round(gbytes[k] / (statistics.median(v) * 1e-3), 1)
            print(json.dumps(line), flush=True)
        for b in cols + [d_ntt, d_out]:
            b.free()
    prog.close()


if __name__ == "__main__":
    main()
