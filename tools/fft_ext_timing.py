"""Timing of the shifted / scaled NTT (ecg_fft_dev_ex) on device-resident data.

Per field, in one process: the plain transform, then coset / inverse /
inverse-coset with the shifts fused into the passes and with the scaling
kernel around the plain transform (ecg_fft_set_fused(0)).  The first call of
each fused mode (it builds the table set) and the second (cached slot) are
reported on their own; after three warm-up calls the configurations of one
omega are timed interleaved, REPS calls each, host clock around the call
(ecg_fft_dev* returns after a stream synchronise).  One JSON line per
configuration.

With --baseline-lib the driver alternates, ROUNDS times, a child process on
this build with one on the other build of the library (plain transform only:
the older build has no other), so both see the same box in the same minutes.

Usage: python tools/fft_ext_timing.py [--log-n 24] [--reps 30] [--rounds 3] [--baseline-lib PATH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"bls12_381_fr": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
          "bn254_fr": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
# a 2^28-th root of unity of each field (both have two-adicity >= 28)
ROOT_2P28 = {"bls12_381_fr": pow(7, (FIELDS["bls12_381_fr"] - 1) >> 28, FIELDS["bls12_381_fr"]),
             "bn254_fr": pow(5, (FIELDS["bn254_fr"] - 1) >> 28, FIELDS["bn254_fr"])}


def worker(args):
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "0g-ec-gpu_amd"))
    import ecgpu

    log_n, n = args.log_n, 1 << args.log_n
    prog = ecgpu.program(ecgpu.Device(0))
    for fname, r in FIELDS.items():
        def mont(v):
            return np.array([((v << 256) % r >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)

        w = pow(ROOT_2P28[fname], 1 << (28 - log_n), r)
        assert pow(w, n // 2, r) == r - 1
        inv = lambda x: pow(x, -1, r)
        om, om_inv, g, g_inv, n_inv = mont(w), mont(inv(w)), mont(7), mont(inv(7)), mont(inv(n))
        modes = {"plain": (om, {})}
        if not args.plain_only:
            modes.update({"coset": (om, {"in_shift": g}), "inverse": (om_inv, {"scale": n_inv}),
                          "inverse_coset": (om_inv, {"out_shift": g_inv, "scale": n_inv})})
        a = np.random.default_rng(1).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)  # < r: any such value is a valid Montgomery form
        d = ecgpu.DeviceBuffer.upload(prog, a)

        def call(mode, fused):
            if mode != "plain":
                ecgpu.fft_set_fused(fused)
            t = time.perf_counter()
            ecgpu.fft_dev(prog, fname, d, modes[mode][0], log_n, **modes[mode][1])
            return (time.perf_counter() - t) * 1e3

        # One phase per omega: the unfused path runs the plain transform, whose
        # single table slot is keyed by omega; alternating omega and omega^-1
        # would charge a plain-table rebuild to whichever call comes next.
        phases = [[("plain", 1)]]
        if not args.plain_only:
            phases += [[("coset", 1), ("coset", 0)],
                       [("inverse", 1), ("inverse", 0), ("inverse_coset", 1), ("inverse_coset", 0)]]
        first, ms = {}, {}
        for cfgs in phases:
            for c in cfgs:
                first[c] = [call(*c) for _ in range(3)]  # table build, cached slot, warm-up
                ms[c] = []
            for _ in range(args.reps):
                for c in cfgs:
                    ms[c].append(call(*c))
        for (m, f), v in ms.items():
            print(json.dumps({"lib": args.tag, "field": fname, "log_n": log_n, "mode": m,
                              "path": "plain" if m == "plain" else "fused" if f else "unfused",
                              "first_ms": round(first[(m, f)][0], 3), "second_ms": round(first[(m, f)][1], 3),
                              "min_ms": round(min(v), 3), "median_ms": round(statistics.median(v), 3),
                              "max_ms": round(max(v), 3), "reps": len(v)}), flush=True)
        d.free()
    prog.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", default="this")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    base = [sys.executable, os.path.abspath(__file__), "--worker", "--log-n", str(args.log_n), "--reps", str(args.reps)]
    for rnd in range(args.rounds):
        print(f"# round {rnd}", flush=True)
        subprocess.run(base + ["--tag", "this"], check=True, timeout=300)
        if args.baseline_lib:
            env = dict(os.environ, ECGPU_LIB=os.path.abspath(args.baseline_lib))
            subprocess.run(base + ["--tag", "baseline", "--plain-only"], check=True, timeout=300, env=env)


if __name__ == "__main__":
    main()
