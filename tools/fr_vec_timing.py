"""Timing of the fused Fr sums of products (ecg_fr_lincomb_dev) next to the plain
NTT and the batch inversion, on device-resident 2^log_n data, both fields.

Per field and round the legs are interleaved call by call after three warm-up
calls each.  Host clock around each call; every leg ends in a stream
synchronise (ecg_fft_dev does itself, a total through sum_out, the others
through Program.synchronize).  One JSON line per leg and round, then per leg the
round medians with the algorithmic bytes -- 32 B per element for every vector
read and every vector written, a vector named twice counted once -- over the
median time, and the ratio to the same run's
batch inversion.  `lincomb8_chain7` is the 8-term combination as seven chained
two-term calls on the same data (21 vector passes where the single call makes 9).
Not measured here: hardware counters, and the kernel without the host call.

Usage: python tools/fr_vec_timing.py [--log-n 24] [--reps 30] [--rounds 3]"""
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
        cs = [ecgpu.fr_mont_from_int(fname, 0x123456789ABCDEF + j) for j in range(8)]
        a = np.random.default_rng(1).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)  # < r: any such value is a valid Montgomery form
        v = [ecgpu.DeviceBuffer.upload(prog, np.roll(a, j, axis=0)) for j in range(8)]
        d_ntt, d_out = ecgpu.DeviceBuffer.upload(prog, a), ecgpu.DeviceBuffer(prog, a.nbytes)

        def lincomb(terms, out=d_out, **kw):
            def call():
                ecgpu.fr_lincomb_dev(prog, fname, n, terms, out, **kw)
                prog.synchronize()
            return call

        def chain7():
            ecgpu.fr_lincomb_dev(prog, fname, n, [(cs[0], v[0], None, False), (cs[1], v[1], None, False)], d_out)
            for j in range(2, 8):
                ecgpu.fr_lincomb_dev(prog, fname, n, [(None, d_out, None, False), (cs[j], v[j], None, False)], d_out)
            prog.synchronize()

        def inverse():
            ecgpu.batch_inverse_dev(prog, fname, v[0], n, d_out)
            prog.synchronize()

        # leg -> (call, vectors read + vectors written per element)
        legs = {"ntt_plain": (lambda: ecgpu.fft_dev(prog, fname, d_ntt, om, args.log_n), None),
                "batch_inverse": (inverse, 2),
                "hadamard": (lincomb([(None, v[0], v[1], False)]), 3),
                "hadamard_in_place": (lincomb([(None, d_ntt, v[1], False)], d_ntt), 3),  # one vector read and written
                "ab_minus_c": (lincomb([(None, v[0], v[1], False), (ecgpu.fr_mont_from_int(fname, r - 1), v[2], None,
                                                                     False)]), 4),
                "lincomb8": (lincomb([(cs[j], v[j], None, False) for j in range(8)]), 9),
                "lincomb8_chain7": (chain7, 21),
                "abg": (lincomb([(None, v[0], v[1], True)], ratio=om), 3),
                "total_only": (lincomb([(None, v[0], v[1], False)], None, want_sum=True), 2)}
        medians = {k: [] for k in legs}
        for rnd in range(args.rounds):
            ms = {k: [] for k in legs}
            for f, _ in legs.values():
                for _ in range(3):
                    f()
            for _ in range(args.reps):
                for k, (f, _) in legs.items():
                    t = time.perf_counter()
                    f()
                    ms[k].append((time.perf_counter() - t) * 1e3)
            for k, x in ms.items():
                medians[k].append(statistics.median(x))
                print(json.dumps({"field": fname, "log_n": args.log_n, "round": rnd, "leg": k, "min_ms": round(min(x), 3),
                                  "median_ms": round(medians[k][-1], 3), "max_ms": round(max(x), 3), "reps": len(x)}),
                      flush=True)
        inv = statistics.median(medians["batch_inverse"])
        for k, x in medians.items():
            med, vecs = statistics.median(x), legs[k][1]
            print(json.dumps({"field": fname, "leg": k, "round_medians_ms": [round(y, 3) for y in x],
                              "spread_ms": round(max(x) - min(x), 3), "vs_batch_inverse": round(med / inv, 3),
                              "algorithmic_TB_per_s": None if vecs is None else round(vecs * 32 * n / med / 1e9, 3)}),
                  flush=True)
        for b in v + [d_ntt, d_out]:
            b.free()
    prog.close()


if __name__ == "__main__":
    main()
