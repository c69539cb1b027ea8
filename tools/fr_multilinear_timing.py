"""Timing of the multilinear Fr calls (ecg_fr_sumcheck_round_dev, ecg_fr_mle_fix_dev,
ecg_fr_eq_table_dev) next to ecg_fr_lincomb_dev and the batch inversion, on
device-resident tables of 2^log_n entries, both fields.

Per field and round the legs are interleaved call by call after three warm-up
calls each.  Host clock around each call; every leg ends in a stream
synchronise (the round, evaluate and the eq table do themselves, the others
through a total or Program.synchronize).  One JSON line per leg and round, then
per leg the round medians with the algorithmic bytes -- 32 B per entry read and
per entry written -- over the median time, and the ratios to the same run's
<a, b> total (`inner_product`), Hadamard product and batch inversion.
`fold_round_f3` is the fused bind + round over three columns; `fix1_x3_round_f3`
is what it replaces: three one-variable binds, then the unfused round on the
half-length tables.
Not measured here: hardware counters, and the kernels without the host call.

Usage: python tools/fr_multilinear_timing.py [--log-n 24] [--reps 30] [--rounds 3]"""
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

GATE = [(0, 1, 2), (0, 3, 4), (0, 5, 2, 4), (0, 6, 7), (0,)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    ln, n = args.log_n, 1 << args.log_n
    prog = ecgpu.program(ecgpu.Device(0))
    for fname in ("bls12_381_fr", "bn254_fr"):
        cs = np.stack([ecgpu.fr_mont_from_int(fname, 0x123456789ABCDEF + j) for j in range(max(ln, 8))])
        a = np.random.default_rng(1).integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 60) - 1)  # < r: any such value is a valid Montgomery form
        v = [ecgpu.DeviceBuffer.upload(prog, np.roll(a, j, axis=0)) for j in range(8)]
        half = [ecgpu.DeviceBuffer(prog, a.nbytes // 2) for _ in range(3)]
        d_out = ecgpu.DeviceBuffer(prog, a.nbytes)

        def rnd(cols, products, **kw):
            return lambda: ecgpu.fr_sumcheck_round_dev(prog, fname, ln, cols, products, **kw)

        def separate():
            for j in range(3):
                ecgpu.fr_mle_fix_dev(prog, fname, v[j], ln, cs[:1], half[j])
            ecgpu.fr_sumcheck_round_dev(prog, fname, ln - 1, half, [(0, 1, 2)])

        def synced(f):
            def call():
                f()
                prog.synchronize()
            return call

        # leg -> (call, entries read + entries written per table entry)
        legs = {"inner_product": (lambda: ecgpu.fr_lincomb_dev(prog, fname, n, [(None, v[0], v[1], False)], None,
                                                               want_sum=True), 2),
                "hadamard": (synced(lambda: ecgpu.fr_lincomb_dev(prog, fname, n, [(None, v[0], v[1], False)], d_out)), 3),
                "batch_inverse": (synced(lambda: ecgpu.batch_inverse_dev(prog, fname, v[0], n, d_out)), 2),
                "round_f2": (rnd(v[:2], [(0, 1)]), 2),
                "round_f3": (rnd(v[:3], [(0, 1, 2)]), 3),
                "round_f4": (rnd(v[:4], [(0, 1, 2, 3)]), 4),
                "round_gate": (rnd(v, GATE, coeffs=cs[:5]), 8),
                "fold_round_f3": (rnd(v[:3], [(0, 1, 2)], fold_r=cs[0], d_folded=half), 4.5),
                "fix1_x3_round_f3": (separate, 6),
                "evaluate": (lambda: ecgpu.fr_mle_fix_dev(prog, fname, v[0], ln, cs[:ln]), 1),
                "eq_table": (lambda: ecgpu.fr_eq_table_dev(prog, fname, cs[:ln], d_out), 1)}
        medians = {k: [] for k in legs}
        for r in range(args.rounds):
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
                print(json.dumps({"field": fname, "log_n": ln, "round": r, "leg": k, "min_ms": round(min(x), 3),
                                  "median_ms": round(medians[k][-1], 3), "max_ms": round(max(x), 3), "reps": len(x)}),
                      flush=True)
        base = {k: statistics.median(medians[k]) for k in ("inner_product", "hadamard", "batch_inverse")}
        for k, x in medians.items():
            med = statistics.median(x)
            print(json.dumps({"field": fname, "leg": k, "round_medians_ms": [round(y, 3) for y in x],
                              "spread_ms": round(max(x) - min(x), 3),
                              **{"vs_" + b: round(med / t, 3) for b, t in base.items()},
                              "algorithmic_TB_per_s": round(legs[k][1] * 32 * n / med / 1e9, 3)}), flush=True)
        for b in v + half + [d_out]:
            b.free()
    prog.close()


if __name__ == "__main__":
    main()
