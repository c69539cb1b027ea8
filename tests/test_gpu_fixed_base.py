"""Fixed-base batch scalar multiplication (ecg_fixed_base_*, csrc/fixed_base.hip)
against the Python oracle's double-and-add, bit-exact on the output words."""
import numpy as np
import pytest

import ecgpu
import py_oracle as po

CURVES = ["bls12_381", "bn254"]
WINDOWS = [0, 2, 5, 16]  # the default, the smallest, one that does not divide the bit length, the largest
N_MAX = 300


def window_of(curve, window):
    return ecgpu.fixed_base_plan_info(curve, window)[1].bit_length()  # rows = 2^(c-1)


def scalar_list(curve, c, n=N_MAX):
    """The edge scalars of window c (all taken mod r), then Xoshiro256ss elements up to n."""
    fr = po.CURVES[curve].fr
    r, W = fr.modulus, -(-(fr.bits + 1) // c)
    s = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, 2 ** (c - 1), 2 ** (c - 1) + 1, 2**c - 1, 2**c]
    for w in (0, 1, W - 1):
        s += [2 ** (c * w), 2 ** (c * w) - 1]
    # every digit 2^(c-1) before recoding, over the windows that keep it below r: the longest carry chain
    s += [sum(2 ** (c - 1) << (c * w) for w in range((fr.bits - 1) // c)), 2 ** (fr.bits - 1)]
    rng = po.Xoshiro256ss(0xF1BA5E)
    return ([x % r for x in s] + [rng.field_element(fr) for _ in range(n - len(s))])[:n]


def record(curve, base, s):
    """[x | y] Montgomery words of s * base, zeros for the identity."""
    cv = po.CURVES[curve]
    a = po.jac_to_affine(po.scalar_mul(base, s, cv.fq.modulus), cv.fq.modulus)
    return [0] * (2 * cv.fq.limbs64) if a is None else [w for v in a for w in po.int_to_limbs(cv.fq.to_mont(v), cv.fq.limbs64)]


GEN = {cv: (po.CURVES[cv].gx, po.CURVES[cv].gy) for cv in CURVES}
SCALARS = {(cv, w): scalar_list(cv, window_of(cv, w)) for cv in CURVES for w in WINDOWS}
# one oracle multiplication per distinct scalar and curve, shared by every test below
EXPECT = {cv: {s: record(cv, GEN[cv], s) for w in WINDOWS for s in SCALARS[cv, w]} for cv in CURVES}
N_EDGE = 18  # the entries of scalar_list before the random fill


def words(ints, limbs=4):
    return np.array([po.int_to_limbs(v, limbs) for v in ints], dtype=np.uint64)


def run(prog, curve, table, scalars, **kw):
    d_s = ecgpu.DeviceBuffer.upload(prog, words(scalars))
    out = ecgpu.fixed_base_mul_dev(prog, curve, table, d_s, len(scalars), **kw)
    return out.read(shape=(len(scalars), -1))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("curve", CURVES)
def test_parity_with_oracle(gpu_programs, curve, window, n):
    prog = gpu_programs[0][0]
    table = ecgpu.fixed_base_table(prog, curve, window=window)
    s = SCALARS[curve, window]
    # n = 1: every edge scalar in a call of its own (default window), else the list's first entry
    calls = [s[:n]] if n > 1 else [[x] for x in s[:N_EDGE if window == 0 else 1]]
    for call in calls:
        got = run(prog, curve, table, call)
        want = np.array([EXPECT[curve][x] for x in call], dtype=np.uint64)
        assert (got == want).all(), [hex(x) for x, g, w in zip(call, got, want) if (g != w).any()][:4]
        assert not got[[x == 0 for x in call]].any()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_other_base(gpu_programs, curve):
    prog, cv = gpu_programs[0][0], po.CURVES[curve]
    base = po.jac_to_affine(po.scalar_mul(GEN[curve], 7, cv.fq.modulus), cv.fq.modulus)
    table = ecgpu.fixed_base_table(prog, curve, base=np.array(record(curve, GEN[curve], 7), dtype=np.uint64))
    s = SCALARS[curve, 0][:65]
    want = np.array([record(curve, base, x) for x in s], dtype=np.uint64)
    assert (run(prog, curve, table, s) == want).all()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_montgomery_scalars(gpu_programs, curve):
    prog, fr = gpu_programs[0][0], po.CURVES[curve].fr
    table = ecgpu.fixed_base_table(prog, curve)
    s = SCALARS[curve, 0][:65]
    got = run(prog, curve, table, [fr.to_mont(x) for x in s], scalars_montgomery=True)
    assert (got == run(prog, curve, table, s)).all()
    assert (got == np.array([EXPECT[curve][x] for x in s], dtype=np.uint64)).all()


@pytest.mark.gpu
def test_output_is_a_base_vector(gpu_programs):
    prog, cv = gpu_programs[0][0], po.BN254
    s = SCALARS["bn254", 0]
    rng = po.Xoshiro256ss(7)
    t = [rng.field_element(cv.fr) for _ in s]
    d_bases = ecgpu.fixed_base_mul_dev(prog, "bn254", ecgpu.fixed_base_table(prog, "bn254"),
                                       ecgpu.DeviceBuffer.upload(prog, words(s)), len(s))
    jac = ecgpu.msm_dev(prog, "bn254", d_bases, ecgpu.DeviceBuffer.upload(prog, words(t)), len(s)).reshape(3, -1)
    got = po.jac_to_affine([cv.fq.from_mont(po.limbs_to_int(c)) for c in jac], cv.fq.modulus)
    k = sum(a * b for a, b in zip(s, t)) % cv.fr.modulus
    assert got == po.jac_to_affine(po.scalar_mul(GEN["bn254"], k, cv.fq.modulus), cv.fq.modulus)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["identity", "off_curve", "window_1", "window_17", "g2", "mismatch"])
def test_rejections(gpu_programs, case):
    prog, cv = gpu_programs[0][0], po.BLS12_381
    off = words([cv.fq.to_mont(cv.gx), cv.fq.to_mont(cv.gy + 1)], 6).reshape(-1)
    with pytest.raises(ecgpu.EcError, match="bls12_381_g2" if case == "g2" else None):
        if case == "mismatch":
            table = ecgpu.fixed_base_table(prog, "bls12_381", window=5)
            table.window = 6
            run(prog, "bls12_381", table, [1, 2])
        else:
            ecgpu.fixed_base_table(prog, "bls12_381_g2" if case == "g2" else "bls12_381",
                                   base={"identity": np.zeros(12, np.uint64), "off_curve": off}.get(case),
                                   window={"window_1": 1, "window_17": 17}.get(case, 0))


@pytest.mark.parametrize("c", [2, 5, 8, 16])
@pytest.mark.parametrize("curve", CURVES)
def test_plan_info(curve, c):
    W = -(-(po.CURVES[curve].fr.bits + 1) // c)
    assert ecgpu.fixed_base_plan_info(curve, c) == (W, 2 ** (c - 1), W * 2 ** (c - 1) * 128)  # one 128-B line per entry
    assert ecgpu.fixed_base_plan_info(curve, 0) == ecgpu.fixed_base_plan_info(curve, window_of(curve, 0))
