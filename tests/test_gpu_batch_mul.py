"""Variable-base batch scalar multiplication (ecg_batch_mul_dev, csrc/batch_mul.hip)
against the Python oracle's double-and-add, bit-exact on the output words."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

import ecgpu
import py_oracle as po

CURVES = ["bls12_381", "bn254"]
GROUP = 512                # outputs per normalisation group (one inversion)
N_BIG = 2 * GROUP + 37     # more than two groups and a ragged tail
M128 = (1 << 128) - 1

_spec = importlib.util.spec_from_file_location(
    "gen_params", os.path.join(os.path.dirname(__file__), "..", "tools", "gen_params.py"))
gp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gp)
BN_GLV = gp.glv_lattice_consts(po.BN254, gp.GLV_LATTICE["bn254"])
LAMBDA = {"bls12_381": gp.GLV["bls12_381"][1], "bn254": BN_GLV["lam"]}


def bn254_split(k):
    """The device's lattice split restated (tests/test_oracle.py::test_bn254_glv_lattice): signed halves."""
    g = BN_GLV
    c1, c2 = (k * g["g1"] + (1 << 319)) >> 320, (k * g["g2"] + (1 << 319)) >> 320
    halves = ((k - c1 * g["a1"] - c2 * g["a2"]) & M128, (c1 * g["nb1"] - c2 * g["b2"]) & M128)
    return [v - (1 << 128) if v >> 127 else v for v in halves]


def edge_scalars(curve):
    r, lam = po.CURVES[curve].fr.modulus, LAMBDA[curve]
    # halves whose 32 recoded nibbles are all -8 / all +7; BN254's halves stay below 2^126: its top nibble is free
    nib = 32 if curve == "bls12_381" else 31
    lo8, hi7 = (1 << 4 * nib) - int("8" * nib, 16), int("7" * nib, 16)
    s = [0, 1, 2, r - 1, r - 2, lam, lam + 1, lam - 1, (lam + 1) * 5, 1 << 127, (1 << 128) - 1, 1 << 128,
         lo8 * (lam + 1), hi7 * (lam + 1)]
    if curve == "bn254":  # one scalar per sign combination of the lattice halves
        rng, seen = po.Xoshiro256ss(0xB254), {}
        while len(seen) < 4:
            k = rng.field_element(po.BN254_FR)
            seen.setdefault(tuple(h < 0 for h in bn254_split(k)), k)
        s += [seen[key] for key in sorted(seen)]
    return [x % r for x in s] + [r, r + 1, (1 << 256) - 1]  # the last three stay >= r: reduced on the device


@functools.cache
def gen_multiple(curve, m):
    """m G as an affine pair, None for the identity."""
    cv = po.CURVES[curve]
    return po.jac_to_affine(po.scalar_mul((cv.gx, cv.gy), m % cv.fr.modulus, cv.fq.modulus), cv.fq.modulus)


@functools.cache
def product(curve, pt, s):
    """One oracle product per distinct (point, scalar): s pt, affine or None."""
    cv = po.CURVES[curve]
    if pt is None:
        return None
    return po.jac_to_affine(po.scalar_mul(pt, s % cv.fr.modulus, cv.fq.modulus), cv.fq.modulus)


def words(ints, limbs=4):
    return np.array([po.int_to_limbs(v, limbs) for v in ints], dtype=np.uint64)


def records(curve, pts, jac_z=None):
    """[x | y] Montgomery records (zeros = identity); with jac_z, Jacobian (x z^2, y z^3, z) and (0, 1, 0)."""
    fq = po.CURVES[curve].fq
    q, out = fq.modulus, []
    for i, p in enumerate(pts):
        if jac_z is None:
            c = (0, 0) if p is None else p
        else:
            z = jac_z[i % len(jac_z)]
            c = (0, 1, 0) if p is None else (p[0] * z * z % q, p[1] * z * z * z % q, z)
        out.append([w for v in c for w in po.int_to_limbs(fq.to_mont(v), fq.limbs64)])
    return np.array(out, dtype=np.uint64)


def run(prog, curve, pts, scalars, jac_z=None, in_place=False, **kw):
    d_p = ecgpu.DeviceBuffer.upload(prog, records(curve, pts, jac_z))
    d_s = ecgpu.DeviceBuffer.upload(prog, words(scalars))
    out = ecgpu.batch_mul_dev(prog, curve, d_p, d_s, len(pts), d_p if in_place else None,
                              jacobian=jac_z is not None, **kw)
    return out.read(shape=(len(pts), -1))


def expect(curve, pts, scalars, jacobian=False):
    return records(curve, [product(curve, p, s) for p, s in zip(pts, scalars)], [1] if jacobian else None)


def cycles(curve, n):
    """A short cycle of points (identity, G, -G, small multiples) against a longer, coprime cycle of scalars:
    the 65-cycle holds every edge scalar, so each lane position sees varied data for few oracle products."""
    cv, rng = po.CURVES[curve], po.Xoshiro256ss(0xBA7C4)
    pts = [gen_multiple(curve, m) for m in (1, 0, -1, 2, 3, 7)]
    edge = edge_scalars(curve)
    sc = edge + [rng.field_element(cv.fr) for _ in range(65 - len(edge))]
    return [pts[i % len(pts)] for i in range(n)], [sc[(i * 7) % 65] if n > 65 else sc[i] for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, N_BIG])
@pytest.mark.parametrize("curve", CURVES)
def test_parity_with_oracle(gpu_programs, curve, n):
    prog = gpu_programs[0][0]
    if n == 1:  # every edge scalar in a call of its own, on G
        calls = [([gen_multiple(curve, 1)], [s]) for s in edge_scalars(curve)]
    else:
        calls = [cycles(curve, n)]
    for pts, sc in calls:
        got, want = run(prog, curve, pts, sc), expect(curve, pts, sc)
        assert (got == want).all(), [hex(s) for s, g, w in zip(sc, got, want) if (g != w).any()][:4]


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_same_point_in_every_slot(gpu_programs, curve):
    pts, (_, sc) = [gen_multiple(curve, 3)] * 65, cycles(curve, 65)
    assert (run(gpu_programs[0][0], curve, pts, sc) == expect(curve, pts, sc)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_flags(gpu_programs, curve):
    prog, cv = gpu_programs[0][0], po.CURVES[curve]
    pts, sc = cycles(curve, 65)
    want = expect(curve, pts, sc)
    assert (run(prog, curve, pts, [cv.fr.to_mont(s % cv.fr.modulus) for s in sc], scalars_montgomery=True) == want).all()
    assert (run(prog, curve, pts, sc, in_place=True) == want).all()
    for s in (sc[5], 0):  # lambda; zero
        assert (run(prog, curve, pts, [s], one_scalar=True) == run(prog, curve, pts, [s] * 65)).all()
        assert (run(prog, curve, pts, [s], one_scalar=True) == expect(curve, pts, [s] * 65)).all()
    # Jacobian: Z != 1 in (Z = 0 for the identity), exactly (x, y, 1) / (0, 1, 0) out
    zs = [po.Xoshiro256ss(9).field_element(cv.fq), 1, cv.fq.modulus - 1]
    got = run(prog, curve, pts, sc, jac_z=zs)
    assert (got == expect(curve, pts, sc, jacobian=True)).all()
    assert (run(prog, curve, pts, sc, jac_z=zs, in_place=True) == got).all()


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
def test_inverse_ec_fft(gpu_programs, curve):
    """ec_fft(omega), ec_fft(omega^-1), then n^-1 on every point: the input, normalised."""
    prog, cv = gpu_programs[0][0], po.CURVES[curve]
    n, r = 16, cv.fr.modulus
    pts = [gen_multiple(curve, m) for m in range(n)]  # slot 0 is the identity
    om = cv.fr.omega(n)
    d = ecgpu.DeviceBuffer.upload(prog, records(curve, pts, [5]))
    for w in (om, pow(om, -1, r)):
        ecgpu.ec_fft_dev(prog, curve, d, words([cv.fr.to_mont(w)])[0], 4)
    d_s = ecgpu.DeviceBuffer.upload(prog, words([cv.fr.to_mont(pow(n, -1, r))]))
    ecgpu.batch_mul_dev(prog, curve, d, d_s, n, d, jacobian=True, one_scalar=True, scalars_montgomery=True)
    assert (d.read(shape=(n, -1)) == records(curve, pts, [1])).all()


@pytest.mark.gpu
def test_output_is_a_base_vector(gpu_programs):
    """fixed_base_mul_dev -> batch_mul_dev -> msm_dev = (sum s_i t_i u_i) G."""
    prog, cv, n = gpu_programs[0][0], po.BN254, 300
    rng = po.Xoshiro256ss(11)
    s, t, u = ([rng.field_element(cv.fr) for _ in range(n)] for _ in range(3))
    up = lambda v: ecgpu.DeviceBuffer.upload(prog, words(v))
    d_b = ecgpu.fixed_base_mul_dev(prog, "bn254", ecgpu.fixed_base_table(prog, "bn254"), up(s), n)
    d_b = ecgpu.batch_mul_dev(prog, "bn254", d_b, up(t), n)
    jac = ecgpu.msm_dev(prog, "bn254", d_b, up(u), n).reshape(3, -1)
    got = po.jac_to_affine([cv.fq.from_mont(po.limbs_to_int(c)) for c in jac], cv.fq.modulus)
    assert got == gen_multiple("bn254", sum(a * b * c for a, b, c in zip(s, t, u)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["g2", "flag", "overlap"])
def test_rejections(gpu_programs, case):
    prog = gpu_programs[0][0]
    d_p, d_s = ecgpu.DeviceBuffer(prog, 4 * 96), ecgpu.DeviceBuffer.upload(prog, words([1, 2, 3]))
    with pytest.raises(ecgpu.EcError, match="bls12_381_g2" if case == "g2" else None):
        if case == "flag":
            ecgpu._check(ecgpu.lib().ecg_batch_mul_dev(prog.handle, 0, d_p.ptr, d_s.ptr, 3, 8, d_p.ptr, None), "batch_mul")
        else:
            ecgpu.batch_mul_dev(prog, "bls12_381_g2" if case == "g2" else "bls12_381", d_p, d_s, 3,
                                d_p if case == "g2" else ctypes.c_void_p(d_p.ptr.value + 96).value)
