"""Shifted / scaled NTT (radix_fft_ex: coset, inverse, inverse-coset) against
the CPU oracle's FFT with the shifts applied in Python integers, bit-exact,
on the fused passes and on the unfused scaling-kernel path."""
import numpy as np
import pytest

import coracle as co
import ecgpu
import py_oracle as po
from test_gpu_fft import FIELDS, rand_mont

pytestmark = pytest.mark.gpu

MODES = ["coset", "inverse", "inverse_coset", "general", "plain"]


@pytest.fixture(scope="module")
def kernels(gpu_programs):
    progs, _ = gpu_programs
    return {name: ecgpu.FftKernel.create(progs, name) for name, _ in FIELDS}


@pytest.fixture
def fused(request):
    ecgpu.fft_set_fused(request.param)
    yield request.param
    ecgpu.fft_set_fused(True)


def mode_params(f, log_n, mode):
    """(omega, in_shift, out_shift, scale) as plain integers, None = absent."""
    r, n = f.modulus, 1 << log_n
    w, g = f.omega(n), 7
    inv = lambda x: pow(x, -1, r)
    return {"plain": (w, None, None, None), "coset": (w, g, None, None), "inverse": (inv(w), None, None, inv(n)),
            "inverse_coset": (inv(w), None, inv(g), inv(n)), "general": (w, 5, 11, 3)}[mode]


def mont(f, v):
    return None if v is None else co.u64arr([f.to_mont(v)], 4)[0]


def reference(f, fid, a, log_n, om, s, t, c):
    r = f.modulus
    if s is not None:
        v, x = co.to_ints(a), 1
        for j in range(len(v)):
            v[j], x = v[j] * x % r, x * s % r
        a = co.u64arr(v, 4)
    fft = co.serial_fft(fid, a, mont(f, om), log_n) if log_n <= 12 else co.parallel_fft(fid, a, mont(f, om), log_n, 4)
    if t is None and c is None:
        return fft
    v, x = co.to_ints(fft), 1 if c is None else c
    for k in range(len(v)):
        v[k], x = v[k] * x % r, x * (1 if t is None else t) % r
    return co.u64arr(v, 4)


def check(k, fname, fid, log_n, mode, seed, convenience=False):
    f = po.FIELDS[fname]
    om, s, t, c = mode_params(f, log_n, mode)
    a = rand_mont(f, 1 << log_n, seed)
    ref = reference(f, fid, a, log_n, om, s, t, c)
    if convenience:  # the methods that derive omega^-1, n^-1 and g^-1 themselves
        w, g = mont(f, f.omega(1 << log_n)), mont(f, 7)
        {"plain": lambda: k.radix_fft(a, w, log_n), "coset": lambda: k.coset_fft(a, w, log_n, g),
         "inverse": lambda: k.radix_ifft(a, w, log_n), "inverse_coset": lambda: k.coset_ifft(a, w, log_n, g)}[mode]()
    else:
        k.radix_fft_ex(a, mont(f, om), log_n, in_shift=mont(f, s), out_shift=mont(f, t), scale=mont(f, c))
    assert (a == ref).all(), (fname, log_n, mode)


@pytest.mark.parametrize("fused", [1, 0], indirect=True)
@pytest.mark.parametrize("mode", MODES[:4])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_parity_small(kernels, fname, fid, mode, fused):
    for log_n in (1, 2, 3, 10, 11, 13):
        check(kernels[fname], fname, fid, log_n, mode, 300 + log_n)


@pytest.mark.parametrize("fname,fid,log_n,fused", [("bls12_381_fr", 0, 20, 1), ("bn254_fr", 2, 20, 1),
                                                   ("bls12_381_fr", 0, 21, 1), ("bn254_fr", 2, 21, 1),
                                                   ("bls12_381_fr", 0, 20, 0)], indirect=["fused"])
def test_parity_multi_pass(kernels, fname, fid, log_n, fused):
    check(kernels[fname], fname, fid, log_n, "general", 400 + log_n)


def test_alternation_keeps_every_table_set(kernels):
    for i, mode in enumerate(["plain", "coset", "plain", "inverse", "inverse_coset", "coset", "plain"]):
        check(kernels["bls12_381_fr"], "bls12_381_fr", 0, 13, mode, 500 + i, convenience=True)


def test_device_resident_matches_host_path(kernels, gpu_programs):
    f, log_n = po.BLS12_381_FR, 11
    om, s, t, c = (mont(f, v) for v in mode_params(f, log_n, "general"))
    a = rand_mont(f, 1 << log_n, 600)
    want = a.copy()
    kernels["bls12_381_fr"].radix_fft_ex(want, om, log_n, in_shift=s, out_shift=t, scale=c)
    prog = gpu_programs[0][0]
    d = ecgpu.DeviceBuffer.upload(prog, a)
    ecgpu.fft_dev(prog, "bls12_381_fr", d, om, log_n, in_shift=s, out_shift=t, scale=c)
    assert (d.read(np.uint64, a.shape) == want).all()
    d.free()


def test_errors_and_all_none(kernels):
    f, k = po.BLS12_381_FR, kernels["bls12_381_fr"]
    om, g = mont(f, f.omega(8)), mont(f, 7)
    a = rand_mont(f, 8, 700)
    zero = np.zeros(4, np.uint64)
    r_limbs = co.u64arr([f.modulus], 4)[0]
    for kw in ({"in_shift": zero}, {"out_shift": zero}, {"scale": r_limbs}, {"in_shift": r_limbs}):
        with pytest.raises(ecgpu.EcError):
            k.radix_fft_ex(a.copy(), om, 3, **kw)
    with pytest.raises(ecgpu.EcError, match="log_n"):
        k.radix_fft_ex(np.zeros((1, 4), np.uint64), om, 0, in_shift=g)
    want, got = a.copy(), a.copy()
    k.radix_fft(want, om, 3)
    k.radix_fft_ex(got, om, 3)
    assert (got == want).all()
