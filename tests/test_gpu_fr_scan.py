"""Fr scans on resident data (ecg_poly_div_linear_dev, ecg_batch_inverse_dev)
against Python integers, bit-exact: Horner with %, and out * in == scale.

Sizes sit around the run (8), wave (64 runs) and tile boundaries of
ecgpu.fr_scan_tile(); 1025 tiles + 7 gives the scan kernel's threads more than
one aggregate each."""
import numpy as np
import pytest

import coracle as co
import ecgpu
import py_oracle as po
from test_gpu_fft import FIELDS, rand_mont

pytestmark = pytest.mark.gpu

T = ecgpu.fr_scan_tile()
SIZES = [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5]
LARGE = 1025 * T + 7


@pytest.fixture(scope="module")
def prog(gpu_programs):
    return gpu_programs[0][0]


def words(v):
    return co.u64arr([v], 4)[0]


def div_reference(f, raw, z_word):
    """s_j = p_j + z s_(j+1) on the Montgomery words themselves (the recurrence is
    linear in p); z is the value behind its Montgomery word."""
    r, z = f.modulus, f.from_mont(z_word)
    out, s = [0] * len(raw), 0
    for j in range(len(raw) - 1, -1, -1):
        s = (raw[j] + z * s) % r
        out[j] = s
    return out


def z_words(f, kind):
    r = f.modulus
    return {"0": 0, "1": f.to_mont(1), "r-1": f.to_mont(r - 1), "random": f.to_mont(0x1234567 * 0xABCDEF123 + 99),
            "max": r - 1}[kind]


def run_div(prog, fname, a, z_word, mode):
    """-> (d_out words, value words, input buffer after the call)"""
    n = a.shape[0]
    d = ecgpu.DeviceBuffer.upload(prog, a)
    o = d if mode == "inplace" else ecgpu.DeviceBuffer.upload(prog, np.zeros_like(a))
    val = ecgpu.poly_div_linear_dev(prog, fname, d, n, words(z_word), o, canonical=mode == "canonical")
    got, after = o.read(np.uint64, a.shape), d.read(np.uint64, a.shape)
    d.free()
    o.free()
    return got, val, after


@pytest.mark.parametrize("mode", ["inplace", "out", "canonical"])
@pytest.mark.parametrize("zkind", ["0", "1", "r-1", "random", "max"])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_div_full(prog, fname, fid, zkind, mode):
    f = po.FIELDS[fname]
    for n in SIZES:
        a = rand_mont(f, n, 900 + n)
        if zkind == "max":  # the largest limbs the call sites see
            a[:] = words(f.modulus - 1)
        ref = div_reference(f, co.to_ints(a), z_words(f, zkind))
        if mode == "canonical":
            ref = [f.from_mont(v) for v in ref]
        got, val, after = run_div(prog, fname, a, z_words(f, zkind), mode)
        assert co.to_ints(got) == ref, (n, "d_out")
        assert co.to_ints(val[None])[0] == ref[0], (n, "value_out")
        if mode != "inplace":
            assert (after == a).all(), (n, "input changed")


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_div_eval_only(prog, fname, fid):
    f = po.FIELDS[fname]
    zw = z_words(f, "random")
    for n in SIZES:
        a = rand_mont(f, n, 950 + n)
        d = ecgpu.DeviceBuffer.upload(prog, a)
        val = ecgpu.poly_div_linear_dev(prog, fname, d, n, words(zw))
        assert co.to_ints(val[None])[0] == div_reference(f, co.to_ints(a), zw)[0], n
        assert (d.read(np.uint64, a.shape) == a).all(), n
        d.free()


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_div_large(prog, fname, fid):
    f = po.FIELDS[fname]
    zw = z_words(f, "random")
    a = rand_mont(f, LARGE, 960)
    ref = div_reference(f, co.to_ints(a), zw)
    got, val, _ = run_div(prog, fname, a, zw, "out")
    assert co.to_ints(got) == ref
    assert co.to_ints(val[None])[0] == ref[0]
    d = ecgpu.DeviceBuffer.upload(prog, a)
    assert co.to_ints(ecgpu.poly_div_linear_dev(prog, fname, d, LARGE, words(zw))[None])[0] == ref[0]
    d.free()


def inv_input(f, n, seed, zeros):
    """Random non-zero elements with 1 and r - 1 among them and zeros where asked."""
    a = rand_mont(f, n, seed)
    a[:, 0] |= np.uint64(1)
    if n > 4:
        a[1], a[2] = words(f.to_mont(1)), words(f.to_mont(f.modulus - 1))
    if zeros == "all":
        a[:] = 0
    elif zeros == "edges":  # first, last, both sides of the tile boundary, and tile 1 whole
        a[0] = a[n - 1] = 0
        if n > T:
            a[T - 1] = a[T] = 0
        if n >= 2 * T:
            a[T:2 * T] = 0
    return a


def check_inverse(f, a, got, scale):
    r = f.modulus
    want = (1 if scale is None else scale) * f.R * f.R % r  # out R * in R == scale R^2
    for i, (x, y) in enumerate(zip(co.to_ints(a), co.to_ints(got))):
        assert y < r and (y == 0 if x == 0 else x * y % r == want), i


@pytest.mark.parametrize("zeros", ["none", "edges", "all"])
@pytest.mark.parametrize("scale,inplace", [(None, True), (None, False), (5, True), (5, False)])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_batch_inverse(prog, fname, fid, scale, inplace, zeros):
    f = po.FIELDS[fname]
    sc = None if scale is None else words(f.to_mont(scale))
    for n in SIZES:
        a = inv_input(f, n, 1000 + n, zeros)
        d = ecgpu.DeviceBuffer.upload(prog, a)
        o = d if inplace else ecgpu.DeviceBuffer.upload(prog, np.zeros_like(a))
        ecgpu.batch_inverse_dev(prog, fname, d, n, None if inplace else o, scale=sc)
        check_inverse(f, a, o.read(np.uint64, a.shape), scale)
        if not inplace:
            assert (d.read(np.uint64, a.shape) == a).all(), n
            o.free()
        d.free()


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_batch_inverse_large(prog, fname, fid):
    f = po.FIELDS[fname]
    a = inv_input(f, LARGE, 1100, "edges")
    d = ecgpu.DeviceBuffer.upload(prog, a)
    o = ecgpu.DeviceBuffer.upload(prog, np.zeros_like(a))
    ecgpu.batch_inverse_dev(prog, fname, d, LARGE, o)
    check_inverse(f, a, o.read(np.uint64, a.shape), None)
    ecgpu.batch_inverse_dev(prog, fname, o, LARGE)  # inverse(inverse(a)) == a
    assert (o.read(np.uint64, a.shape) == a).all()
    d.free()
    o.free()


def test_argument_errors(prog):
    f, fname, n = po.BLS12_381_FR, "bls12_381_fr", 70
    a = rand_mont(f, n + 1, 1200)
    d = ecgpu.DeviceBuffer.upload(prog, a)
    z, r_words = words(f.to_mont(3)), words(f.modulus)
    shifted = d.ptr.value + 32
    for call in (lambda: ecgpu.poly_div_linear_dev(prog, "bls12_381_fq", d, n, z, d),
                 lambda: ecgpu.poly_div_linear_dev(prog, fname, d, n, r_words, d),
                 lambda: ecgpu.poly_div_linear_dev(prog, fname, d, n, z, shifted),
                 lambda: ecgpu.poly_div_linear_dev(prog, fname, d, n, z, d, flags=2),
                 lambda: ecgpu.batch_inverse_dev(prog, "bn254_fq", d, n),
                 lambda: ecgpu.batch_inverse_dev(prog, fname, d, n, shifted),
                 lambda: ecgpu.batch_inverse_dev(prog, fname, d, n, scale=r_words)):
        with pytest.raises(ecgpu.EcError):
            call()
    assert ecgpu.poly_div_linear_dev(prog, fname, d, 0, z, d) is not None  # n = 0 is OK
    ecgpu.batch_inverse_dev(prog, fname, d, 0)
    assert (d.read(np.uint64, a.shape) == a).all()
    d.free()
