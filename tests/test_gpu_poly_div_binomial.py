"""Fr division by X^m - c on resident data (ecg_poly_div_binomial_dev) against
the Python-integer recurrence s_j = p_j + c s_(j+m) on the Montgomery words,
bit-exact.

Sizes sit around m, the tile T of ecgpu.fr_scan_tile() and a thread-run
boundary inside a column (24 rows = three runs of 8); the log_m values include
both sides of the strided / column boundary the plan query reports."""
import functools

import numpy as np
import pytest

import coracle as co
import ecgpu
import py_oracle as po
from test_gpu_fft import FIELDS, rand_mont

pytestmark = pytest.mark.gpu

T = ecgpu.fr_scan_tile()
S = max(lm for lm in range(32) if ecgpu.poly_div_binomial_plan(1 << 20, lm)[0] == ecgpu.DIVB_PATH_STRIDED)
PATHS = {0: ecgpu.DIVB_PATH_LINEAR, 1: ecgpu.DIVB_PATH_STRIDED, 2: ecgpu.DIVB_PATH_STRIDED,
         3: ecgpu.DIVB_PATH_STRIDED, S: ecgpu.DIVB_PATH_STRIDED, S + 1: ecgpu.DIVB_PATH_COLUMNS,
         11: ecgpu.DIVB_PATH_COLUMNS, 13: ecgpu.DIVB_PATH_COLUMNS}
C_KINDS = {"0": lambda f: 0, "1": lambda f: f.to_mont(1), "r-1": lambda f: f.to_mont(f.modulus - 1),
           "random": lambda f: f.to_mont(0x1234567 * 0xABCDEF123 + 99), "max": lambda f: f.modulus - 1}


def sizes(log_m):
    m = 1 << log_m
    return sorted({n for n in (1, m - 1, m, m + 1, 2 * m + 3, T - 1, T, T + 1, 2 * T + 5, 24 * m - 1, 24 * m + 1)
                   if n >= 1})


@pytest.fixture(scope="module")
def prog(gpu_programs):
    return gpu_programs[0][0]


def words(v):
    return co.u64arr([v], 4)[0]


@functools.lru_cache(maxsize=None)
def div_reference(fname, n, log_m, ckind):
    """-> (input words, c word, [s_j]); s_j = p_j + c s_(j+m) on the Montgomery words
    themselves (the recurrence is linear in p), c the value behind its word."""
    f, m = po.FIELDS[fname], 1 << log_m
    a = rand_mont(f, n, 2000 + n % 9973 + log_m)
    if ckind == "max":  # the largest limbs the call sites see
        a[:] = words(f.modulus - 1)
    a.setflags(write=False)
    cw = C_KINDS[ckind](f)
    r, c, s = f.modulus, f.from_mont(cw), co.to_ints(a)
    for j in range(n - m - 1, -1, -1):
        s[j] = (s[j] + c * s[j + m]) % r
    return a, cw, s


def run(prog, fname, n, log_m, ckind, mode):
    """One call; asserts all of d_out and, out of place, that the input is unchanged."""
    f = po.FIELDS[fname]
    a, cw, ref = div_reference(fname, n, log_m, ckind)
    d = ecgpu.DeviceBuffer.upload(prog, a)
    o = d if mode == "inplace" else ecgpu.DeviceBuffer.upload(prog, np.zeros_like(a))
    ecgpu.poly_div_binomial_dev(prog, fname, d, n, log_m, words(cw), None if mode == "inplace" else o,
                                canonical=mode == "canonical")
    got, after = co.to_ints(o.read(np.uint64, a.shape)), d.read(np.uint64, a.shape)
    d.free()
    if o is not d:
        o.free()
        assert (after == a).all(), (n, "input changed")
    assert got == ([f.from_mont(v) for v in ref] if mode == "canonical" else ref), (n, log_m, ckind, mode)


@pytest.mark.parametrize("mode", ["inplace", "out", "canonical"])
@pytest.mark.parametrize("log_m", sorted(PATHS))
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_small_shapes(prog, fname, fid, log_m, mode):
    for n in sizes(log_m):
        assert ecgpu.poly_div_binomial_plan(n, log_m)[0] == PATHS[log_m]
        run(prog, fname, n, log_m, "random", mode)


@pytest.mark.parametrize("ckind", ["0", "1", "r-1", "max"])
@pytest.mark.parametrize("log_m", [3, S + 1])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_multiplier_and_limb_extremes(prog, fname, fid, log_m, ckind):
    m = 1 << log_m
    for n in (m + 1, 2 * m + 3, T + 1, 2 * T + 5, 24 * m + 1):
        run(prog, fname, n, log_m, ckind, "out")
        run(prog, fname, n, log_m, ckind, "canonical")


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_log_m_zero_is_the_linear_call(prog, fname, fid):
    f = po.FIELDS[fname]
    z = words(C_KINDS["random"](f))
    for n in (1, T + 1, 2 * T + 5):
        a = rand_mont(f, n, 2100 + n)
        d, o1, o2 = (ecgpu.DeviceBuffer.upload(prog, x) for x in (a, np.zeros_like(a), np.zeros_like(a)))
        ecgpu.poly_div_linear_dev(prog, fname, d, n, z, o1)
        ecgpu.poly_div_binomial_dev(prog, fname, d, n, 0, z, o2)
        assert (o1.read(np.uint64, a.shape) == o2.read(np.uint64, a.shape)).all(), n
        for b in (d, o1, o2):
            b.free()


@pytest.mark.parametrize("log_m,rows,min_segments", [(1, 1025 * T + 7, 1025 * 2), (S + 1, 53, 3), (S + 1, 16500, 1025),
                                                     (13, 53, 3)])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_many_tiles_and_segments(prog, fname, fid, log_m, rows, min_segments):
    """Strided: every chain crosses more than 1024 tiles (more than one aggregate per
    scan thread), ragged last tile.  Columns: at least three row segments, the last short;
    and more than 1024 of them, which a workgroup per column scans."""
    n = rows << log_m if log_m == 1 else (rows << log_m) + 5
    path, segments, seg_rows = ecgpu.poly_div_binomial_plan(n, log_m)
    assert path == PATHS[log_m] and segments >= min_segments
    assert n % T if log_m == 1 else -(-n // (1 << log_m)) % seg_rows
    run(prog, fname, n, log_m, "random", "out")
    div_reference.cache_clear()  # millions of integers: not kept for the rest of the session


def test_argument_errors(prog):
    f, fname, n = po.BLS12_381_FR, "bls12_381_fr", 70
    a = rand_mont(f, n + 1, 2200)
    d = ecgpu.DeviceBuffer.upload(prog, a)
    c, r_words = words(f.to_mont(3)), words(f.modulus)
    for call in (lambda: ecgpu.poly_div_binomial_dev(prog, fname, d, n, 3, r_words),
                 lambda: ecgpu.poly_div_binomial_dev(prog, fname, d, n, 32, c),
                 lambda: ecgpu.poly_div_binomial_dev(prog, fname, d, n, 3, c, d.ptr.value + 32),
                 lambda: ecgpu.poly_div_binomial_dev(prog, fname, d, n, 3, c, flags=2),
                 lambda: ecgpu.poly_div_binomial_dev(prog, "bls12_381_fq", d, n, 3, c)):
        with pytest.raises(ecgpu.EcError):
            call()
        assert ecgpu.last_error()
    rc = ecgpu.lib().ecg_poly_div_binomial_dev(prog.handle, 0, d.ptr, n, 3, c.ctypes.data_as(ecgpu._u64p), None, 0, None)
    assert rc == ecgpu.ECG_ERR_INVALID and "d_out" in ecgpu.last_error()
    for log_m in (0, 3, 9):
        ecgpu.poly_div_binomial_dev(prog, fname, d, 0, log_m, c)  # n = 0 is OK
    assert (d.read(np.uint64, a.shape) == a).all()
    d.free()
