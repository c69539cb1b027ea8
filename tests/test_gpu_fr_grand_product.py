"""Fr grand products on resident data (ecg_fr_grand_product_dev) against Python
integers, bit-exact: f_i = N_i * pow(D_i, r - 2, r) % r per element (so a zero
denominator gives 0), then a serial running product from init.

Sizes as in test_gpu_fr_scan: around the run (8), wave (64 runs) and tile
boundaries of ecgpu.fr_scan_tile(); 1025 tiles + 7 gives the scan kernel's
threads more than one aggregate each."""
import functools

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
SHAPES = [(1, 0), (1, 1), (2, 1), (1, 2), (3, 3), (4, 4)]
MODES = [(s, m) for s in SHAPES for m in ("out", "num0", "den_last", "canonical") if s[1] or m != "den_last"]


@pytest.fixture(scope="module")
def prog(gpu_programs):
    return gpu_programs[0][0]


def words(v):
    return co.u64arr([v], 4)[0]


@functools.lru_cache(maxsize=None)
def case(fname, kn, kd, n, kind="random"):
    """(numerator columns, denominator columns, ratios f_i as integers), computed once
    per case and shared; the columns are read-only."""
    f = po.FIELDS[fname]
    r = f.modulus
    cols = [rand_mont(f, n, 7000 + 97 * j + n) for j in range(kn + kd)]
    for c in cols[kn:]:
        c[:, 0] |= np.uint64(1)  # denominators non-zero unless the case says so
    if kind == "den_last":  # outputs unchanged, total 0
        cols[-1][n - 1] = 0
    elif kind == "den_edges":  # index 0, both sides of the tile boundary, and tile 1 whole
        cols[kn][0] = 0
        if n > T:
            cols[kn][T - 1] = cols[kn][T] = 0
        if n >= 2 * T:
            cols[-1][T:2 * T] = 0
    elif kind == "num_middle":
        cols[0][n // 2] = 0
    elif kind == "max":  # r - 1 everywhere: the largest limbs the call sites see
        for c in cols:
            c[:] = words(r - 1)
    rinv = pow(f.R, -1, r)
    prod = []
    for side in (cols[:kn], cols[kn:]):
        p = [1] * n
        for c in side:
            p = [a * w * rinv % r for a, w in zip(p, co.to_ints(c))]
        prod.append(p)
    for c in cols:
        c.flags.writeable = False
    return cols[:kn], cols[kn:], [a * pow(d, r - 2, r) % r for a, d in zip(*prod)]


def check(prog, fname, kn, kd, n, kind, mode, init):
    """One call against the serial product: d_out, the total, and the untouched inputs."""
    f = po.FIELDS[fname]
    r = f.modulus
    nums, dens, ratios = case(fname, kn, kd, n, kind)
    z = 1 if init is None else f.from_mont(co.to_ints(init[None])[0])
    want = []
    for fi in ratios + [1]:
        want.append(z if mode == "canonical" else f.to_mont(z))
        z = z * fi % r
    bufs = [ecgpu.DeviceBuffer.upload(prog, c) for c in nums + dens]
    fresh = mode in ("out", "canonical")
    o = ecgpu.DeviceBuffer.upload(prog, np.zeros_like(nums[0])) if fresh else bufs[0 if mode == "num0" else -1]
    total = ecgpu.fr_grand_product_dev(prog, fname, n, bufs[:kn], bufs[kn:], None if mode == "num0" else o, init=init,
                                       canonical=mode == "canonical", want_total=True)
    assert co.to_ints(o.read(np.uint64, (n, 4))) == want[:n], (n, "d_out")
    assert co.to_ints(total[None])[0] == want[n], (n, "total")
    for b, c in zip(bufs, nums + dens):
        if b is not o:
            assert (b.read(np.uint64, c.shape) == c).all(), (n, "input changed")
        b.free()
    if fresh:
        o.free()
    return want[n]


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("shape,mode", MODES)
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_grand_product(prog, fname, fid, shape, mode, with_init):
    f = po.FIELDS[fname]
    init = words(f.to_mont(0xABCDEF12345 * 77 + 5)) if with_init else None
    for n in SIZES:
        check(prog, fname, *shape, n, "random", mode, init)


@pytest.mark.parametrize("kind,shape", [("den_last", (2, 2)), ("den_edges", (2, 2)), ("den_edges", (1, 2)),
                                        ("num_middle", (2, 1)), ("num_middle", (1, 0)), ("max", (4, 4)),
                                        ("max", (2, 1)), ("max", (1, 0))])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_zeros_and_largest_limbs(prog, fname, fid, kind, shape):
    f = po.FIELDS[fname]
    init = words(f.to_mont(3))
    for n in SIZES:
        total = check(prog, fname, *shape, n, kind, "out", init)
        if kind == "den_last" or kind == "den_edges":
            assert total == 0, n


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_large_by_recurrence(prog, fname, fid):
    """Shape (2, 1), so an index-dependent power of R / R' cannot hide; no per-element
    inversion: out[i+1] D_i == out[i] N_i on the Montgomery words (one R more on the left)."""
    f = po.FIELDS[fname]
    r, n = f.modulus, LARGE
    a, b, d = (rand_mont(f, n, 7100 + j) for j in range(3))
    d[:, 0] |= np.uint64(1)
    init = words(f.to_mont(0x1234567 * 0xABCDEF123 + 99))
    bufs = [ecgpu.DeviceBuffer.upload(prog, c) for c in (a, b, d)]
    o = ecgpu.DeviceBuffer.upload(prog, np.zeros_like(a))
    total = ecgpu.fr_grand_product_dev(prog, fname, n, bufs[:2], bufs[2:], o, init=init, want_total=True)

    def ints(v):  # co.to_ints, through bytes: 2 M rows in a fraction of a second
        raw = np.ascontiguousarray(v, dtype="<u8").tobytes()
        return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]

    out = ints(o.read(np.uint64, a.shape)) + ints(total)
    for x in bufs + [o]:
        x.free()
    assert out[0] == ints(init)[0]
    assert max(out) < r
    R = f.R
    for i, (x, y, w) in enumerate(zip(ints(a), ints(b), ints(d))):
        assert (out[i + 1] * w * R - out[i] * x * y) % r == 0, i


def test_argument_errors(prog):
    f, fname, n = po.BLS12_381_FR, "bls12_381_fr", 70
    a = rand_mont(f, n + 1, 7200)
    d = ecgpu.DeviceBuffer.upload(prog, a)
    gp = functools.partial(ecgpu.fr_grand_product_dev, prog)
    for call in (lambda: gp("bls12_381_fq", n, [d]),
                 lambda: gp(fname, n, [], [d], d),
                 lambda: gp(fname, n, [d] * 5),
                 lambda: gp(fname, n, [d], [d] * 5),
                 lambda: gp(fname, n, [d, 0], [d], d),
                 lambda: gp(fname, n, [d], [0], d),
                 lambda: gp(fname, n, [d], init=words(f.modulus)),
                 lambda: gp(fname, n, [d], flags=2),
                 lambda: gp(fname, n, [d], [d], d.ptr.value + 32),
                 lambda: gp(fname, 2**32 + 1, [d])):
        with pytest.raises(ecgpu.EcError):
            call()
    init = words(f.to_mont(9))
    assert (gp(fname, 0, [d], [d], init=init, want_total=True) == init).all()  # n = 0 is OK: the total is init
    assert co.to_ints(gp(fname, 0, [d], canonical=True, want_total=True)[None])[0] == 1
    assert (d.read(np.uint64, a.shape) == a).all()
    d.free()
