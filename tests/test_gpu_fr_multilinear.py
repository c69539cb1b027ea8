"""Multilinear Fr on the device (ecg_fr_sumcheck_round_dev, ecg_fr_mle_fix_dev,
ecg_fr_eq_table_dev) against Python integers, bit-exact.  Tables pair the
entries 2b and 2b + 1: the lowest variable goes first.

Round sizes sit around the tile T = ecgpu.fr_sumcheck_tile() (512 elements; 1024
with the fused fold).  BIG = 2^21 is 4096 tiles (2048 with the fold): a two-column
call needs 32 KB (48 KB) of LDS per workgroup, so at most 5 (3) workgroups fit
each of the 256 compute units and the persistent grid is at most 1280 (768)
workgroups: every workgroup walks three tiles or more, and the fold launch sees
more partials than it has threads."""
from math import prod

import numpy as np
import pytest

import coracle as co
import ecgpu
import py_oracle as po
from test_gpu_fft import FIELDS, rand_mont

pytestmark = pytest.mark.gpu

LT = ecgpu.fr_sumcheck_tile().bit_length() - 1
BIG = 21
GATE = [(0, 1, 2), (0, 3, 4), (0, 5, 2, 4), (0, 6, 7), (0,)]  # eq (qL a + qR b + qM a b + qO c) + c5 eq
# name -> (columns, products, coefficients as field values | None)
SHAPES = {"f1": (1, [(0,)], None), "f2": (2, [(0, 1)], None), "f3": (3, [(0, 1, 2)], None),
          "f4": (4, [(0, 1, 2, 3)], [0xC0FFEE1234567]), "square": (1, [(0, 0)], None),
          "gate": (8, GATE, [3, 2**200 + 5, -1, 0xABCDEF, 7**80]),
          "worst": (8, [tuple((j + i) % 8 for i in range(4)) for j in range(8)], "top")}


@pytest.fixture(scope="module")
def prog(gpu_programs):
    return gpu_programs[0][0]


def words(vs):
    return co.u64arr(list(vs), 4)


def inputs(f, name, log_n, seed):
    """-> (column word arrays, products, coefficient words | None)"""
    k, products, cs = SHAPES[name]
    if cs == "top":  # pairs alternate (r - 1, 0) and (0, r - 1) as words, coefficient words r - 1
        top = f.modulus - 1
        col = words(([top, 0, 0, top] * (1 << log_n))[:1 << log_n])
        return [col.copy() for _ in range(k)], products, words([top] * len(products))
    cols = [rand_mont(f, 1 << log_n, seed + j) for j in range(k)]
    return cols, products, None if cs is None else words(f.to_mont(c % f.modulus) for c in cs)


def ints(a):
    """The rows of an (n, 4) u64 array as integers (what co.to_ints gives, fast enough for 2^21 rows)."""
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def values(f, a):
    rinv = pow(f.R, -1, f.modulus)
    return [w * rinv % f.modulus for w in ints(a)]


def fold_ref(r, col, x):
    """Binds the lowest variable to x; linear, so it maps words to words as well as values to values."""
    return [(lo + x * (hi - lo)) % r for lo, hi in zip(col[0::2], col[1::2])]


def round_ref(f, cols, products, cs):
    """The round polynomial's values at t = 0 .. d; cols are lists of Montgomery words, cs field values."""
    r, rinv = f.modulus, pow(f.R, -1, f.modulus)
    d = max(len(p) for p in products)
    at = [[c[0::2] for c in cols], [c[1::2] for c in cols]] + [[fold_ref(r, c, t) for c in cols] for t in range(2, d + 1)]
    return [sum(c * pow(rinv, len(p), r) * sum(prod(xs) for xs in zip(*(ct[j] for j in p))) for p, c in zip(products, cs))
            % r for ct in at]


def device_round(prog, f, fname, log_n, cols, products, cw, fold=None, **kw):
    """-> (values of the evaluations, folded tables' words | None, inputs unchanged)"""
    dev = [ecgpu.DeviceBuffer.upload(prog, c) for c in cols]
    out = None if fold is None else [ecgpu.DeviceBuffer(prog, c.nbytes // 2) for c in cols]
    ev = ecgpu.fr_sumcheck_round_dev(prog, fname, log_n, dev, products, coeffs=cw,
                                     fold_r=None if fold is None else words([f.to_mont(fold)])[0], d_folded=out, **kw)
    same = all((d.read(np.uint64, c.shape) == c).all() for d, c in zip(dev, cols))
    folded = None if out is None else [o.read(np.uint64, (len(c) // 2, 4)) for o, c in zip(out, cols)]
    for d in dev + (out or []):
        d.free()
    return (ints(ev) if kw.get("canonical") else values(f, ev)), folded, same


def check_round(prog, fname, name, log_n, fold=None):
    f = po.FIELDS[fname]
    cols, products, cw = inputs(f, name, log_n, 3000 + 16 * log_n)
    tabs = [ints(c) for c in cols]
    cs = [1] * len(products) if cw is None else values(f, cw)
    if fold is not None:
        tabs = [fold_ref(f.modulus, t, fold) for t in tabs]
    ref = round_ref(f, tabs, products, cs)
    got, folded, same = device_round(prog, f, fname, log_n, cols, products, cw, fold)
    assert got == ref and same, (name, log_n)
    if fold is not None:
        assert [ints(x) for x in folded] == tabs, (name, log_n, "folded")
        assert device_round(prog, f, fname, log_n - 1, folded, products, cw)[0] == got, (name, log_n, "unfused")
    else:
        assert device_round(prog, f, fname, log_n, cols, products, cw, canonical=True)[0] == ref, (name, log_n)


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_round(prog, fname, fid, name):
    for log_n in (1, 2, LT - 1, LT, LT + 1):
        check_round(prog, fname, name, log_n)


@pytest.mark.parametrize("name", ["f2", "f4", "gate", "worst"])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_fused_fold(prog, fname, fid, name):
    for log_n in (2, LT - 1, LT, LT + 1, LT + 2):
        check_round(prog, fname, name, log_n, fold=0x1234567 * 0xABCDEF123 + log_n)


@pytest.mark.parametrize("fold", [None, 2**250 + 99])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_round_many_tiles(prog, fname, fid, fold):
    check_round(prog, fname, "f2", BIG, fold)


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_whole_sumcheck(prog, fname, fid):
    """g_0(0) + g_0(1) is the sum over the cube and g_i(0) + g_i(1) = g_(i-1)(r_(i-1)), every round fused."""
    f, v = po.FIELDS[fname], 10
    r = f.modulus
    cols = [rand_mont(f, 1 << v, 3500 + j) for j in range(3)]
    cur = [ecgpu.DeviceBuffer.upload(prog, c) for c in cols]
    nxt = [ecgpu.DeviceBuffer(prog, c.nbytes // 2) for c in cols]
    claim = sum(prod(xs) for xs in zip(*(values(f, c) for c in cols))) % r
    for i in range(v):
        ch = None if i == 0 else words([f.to_mont(pow(7, 1000 + i, r))])[0]
        g = values(f, ecgpu.fr_sumcheck_round_dev(prog, fname, v - i + (i > 0), cur, [(0, 1, 2)], fold_r=ch,
                                                  d_folded=nxt if i else None))
        assert (g[0] + g[1]) % r == claim, i
        if i:
            cur, nxt = nxt, cur
        x = pow(7, 1001 + i, r)  # the next challenge; g(x) by Lagrange over t = 0 .. 3
        claim = sum(e * prod((x - s) * pow(t - s, -1, r) for s in range(4) if s != t) for t, e in enumerate(g)) % r
    for d in cur + nxt:
        d.free()


def eq_ref(r, point, scale=1):
    tab = [scale]
    for x in point:
        tab = [t * (1 - x) % r for t in tab] + [t * x % r for t in tab]
    return tab


@pytest.mark.parametrize("log_n", [5, 13])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_fix(prog, fname, fid, log_n):
    """m at the in-register (3), in-wave (9) and in-tile (11) boundaries and one past each; 13 needs two launches."""
    f = po.FIELDS[fname]
    r = f.modulus
    a = rand_mont(f, 1 << log_n, 3600 + log_n)
    point = [pow(5, 77 + j, r) for j in range(log_n)]
    pw = words(f.to_mont(x) for x in point)
    d_in, d_out = ecgpu.DeviceBuffer.upload(prog, a), ecgpu.DeviceBuffer(prog, a.nbytes // 2)
    ref = [values(f, a)]
    for x in point:
        ref.append(fold_ref(r, ref[-1], x))
    for m in sorted({m for m in (1, 3, 4, 9, 10, 11, 12, log_n) if m <= log_n}):
        val = ecgpu.fr_mle_fix_dev(prog, fname, d_in, log_n, pw[:m], d_out)
        assert values(f, d_out.read(np.uint64, (-1, 4))[:1 << (log_n - m)]) == ref[m], m
        assert (val is None) == (m < log_n)
    assert values(f, val[None]) == ref[log_n]
    assert ints(ecgpu.fr_mle_fix_dev(prog, fname, d_in, log_n, pw, canonical=True)[None]) == ref[log_n]
    ecgpu.fr_mle_fix_dev(prog, fname, d_in, log_n, pw[:4], d_out, canonical=True)
    assert ints(d_out.read(np.uint64, (-1, 4))[:1 << (log_n - 4)]) == ref[4]
    d_eq = ecgpu.DeviceBuffer(prog, a.nbytes)  # evaluate = <eq(point), f>, the eq table the device's
    ecgpu.fr_eq_table_dev(prog, fname, pw, d_eq)
    eq = values(f, d_eq.read(np.uint64, a.shape))
    assert sum(e * x for e, x in zip(eq, ref[0])) % r == ref[log_n][0]
    assert (d_in.read(np.uint64, a.shape) == a).all()
    for d in (d_in, d_out, d_eq):
        d.free()


@pytest.mark.parametrize("log_n", [1, 2, 7, 8, 13])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_eq_table(prog, fname, fid, log_n):
    f = po.FIELDS[fname]
    r = f.modulus
    point = [pow(11, 300 + j, r) for j in range(log_n)]
    d = ecgpu.DeviceBuffer(prog, 32 << log_n)
    for scale in (None, r - 12345):
        ecgpu.fr_eq_table_dev(prog, fname, words(f.to_mont(x) for x in point), d,
                              scale=None if scale is None else words([f.to_mont(scale)])[0])
        assert values(f, d.read(np.uint64, (1 << log_n, 4))) == eq_ref(r, point, scale or 1), scale
    ecgpu.fr_eq_table_dev(prog, fname, words(f.to_mont(x) for x in point), d, canonical=True)
    assert ints(d.read(np.uint64, (1 << log_n, 4))) == eq_ref(r, point)
    d.free()


def test_argument_errors(prog):
    f, fname, log_n = po.BLS12_381_FR, "bls12_381_fr", 4
    a = rand_mont(f, 1 << log_n, 3700)
    d, o = ecgpu.DeviceBuffer.upload(prog, a), ecgpu.DeviceBuffer(prog, a.nbytes)
    one, big = words([f.to_mont(1)])[0], words([f.modulus])[0]
    ok = dict(field=fname, log_n=log_n, cols=[d], products=[(0,)])
    for kw in (dict(products=[]), dict(products=[(0,)] * 9), dict(products=[()]), dict(products=[(0,) * 5]),
               dict(cols=[d] * 9), dict(cols=[]), dict(products=[(1,)]), dict(cols=[0]), dict(log_n=0), dict(log_n=33),
               dict(field="bls12_381_fq"), dict(coeffs=big[None]), dict(flags=2), dict(fold_r=one),
               dict(fold_r=big, d_folded=[o]), dict(fold_r=one, d_folded=[0]), dict(fold_r=one, d_folded=[d]),
               dict(fold_r=one, d_folded=[d.ptr.value + a.nbytes // 2]), dict(fold_r=one, d_folded=[o], log_n=1),
               dict(cols=[d, d], products=[(0, 1)], fold_r=one, d_folded=[o, o.ptr.value + 32]),
               dict(cols=[d.ptr.value + 8])):
        kw = {**ok, **kw}
        with pytest.raises(ecgpu.EcError):
            ecgpu.fr_sumcheck_round_dev(prog, kw.pop("field"), kw.pop("log_n"), kw.pop("cols"), kw.pop("products"), **kw)
    pt = np.tile(one, (log_n, 1))
    for args, kw in (((d, log_n, pt[:0], o), {}), ((d, log_n - 1, pt, o), {}), ((d, 33, pt, o), {}),
                     ((d, log_n, pt[:2], None), {}), ((d, log_n, pt[:2], d.ptr.value + 32), {}),
                     ((d, log_n, np.tile(big, (2, 1)), o), {}), ((d, log_n, pt, o), dict(flags=4)), ((0, log_n, pt, o), {})):
        with pytest.raises(ecgpu.EcError):
            ecgpu.fr_mle_fix_dev(prog, fname, *args, **kw)
    for args, kw in (((pt[:0], o), {}), ((np.tile(big, (2, 1)), o), {}), ((pt, o), dict(scale=big)),
                     ((pt, o), dict(flags=2)), ((pt, 0), {}), ((pt, o.ptr.value + 8), {})):
        with pytest.raises(ecgpu.EcError):
            ecgpu.fr_eq_table_dev(prog, fname, *args, **kw)
    with pytest.raises(ecgpu.EcError):
        ecgpu.fr_eq_table_dev(prog, "bn254_fq", pt, o)
    assert (d.read(np.uint64, a.shape) == a).all()
    d.free(), o.free()
