"""Fused sums of products over resident Fr vectors (ecg_fr_lincomb_dev) against
Python integers, bit-exact.

Sizes sit around the wave (64) and tile boundaries of ecgpu.fr_lincomb_tile();
1025 tiles + 7 gives every workgroup several tiles and the fold many partials."""
import numpy as np
import pytest

import coracle as co
import ecgpu
import py_oracle as po
from test_gpu_fft import FIELDS, rand_mont

pytestmark = pytest.mark.gpu

T = ecgpu.fr_lincomb_tile()
SIZES = [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5]


@pytest.fixture(scope="module")
def prog(gpu_programs):
    return gpu_programs[0][0]


def words(v):
    return co.u64arr([v], 4)[0]


def reference(f, n, terms, ratio=None, index0=0, canonical=False):
    """terms: (coefficient word | None, a | None, b | None, geo), a and b lists of Montgomery words."""
    r, rinv = f.modulus, pow(f.R, -1, f.modulus)
    g = None if ratio is None else ratio * rinv % r
    out = []
    for i in range(n):
        s = sum((1 if c is None else c * rinv) * (1 if a is None else a[i] * rinv) * (1 if b is None else b[i] * rinv)
                * (pow(g, index0 + i, r) if geo else 1) for c, a, b, geo in terms)
        out.append(s % r if canonical else s * f.R % r)
    return out


def run(prog, fname, n, terms, out="new", ratio=None, **kw):
    """terms as for reference() but with (n, 4) arrays; one device buffer per distinct array.
    out: "new", None (total only) or one of the arrays (in place).
    -> (output words | None, total | None, every input but `out` unchanged)"""
    bufs = {id(x): (x, ecgpu.DeviceBuffer.upload(prog, x)) for t in terms for x in t[1:3] if x is not None}
    dev = [(None if t[0] is None else words(t[0]), *(None if x is None else bufs[id(x)][1] for x in t[1:3]), t[3])
           for t in terms]
    if isinstance(out, str):
        bufs[out] = (None, ecgpu.DeviceBuffer.upload(prog, np.zeros((max(n, 1), 4), np.uint64)))
    o = None if out is None else bufs[out if isinstance(out, str) else id(out)][1]
    total = ecgpu.fr_lincomb_dev(prog, fname, n, dev, o, ratio=None if ratio is None else words(ratio), **kw)
    got = None if o is None else co.to_ints(o.read(np.uint64, (n, 4)))
    same = all((d.read(np.uint64, x.shape) == x).all() for x, d in bufs.values() if x is not None and x is not out)
    for _, d in bufs.values():
        d.free()
    return got, None if total is None else co.to_ints(total[None])[0], same


def form(f, name, n, seed):
    """-> (terms, ratio word, canonical)"""
    r = f.modulus
    a, b, c = (rand_mont(f, n, seed + j) for j in range(3))
    cw, g, top = f.to_mont(0xC0FFEE1234567), f.to_mont(f.omega(1 << 20)), r - 1
    if name == "max8":  # the largest limbs the lazy sums see: 16 distinct vectors of r - 1
        full = [np.tile(words(top), (n, 1)) for _ in range(16)]
        return [(top, full[2 * j], full[2 * j + 1], True) for j in range(8)], top, False
    return {"hadamard": ([(None, a, b, False)], None, False),
            "a_plus_cb": ([(None, a, None, False), (cw, None, b, False)], None, False),
            "ab_minus_c": ([(None, a, b, False), (f.to_mont(r - 1), c, None, False)], None, False),
            "omega_minus_z": ([(None, None, None, True), (f.to_mont(r - 12345), None, None, False)], g, False),
            "abg": ([(None, a, b, True)], g, False),
            "canonical": ([(cw, a, b, False), (None, c, None, True), (cw, a, None, True)], g, True)}[name]


def ints(terms):
    return [(c, *(None if x is None else co.to_ints(x) for x in ab), geo) for c, *ab, geo in terms]


FORMS = ["hadamard", "a_plus_cb", "ab_minus_c", "omega_minus_z", "abg", "max8", "canonical"]


@pytest.mark.parametrize("name", FORMS)
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_forms(prog, fname, fid, name):
    f = po.FIELDS[fname]
    for n in SIZES:
        terms, g, canon = form(f, name, n, 2000 + n)
        ref = reference(f, n, ints(terms), g, 0, canon)
        got, total, same = run(prog, fname, n, terms, ratio=g, canonical=canon, want_sum=True)
        assert got == ref and same, n
        assert total == sum(ref) % f.modulus, (n, "total")
        _, only, same = run(prog, fname, n, terms, out=None, ratio=g, canonical=canon, want_sum=True)
        assert only == total and same, (n, "total only")


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_in_place(prog, fname, fid):
    """d_out = A_0, the same buffer also B_1."""
    f = po.FIELDS[fname]
    for n in SIZES:
        x, y, z = (rand_mont(f, n, 2100 + n + j) for j in range(3))
        terms = [(None, x, y, False), (f.to_mont(77), z, x, False)]
        got, _, same = run(prog, fname, n, terms, out=x)
        assert got == reference(f, n, ints(terms)) and same, n


@pytest.mark.parametrize("name", ["omega_minus_z", "abg", "canonical"])
@pytest.mark.parametrize("fname,fid", FIELDS)
def test_index0(prog, fname, fid, name):
    f = po.FIELDS[fname]
    for n in (65, T + 1):
        terms, g, canon = form(f, name, n, 2200 + n)
        for index0 in (0, T - 3, 2**31 + 2**20 - 5, 2**32 - n):
            got, _, _ = run(prog, fname, n, terms, ratio=g, index0=index0, canonical=canon)
            assert got == reference(f, n, ints(terms), g, index0, canon), (n, index0)


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_total_large(prog, fname, fid):
    f, n = po.FIELDS[fname], 1025 * T + 7
    terms, _, _ = form(f, "hadamard", n, 2300)
    ref = reference(f, n, ints(terms))
    got, total, same = run(prog, fname, n, terms, want_sum=True)
    assert got == ref and total == sum(ref) % f.modulus and same
    assert run(prog, fname, n, terms, out=None, want_sum=True)[1] == total


@pytest.mark.parametrize("fname,fid", FIELDS)
def test_barycentric_opening(prog, fname, fid):
    """p(z) from the evaluations without leaving the device: d_i = w^i - z, batch inverse,
    S = sum f_i d_i^-1 w^i; p(z) = (1 - z^n) / n * S (the sign of d_i = w^i - z, not z - w^i)."""
    f, log_n = po.FIELDS[fname], 12
    n, r = 1 << log_n, f.modulus
    om, z = f.omega(n), 0x1234567 * 0xABCDEF123 + 99
    p = rand_mont(f, n, 2400)
    d_p, d_f = ecgpu.DeviceBuffer.upload(prog, p), ecgpu.DeviceBuffer.upload(prog, p)
    d_d = ecgpu.DeviceBuffer(prog, p.nbytes)
    ecgpu.fft_dev(prog, fname, d_f, words(f.to_mont(om)), log_n)
    ecgpu.fr_lincomb_dev(prog, fname, n, [(None, None, None, True), (words(f.to_mont(r - z)), None, None, False)], d_d,
                         ratio=words(f.to_mont(om)))
    ecgpu.batch_inverse_dev(prog, fname, d_d, n)
    s = ecgpu.fr_lincomb_dev(prog, fname, n, [(None, d_f, d_d, True)], ratio=words(f.to_mont(om)), want_sum=True)
    pz = ecgpu.poly_div_linear_dev(prog, fname, d_p, n, words(f.to_mont(z)))
    want = (1 - pow(z, n, r)) * pow(n, -1, r) * f.from_mont(co.to_ints(s[None])[0]) % r
    assert f.from_mont(co.to_ints(pz[None])[0]) == want
    for d in (d_p, d_f, d_d):
        d.free()


def test_argument_errors(prog):
    f, fname, n = po.BLS12_381_FR, "bls12_381_fr", 70
    a = rand_mont(f, n + 1, 2500)
    d = ecgpu.DeviceBuffer.upload(prog, a)
    one, big, g = words(f.to_mont(1)), words(f.modulus), words(f.to_mont(3))
    t = (None, d, None, False)
    for kw in (dict(terms=[]), dict(terms=[t] * 9), dict(terms=[(big, d, None, False)]),
               dict(terms=[(None, d, None, True)], ratio=big), dict(terms=[t], geo_mask=2, ratio=g),
               dict(terms=[(None, d, None, True)]), dict(terms=[t], index0=2**32 - n + 1), dict(terms=[t], flags=2),
               dict(terms=[t], d_out=None), dict(terms=[t], field="bls12_381_fq"),
               dict(terms=[(one, d, d.ptr.value + 8, False)]), dict(terms=[(None, d.ptr.value + 32, None, False)])):
        kw = {"field": fname, "d_out": d, **kw}
        with pytest.raises(ecgpu.EcError):
            ecgpu.fr_lincomb_dev(prog, kw.pop("field"), n, kw.pop("terms"), kw.pop("d_out"), **kw)
    assert (ecgpu.fr_lincomb_dev(prog, fname, 0, [t], d, want_sum=True) == 0).all()  # n = 0 is OK
    assert (d.read(np.uint64, a.shape) == a).all()
    d.free()
