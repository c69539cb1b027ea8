"""The contracts of the reduced-radix field form (csrc/fieldrr.hpp) replayed on
exact Python integers at their worst-case operands.  CPU only.

fieldrr.hpp states bounds -- quasi-normalised (QN) limbs, lazy values of many
p, wide negations, un-carried sums, 64-bit column accumulators (63 bits in the
signed ceil-carry chains of P[0] = 1, BLS12-381 Fr), split columns in the
13 x 30-bit layout -- and uniform random data never comes near any of them.
Here every clause has an operand class that sits ON its bound, for all six
layouts of params_rr.inc:

  * a model of each function on 32 / 64-bit machine integers, the same
    sequence of operations as the C++ (every product variant: split columns,
    the two chains of rr_mul_sum2, the doubled operand of the squarings, the
    ceil form), which tracks every accumulator and fails when one reaches
    2^64 (2^63 in a ceil-form chain) or a limb leaves 32 bits;
  * an exact-integer reference per function (value = sum limb_i 2^(BITS i); a
    product is (ab + m p) / R' with m = -ab / p mod R'; sums and differences
    are a +- ... + K p; rr_reduce_q is v - q p with the documented q);
  * operand generators that assert their own preconditions.

tests/test_gpu_rr_ops.py runs the same classes through the device functions
(ecg_rr_ops) against the same references.

The NTT's call sites (ntt_pass.hpp) get classes of their own, derived from
the K p rows and the add_nc / sub_nc sequence of the butterflies: limbs up to
2 (2^29 - 1) + max(16p row) = 2.5 x 2^30.  Against a twiddle with eight limbs
of 2^29 - 1 such an operand puts more than 2^63 into column 7, which the
signed ceil-carry chains misread (test_ceil_form_cannot_take_ntt_operands
pins that), so those products name their operand's limb bound and run in the
unsigned general form (rr_use_ceil); the model picks the form by the same
rule.

Layout.use_ceil, col_bound and ntt_limbs are hand-written copies of
rr_use_ceil, rr_col_bound and NttLimbs: this file checks that the RULE is
sound (no chain it sends to the ceil form reaches 2^63), not that the C++
still follows it.  A change of the C++ rule alone shows in the device run of
the mul_ntt / mul2_ntt classes (tests/test_gpu_rr_ops.py), whose operands
overflow a ceil chain, and in the header's own static_asserts."""
import math
import random

import pytest

import py_oracle as po
from test_params_rr import parse, value

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
BASE = {"bls12_381_fr": po.BLS12_381_FR, "bn254_fr": po.BN254_FR, "bls12_381_fq13": po.BLS12_381_FQ,
        "bls12_381_fq": po.BLS12_381_FQ, "bn254_fq9": po.BN254_FQ, "bn254_fq": po.BN254_FQ}
NTT_LAYOUTS = ("bls12_381_fr", "bn254_fr")
LIMB_LAZY = 2833000000  # "limbs < 2^31.4" (rr_reduce_q); NttLimbs asserts the P-form below it


class Violation(AssertionError):
    """An accumulator or a limb left the range the code relies on."""


class Layout:
    def __init__(self, name, d):
        self.name, self.f = name, BASE[name]
        self.p = self.f.modulus
        self.NL, self.B, self.SLACK, self.INV = d["NL"], d["BITS"], d["SLACK_LOG2"], d["INV"]
        self.P, self.KP, self.KPD, self.KP_OK, self.KPD_OK = d["P"], d["KP"], d["KPD"], d["KP_OK"], d["KPD_OK"]
        self.TO_RR, self.FROM_RR = d["TO_RR"], d["FROM_RR"]
        self.MASK = (1 << self.B) - 1
        self.T = 1 << (self.B * (self.NL - 1))          # weight of the top limb
        self.RP = 1 << (self.B * self.NL)               # R'
        self.QN = (1 << self.B) + (1 << (32 - self.B)) - 1   # largest QN limb below the top one
        self.words = 2 * ((self.p.bit_length() + 63) // 64)  # 32-bit words of the boundary form
        self.bound = (self.p * self.p << self.SLACK) // 2    # a b <= 2^SLACK p^2 / 2
        self.pinv = pow(self.p, -1, self.RP)
        assert value(self.P, self.B) == self.p

    def val(self, limbs):
        return value(limbs, self.B)

    def exact(self, v):
        assert 0 <= v < self.T << 32
        return [(v >> (self.B * i)) & self.MASK for i in range(self.NL - 1)] + [v >> (self.B * (self.NL - 1))]

    def ks(self, deep=False):
        ok = self.KP_OK if (not deep or self.B > 29) else self.KPD_OK
        return [2 << j for j in range(8) if (ok >> j) & 1]

    def kp(self, k, deep=False):
        return (self.KPD if deep and self.B <= 29 else self.KP)[k.bit_length() - 2]

    # ---- the column bounds of fieldrr.hpp (rr_col_fits, rr_col_bound, rr_use_ceil) ----
    def col_fits(self, k, sets):
        lim, nl = 1 << self.B, self.NL
        half = k + 1 if k < nl else 2 * nl - 1 - k
        s = sets * half * (lim + 3) ** 2 + (1 << 37)
        j0, j1 = (0, k) if k < nl else (k - nl + 1, nl - 1)
        return s + sum((lim - 1) * self.P[j] for j in range(j0, j1 + 1)) < 1 << 64

    def split(self, k, sets=1):
        return self.B > 29 and not self.col_fits(k, sets)

    def col_bound(self, k, amax):
        nl, top = self.NL, 64 * (self.P[-1] + 1)
        j0, j1 = (0, k) if k < nl else (k - nl + 1, nl - 1)
        s = 1 << 37
        for i in range(j0, j1 + 1):
            s += (top if i == nl - 1 else amax) * (top if k - i == nl - 1 else self.QN) + self.MASK * self.P[k - i]
        return s

    def use_ceil(self, amax=0):
        if amax:
            assert self.B <= 29 and all(self.col_bound(k, amax) < 1 << 64 for k in range(2 * self.NL - 1))
        return self.P[0] == 1 and all(self.col_bound(k, amax or self.QN) < 1 << 63 for k in range(2 * self.NL - 1))

    # ---- the NTT's limb bounds (fieldrr.hpp NttLimbs) ----
    def ntt_limbs(self):
        e = self.MASK
        kmax = lambda k: max(self.kp(k)[:-1])
        d, s, a0, a1, b1 = e + kmax(8), 2 * e, 4 * e, 2 * e + kmax(16), e + kmax(4)
        pf = max(a0, a1)
        assert a1 >= b1 and pf >= d and s <= (2 << self.B) - 2 and pf < LIMB_LAZY
        return {"E": e, "D": d, "S": s, "A0": a0, "A1": a1, "B1": b1, "PF": pf}


LAYOUTS = {n: Layout(n, d) for n, d in parse().items()}
assert sorted(LAYOUTS) == sorted(BASE)


# ---------------------------------------------------------------------------
# machine-integer models (same operation order as fieldrr.hpp)
# ---------------------------------------------------------------------------
class Acc:
    """A 64-bit accumulator that refuses to wrap."""

    def __init__(self, limit_log2, v=0):
        self.lim, self.v, self.peak = 1 << limit_log2, v, v

    def add(self, x):
        self.v += x
        self.peak = max(self.peak, self.v)
        if self.v >= self.lim:
            raise Violation(f"accumulator reaches {self.v / self.lim:.3f} x 2^{self.lim.bit_length() - 1}")


def u32(x, what="limb"):
    if not 0 <= x <= M32:
        raise Violation(f"{what} {x} leaves 32 bits")
    return x


def m_mul(L, a, b, amax=0, force_ceil=None):
    """rr_mul (and each chain of rr_mul2)."""
    nl, B, MASK, P = L.NL, L.B, L.MASK, L.P
    ceil = L.use_ceil(amax) if force_ceil is None else force_ceil
    m, r = [0] * nl, [0] * nl
    # ceil form: z = x - 1, kept here as x with the 2^63 limit on z
    acc = Acc(63 if ceil else 64)
    for k in range(2 * nl - 1):
        i0, i1 = (0, k) if k < nl else (k - nl + 1, nl - 1)
        for i in range(i0, i1 + 1):
            acc.add(a[i] * b[k - i])
        h = 0
        if L.split(k):
            assert not ceil
            h, acc.v = acc.v >> B, acc.v & MASK
        for i in range(i0, min(i1, k - 1) + 1):
            acc.add(m[i] * P[k - i])
        if k < nl:
            if ceil:      # m = -x mod 2^B, carry = ceil(x / 2^B); z = x - 1 < 2^63 is what Acc checked
                m[k] = -acc.v & MASK
                acc.v = -(-acc.v >> B)
            else:
                m[k] = ((acc.v & M32) * L.INV & M32) & MASK
                acc.add(m[k] * P[0])
                assert acc.v & MASK == 0
                acc.v >>= B
        else:
            r[k - nl] = acc.v & MASK
            acc.v >>= B
        acc.add(h)
    r[nl - 1] = u32(acc.v, "top limb")
    return r


def m_sqr(L, a):
    """rr_sqr (and each chain of rr_sqr2): off-diagonal products against 2 a."""
    nl, B, MASK, P = L.NL, L.B, L.MASK, L.P
    a2 = [u32(2 * x, "doubled limb") for x in a]
    m, r = [0] * nl, [0] * nl
    acc = Acc(64)
    for k in range(2 * nl - 1):
        i0, i1 = (0, k) if k < nl else (k - nl + 1, nl - 1)
        i = i0
        while 2 * i < k:
            acc.add(a2[i] * a[k - i])
            i += 1
        if k % 2 == 0:
            acc.add(a[k // 2] ** 2)
        h = 0
        if L.split(k):
            h, acc.v = acc.v >> B, acc.v & MASK
        for i in range(i0, min(i1, k - 1) + 1):
            acc.add(m[i] * P[k - i])
        if k < nl:
            m[k] = ((acc.v & M32) * L.INV & M32) & MASK
            acc.add(m[k] * P[0])
        else:
            r[k - nl] = acc.v & MASK
        acc.v >>= B
        acc.add(h)
    r[nl - 1] = u32(acc.v, "top limb")
    return r


def m_mul_sum2(L, a, b, c, d):
    """rr_mul_sum2: chain 0 = a b + carry, chain 1 = c d restarted per column,
    the m p products dealt alternately to the two, merged before the digit."""
    nl, B, MASK, P = L.NL, L.B, L.MASK, L.P
    m, r = [0] * nl, [0] * nl
    x0 = Acc(64)
    for k in range(2 * nl - 1):
        i0, i1 = (0, k) if k < nl else (k - nl + 1, nl - 1)
        x1 = Acc(64)
        for i in range(i0, i1 + 1):
            x0.add(a[i] * b[k - i])
            x1.add(c[i] * d[k - i])
        sp, h = L.split(k, 2), 0
        if sp:
            h = (x0.v >> B) + (x1.v >> B)
            x0.v, x1.v = (x0.v & MASK) + (x1.v & MASK), 0
        j1 = k - 1 if k < nl else nl - 1
        j = i0
        while j + 1 <= j1:
            x0.add(m[j] * P[k - j])
            x1.add(m[j + 1] * P[k - j - 1])
            j += 2
        if j == j1:
            x0.add(m[j] * P[k - j])
        x0.add(x1.v)
        if k < nl:
            m[k] = ((x0.v & M32) * L.INV & M32) & MASK
            x0.add(m[k] * P[0])
        else:
            r[k - nl] = x0.v & MASK
        x0.v >>= B
        x0.add(h)
    r[nl - 1] = u32(x0.v, "top limb")
    return r


def m_carry(L, s):
    B, MASK, nl = L.B, L.MASK, L.NL
    for x in s:
        u32(x)
    return [s[0] & MASK] + [(s[i] & MASK) + (s[i - 1] >> B) for i in range(1, nl - 1)] + \
        [u32(s[nl - 1] + (s[nl - 2] >> B), "top limb")]


def m_lin(L, plus, minus, row=None):
    """limb-wise sum(plus) + row - sum(minus), each step inside 32 bits the way the C++ orders it"""
    out = []
    for i in range(L.NL):
        s = plus[0][i] if plus else 0
        if row is not None:
            s = u32(s + row[i]) if plus else row[i]
        for x in plus[1:]:
            s = u32(s + x[i])
        for x in minus:
            s = u32(s - x[i], "difference limb")
        out.append(s)
    return out


def m_carry_seq(L, a):
    r, c = [], 0
    for i in range(L.NL - 1):
        t = a[i] + c
        r.append(t & L.MASK)
        c = t >> L.B
    return r + [u32(a[-1] + c, "top limb")]


def reduce_q_quotient(L, top):
    return top * ((1 << 32) // (L.P[-1] + 1)) >> 32


def m_reduce_q(L, a):
    q, r, c = reduce_q_quotient(L, a[-1]), [], 0
    for i in range(L.NL - 1):
        t = a[i] + c - q * L.P[i]
        assert abs(t) < 1 << 63
        r.append(t & L.MASK)
        c = t >> L.B
    return r + [u32(a[-1] + c - q * L.P[-1], "top limb")]


def m_canon(L, a, top_masked=False):
    t, br = [], 0
    for i in range(L.NL):
        d = a[i] - L.P[i] + br
        assert -(1 << 31) <= d < 1 << 31
        t.append(d & L.MASK if (i + 1 < L.NL or top_masked) else d & M32)
        br = d >> L.B
    return t if br == 0 else list(a)


def unpack(L, w):
    v = sum(x << (32 * i) for i, x in enumerate(w))
    return [(v >> (L.B * i)) & L.MASK for i in range(L.NL)]


def pack(L, limbs):
    v = L.val(limbs)
    return [(v >> (32 * j)) & M32 for j in range(L.words)]


def words_row(L, v):
    """v as the first `words` 32-bit words of an NL-word row"""
    return [(v >> (32 * j)) & M32 for j in range(L.words)] + [0] * (L.NL - L.words)


def model(L, op, ops, k=0):
    """(out0, out1, flag) as the device functions compute them"""
    a, b, c, d = (list(ops) + [None] * 4)[:4]
    z = [0] * L.NL
    if op == "mul":
        return m_mul(L, a, b), z, 0
    if op == "mul_ntt":
        return m_mul(L, a, b, L.ntt_limbs()["PF"]), z, 0
    if op == "mul2":
        return m_mul(L, a, b), m_mul(L, c, d), 0
    if op == "mul2_ntt":
        pf = L.ntt_limbs()["PF"]
        return m_mul(L, a, b, pf), m_mul(L, c, d, pf), 0
    if op == "sqr":
        return m_sqr(L, a), z, 0
    if op == "sqr2":
        return m_sqr(L, a), m_sqr(L, b), 0
    if op == "mul_sum2":
        return m_mul_sum2(L, a, b, c, d), z, 0
    if op == "add":
        return m_carry(L, m_lin(L, [a, b], [])), z, 0
    if op == "sub":
        return m_carry(L, m_lin(L, [a], [b], L.kp(k))), z, 0
    if op == "neg":
        return m_carry(L, m_lin(L, [], [a], L.kp(k))), z, 0
    if op in ("sub2", "sub3"):
        subs = [b, c] if op == "sub2" else [b, c, d]
        if L.B > 29:  # no deep borrow: the subtrahends are summed (rr_add) first
            t = subs[-1]
            for x in reversed(subs[:-1]):
                t = m_carry(L, m_lin(L, [x, t], []))
            return m_carry(L, m_lin(L, [a], [t], L.kp(k))), z, 0
        return m_carry(L, m_lin(L, [a], subs, L.kp(k, deep=True))), z, 0
    if op == "neg_wide":
        return m_lin(L, [], [a], L.kp(k)), z, 0
    if op == "add_nc":
        return m_lin(L, [a, b], []), z, 0
    if op == "sub_nc":
        return m_lin(L, [a], [b], L.kp(k)), z, 0
    if op == "carry":
        return m_carry(L, a), z, 0
    if op == "carry_seq":
        return m_carry_seq(L, a), z, 0
    if op == "reduce_q":
        return m_reduce_q(L, a), z, 0
    if op == "canon_lt2p":
        return m_canon(L, a), z, 0
    if op == "from_std":
        return m_mul(L, unpack(L, a[:L.words]), L.TO_RR), z, 0
    if op == "to_std":
        y = m_canon(L, m_mul(L, a, L.FROM_RR), top_masked=True)
        return pack(L, y) + [0] * (L.NL - L.words), z, 0
    if op == "is_zero_prod":
        return z, z, int(not any(a) or a == L.P)
    if op == "maybe_zero_prod":
        return z, z, int(a[0] == 0 or a[0] == L.P[0])
    raise KeyError(op)


# ---------------------------------------------------------------------------
# exact-integer references and the documented output forms
# ---------------------------------------------------------------------------
def mont(L, x):
    """(x + m p) / R' with m = -x / p mod R'"""
    m = -x * L.pinv % L.RP
    q, rem = divmod(x + m * L.p, L.RP)
    assert rem == 0
    return q


def expect(L, op, ops, k=0):
    """{'v0', 'v1', 'flag', 'form', 'lt'}: output values as exact integers (None:
    not an output), the limb form of the outputs and an upper bound of v0."""
    v = [L.val(x) for x in ops]
    p, e = L.p, {"v0": None, "v1": None, "flag": None, "form": "exact", "lt": None}
    half = lambda x: p + p // 2 if x <= L.bound else None   # the 1.5 p output bound, inside the contract
    if op in ("mul", "mul_ntt"):
        e.update(v0=mont(L, v[0] * v[1]), lt=half(v[0] * v[1]))
    elif op in ("mul2", "mul2_ntt"):
        e.update(v0=mont(L, v[0] * v[1]), v1=mont(L, v[2] * v[3]), lt=half(v[0] * v[1]))
    elif op == "sqr":
        e.update(v0=mont(L, v[0] ** 2), lt=half(v[0] ** 2))
    elif op == "sqr2":
        e.update(v0=mont(L, v[0] ** 2), v1=mont(L, v[1] ** 2), lt=half(v[0] ** 2))
    elif op == "mul_sum2":
        e.update(v0=mont(L, v[0] * v[1] + v[2] * v[3]), lt=half(v[0] * v[1] + v[2] * v[3]))
    elif op == "add":
        e.update(v0=v[0] + v[1], form="qn")
    elif op == "sub":
        e.update(v0=v[0] - v[1] + k * p, form="qn")
    elif op == "neg":
        e.update(v0=k * p - v[0], form="qn")
    elif op == "sub2":
        e.update(v0=v[0] + k * p - v[1] - v[2], form="qn")
    elif op == "sub3":
        e.update(v0=v[0] + k * p - v[1] - v[2] - v[3], form="qn")
    elif op == "neg_wide":
        e.update(v0=k * p - v[0], form="wide")
    elif op == "add_nc":
        e.update(v0=v[0] + v[1], form="raw")
    elif op == "sub_nc":
        e.update(v0=v[0] + k * p - v[1], form="raw")
    elif op == "carry":
        e.update(v0=v[0], form="qn")
    elif op == "carry_seq":
        e.update(v0=v[0])
    elif op == "reduce_q":
        top = ops[0][-1]
        e.update(v0=v[0] - reduce_q_quotient(L, top) * p)
        if v[0] < 64 * p and max(ops[0][:-1]) <= LIMB_LAZY:
            e["lt"] = p + (p * top >> 32) + (L.T << 7)
    elif op == "canon_lt2p":
        assert v[0] < 2 * p
        e.update(v0=v[0] % p, lt=p)
    elif op == "from_std":
        w = sum(x << (32 * i) for i, x in enumerate(ops[0][:L.words]))
        assert w < p
        e.update(v0=mont(L, w * L.val(L.TO_RR)), lt=p + p // 2)
    elif op == "to_std":
        e.update(v0=v[0] * L.f.R * pow(L.RP, -1, p) % p, form="std", lt=p)
    elif op == "is_zero_prod":
        assert v[0] < 2 * p
        e.update(flag=int(v[0] % p == 0), form=None)
    elif op == "maybe_zero_prod":   # necessary condition, decided on the low limb
        e.update(flag=int(ops[0][0] in (0, L.P[0])), form=None)
        assert e["flag"] or v[0] % p
    else:
        raise KeyError(op)
    return e


def check_output(L, op, ops, k, out0, out1, flag):
    """out0 / out1 / flag (from the model or the device) against the reference"""
    e = expect(L, op, ops, k)
    tag = (L.name, op, k)
    if e["flag"] is not None:
        assert flag == e["flag"], tag
        return
    got = sum(x << (32 * i) for i, x in enumerate(out0)) if e["form"] == "std" else L.val(out0)
    assert got == e["v0"], (tag, "value", got - e["v0"])
    if e["lt"] is not None:
        assert got < e["lt"], (tag, "bound", got / L.p)
    low_max = {"exact": L.MASK, "qn": L.QN, "wide": 3 * (1 << L.B) - 1, "raw": M32, "std": M32}[e["form"]]
    assert all(0 <= x <= low_max for x in out0[:-1]) and 0 <= out0[-1] <= M32, (tag, "form", e["form"])
    if e["form"] == "std":
        assert all(x == 0 for x in out0[L.words:]), tag
    if e["v1"] is not None:   # second output: the single product's result, limb for limb
        single = model(L, {"mul2": "mul", "sqr2": "sqr", "mul2_ntt": "mul_ntt"}[op],
                       ops[2:] if op != "sqr2" else ops[1:2], k)[0]
        assert L.val(out1) == e["v1"] and list(out1) == single, (tag, "second output")
        first = model(L, {"mul2": "mul", "sqr2": "sqr", "mul2_ntt": "mul_ntt"}[op], ops[:2] if op != "sqr2" else ops[:1], k)[0]
        assert list(out0) == first, (tag, "first output")


# ---------------------------------------------------------------------------
# operand generators (each asserts its own preconditions)
# ---------------------------------------------------------------------------
def shaped(L, target, pattern, low=None):
    """limbs of the largest value <= target whose limbs below the top one follow
    `pattern` at height `low` (default: the QN maximum)"""
    low = L.QN if low is None else low
    n = L.NL - 1
    lows = {"max": [low] * n, "zero": [0] * n, "alt0": [low * (i % 2 == 0) for i in range(n)],
            "alt1": [low * (i % 2) for i in range(n)]}.get(pattern)
    if lows is None:   # ("one", i) or ("range", i0, i1): limbs i0..i1 at `low`
        i0, i1 = (pattern[1], pattern[1]) if pattern[0] == "one" else pattern[1:]
        lows = [low * (i0 <= i <= i1) for i in range(n)]
    lv = value(lows, L.B)
    assert target >= lv, "target below the pattern's own value"
    r = lows + [(target - lv) // L.T]
    assert r[-1] <= M32 and target - L.T < L.val(r) <= target
    return r


def rand_qn(L, rng, target, low=None):
    low = L.QN if low is None else low
    while True:
        lows = [rng.choice((0, low, rng.randrange(low + 1))) for _ in range(L.NL - 1)]
        lv = value(lows, L.B)
        if lv <= target:
            t = (target - lv) // L.T
            return lows + [rng.randrange(t + 1) if rng.random() < 0.5 else t]


PATTERNS = ["max", "zero", "alt0", "alt1", ("one", 0), ("one", 3)]


def edges(L):
    p = L.p
    return [L.exact(v) for v in (0, 1, p - 1, p, p + 1, p + p // 2 - 1)]


def product_targets(L):
    """(value bound of a, value bound of b) with a b <= 2^SLACK p^2 / 2"""
    p, bd = L.p, 1 << (L.SLACK - 1)
    t = [(bd * p, p), (math.isqrt(L.bound), math.isqrt(L.bound))]
    if bd >= 64:
        t.append((64 * p, bd // 64 * p))
    for x, y in t:
        assert x * y <= L.bound
    return t


def split_columns(L):
    return [k for k in range(2 * L.NL - 1) if L.split(k)]


def pair_rows(L, rng, ta, tb, n_rand):
    rows = [(shaped(L, ta, pa), shaped(L, tb, pb)) for pa in PATTERNS for pb in ("max", "zero", "alt1")]
    rows += [(y, x) for x, y in rows[:6]]
    rows += [(rand_qn(L, rng, ta), rand_qn(L, rng, tb)) for _ in range(n_rand)]
    for k in split_columns(L):   # maxed limbs exactly where they feed split column k
        i0, i1 = (0, k) if k < L.NL else (k - L.NL + 1, L.NL - 1)
        i1 = min(i1, L.NL - 2)
        rows.append((shaped(L, ta, ("range", i0, i1)), shaped(L, tb, ("range", max(0, k - i1), min(k - i0, L.NL - 2)))))
    return rows


def classes(L, n_rand=40, seed=1):
    """yields (op, k, class name, rows); a row is a tuple of operand limb lists"""
    rng = random.Random(f"{L.name}/{seed}")
    p, T = L.p, L.T
    ed = edges(L)
    tg = product_targets(L)

    # ---- products ----
    pairs = [(x, y) for x in ed for y in ed]
    yield "mul", 0, "edges", pairs
    yield "sqr", 0, "edges", [(x,) for x in ed]
    for n, (ta, tb) in enumerate(tg):
        rows = pair_rows(L, rng, ta, tb, n_rand)
        yield "mul", 0, f"bound{n}", rows
        yield "mul2", 0, f"bound{n}", [r + s for r, s in zip(rows, rows[1:] + rows[:1])]
        # a b + c d <= bound: halve one factor of each product
        half = pair_rows(L, rng, ta, tb // 2, n_rand)
        sum2 = [r + s for r, s in zip(half, half[3:] + half[:3])]
        # two product sets at once: all four operands with every low limb at the QN maximum ...
        qa, qb = shaped(L, ta, "max"), shaped(L, tb // 2, "max")
        assert all(x == L.QN for o in (qa, qb) for x in o[:-1]) and 2 * L.val(qa) * L.val(qb) <= L.bound
        sum2 += [(qa, qb, qa, qb), (qb, qa, qa, qb), (qa, qb, qb, qa)]
        # ... and maxed exactly where they feed column k, for every column rr_mul_sum2 splits (two sets)
        for k in range(2 * L.NL - 1):
            if L.split(k, 2):
                i0, i1 = (0, k) if k < L.NL else (k - L.NL + 1, L.NL - 1)
                i1 = min(i1, L.NL - 2)
                ra = shaped(L, ta, ("range", i0, i1))
                rb = shaped(L, tb // 2, ("range", max(0, k - i1), min(k - i0, L.NL - 2)))
                sum2 += [(ra, rb, ra, rb), (ra, rb, rb, ra)]
        yield "mul_sum2", 0, f"bound{n}", sum2
    ts = math.isqrt(L.bound)
    sq = [(shaped(L, ts, pa),) for pa in PATTERNS] + [(rand_qn(L, rng, ts),) for _ in range(n_rand)]
    for k in split_columns(L):
        i0, i1 = (0, k) if k < L.NL else (k - L.NL + 1, L.NL - 1)
        sq.append((shaped(L, ts, ("range", i0, min(i1, L.NL - 2))),))
    yield "sqr", 0, "bound", sq
    yield "sqr2", 0, "bound", [r + s for r, s in zip(sq, sq[1:] + sq[:1])]
    yield "mul_sum2", 0, "edges", [(w, x, y, z) for w, x in pairs[::5] for y, z in pairs[1::11]]
    if L.B <= 29:   # a wide negation against a product output
        k = 4
        assert k * p * (p + p // 2) <= L.bound
        wide = [model(L, "neg_wide", (x,), k)[0] for x in ed + [L.exact(rng.randrange(p + p // 2)) for _ in range(n_rand)]]
        outs = ed[2:] + [L.exact(p + p // 2 - 1)] + [shaped(L, p + p // 2 - 1, "max", L.MASK)]
        yield "mul", 0, "neg_wide", [(w, y) for w in wide for y in outs]
        yield "mul2", 0, "neg_wide", [(w, y, w2, y) for w, w2 in zip(wide, wide[1:] + wide[:1]) for y in outs[-2:]]

    # ---- sums and differences ----
    lazy = [shaped(L, t, pa) for t in (2 * p, 64 * p) for pa in PATTERNS] + ed
    yield "add", 0, "qn", [(x, y) for x in lazy[::2] for y in lazy[1::3]] + \
        [(rand_qn(L, rng, 64 * p), rand_qn(L, rng, 64 * p)) for _ in range(n_rand)]
    yield "add_nc", 0, "qn", [(x, y) for x in lazy[::3] for y in lazy[::4]]
    for k in L.ks():
        subs = [shaped(L, k * p // 2, pa) for pa in PATTERNS]   # value on the K p / 2 bound, QN-max limbs
        assert all(k * p // 2 - T < L.val(x) <= k * p // 2 for x in subs)
        mins = [ed[0], shaped(L, 64 * p, "max"), shaped(L, 2 * p, "zero")]
        rnd = [(rand_qn(L, rng, 64 * p), rand_qn(L, rng, k * p // 2)) for _ in range(n_rand // 4)]
        yield "sub", k, "half", [(a, b) for a in mins for b in subs] + rnd
        yield "sub_nc", k, "half", [(a, b) for a in mins for b in subs] + rnd
        yield "neg", k, "half", [(b,) for b in subs] + [(r[1],) for r in rnd] + [(x,) for x in ed]
        yield "neg_wide", k, "half", [(b,) for b in subs] + [(r[1],) for r in rnd] + [(x,) for x in ed]
    for k in L.ks(deep=True):   # b + c (+ d) on the bound, every one with QN-max limbs
        h = k * p // 2
        two = [(a, shaped(L, h // 2, pa), shaped(L, h - h // 2, pb)) for a in (ed[0], shaped(L, 64 * p, "max"))
               for pa, pb in (("max", "max"), ("alt0", "alt1"), ("zero", "max"))]
        three = [(a, shaped(L, h // 3, pa), shaped(L, h // 3, pb), shaped(L, h - 2 * (h // 3), "max"))
                 for a in (ed[0], shaped(L, 64 * p, "max")) for pa, pb in (("max", "max"), ("alt0", "alt1"))]
        yield "sub2", k, "half", two
        yield "sub3", k, "half", three

    # ---- carries ----
    raw = [[M32] * (L.NL - 1) + [0], [M32] * (L.NL - 1) + [M32 - (M32 >> L.B) - 1], [0] * L.NL,
           [M32 * (i % 2) for i in range(L.NL - 1)] + [7]] + \
          [[rng.randrange(1 << 32) for _ in range(L.NL - 1)] + [rng.randrange(1 << 31)] for _ in range(n_rand)]
    yield "carry", 0, "raw", [(x,) for x in raw]
    yield "carry_seq", 0, "raw", [(x,) for x in raw]

    # ---- rr_reduce_q ----
    kmax = min(max(L.ks()), 63)
    rq = [L.exact(j * p + dlt) for j in range(1, kmax + 1) for dlt in (-1, 0, 1)] + [L.exact(0), L.exact(64 * p - 1)]
    magic = (1 << 32) // (L.P[-1] + 1)
    for j in range(1, 65):   # top limbs where the quotient estimate steps from j - 1 to j
        t = -(-(j << 32) // magic)
        for top in (t - 1, t):
            for lows in ([0] * (L.NL - 1), [L.MASK] * (L.NL - 1)):
                if L.val(lows + [top]) < 64 * p:
                    rq.append(lows + [top])
    if L.B <= 29:   # un-carried limbs up to 2^31.4
        rq += [shaped(L, t, pa, LIMB_LAZY) for t in (64 * p - 1, 21 * p, 8 * p) for pa in PATTERNS if pa != "zero"]
        rq += [rand_qn(L, rng, 64 * p - 1, LIMB_LAZY) for _ in range(n_rand)]
    assert all(L.val(x) < 64 * p for x in rq)
    yield "reduce_q", 0, "steps", [(x,) for x in rq]

    # ---- rr_canon_lt2p / rr_to_std / predicates ----
    lt2p = [L.exact(v) for v in (0, p - 1, p, p + 1, 2 * p - 1, p - T, p + T, p - 1 - T)]
    lt2p += [L.P[:-1] + [t] for t in (L.P[-1] - 1, L.P[-1], L.P[-1] + 1, 0)]          # P's own low limbs
    lt2p += [[L.P[0] - 1] + L.P[1:-1] + [t] for t in (L.P[-1], L.P[-1] + 1)]           # borrow through every limb
    lt2p += [L.exact(rng.randrange(2 * p)) for _ in range(n_rand)]
    assert all(L.val(x) < 2 * p and max(x[:-1]) <= L.MASK for x in lt2p)
    yield "canon_lt2p", 0, "edges", [(x,) for x in lt2p]
    yield "is_zero_prod", 0, "edges", [(x,) for x in lt2p]
    yield "maybe_zero_prod", 0, "edges", [(x,) for x in lt2p]
    yield "to_std", 0, "edges", [(x,) for x in lt2p + lazy] + [(rand_qn(L, rng, 64 * p),) for _ in range(n_rand)]
    yield "from_std", 0, "edges", [(words_row(L, v),) for v in [0, 1, p - 1, p // 2, (1 << (p.bit_length() - 1)) - 1] +
                                   [rng.randrange(p) for _ in range(n_rand)]]

    # ---- the NTT's call sites (ntt_pass.hpp), Fr layouts ----
    if L.name in NTT_LAYOUTS:
        yield from ntt_classes(L, rng, n_rand)


def ntt_classes(L, rng, n_rand):
    """Operands the butterflies hand to rr_mul / rr_mul2 / rr_reduce_q /
    rr_carry_seq, built by the butterflies' own add_nc / sub_nc sequence from
    E-form elements (exact limbs, value <= 2.5 r) with every limb at 2^29 - 1,
    against the largest-limbed entry a twiddle table (exact, canonical) holds."""
    r, lim = L.p, L.ntt_limbs()
    emax = [shaped(L, t, "max", L.MASK) for t in (r - 1, 5 * r // 2)]     # E-form, all limbs 2^29 - 1
    prod_max = shaped(L, r + r // 2 - 1, "max", L.MASK)                   # a product output
    zero = L.exact(0)
    tw = [L.MASK] * (L.NL - 1) + [L.P[-1] - 1]                            # largest canonical limbs
    assert L.val(tw) < r
    tws = [tw, L.exact(r - 1), L.exact(L.val([0x1fffffba, 0x22f] + [0] * 7) % r), zero, L.exact(1)] + \
          [L.exact(rng.randrange(r)) for _ in range(n_rand // 4)]
    nc = lambda op, ops, k=0: model(L, op, ops, k)[0]
    site = {}
    for e in emax:
        s_hi, s_lo = nc("add_nc", (e, e)), nc("add_nc", (zero, zero))
        site["d+"] = nc("sub_nc", (e, zero), 8)           # e0 + 8r - e2, e2 = 0
        site["d-"] = nc("sub_nc", (zero, e), 8)
        site["a1+"] = nc("sub_nc", (s_hi, s_lo), 16)      # s0 + 16r - s1, s1 = 0
        site["a1-"] = nc("sub_nc", (s_lo, s_hi), 16)
        site["a0"] = nc("add_nc", (s_hi, s_hi))           # s0 + s1
        site["b1+"] = nc("sub_nc", (prod_max, zero), 4)   # d0 + 4r - d1
        site["b1-"] = nc("sub_nc", (zero, prod_max), 4)
        site["b0"] = nc("add_nc", (prod_max, prod_max))
        site["u-"] = nc("sub_nc", (e, zero), 8)           # the odd last round
        assert max(site["d+"][:-1]) == lim["D"] and max(site["a1+"][:-1]) == lim["A1"] and \
            max(site["a0"][:-1]) == lim["A0"] and max(site["b1+"][:-1]) == lim["B1"]
        for x in site.values():
            assert max(x[:-1]) <= lim["PF"] and L.val(x) <= 21 * r
        ops = list(site.values())
        yield "mul_ntt", 0, "sites", [(x, w) for x in ops for w in tws]
        yield "mul2_ntt", 0, "sites", [(x, w, y, w) for x, y in zip(ops, ops[1:] + ops[:1]) for w in tws[:3]]
        # rr_reduce_q: s0 + s1, the h = 1 difference, rr_store_std's P-form input
        yield "reduce_q", 0, "sites", [(x,) for x in ops]
        yield "carry_seq", 0, "sites", [(site["b0"],), (nc("add_nc", (e, e)),)]
    rnd = [rand_qn(L, rng, 21 * r, lim["PF"]) for _ in range(n_rand)]
    yield "mul_ntt", 0, "random", [(x, rng.choice(tws)) for x in rnd]
    # the first pass's shift product (MUL_IN): canonical input x exact entry, the QN contract
    yield "mul", 0, "mul_in", [(x, w) for x in (emax[0], L.exact(r - 1), zero) for w in tws]


ALL_CASES = [(n, op, k, cname) for n, L in sorted(LAYOUTS.items()) for op, k, cname, _ in classes(L, n_rand=2)]


_ROWS = {}


def rows_of(L, op, k, cname, n_rand=200):
    """the rows of one class, every layout's classes generated once"""
    if (L.name, n_rand) not in _ROWS:
        _ROWS[L.name, n_rand] = {(o, kk, c): rows for o, kk, c, rows in classes(L, n_rand)}
    return _ROWS[L.name, n_rand][op, k, cname]


# ---------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_contracts_hold_at_every_operand_class(name):
    """No accumulator reaches 2^64 (2^63 in a ceil-form chain), no limb leaves
    32 bits, and every output equals the integer reference in its documented
    form -- at every operand class."""
    L = LAYOUTS[name]
    seen = set()
    for op, k, cname, rows in classes(L):
        assert rows, (op, cname)
        seen.add(op)
        for ops in rows:
            try:
                out0, out1, flag = model(L, op, ops, k)
            except Violation as v:
                raise AssertionError(f"{name} {op}<{k}> class {cname}: {v}") from None
            check_output(L, op, ops, k, out0, out1, flag)
    want = {"mul", "mul2", "sqr", "sqr2", "mul_sum2", "add", "sub", "neg", "sub2", "sub3", "neg_wide", "add_nc",
            "sub_nc", "carry", "carry_seq", "reduce_q", "canon_lt2p", "from_std", "to_std", "is_zero_prod",
            "maybe_zero_prod"}
    assert want <= seen, want - seen


def test_layout_facts():
    """What the classes rely on: which layout splits which columns, which uses
    the ceil form, and the NTT's limb bounds from the K p rows."""
    assert {n: split_columns(L) for n, L in LAYOUTS.items() if split_columns(L)} == {"bls12_381_fq13": [10, 11, 12, 13, 14]}
    L13 = LAYOUTS["bls12_381_fq13"]
    assert {k for k in range(25) if L13.split(k, 2)} >= {10, 11, 12, 13, 14} and L13.KPD_OK == 0
    assert [n for n, L in LAYOUTS.items() if L.P[0] == 1] == ["bls12_381_fr"]
    fr = LAYOUTS["bls12_381_fr"]
    assert fr.use_ceil() and not fr.use_ceil(fr.ntt_limbs()["PF"])
    for n in NTT_LAYOUTS:
        lim = LAYOUTS[n].ntt_limbs()
        assert lim["PF"] == lim["A1"] == 2 * ((1 << 29) - 1) + max(LAYOUTS[n].kp(16)[:-1])
        assert 2.4 * 2 ** 30 < lim["PF"] < 2.5 * 2 ** 30 and lim["D"] < 2 ** 31 and lim["B1"] < 2 ** 31


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_mul_sum2_rows_reach_the_two_set_bound(name):
    """rr_mul_sum2's own worst case is in its classes: a row whose four operands
    all have every low limb at the QN maximum (on every product target), and, for
    each column the two-set criterion splits, a row maxed on that column's limbs."""
    L = LAYOUTS[name]
    full = lambda o: all(x == L.QN for x in o[:-1])
    bounds = [rows for op, k, c, rows in classes(L, n_rand=0) if op == "mul_sum2" and c.startswith("bound")]
    assert len(bounds) == len(product_targets(L))
    for rows in bounds:
        assert any(all(full(o) for o in r) for r in rows)
        for k in range(2 * L.NL - 1):
            if L.split(k, 2):
                i0, i1 = (0, k) if k < L.NL else (k - L.NL + 1, min(k, L.NL - 1))
                want = [int(i0 <= i <= i1) * L.QN for i in range(L.NL - 1)]
                assert any(r[0][:-1] == want and r[2][:-1] == want for r in rows), k
    if name == "bls12_381_fq13":
        assert [k for k in range(25) if L.split(k, 2)] == list(range(6, 19))


def test_ceil_form_cannot_take_ntt_operands():
    """The finding behind rr_use_ceil: at the NTT's largest operand classes --
    s0 + 16r - s1 (1.20 x 2^63 in column 7) and s0 + s1 (1.16 x 2^63), both
    P-form outputs and the first also an operand inside the step -- the signed
    ceil-carry chains of BLS12-381 Fr pass 2^63 and then return a value that
    is not a b / R' mod r, while the general form is exact on the same
    operands.  (e0 + 8r - e2 and d0 + 4r - d1 reach 0.96 and 0.98 x 2^63 by
    their own rows; the limb bound the products name does not tell them
    apart, so they run in the general form too.)  Quasi-normalised operands
    (the default contract) stay below 2^63."""
    L = LAYOUTS["bls12_381_fr"]
    r, rinv = L.p, pow(L.RP, -1, L.p)
    e = shaped(L, r - 1, "max", L.MASK)
    tw = [L.MASK] * 8 + [L.P[-1] - 1]
    s0 = model(L, "add_nc", (e, e))[0]
    for a in (model(L, "sub_nc", (s0, L.exact(0)), 16)[0], model(L, "add_nc", (s0, s0))[0]):
        with pytest.raises(Violation):
            m_mul(L, a, tw, force_ceil=True)
        g = m_mul(L, a, tw, force_ceil=False)
        assert L.val(g) == mont(L, L.val(a) * L.val(tw)) and L.val(g) % r == L.val(a) * L.val(tw) * rinv % r
        # the wrapped ceil chain of the device (64-bit z, arithmetic shift) is wrong there
        from test_params_rr import _mont_columns
        c = _mont_columns(a, tw, L.P, L.NL, L.B, L.INV, True)
        assert L.val(c) % r != L.val(a) * L.val(tw) * rinv % r
    # the issue's own operands (limbs 2^31 - 1, value ~ 20 r; b < r with limbs 2^29 - 1)
    a = shaped(L, 20 * r, "max", (1 << 31) - 1)
    with pytest.raises(Violation):
        m_mul(L, a, tw, force_ceil=True)
    assert L.val(m_mul(L, a, tw, amax=(1 << 31) - 1)) == mont(L, L.val(a) * L.val(tw))
    # QN operands at the product bound: the ceil form holds
    for ta, tb in product_targets(L):
        m_mul(L, shaped(L, ta, "max"), shaped(L, tb, "max"), force_ceil=True)


def test_model_matches_the_wrapping_column_loop():
    """The overflow-refusing model and test_params_rr's wrapping loop agree
    wherever nothing overflows (both forms)."""
    from test_params_rr import _mont_columns
    for name in ("bls12_381_fr", "bn254_fr", "bn254_fq9"):
        L = LAYOUTS[name]
        for ta, tb in product_targets(L):
            for a, b in pair_rows(L, random.Random(5), ta, tb, 20):
                assert m_mul(L, a, b) == _mont_columns(a, b, L.P, L.NL, L.B, L.INV, L.use_ceil())
