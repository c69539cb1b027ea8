"""The reduced-radix primitives of csrc/fieldrr.hpp on the device, one
function per launch on RAW limbs (ecg_rr_ops), at the operand classes of
tests/test_rr_contracts.py: quasi-normalised limbs at their maximum, lazy
values on the product bound, subtrahends of exactly K p / 2, wide negations,
the split columns of the 13 x 30-bit layout, rr_reduce_q's quotient steps,
long borrow chains, and the NTT's un-carried butterfly operands against the
largest-limbed twiddle.  Every output must EQUAL the exact-integer reference
as an integer (not merely mod p), have the documented limb form, and both
outputs of the paired products must equal the single product's limbs.  No
tolerance anywhere."""
import numpy as np
import pytest

import ecgpu
from test_rr_contracts import ALL_CASES, LAYOUTS, check_output, rows_of

pytestmark = pytest.mark.gpu

OPS = {"mul": ecgpu.RROP_MUL, "mul2": ecgpu.RROP_MUL2, "sqr": ecgpu.RROP_SQR, "sqr2": ecgpu.RROP_SQR2,
       "mul_sum2": ecgpu.RROP_MUL_SUM2, "add": ecgpu.RROP_ADD, "sub": ecgpu.RROP_SUB, "neg": ecgpu.RROP_NEG,
       "sub2": ecgpu.RROP_SUB2, "sub3": ecgpu.RROP_SUB3, "neg_wide": ecgpu.RROP_NEG_WIDE,
       "add_nc": ecgpu.RROP_ADD_NC, "sub_nc": ecgpu.RROP_SUB_NC, "carry": ecgpu.RROP_CARRY,
       "carry_seq": ecgpu.RROP_CARRY_SEQ, "reduce_q": ecgpu.RROP_REDUCE_Q, "canon_lt2p": ecgpu.RROP_CANON_LT2P,
       "from_std": ecgpu.RROP_FROM_STD, "to_std": ecgpu.RROP_TO_STD, "is_zero_prod": ecgpu.RROP_IS_ZERO_PROD,
       "maybe_zero_prod": ecgpu.RROP_MAYBE_ZERO_PROD, "mul_ntt": ecgpu.RROP_MUL_NTT,
       "mul2_ntt": ecgpu.RROP_MUL2_NTT}


@pytest.mark.parametrize("name,op,k,cname", ALL_CASES, ids=["-".join(map(str, c)) for c in ALL_CASES])
def test_rr_op_equals_integers(gpu_programs, name, op, k, cname):
    prog = gpu_programs[0][0]
    L = LAYOUTS[name]
    rows = rows_of(L, op, k, cname)   # the class's edge rows plus seeded random rows inside the class
    assert 1 <= len(rows) <= 4096
    arrs = [np.array([r[j] for r in rows], dtype=np.uint32) for j in range(len(rows[0]))]
    out0, out1, flags = ecgpu.rr_ops(prog, name, OPS[op], *arrs, k=k)
    for i, ops in enumerate(rows):
        check_output(L, op, ops, k, out0[i].tolist(), out1[i].tolist(), int(flags[i]))


def test_rr_ops_covers_every_layout_and_op():
    assert {c[0] for c in ALL_CASES} == set(ecgpu.RR_LAYOUTS) == set(LAYOUTS)
    for name in LAYOUTS:
        ops = {c[1] for c in ALL_CASES if c[0] == name}
        assert ops >= set(OPS) - {"mul_ntt", "mul2_ntt"}, (name, set(OPS) - ops)
        assert (LAYOUTS[name].NL, LAYOUTS[name].B) == ecgpu.RR_LAYOUTS[name][1:]
    assert all({"mul_ntt", "mul2_ntt"} <= {c[1] for c in ALL_CASES if c[0] == n} for n in ("bls12_381_fr", "bn254_fr"))


def test_rr_ops_rejects(gpu_programs):
    prog = gpu_programs[0][0]
    a = np.zeros((4, 9), np.uint32)
    with pytest.raises(ecgpu.EcError, match="layout"):
        ecgpu.rr_ops(prog, 6, ecgpu.RROP_ADD, a, a)                       # bad layout
    with pytest.raises(ecgpu.EcError, match="op"):
        ecgpu.rr_ops(prog, "bn254_fr", 23, a, a)                          # bad op
    with pytest.raises(ecgpu.EcError, match="op"):
        ecgpu.rr_ops(prog, "bn254_fr", -1, a, a)
    with pytest.raises(ecgpu.EcError, match="not representable"):
        ecgpu.rr_ops(prog, "bls12_381_fr", ecgpu.RROP_SUB, a, a, k=32)    # Fr holds rows up to 16 r
    with pytest.raises(ecgpu.EcError, match="not representable"):
        ecgpu.rr_ops(prog, "bn254_fr", ecgpu.RROP_NEG, a, k=3)            # not a power of two
    with pytest.raises(ecgpu.EcError, match="not representable"):
        ecgpu.rr_ops(prog, "bn254_fq", ecgpu.RROP_SUB2, np.zeros((4, 10), np.uint32), np.zeros((4, 10), np.uint32),
                     np.zeros((4, 10), np.uint32), k=4)                   # 10 x 28: deep-borrow rows from 8 p
    with pytest.raises(ecgpu.EcError, match="null"):
        ecgpu.rr_ops(prog, "bn254_fr", ecgpu.RROP_MUL, a)                 # binary op without b
    with pytest.raises(ecgpu.EcError, match="scalar-field"):
        ecgpu.rr_ops(prog, "bn254_fq9", ecgpu.RROP_MUL_NTT, a, a)
    rc = ecgpu.lib().ecg_rr_ops(prog.handle, 0, ecgpu.RROP_MUL2, 0, a.ctypes.data_as(ecgpu._u32p),
                                a.ctypes.data_as(ecgpu._u32p), a.ctypes.data_as(ecgpu._u32p),
                                a.ctypes.data_as(ecgpu._u32p), 4, a.ctypes.data_as(ecgpu._u32p), None, None)
    assert rc == ecgpu.ECG_ERR_INVALID and "null output" in ecgpu.last_error()
