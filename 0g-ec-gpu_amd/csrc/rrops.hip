// One reduced-radix primitive of fieldrr.hpp per launch, on RAW limbs
// (ecg_rr_ops).  ecg_field_ops enters every operand through rr_from_std, so
// it only ever sees product outputs (exact limbs, value < 1.5 p); the
// contracts of fieldrr.hpp are stated for quasi-normalised limbs, lazy values
// of many p, wide negations and un-carried sums, and this entry hands exactly
// such operands to the same inline functions the MSM / NTT kernels call.  No
// arithmetic of its own: tests/test_gpu_rr_ops.py compares the outputs with
// exact integers.
#include <type_traits>

#include "ctx.hpp"
#include "fieldrr.hpp"

namespace ecg {

// fn(integral_constant<int, K>) for the runtime k among the K p rows of OK's set bits
template <uint32_t OK, int J = 0, class Fn>
ECG_DEV void kp_dispatch(int k, Fn&& fn) {
  if constexpr (J < 8) {
    if constexpr ((OK >> J) & 1) {
      if (k == (2 << J)) {
        fn(std::integral_constant<int, (2 << J)>{});
        return;
      }
    }
    kp_dispatch<OK, J + 1>(k, fn);
  }
}

// rows the deep-borrow forms use: rr_sub2 / rr_sub3 fall back to rr_sub<K> of
// the summed subtrahends where BITS > 29 leaves no room for a deep borrow
template <class Q>
constexpr uint32_t rr_deep_ok() {
  return Q::BITS > 29 ? Q::KP_OK : Q::KPD_OK;
}

template <class Q>
constexpr bool rr_is_ntt_field() {  // the layouts ntt_pass.hpp instantiates
  return std::is_same<Q, params::bls12_381_fr_rr>::value || std::is_same<Q, params::bn254_fr_rr>::value;
}

template <class Q>
__global__ void rr_ops_kernel(int op, int k, const FpR<Q>* __restrict__ pa, const FpR<Q>* __restrict__ pb,
                              const FpR<Q>* __restrict__ pc, const FpR<Q>* __restrict__ pd, size_t n,
                              FpR<Q>* __restrict__ out0, FpR<Q>* __restrict__ out1, uint32_t* __restrict__ flags) {
  using F = FpR<Q>;
  using S = Fp<typename Q::Base>;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const F a = load(&pa[i]), b = load(&pb[i]), c = load(&pc[i]), d = load(&pd[i]);
  F r0 = F::zero(), r1 = F::zero();
  uint32_t fl = 0;
  switch (op) {
    case ECG_RROP_MUL: r0 = rr_mul(a, b); break;
    case ECG_RROP_MUL2: rr_mul2(a, b, c, d, r0, r1); break;
    case ECG_RROP_SQR: r0 = rr_sqr(a); break;
    case ECG_RROP_SQR2: rr_sqr2(a, b, r0, r1); break;
    case ECG_RROP_MUL_SUM2: r0 = rr_mul_sum2(a, b, c, d); break;
    case ECG_RROP_ADD: r0 = rr_add(a, b); break;
    case ECG_RROP_SUB: kp_dispatch<Q::KP_OK>(k, [&](auto K) { r0 = rr_sub<decltype(K)::value>(a, b); }); break;
    case ECG_RROP_NEG: kp_dispatch<Q::KP_OK>(k, [&](auto K) { r0 = rr_neg<decltype(K)::value>(a); }); break;
    case ECG_RROP_SUB2:
      kp_dispatch<rr_deep_ok<Q>()>(k, [&](auto K) { r0 = rr_sub2<decltype(K)::value>(a, b, c); });
      break;
    case ECG_RROP_SUB3:
      kp_dispatch<rr_deep_ok<Q>()>(k, [&](auto K) { r0 = rr_sub3<decltype(K)::value>(a, b, c, d); });
      break;
    case ECG_RROP_NEG_WIDE: kp_dispatch<Q::KP_OK>(k, [&](auto K) { r0 = rr_neg_wide<decltype(K)::value>(a); }); break;
    case ECG_RROP_ADD_NC: r0 = rr_add_nc(a, b); break;
    case ECG_RROP_SUB_NC: kp_dispatch<Q::KP_OK>(k, [&](auto K) { r0 = rr_sub_nc<decltype(K)::value>(a, b); }); break;
    case ECG_RROP_CARRY: r0 = rr_carry<Q>(a.v); break;
    case ECG_RROP_CARRY_SEQ: r0 = rr_carry_seq(a); break;
    case ECG_RROP_REDUCE_Q: r0 = rr_reduce_q(a); break;
    case ECG_RROP_CANON_LT2P: r0 = rr_canon_lt2p(a); break;
    case ECG_RROP_FROM_STD: {  // the first L words of the row: x R, canonical
      S x;
#pragma unroll
      for (int j = 0; j < S::L; j++) x.v[j] = a.v[j];
      r0 = rr_from_std<Q>(x);
      break;
    }
    case ECG_RROP_TO_STD: {  // -> the first L words of the row
      const S y = rr_to_std(a);
#pragma unroll
      for (int j = 0; j < S::L; j++) r0.v[j] = y.v[j];
      break;
    }
    case ECG_RROP_IS_ZERO_PROD: fl = rr_is_zero_prod(a); break;
    case ECG_RROP_MAYBE_ZERO_PROD: fl = rr_maybe_zero_prod(a); break;
    case ECG_RROP_MUL_NTT:  // the NTT's products: a with un-carried limbs (NttLimbs<Q>::PF), b an exact twiddle
      if constexpr (rr_is_ntt_field<Q>()) r0 = rr_mul<NttLimbs<Q>::PF>(a, b);
      break;
    case ECG_RROP_MUL2_NTT:
      if constexpr (rr_is_ntt_field<Q>()) rr_mul2<NttLimbs<Q>::PF>(a, b, c, d, r0, r1);
      break;
    default: break;
  }
  store(&out0[i], r0);
  store(&out1[i], r1);
  flags[i] = fl;
}

static int rr_op_operands(int op) {
  switch (op) {
    case ECG_RROP_MUL2: case ECG_RROP_MUL_SUM2: case ECG_RROP_SUB3: case ECG_RROP_MUL2_NTT: return 4;
    case ECG_RROP_SUB2: return 3;
    case ECG_RROP_MUL: case ECG_RROP_SQR2: case ECG_RROP_ADD: case ECG_RROP_SUB: case ECG_RROP_ADD_NC:
    case ECG_RROP_SUB_NC: case ECG_RROP_MUL_NTT: return 2;
    default: return 1;
  }
}

template <class Q>
static int rr_ops_t(ecg_ctx* ctx, int op, int k, const uint32_t* const* in, size_t n, uint32_t* out0, uint32_t* out1,
                    uint32_t* flags, hipStream_t s) {
  using F = FpR<Q>;
  uint32_t ok = 0;  // the K p rows op may name; 0: op takes no K
  switch (op) {
    case ECG_RROP_SUB: case ECG_RROP_NEG: case ECG_RROP_NEG_WIDE: case ECG_RROP_SUB_NC: ok = Q::KP_OK; break;
    case ECG_RROP_SUB2: case ECG_RROP_SUB3: ok = rr_deep_ok<Q>(); break;
    default: break;
  }
  const bool takes_k = op == ECG_RROP_SUB || op == ECG_RROP_NEG || op == ECG_RROP_NEG_WIDE || op == ECG_RROP_SUB_NC ||
                       op == ECG_RROP_SUB2 || op == ECG_RROP_SUB3;
  if (takes_k) {
    int j = -1;
    for (int t = 0; t < 8; t++)
      if (k == (2 << t)) j = t;
    if (j < 0 || !((ok >> j) & 1)) {
      set_error("rr_ops: %d p is not representable for op %d in this layout (rows 0x%x)", k, op, ok);
      return ECG_ERR_INVALID;
    }
  }
  if ((op == ECG_RROP_MUL_NTT || op == ECG_RROP_MUL2_NTT) && !rr_is_ntt_field<Q>()) {
    set_error("rr_ops: the NTT's products exist for the scalar-field layouts only");
    return ECG_ERR_INVALID;
  }
  const size_t bytes = n * sizeof(F);
  void *din[4], *d0, *d1, *dfl;
  static const char* names[4] = {"rrops_a", "rrops_b", "rrops_c", "rrops_d"};
  for (int t = 0; t < 4; t++) {
    if (in[t]) {
      ECG_TRY(ws_get(ctx, names[t], bytes, &din[t]));
      ECG_HIP(hipMemcpyAsync(din[t], in[t], bytes, hipMemcpyHostToDevice, s));
    } else {
      din[t] = din[0];  // an operand op does not take: the kernel loads a again
    }
  }
  ECG_TRY(ws_get(ctx, "rrops_out0", bytes, &d0));
  ECG_TRY(ws_get(ctx, "rrops_out1", bytes, &d1));
  ECG_TRY(ws_get(ctx, "rrops_flags", n * sizeof(uint32_t), &dfl));
  hipLaunchKernelGGL((rr_ops_kernel<Q>), dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, s, op, k, (const F*)din[0],
                     (const F*)din[1], (const F*)din[2], (const F*)din[3], n, (F*)d0, (F*)d1, (uint32_t*)dfl);
  ECG_HIP(hipGetLastError());
  ECG_HIP(hipMemcpyAsync(out0, d0, bytes, hipMemcpyDeviceToHost, s));
  if (out1) ECG_HIP(hipMemcpyAsync(out1, d1, bytes, hipMemcpyDeviceToHost, s));
  if (flags) ECG_HIP(hipMemcpyAsync(flags, dfl, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  ECG_HIP(hipStreamSynchronize(s));
  return ECG_OK;
}

}  // namespace ecg

using namespace ecg;

extern "C" int ecg_rr_ops(ecg_ctx* ctx, int layout, int op, int k, const uint32_t* a, const uint32_t* b,
                          const uint32_t* c, const uint32_t* d, size_t n, uint32_t* out0, uint32_t* out1,
                          uint32_t* flags) {
  ECG_ENTER(ctx);
  if (op < ECG_RROP_MUL || op > ECG_RROP_MUL2_NTT) {
    set_error("rr_ops: unknown op %d", op);
    return ECG_ERR_INVALID;
  }
  const uint32_t* in[4] = {a, b, c, d};
  const int need = rr_op_operands(op);
  for (int t = 0; t < 4; t++) {
    if (t < need && !in[t]) {
      set_error("rr_ops: op %d takes %d operands, operand %d is null", op, need, t);
      return ECG_ERR_INVALID;
    }
    if (t >= need) in[t] = nullptr;
  }
  const bool two = op == ECG_RROP_MUL2 || op == ECG_RROP_SQR2 || op == ECG_RROP_MUL2_NTT;
  const bool pred = op == ECG_RROP_IS_ZERO_PROD || op == ECG_RROP_MAYBE_ZERO_PROD;
  if (!out0 || (two && !out1) || (pred && !flags)) {
    set_error("rr_ops: null output for op %d", op);
    return ECG_ERR_INVALID;
  }
  if (layout < ECG_RR_BLS12_381_FR || layout > ECG_RR_BN254_FQ10) {
    set_error("rr_ops: unknown layout %d", layout);
    return ECG_ERR_INVALID;
  }
  hipStream_t s = ctx->stream;
  switch (layout) {
    case ECG_RR_BLS12_381_FR:
      return n ? rr_ops_t<params::bls12_381_fr_rr>(ctx, op, k, in, n, out0, out1, flags, s) : ECG_OK;
    case ECG_RR_BN254_FR: return n ? rr_ops_t<params::bn254_fr_rr>(ctx, op, k, in, n, out0, out1, flags, s) : ECG_OK;
    case ECG_RR_BLS12_381_FQ13:
      return n ? rr_ops_t<params::bls12_381_fq13_rr>(ctx, op, k, in, n, out0, out1, flags, s) : ECG_OK;
    case ECG_RR_BLS12_381_FQ14:
      return n ? rr_ops_t<params::bls12_381_fq_rr>(ctx, op, k, in, n, out0, out1, flags, s) : ECG_OK;
    case ECG_RR_BN254_FQ9: return n ? rr_ops_t<params::bn254_fq9_rr>(ctx, op, k, in, n, out0, out1, flags, s) : ECG_OK;
    default: return n ? rr_ops_t<params::bn254_fq_rr>(ctx, op, k, in, n, out0, out1, flags, s) : ECG_OK;
  }
}
