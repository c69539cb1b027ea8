// Scans over Fr on device-resident data:
//   ecg_poly_div_linear_dev  p(X) = q(X)(X - z) + p(z): the suffix scan of the
//                            affine maps s -> p_j + z s (Horner from the top);
//   ecg_batch_inverse_dev    out_i = scale / a_i, zeros kept: prefix and suffix
//                            products around ONE field inversion (Montgomery's
//                            trick).
//
// Three launches per call and no waiting between workgroups inside a kernel:
//   reduce  every tile (FRS_TILE consecutive elements, one workgroup) leaves one
//           aggregate in global memory;
//   scan    ONE workgroup scans the aggregates (a power-of-two run per thread,
//           then the block scan below) and leaves each tile its carry-in;
//   apply   every tile recomputes its elements from its carry-in and stores.
//
// Tile.  256 threads x 8 consecutive elements.  Global memory is only touched
// as consecutive uint4: lane l of a load / store takes uint4 l of a 4-KB span.
// The transposition to thread-contiguous runs goes through LDS in the 32-B
// boundary form; slot j of the tile's uint4 image sits at j + j / 16, i.e. one
// uint4 of padding per thread run, so the 16 ds_read_b128 of a thread are
// 272 B apart between lanes and meet no bank twice.  4352 uint4 = 68 KB: two
// workgroups per CU.  The tail tile pads with zero words, which both operators
// read as their identity (a zero coefficient; a zero element enters the
// products as 1).
//
// Arithmetic: the 9 x 29-bit reduced-radix form (fieldrr.hpp), and no
// conversion product at either end.  As in the NTT (ntt_pass.hpp), the
// caller's word x R (< r) is re-read as a 9-limb integer, i.e. as the
// reduced-radix form of x R / R' (R' = 2^261).
//  * The division is linear in p: with z and its powers in the true R' form,
//    rr_mul(z R', s R) = z s R, so every s_j comes out as the integer s_j R --
//    the boundary form once canonical and packed.  ECG_POLY_OUT_CANONICAL is
//    one product by R' / R on the way out.
//  * The inversion is not linear: the products run over the values a_i R / R',
//    so (prod)^-1 carries (R' / R)^k and an output wants a_i^-1 R / R'.  The
//    missing (R / R')^2 goes into the one constant K = scale R^2 / R' that the
//    scan kernel multiplies the inverse by (made on the host, host_field.hpp).
//
// Operand classes.  Every product below is the plain rr_mul / rr_mul2 with two
// QN operands (AMAX = 0); the uniform multipliers z^(2^k) arrive as kernel
// arguments (scalar registers) and are copied to vector registers, 9 v_mov per
// product, so that the ceil-carry column form of BLS12-381 keeps serving them:
// the mad64s forms take the uniform operand second and the modulus digits are
// already there.  Classes named at the call sites:
//   C  canonical: exact limbs, value < p (inputs, table entries, constants);
//   M  product output: exact limbs, value < 1.5 p;
//   Sk carried sum (rr_add: QN) of value < k p.
// The tightest slack is BLS12-381 Fr's: a b <= 2^6 p^2 / 2 = 32 p^2.  Aggregates
// and carries go to memory through rr_reduce_q (< 1.1 p, exact limbs: "N").
// The geometry constants, the table, the limb / lane helpers, the tile staging,
// the division's wave reduce and block scan, the product block scan and the
// host side of the R' form are in fr_scan.hpp, shared with fr_div_binomial.hip
// and fr_grand_product.hip.
#include <cstring>

#include "ctx.hpp"
#include "fieldrr.hpp"
#include "fieldrr_inv.hpp"
#include "fr_scan.hpp"
#include "host_field.hpp"

namespace ecg {

// ---------------------------------------------------------------------------
// division: h_left + M^len h_right with uniform multipliers
// ---------------------------------------------------------------------------
// Horner value of the thread's run, sum_k p_k z^k: S2.5
template <class Q>
ECG_DEV FpR<Q> frs_div_run(const uint4* lds, const FpR<Q>& z) {
  FpR<Q> h = frs_get<Q>(lds, FRS_E - 1);
#pragma unroll
  for (int k = FRS_E - 2; k >= 0; k--) h = rr_add(frs_get<Q>(lds, k), rr_mul(h, z));  // (C | S2.5) x C -> C + M
  return h;
}

template <class Q>
__global__ void __launch_bounds__(FRS_THREADS)
    frs_div_reduce_kernel(const uint4* __restrict__ p, size_t n, FrsTable tab, FpR<Q>* __restrict__ agg) {
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wagg[FRS_WAVES][9];
  frs_stage_in(p, blockIdx.x, n, lds);
  __syncthreads();
  const FpR<Q> h = frs_div_wave_reduce(frs_div_run<Q>(lds, frs_limbs<Q>(tab.pw[0])), tab, 3);
  frs_put_limbs(wagg[threadIdx.x >> 6], rr_reduce_q(frs_bcast(h, 0)));
  __syncthreads();
  if (threadIdx.x == 0) {
    FpR<Q> a = frs_limbs<Q>(wagg[FRS_WAVES - 1]);
    for (int w = FRS_WAVES - 2; w >= 0; w--)
      a = rr_add(frs_limbs<Q>(wagg[w]), rr_mul(a, frs_limbs<Q>(tab.pw[9])));  // N + (N | S2.6) x C
    store(&agg[blockIdx.x], rr_reduce_q(a));
  }
}

// One workgroup: thread i owns the aggregates [i R, (i + 1) R), R = 2^lg_run
// (zero beyond the last tile).  carry[t] = sum_{u > t} A_u (z^T)^(u-t-1), N;
// value = A_0 + z^T carry[0] = p(z) in the output form.
template <class Q>
__global__ void __launch_bounds__(FRS_SCAN_THREADS)
    frs_div_scan_kernel(const FpR<Q>* __restrict__ agg, size_t ntiles, uint32_t lg_run, FrsTable tab,
                        FpR<Q>* __restrict__ carry, uint4* __restrict__ value, uint32_t canonical) {
  __shared__ uint32_t wagg[FRS_SCAN_WAVES][9];
  const size_t i0 = (size_t)threadIdx.x << lg_run;
  const int run = 1 << lg_run;
  const FpR<Q> zt = frs_limbs<Q>(tab.pw[FRS_LOG_TILE]);
  FpR<Q> h = FpR<Q>::zero();
  for (int k = run - 1; k >= 0; k--)
    if (i0 + k < ntiles) h = rr_add(load(&agg[i0 + k]), rr_mul(h, zt));  // N + S2.6 x C
  FpR<Q> c = frs_div_block_scan<Q, FRS_SCAN_WAVES>(h, FpR<Q>::zero(), tab, FRS_LOG_TILE + (int)lg_run, wagg);
  for (int k = run - 1; k >= 0; k--) {
    if (i0 + k >= ntiles) continue;
    store(&carry[i0 + k], rr_reduce_q(c));
    c = rr_add(load(&agg[i0 + k]), rr_mul(c, zt));  // N + (S13.1 | S2.6) x C
  }
  if (threadIdx.x == 0) {
    const FpR<Q> v = canonical ? frs_div_out<Q, true>(c, tab) : frs_div_out<Q, false>(c, tab);
    uint32_t w[8];
    rr_pack<Q, 8>(v.v, w);
    value[0] = make_uint4(w[0], w[1], w[2], w[3]);
    value[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

// p and out may be the same buffer: a tile reads only what it alone writes.
template <class Q, bool CANON>
__global__ void __launch_bounds__(FRS_THREADS)
    frs_div_apply_kernel(const uint4* p, size_t n, FrsTable tab, const FpR<Q>* __restrict__ carry, uint4* out) {
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wagg[FRS_WAVES][9];
  frs_stage_in(p, blockIdx.x, n, lds);
  __syncthreads();
  const FpR<Q> z = frs_limbs<Q>(tab.pw[0]);
  FpR<Q> c = frs_div_block_scan<Q, FRS_WAVES>(frs_div_run<Q>(lds, z), load(&carry[blockIdx.x]), tab, 3, wagg);
#pragma unroll
  for (int k = FRS_E - 1; k >= 0; k--) {
    c = rr_add(frs_get<Q>(lds, k), rr_mul(c, z));  // C + (S13.1 | S2.5) x C = S2.5
    frs_put(lds, k, frs_div_out<Q, CANON>(c, tab));
  }
  __syncthreads();
  frs_stage_out(out, blockIdx.x, n, lds);
}

// ---------------------------------------------------------------------------
// inversion: products (every operand C or M: at most 2.25 p^2 per product)
// ---------------------------------------------------------------------------
template <class Q>
__global__ void __launch_bounds__(FRS_THREADS)
    frs_inv_reduce_kernel(const uint4* __restrict__ a, size_t n, FpR<Q>* __restrict__ agg) {
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wtot[FRS_WAVES][9];
  frs_stage_in(a, blockIdx.x, n, lds);
  __syncthreads();
  bool zf;
  FpR<Q> g = frs_get_nz<Q>(lds, 0, zf);
#pragma unroll
  for (int k = 1; k < FRS_E; k++) g = rr_mul(g, frs_get_nz<Q>(lds, k, zf));  // (C | M) x C
#pragma unroll
  for (int k = 0; k < 6; k++) g = rr_mul(g, frs_shift<true>(g, 1 << k));  // M x M; lane 0 ends with the wave's product
  frs_put_limbs(wtot[threadIdx.x >> 6], frs_bcast(g, 0));
  __syncthreads();
  if (threadIdx.x == 0) {
    FpR<Q> t = frs_limbs<Q>(wtot[0]);
    for (int w = 1; w < FRS_WAVES; w++) t = rr_mul(t, frs_limbs<Q>(wtot[w]));
    store(&agg[blockIdx.x], t);
  }
}

// One workgroup: thread i owns the aggregates [i R, (i + 1) R) (1 beyond the
// last tile).  pfx[t] = product of the tiles before t; inv[t] = K / (product
// through the end of tile t), K = tab.cst; ONE rr_inv_fermat, by wave 0.
template <class Q>
__global__ void __launch_bounds__(FRS_SCAN_THREADS)
    frs_inv_scan_kernel(const FpR<Q>* __restrict__ agg, size_t ntiles, uint32_t lg_run, FrsTable tab,
                        FpR<Q>* __restrict__ pfx, FpR<Q>* __restrict__ inv) {
  __shared__ uint32_t wtot[FRS_SCAN_WAVES][9];
  __shared__ uint32_t kinv[9];
  const size_t i0 = (size_t)threadIdx.x << lg_run;
  const int run = 1 << lg_run;
  FpR<Q> g = FpR<Q>::one();
  for (int k = 0; k < run; k++)
    if (i0 + k < ntiles) g = rr_mul(g, load(&agg[i0 + k]));  // M x M
  FpR<Q> pre = frs_mul_block_scan<Q, FRS_SCAN_WAVES, false>(g, wtot);
  FpR<Q> suf = frs_mul_block_scan<Q, FRS_SCAN_WAVES, true>(g, wtot);
  if (threadIdx.x < 64) {  // wave 0, thread 0's values on every lane: total = g_0 * (what follows thread 0)
    const FpR<Q> total = rr_mul(frs_bcast(g, 0), frs_bcast(suf, 0));
    frs_put_limbs(kinv, rr_mul(rr_inv_fermat(total), frs_limbs<Q>(tab.cst)));  // M x C
  }
  __syncthreads();
  suf = rr_mul(suf, frs_limbs<Q>(kinv));  // K / (product through the end of this thread's run)
  for (int k = 0; k < run; k++) {
    if (i0 + k >= ntiles) break;
    store(&pfx[i0 + k], pre);
    pre = rr_mul(pre, load(&agg[i0 + k]));
  }
  for (int k = run - 1; k >= 0; k--) {
    if (i0 + k >= ntiles) continue;
    store(&inv[i0 + k], suf);
    suf = rr_mul(suf, load(&agg[i0 + k]));
  }
}

// a and out may be the same buffer.  Per run: the prefixes pre_e = a_0 .. a_(e-1)
// stay in registers; K_i = pfx_t (threads before) x inv_t (threads after) =
// K / g_i; the backward sweep pairs out_e = acc pre_e with acc = acc a_e.
template <class Q>
__global__ void __launch_bounds__(FRS_THREADS)
    frs_inv_apply_kernel(const uint4* a, size_t n, const FpR<Q>* __restrict__ pfx, const FpR<Q>* __restrict__ inv,
                         uint4* out) {
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wtot[FRS_WAVES][9];
  frs_stage_in(a, blockIdx.x, n, lds);
  __syncthreads();
  bool zf;
  FpR<Q> pre[FRS_E];  // pre[e], e >= 1; pre[0] = 1 is never multiplied
  pre[1] = frs_get_nz<Q>(lds, 0, zf);
#pragma unroll
  for (int e = 2; e < FRS_E; e++) pre[e] = rr_mul(pre[e - 1], frs_get_nz<Q>(lds, e - 1, zf));  // (C | M) x C
  const FpR<Q> g = rr_mul(pre[FRS_E - 1], frs_get_nz<Q>(lds, FRS_E - 1, zf));
  const FpR<Q> before = frs_mul_block_scan<Q, FRS_WAVES, false>(g, wtot);
  const FpR<Q> after = frs_mul_block_scan<Q, FRS_WAVES, true>(g, wtot);
  FpR<Q> x, y;
  rr_mul2(before, load(&pfx[blockIdx.x]), after, load(&inv[blockIdx.x]), x, y);  // M x M twice
  FpR<Q> acc = rr_mul(x, y);
#pragma unroll
  for (int e = FRS_E - 1; e >= 1; e--) {
    const FpR<Q> ae = frs_get_nz<Q>(lds, e, zf);
    FpR<Q> o, next;
    rr_mul2(acc, pre[e], acc, ae, o, next);  // M x M, M x C
    acc = next;
    frs_put(lds, e, frs_pick(zf, FpR<Q>::zero(), rr_canon_lt2p(o)));
  }
  frs_get<Q>(lds, 0, zf);
  frs_put(lds, 0, frs_pick(zf, FpR<Q>::zero(), rr_canon_lt2p(acc)));
  __syncthreads();
  frs_stage_out(out, blockIdx.x, n, lds);
}


// ---------------------------------------------------------------------------
// host side: the uniform table (fr_scan.hpp, host_field.hpp), workspace, launches
// ---------------------------------------------------------------------------
template <class P, class Q>
static int frs_div_t(ecg_ctx* ctx, const void* d_coeffs, size_t n, const uint64_t* z, void* d_out,
                     uint64_t* value_out, bool canonical, hipStream_t s) {
  using F = FpR<Q>;
  using H = host::HFp<P>;
  if (!frs_below_r<P>(z)) {
    set_error("poly_div_linear: z is not a reduced field element (>= r)");
    return ECG_ERR_INVALID;
  }
  FrsTable tab;
  H zp, one = H::zero();
  memcpy(zp.v, z, sizeof(zp.v));
  for (int k = 0; k < FRS_NPOW; k++) {  // z^(2^k) R by squaring, each to the R' form
    frs_to_rr<P, Q>(zp, tab.pw[k]);
    zp = host::hmul(zp, zp);
  }
  one.v[0] = 1;
  frs_to_rr<P, Q>(one, tab.cst);  // R' / R

  const size_t ntiles = (n + FRS_TILE - 1) >> FRS_LOG_TILE;
  const uint32_t lg_run = frs_lg_run(ntiles);
  const bool eval_only = d_out == nullptr;
  void *agg, *carry, *val;
  ECG_TRY(ws_get(ctx, "fr_scan_agg", ntiles * sizeof(F), &agg));
  ECG_TRY(ws_get(ctx, "fr_scan_carry", ntiles * sizeof(F), &carry));
  ECG_TRY(ws_get(ctx, "fr_scan_value", 32, &val));
  hipLaunchKernelGGL(frs_div_reduce_kernel<Q>, dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s, (const uint4*)d_coeffs,
                     n, tab, (F*)agg);
  hipLaunchKernelGGL(frs_div_scan_kernel<Q>, dim3(1), dim3(FRS_SCAN_THREADS), 0, s, (const F*)agg, ntiles, lg_run, tab,
                     (F*)carry, (uint4*)val, (uint32_t)(canonical && !eval_only));
  if (!eval_only) {
    if (canonical)
      hipLaunchKernelGGL((frs_div_apply_kernel<Q, true>), dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s,
                         (const uint4*)d_coeffs, n, tab, (const F*)carry, (uint4*)d_out);
    else
      hipLaunchKernelGGL((frs_div_apply_kernel<Q, false>), dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s,
                         (const uint4*)d_coeffs, n, tab, (const F*)carry, (uint4*)d_out);
  }
  ECG_HIP(hipGetLastError());
  if (value_out) {
    void* h;
    ECG_TRY(hws_get(ctx, "fr_scan_value_h", 32, &h));
    ECG_HIP(hipMemcpyAsync(h, val, 32, hipMemcpyDeviceToHost, s));
    ECG_HIP(hipStreamSynchronize(s));
    memcpy(value_out, h, 32);
  }
  return ECG_OK;
}

template <class P, class Q>
static int frs_inv_t(ecg_ctx* ctx, const void* d_in, void* d_out, size_t n, const uint64_t* scale, hipStream_t s) {
  using F = FpR<Q>;
  using H = host::HFp<P>;
  if (scale && !frs_below_r<P>(scale)) {
    set_error("batch_inverse: scale is not a reduced field element (>= r)");
    return ECG_ERR_INVALID;
  }
  // K = scale R^2 / R' as plain limbs.  hinv reads R' mod r as (R' / R) R and
  // returns (R / R') R = R^2 / R'; hmul(scale R, R^2 / R') = scale R^2 / R'.
  FrsTable tab;
  memset(&tab, 0, sizeof(tab));
  H sc;
  memcpy(sc.v, scale ? scale : P::ONE, sizeof(sc.v));
  frs_to_limbs<P, Q>(host::hmul(sc, host::hinv(frs_from_limbs<P, Q>(Q::ONE))), tab.cst);

  const size_t ntiles = (n + FRS_TILE - 1) >> FRS_LOG_TILE;
  void *agg, *pfx, *inv;
  ECG_TRY(ws_get(ctx, "fr_scan_agg", ntiles * sizeof(F), &agg));
  ECG_TRY(ws_get(ctx, "fr_scan_pfx", ntiles * sizeof(F), &pfx));
  ECG_TRY(ws_get(ctx, "fr_scan_inv", ntiles * sizeof(F), &inv));
  hipLaunchKernelGGL(frs_inv_reduce_kernel<Q>, dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s, (const uint4*)d_in, n,
                     (F*)agg);
  hipLaunchKernelGGL(frs_inv_scan_kernel<Q>, dim3(1), dim3(FRS_SCAN_THREADS), 0, s, (const F*)agg, ntiles,
                     frs_lg_run(ntiles), tab, (F*)pfx, (F*)inv);
  hipLaunchKernelGGL(frs_inv_apply_kernel<Q>, dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s, (const uint4*)d_in, n,
                     (const F*)pfx, (const F*)inv, (uint4*)d_out);
  ECG_HIP(hipGetLastError());
  return ECG_OK;
}

}  // namespace ecg

using namespace ecg;

extern "C" size_t ecg_fr_scan_tile(void) { return FRS_TILE; }

extern "C" int ecg_poly_div_linear_dev(ecg_ctx* ctx, int field_id, const void* d_coeffs, size_t n, const uint64_t* z,
                                       void* d_out, uint64_t* value_out, uint32_t flags, void* stream) {
  ECG_ENTER(ctx);
  if (flags & ~(uint32_t)ECG_POLY_OUT_CANONICAL) {
    set_error("poly_div_linear: unknown flag bits 0x%x", flags);
    return ECG_ERR_INVALID;
  }
  const int rc = frs_check("poly_div_linear", field_id, d_coeffs, n);
  if (rc != ECG_OK) return rc < 0 ? rc : ECG_OK;
  if (!z) {
    set_error("poly_div_linear: null pointer");
    return ECG_ERR_INVALID;
  }
  const char *a = (const char*)d_coeffs, *b = (const char*)d_out;
  if (b && b != a && b < a + n * 32 && a < b + n * 32) {
    set_error("poly_div_linear: d_out overlaps d_coeffs (in place, d_out == d_coeffs, is allowed)");
    return ECG_ERR_INVALID;
  }
  const bool canonical = flags & ECG_POLY_OUT_CANONICAL;
  hipStream_t s = pick_stream(ctx, stream);
  return field_id == ECG_FIELD_BLS12_381_FR
             ? frs_div_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, d_coeffs, n, z, d_out, value_out,
                                                                        canonical, s)
             : frs_div_t<params::bn254_fr, params::bn254_fr_rr>(ctx, d_coeffs, n, z, d_out, value_out, canonical, s);
}

extern "C" int ecg_batch_inverse_dev(ecg_ctx* ctx, int field_id, const void* d_in, void* d_out, size_t n,
                                     const uint64_t* scale, void* stream) {
  ECG_ENTER(ctx);
  const int rc = frs_check("batch_inverse", field_id, d_in, n);
  if (rc != ECG_OK) return rc < 0 ? rc : ECG_OK;
  const char *a = (const char*)d_in, *b = (const char*)d_out;
  if (!b || (b != a && b < a + n * 32 && a < b + n * 32)) {
    set_error(b ? "batch_inverse: d_out overlaps d_in (in place, d_out == d_in, is allowed)"
                : "batch_inverse: null pointer");
    return ECG_ERR_INVALID;
  }
  hipStream_t s = pick_stream(ctx, stream);
  return field_id == ECG_FIELD_BLS12_381_FR
             ? frs_inv_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, d_in, d_out, n, scale, s)
             : frs_inv_t<params::bn254_fr, params::bn254_fr_rr>(ctx, d_in, d_out, n, scale, s);
}
