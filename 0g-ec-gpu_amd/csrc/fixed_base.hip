// Fixed-base batch scalar multiplication on G1: out_i = s_i B
// for n resident scalars and ONE base B -- arkworks' FixedBase::msm.
//   ecg_fixed_base_table    the comb table of B, built once on the device;
//   ecg_fixed_base_mul_dev  one launch: digits, W gathers + mixed additions,
//                           normalisation and the [x, y] records.
//
// Comb over signed windows.  With window c and W = ceil((bits(r) + 1) / c),
//   s = sum_w d_w 2^(c w),  d_w in [-2^(c-1), 2^(c-1) - 1] for w < W - 1 and
//   d_(W-1) in [0, 2^(c-1)] (the top window takes the last carry and is not
//   recoded: s < r < 2^bits(r) leaves its raw digit below 2^(c-1)),
// and the table holds T[w][d] = d 2^(c w) B for d = 1 .. 2^(c-1): affine,
// reduced-radix limbs (the MSM's G1 layouts, curve_rr.hpp RR1of), one 128-B
// line per record as the MSM's prepared bases (msm_impl.hpp BaseLayout), read
// as whole uint4.  s B = sum_w sign(d_w) T[w][|d_w|]: W mixed additions, no
// doubling; the negation is one rr_neg of y at use (pa_neg_y).  r is prime and
// B != O, so no entry is the identity.
//
// Why the sum is safe.  The partial sum before window k is a_k B with
// |a_k| <= 2^(c-1) (2^(c k) - 1) / (2^c - 1) < (2/3) 2^(c k), and the addend is
// t B with 2^(c k) <= |t| <= 2^(c-1) 2^(c k): as integers a_k != +-t.  Below the
// top window c (k + 1) <= bits(r), so |a_k| + |t| < (2/3) 2^bits(r) < r for both
// curves (r / 2^bits(r) = 0.906, 0.756) and a_k != +-t (mod r) either: no partial
// sum meets +- its next addend.  For the top window the same bound on |a_k| + |t|
// is (2/3) 2^(c W), which is above r, and a_k = t - r is not excluded by size
// alone.  So the kernel does not rest on the argument: every addition is the
// complete rr_add_affine (identity accumulator, P = Q, P = -Q), whose
// exceptional branch sits behind a test that waves almost never pass.  A zero
// digit adds nothing: the lane still computes (entry 0 of the row) and a limb
// select keeps its accumulator.
//
// The kernel.  256 threads, one output per thread and tile, FB_TILES tiles per
// workgroup, a tile's accumulator in registers:
//  * the eight scalar words (Montgomery -> canonical on request, then mod r)
//    are a 256-bit shift register: a digit is the low c bits plus the carry,
//    then the words move down by c -- no indexed register reads;
//  * a window's record is gathered right before its addition: the other waves
//    of the SIMD cover the load (an addition is ~5000 mads, a gather from L2
//    well under a tenth of that), and holding the next record across the
//    addition took the 13-limb kernel past 256 registers (84 B of scratch);
//  * normalisation in the same launch: per tile u = ZZ ZZZ (1 for an identity
//    result), a = X ZZZ, b = Y ZZ, exclusive prefix and suffix products of u
//    over the workgroup (six shuffle levels per wave, wave totals through
//    LDS) and (a, b) (before after), so that (x, y) = (a, b) / total; the
//    earlier tiles' pairs wait in LDS.  Then ONE Fermat inversion per
//    workgroup (256 FB_TILES outputs) by wave 0, of the product of the tile
//    totals, and x = a K / total, y = b K / total.  K = R mod p turns the
//    reduced-radix form into the boundary's Montgomery form on the way (one
//    product per workgroup instead of two per output); the table build passes
//    K = 1 and keeps the limbs;
//  * the records leave as consecutive uint4 through an LDS transposition
//    (6 or 4 uint4 per lane, one uint4 of padding per lane); every lane
//    computes everything, only the global store is predicated on index < n.
// Operand classes: the G1 layouts are the tight ones, and every product below
// has operands X <= 1.02 p, Y <= 1.25 p or product outputs (< 1.25 p).
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "ctx.hpp"
#include "host_field.hpp"
#include "norm_group.hpp"  // the scalar load and the workgroup normalisation (shared with batch_mul.hip)

namespace ecg {

constexpr size_t FB_REC_BYTES = 128;     // one table record: [x | y] limbs, padded to a line
constexpr uint32_t FB_MIN_WINDOW = 2, FB_MAX_WINDOW = 16;
// the fastest of c = 8, 12, 16 at n = 2^24 on both curves (profiles/fixed_base/timing.txt)
constexpr uint32_t FB_DEFAULT_WINDOW = 16;

// ---------------------------------------------------------------------------
// the multiplication kernel
// ---------------------------------------------------------------------------
// Next signed digit, low to high: |d| (0 .. 2^(c-1)) and its sign; s moves down by c bits.
ECG_DEV void fb_digit(uint32_t* s, uint32_t c, bool top, uint32_t& carry, uint32_t& mag, bool& neg) {
  const uint32_t d = (s[0] & ((1u << c) - 1)) + carry;
#pragma unroll
  for (int k = 0; k < 7; k++) s[k] = (s[k] >> c) | (s[k + 1] << (32 - c));
  s[7] >>= c;
  neg = !top && d >= (1u << (c - 1));
  carry = neg ? 1u : 0u;
  mag = min(neg ? (1u << c) - d : d, 1u << (c - 1));  // (in range already for s < r: the min guards the gather)
}

// T[w][max(mag, 1)]
template <class Q>
ECG_DEV Affine<FpR<Q>> fb_entry(const char* __restrict__ table, uint32_t w, uint32_t c, uint32_t mag) {
  const size_t idx = ((size_t)w << (c - 1)) + (mag ? mag - 1 : 0);
  return load_affine(reinterpret_cast<const FpR<Q>*>(table + idx * FB_REC_BYTES));
}

// Tiles of 256 outputs per workgroup: the inversion is a serial chain as long
// as ~40 additions, run by one wave, so each workgroup spreads it over FB_TILES
// tiles.  The earlier tiles wait in LDS as (a, b), 2 NL words per thread.
constexpr int FB_TILES = 2;

template <class FrP, class Q>
__global__ void __launch_bounds__(FB_THREADS) __attribute__((amdgpu_waves_per_eu(fb_waves<Q>())))
    fb_mul_kernel(const char* __restrict__ table, const uint4* __restrict__ scalars, size_t n, uint32_t c, uint32_t W,
                  uint32_t mont, uint4* __restrict__ out) {
  using F = FpR<Q>;
  constexpr int NL = Q::NL, T = FB_TILES;
  constexpr int L = Fp<typename Q::Base>::L;  // 32-bit words per boundary coordinate
  constexpr int RV = 2 * L / 4;               // uint4 per output record
  static_assert(2 * L % 4 == 0, "a record is whole uint4");
  __shared__ uint4 stage[FB_THREADS * (RV + 1)];
  __shared__ uint32_t stash[T - 1][2 * NL][FB_THREADS];  // word k of thread t at [k][t]: no bank met twice
  __shared__ uint32_t wtot[FB_WAVES][NL];
  __shared__ uint32_t tot[T][NL], kinv[T][NL];

  F a, b;  // the last tile's pair stays in registers
  uint32_t ids = 0;  // bit t: this thread's output of tile t is the identity
  for (int t = 0; t < T; t++) {
    uint32_t s[8];
    fb_load_scalar<FrP>(scalars, ((size_t)blockIdx.x * T + t) * FB_THREADS + threadIdx.x, n, mont, s);
    uint32_t carry = 0;
    XYZZ<F> acc = xyzz_zero<F>();
    for (uint32_t w = 0; w < W; w++) {
      uint32_t mag;
      bool neg;
      fb_digit(s, c, w + 1 == W, carry, mag, neg);
      const Affine<F> e = fb_entry<Q>(table, w, c, mag);
      Affine<F> g;
      g.x = e.x;
      g.y = rr_pick(neg, pa_neg_y(e.y), e.y);
      const XYZZ<F> r = rr_add_affine(acc, g);
      rr_sel(acc, mag != 0, r);
    }
    bool id;
    fb_norm_tile<Q>(acc, wtot, tot[t], a, b, id);
    ids |= (id ? 1u : 0u) << t;
    if (t < T - 1) {
#pragma unroll
      for (int k = 0; k < NL; k++) {
        stash[t][k][threadIdx.x] = a.v[k];
        stash[t][NL + k][threadIdx.x] = b.v[k];
      }
    }
  }
  __syncthreads();
  fb_norm_invert<true, T, Q>(tot, kinv);
  __syncthreads();

  for (int t = 0; t < T; t++) {
    F at = a, bt = b, x, y;
    if (t < T - 1) {
#pragma unroll
      for (int k = 0; k < NL; k++) {
        at.v[k] = stash[t][k][threadIdx.x];
        bt.v[k] = stash[t][NL + k][threadIdx.x];
      }
    }
    const F ki = fb_limbs<Q>(kinv[t]);
    rr_mul2(at, ki, bt, ki, x, y);
    uint32_t wd[2 * L];
    rr_pack<Q, L>(rr_canon_lt2p(x).v, wd);
    rr_pack<Q, L>(rr_canon_lt2p(y).v, wd + L);
    if (t > 0) __syncthreads();  // the stage is read by the previous tile's stores
#pragma unroll
    for (int j = 0; j < RV; j++)
      stage[(RV + 1) * threadIdx.x + j] = (ids >> t) & 1 ? make_uint4(0, 0, 0, 0)
                                                : make_uint4(wd[4 * j], wd[4 * j + 1], wd[4 * j + 2], wd[4 * j + 3]);
    __syncthreads();
    const size_t base = ((size_t)blockIdx.x * T + t) * FB_THREADS;
#pragma unroll
    for (int q = 0; q < RV; q++) {
      const uint32_t J = q * FB_THREADS + threadIdx.x, owner = J / RV;
      if (base + owner < n) out[base * RV + J] = stage[J + owner];  // (RV + 1) owner + J % RV
    }
  }
}

// ---------------------------------------------------------------------------
// the table build: thread (w, d) computes d head_w, heads = 2^(c w) B from the host
// ---------------------------------------------------------------------------
template <class P, class Q>
__global__ void __launch_bounds__(FB_THREADS)
    fb_table_kernel(const uint64_t* __restrict__ heads, uint32_t c, uint32_t W, char* __restrict__ table) {
  using F = FpR<Q>;
  __shared__ uint32_t wtot[FB_WAVES][Q::NL];
  __shared__ uint32_t tot[1][Q::NL], kinv[1][Q::NL];
  const size_t idx = (size_t)blockIdx.x * FB_THREADS + threadIdx.x;
  const bool live = idx < ((size_t)W << (c - 1));
  const uint32_t w = live ? (uint32_t)(idx >> (c - 1)) : 0u;
  const uint32_t d = live ? ((uint32_t)idx & ((1u << (c - 1)) - 1)) + 1 : 1u;
  Fp<P> hx, hy;
  from_u64_words(hx, heads + (size_t)w * 2 * P::N);
  from_u64_words(hy, heads + (size_t)w * 2 * P::N + P::N);
  Affine<F> h;
  h.x = rr_from_std<Q>(hx);
  h.y = rr_from_std<Q>(hy);
  XYZZ<F> acc = xyzz_zero<F>();
  for (int b = (int)c - 1; b >= 0; b--) {  // d <= 2^(c-1): a uniform trip count, the identity doubles to itself
    acc = rr_dbl(acc);
    const XYZZ<F> r = rr_add_affine(acc, h);
    rr_sel(acc, ((d >> b) & 1) != 0, r);
  }
  F a, b, x, y;
  bool id;
  fb_norm_tile<Q>(acc, wtot, tot[0], a, b, id);
  __syncthreads();
  fb_norm_invert<false, 1, Q>(tot, kinv);
  __syncthreads();
  const F ki = fb_limbs<Q>(kinv[0]);
  rr_mul2(a, ki, b, ki, x, y);
  Affine<F> o;
  o.x = rr_canon_lt2p(x);
  o.y = rr_canon_lt2p(y);
  if (live) store_affine(reinterpret_cast<F*>(table + idx * FB_REC_BYTES), o);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct FbTable {
  int curve;
  uint32_t c;
};
static std::mutex g_fb_mu;
static std::map<const void*, FbTable> g_fb_tables;  // by device address, until ecg_dev_free

void fb_table_forget(const void* p) {
  std::lock_guard<std::mutex> lk(g_fb_mu);
  g_fb_tables.erase(p);
}

static uint32_t fb_scalar_bits(int curve_id) {
  return curve_id == ECG_CURVE_BLS12_381 ? params::bls12_381_fr::BITS : params::bn254_fr::BITS;
}
static uint32_t fb_windows(int curve_id, uint32_t c) { return (fb_scalar_bits(curve_id) + 1 + c - 1) / c; }

// curve and window checks shared by the three entries; c: 0 becomes the default
static int fb_check(const char* what, int curve_id, uint32_t& c) {
  if (curve_id != ECG_CURVE_BLS12_381 && curve_id != ECG_CURVE_BN254) {
    const char* name = ecg_curve_name(curve_id);
    set_error("%s: curve %s (id %d) has no fixed-base kernel (G1 of bls12_381 and bn254 only)", what,
              name ? name : "?", curve_id);
    return ECG_ERR_INVALID;
  }
  if (c == 0) c = FB_DEFAULT_WINDOW;
  if (c < FB_MIN_WINDOW || c > FB_MAX_WINDOW) {
    set_error("%s: window_bits %u outside %u..%u", what, c, FB_MIN_WINDOW, FB_MAX_WINDOW);
    return ECG_ERR_INVALID;
  }
  return ECG_OK;
}

template <class C, class Q>
static int fb_table_t(ecg_ctx* ctx, const uint64_t* base_xy, uint32_t c, uint32_t W, char* d_table, hipStream_t s) {
  using P = typename C::FqParams;
  using H = host::HFp<P>;
  constexpr int N = P::N;
  H x, y, b;
  memcpy(x.v, base_xy ? base_xy : C::Gen::GX, sizeof x.v);
  memcpy(y.v, base_xy ? base_xy + N : C::Gen::GY, sizeof y.v);
  memcpy(b.v, C::Gen::B, sizeof b.v);
  if (x.is_zero() && y.is_zero()) {
    set_error("fixed_base_table: the base is the identity");
    return ECG_ERR_INVALID;
  }
  if (host::geq_p<P>(x.v) || host::geq_p<P>(y.v) ||
      !(host::hmul(y, y) == host::hadd(host::hmul(host::hmul(x, x), x), b))) {
    set_error("fixed_base_table: the base is not a point of the curve");
    return ECG_ERR_INVALID;
  }
  // row heads 2^(c w) B: one doubling chain, each head normalised on the way
  std::vector<uint64_t> heads((size_t)W * 2 * N), jac(3 * N);
  host::HXYZZ<P> p{x, y, H::one(), H::one()};
  for (uint32_t w = 0; w < W; w++) {
    host::hto_jac_norm(p, jac.data());
    memcpy(&heads[(size_t)w * 2 * N], jac.data(), 2 * N * 8);
    for (uint32_t k = 0; k < c && w + 1 < W; k++) p = host::hdbl(p);
  }
  void* d_heads;
  ECG_TRY(ws_get(ctx, "fixed_base_heads", heads.size() * 8, &d_heads));
  ECG_HIP(hipMemcpyAsync(d_heads, heads.data(), heads.size() * 8, hipMemcpyHostToDevice, s));
  const size_t total = (size_t)W << (c - 1);
  ECG_HIP(hipMemsetAsync(d_table, 0, total * FB_REC_BYTES, s));  // the records' padding
  hipLaunchKernelGGL((fb_table_kernel<P, Q>), dim3((uint32_t)((total + FB_THREADS - 1) / FB_THREADS)),
                     dim3(FB_THREADS), 0, s, (const uint64_t*)d_heads, c, W, d_table);
  ECG_HIP(hipGetLastError());
  ECG_HIP(hipStreamSynchronize(s));  // heads is host memory of this call
  return ECG_OK;
}

template <class C>
using FbQ = typename RR1of<typename C::FqParams>::Q;

}  // namespace ecg

using namespace ecg;

extern "C" int ecg_fixed_base_plan_info(int curve_id, uint32_t window_bits, uint32_t* windows, uint32_t* row_entries,
                                        size_t* table_bytes) {
  uint32_t c = window_bits;
  ECG_TRY(fb_check("fixed_base_plan_info", curve_id, c));
  const uint32_t W = fb_windows(curve_id, c);
  if (windows) *windows = W;
  if (row_entries) *row_entries = 1u << (c - 1);
  if (table_bytes) *table_bytes = ((size_t)W << (c - 1)) * FB_REC_BYTES;
  return ECG_OK;
}

extern "C" int ecg_fixed_base_table(ecg_ctx* ctx, int curve_id, const uint64_t* base_xy, uint32_t window_bits,
                                    void** d_table) {
  ECG_ENTER(ctx);
  uint32_t c = window_bits;
  ECG_TRY(fb_check("fixed_base_table", curve_id, c));
  if (!d_table) {
    set_error("fixed_base_table: null pointer");
    return ECG_ERR_INVALID;
  }
  *d_table = nullptr;
  const uint32_t W = fb_windows(curve_id, c);
  const size_t bytes = ((size_t)W << (c - 1)) * FB_REC_BYTES;
  void* t = nullptr;
  if (hipMalloc(&t, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("fixed_base_table: device allocation of %zu bytes failed", bytes);
    return ECG_ERR_NOMEM;
  }
  const int rc = curve_id == ECG_CURVE_BLS12_381
                     ? fb_table_t<BLS12_381, FbQ<BLS12_381>>(ctx, base_xy, c, W, (char*)t, ctx->stream)
                     : fb_table_t<BN254, FbQ<BN254>>(ctx, base_xy, c, W, (char*)t, ctx->stream);
  if (rc != ECG_OK) {
    (void)hipFree(t);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_fb_mu);
    g_fb_tables[t] = FbTable{curve_id, c};
  }
  *d_table = t;
  return ECG_OK;
}

extern "C" int ecg_fixed_base_mul_dev(ecg_ctx* ctx, int curve_id, const void* d_table, uint32_t window_bits,
                                      const void* d_scalars, size_t n, uint32_t flags, void* d_out, void* stream) {
  ECG_ENTER(ctx);
  uint32_t c = window_bits;
  ECG_TRY(fb_check("fixed_base_mul", curve_id, c));
  if (flags & ~(uint32_t)ECG_FB_SCALARS_MONTGOMERY) {
    set_error("fixed_base_mul: unknown flag bits 0x%x", flags);
    return ECG_ERR_INVALID;
  }
  if (n == 0) return ECG_OK;
  if (!d_table || !d_scalars || !d_out) {
    set_error("fixed_base_mul: null pointer");
    return ECG_ERR_INVALID;
  }
  if (n >> 32) {
    set_error("fixed_base_mul: n = %zu is above 2^32", n);
    return ECG_ERR_INVALID;
  }
  {
    std::lock_guard<std::mutex> lk(g_fb_mu);
    const auto it = g_fb_tables.find(d_table);
    if (it == g_fb_tables.end()) {
      set_error("fixed_base_mul: d_table is not a table of ecg_fixed_base_table");
      return ECG_ERR_INVALID;
    }
    if (it->second.curve != curve_id || it->second.c != c) {
      set_error("fixed_base_mul: the table was built for curve %d with window %u, the call names curve %d, window %u",
                it->second.curve, it->second.c, curve_id, c);
      return ECG_ERR_INVALID;
    }
  }
  const uint32_t W = fb_windows(curve_id, c), mont = flags & ECG_FB_SCALARS_MONTGOMERY ? 1u : 0u;
  const size_t per = (size_t)FB_THREADS * FB_TILES;
  const dim3 grid((uint32_t)((n + per - 1) / per)), block(FB_THREADS);
  hipStream_t s = pick_stream(ctx, stream);
  if (curve_id == ECG_CURVE_BLS12_381)
    hipLaunchKernelGGL((fb_mul_kernel<params::bls12_381_fr, FbQ<BLS12_381>>), grid, block, 0, s, (const char*)d_table,
                       (const uint4*)d_scalars, n, c, W, mont, (uint4*)d_out);
  else
    hipLaunchKernelGGL((fb_mul_kernel<params::bn254_fr, FbQ<BN254>>), grid, block, 0, s, (const char*)d_table,
                       (const uint4*)d_scalars, n, c, W, mont, (uint4*)d_out);
  ECG_HIP(hipGetLastError());
  if (!stream) ECG_HIP(hipStreamSynchronize(s));
  return ECG_OK;
}
