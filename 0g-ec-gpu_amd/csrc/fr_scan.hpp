// What the Fr scan kernels share (fr_scan.hip, fr_div_binomial.hip,
// fr_grand_product.hip): the tile geometry, the
// kernel-argument table of uniform multipliers, limb / lane helpers, the tile's
// staging through LDS, the division's wave reduce and block scan, the product
// block scan, and the host side of the R' form.  Operand classes (C, M, Sk, N)
// as in fr_scan.hip's header.
#pragma once
#include <cstring>

#include "ctx.hpp"
#include "fieldrr.hpp"
#include "host_field.hpp"

namespace ecg {

constexpr int FRS_THREADS = 256;                      // threads per tile
constexpr int FRS_E = 8;                              // consecutive elements per thread
constexpr int FRS_LOG_TILE = 11;                      // 2048 elements per tile
constexpr int FRS_TILE = 1 << FRS_LOG_TILE;
constexpr int FRS_WAVES = FRS_THREADS / 64;
constexpr int FRS_SLOTS = 2 * FRS_TILE + 2 * FRS_TILE / 16;  // uint4 slots with the padding
constexpr int FRS_SCAN_THREADS = 1024;                // the scan kernel's one workgroup
constexpr int FRS_SCAN_WAVES = FRS_SCAN_THREADS / 64;
constexpr int FRS_NPOW = 30;                          // z^(2^k), k < 30
constexpr int FRS_MAX_LOG_RUN = FRS_NPOW - 1 - 6 - FRS_LOG_TILE;  // the block scan reads pw[11 + lgR + 6]
static_assert(FRS_THREADS * FRS_E == FRS_TILE && FRS_E == 8, "a thread's run is 16 uint4 slots");

// Kernel-argument table (wave-uniform): pw[k] = z^(2^k) in the R' form (C);
// cst = R' / R (ECG_POLY_OUT_CANONICAL) or K = scale R^2 / R' (inversion).
struct FrsTable {
  uint32_t pw[FRS_NPOW][9];
  uint32_t cst[9];
};

template <class Q>
ECG_DEV FpR<Q> frs_limbs(const uint32_t* p) {
  static_assert(Q::NL == 9, "Fr layouts: 9 limbs");
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = p[i];
  return r;
}
template <class Q>
ECG_DEV void frs_put_limbs(uint32_t* p, const FpR<Q>& a) {
#pragma unroll
  for (int i = 0; i < 9; i++) p[i] = a.v[i];
}
template <class Q>
ECG_DEV FpR<Q> frs_pick(bool c, const FpR<Q>& a, const FpR<Q>& b) {
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}
// the value of lane + d (DOWN) / lane - d (UP); a lane without a partner reads itself
template <bool DOWN, class Q>
ECG_DEV FpR<Q> frs_shift(const FpR<Q>& a, int d) {
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = DOWN ? __shfl_down(a.v[i], d, 64) : __shfl_up(a.v[i], d, 64);
  return r;
}
template <class Q>
ECG_DEV FpR<Q> frs_bcast(const FpR<Q>& a, int lane) {
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = __shfl(a.v[i], lane, 64);
  return r;
}
// lazy value (QN, < 64 p) -> canonical limbs
template <class Q>
ECG_DEV FpR<Q> frs_canon(const FpR<Q>& a) {
  return rr_canon_lt2p(rr_reduce_q(a));
}

// ---------------------------------------------------------------------------
// tile staging: global <-> LDS as consecutive uint4, thread runs out of LDS
// ---------------------------------------------------------------------------
ECG_DEV uint32_t frs_slot(uint32_t j) { return j + (j >> 4); }

ECG_DEV void frs_stage_in(const uint4* src, size_t tile, size_t n, uint4* lds) {
  const size_t base = tile << FRS_LOG_TILE;
#pragma unroll
  for (int q = 0; q < 2 * FRS_E; q++) {
    const uint32_t j = q * FRS_THREADS + threadIdx.x;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (base + (j >> 1) < n) w = src[2 * base + j];
    lds[frs_slot(j)] = w;
  }
}
ECG_DEV void frs_stage_out(uint4* dst, size_t tile, size_t n, const uint4* lds) {
  const size_t base = tile << FRS_LOG_TILE;
#pragma unroll
  for (int q = 0; q < 2 * FRS_E; q++) {
    const uint32_t j = q * FRS_THREADS + threadIdx.x;
    if (base + (j >> 1) < n) dst[2 * base + j] = lds[frs_slot(j)];
  }
}
// element k of this thread's run: C (canonical input); zero = all-zero words
template <class Q>
ECG_DEV FpR<Q> frs_get(const uint4* lds, int k, bool& zero) {
  const uint32_t s = 17 * threadIdx.x + 2 * k;
  const uint4 lo = lds[s], hi = lds[s + 1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  zero = (lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) == 0;
  FpR<Q> r;
  rr_unpack<Q, 8>(w, r.v);
  return r;
}
template <class Q>
ECG_DEV FpR<Q> frs_get(const uint4* lds, int k) {
  bool z;
  return frs_get<Q>(lds, k, z);
}
// canonical limbs -> the thread's own slot k (read by frs_stage_out after a barrier)
template <class Q>
ECG_DEV void frs_put(uint4* lds, int k, const FpR<Q>& c) {
  uint32_t w[8];
  rr_pack<Q, 8>(c.v, w);
  const uint32_t s = 17 * threadIdx.x + 2 * k;
  lds[s] = make_uint4(w[0], w[1], w[2], w[3]);
  lds[s + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// ---------------------------------------------------------------------------
// division: h_left + M^len h_right with uniform multipliers
// ---------------------------------------------------------------------------
// Wave reduce: lane 0 ends with sum_l g_l M^l, M = pw[m0] (a run's length as a
// power of z).  g S4.1 on entry, S13.1 after six levels; every lane computes.
template <class Q>
ECG_DEV FpR<Q> frs_div_wave_reduce(FpR<Q> g, const FrsTable& tab, int m0) {
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const FpR<Q> o = frs_shift<true>(g, 1 << k);
    g = rr_add(g, rr_mul(o, frs_limbs<Q>(tab.pw[m0 + k])));  // S13.1 x C = 13.1 p^2 -> M
  }
  return g;
}

// Block scan: X_i = sum_{j > i} g_j M^(j-i-1) + M^(threads-1-i) carry_in, the
// value that follows thread i's run.  g S2.6, carry_in N.
//  1. wave totals (tree reduce), broadcast and stored by every lane, N;
//  2. this wave's carry c = sum over the later waves (Horner, M^64) + carry_in:
//     N + M = S2.6, a wave-uniform trip count;
//  3. lane 63 takes g + M c (S4.1); every lane computes, a select keeps it;
//  4. inclusive suffix scan, six levels (S13.1); the exclusive value is the
//     next lane's, lane 63 takes c.
template <class Q, int NW>
ECG_DEV FpR<Q> frs_div_block_scan(FpR<Q> g, const FpR<Q>& carry_in, const FrsTable& tab, int m0,
                                  uint32_t (*wagg)[9]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const FpR<Q> tot = rr_reduce_q(frs_bcast(frs_div_wave_reduce(g, tab, m0), 0));
  frs_put_limbs(wagg[wave], tot);
  __syncthreads();
  FpR<Q> c = carry_in;
  for (int u = NW - 1; u > wave; u--)
    c = rr_add(frs_limbs<Q>(wagg[u]), rr_mul(c, frs_limbs<Q>(tab.pw[m0 + 6])));  // N + (N | S2.6) x C
  const FpR<Q> gi = rr_add(g, rr_mul(c, frs_limbs<Q>(tab.pw[m0])));              // S2.6 + S2.6 x C
  g = frs_pick(lane == 63, gi, g);
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const FpR<Q> o = frs_shift<true>(g, 1 << k);
    const FpR<Q> s = rr_add(g, rr_mul(o, frs_limbs<Q>(tab.pw[m0 + k])));  // S13.1 x C -> M
    g = frs_pick(lane + (1 << k) < 64, s, g);
  }
  const FpR<Q> x = frs_shift<true>(g, 1);
  __syncthreads();  // wagg may be written again
  return frs_pick(lane == 63, c, x);
}

// lazy s R (QN, < 64 p) -> the output words: canonical s R, or s (one product by R' / R)
template <class Q, bool CANON>
ECG_DEV FpR<Q> frs_div_out(const FpR<Q>& s, const FrsTable& tab) {
  if constexpr (CANON)
    return rr_canon_lt2p(rr_mul(s, frs_limbs<Q>(tab.cst)));  // S13.1 x C -> M
  else
    return frs_canon(s);
}

// ---------------------------------------------------------------------------
// products: zero read as 1, the exclusive block scan
// ---------------------------------------------------------------------------
// element k of the run with zero read as 1
template <class Q>
ECG_DEV FpR<Q> frs_get_nz(const uint4* lds, int k, bool& zero) {
  const FpR<Q> a = frs_get<Q>(lds, k, zero);
  return frs_pick(zero, FpR<Q>::one(), a);
}

// Exclusive product scan over the block: the product of the g of every earlier
// (UP) / later (DOWN) thread, 1 at the edge.  Wave scan by six levels, wave
// totals through LDS (stored by every lane), then the other waves' totals
// multiplied up with a wave-uniform trip count.
template <class Q, int NW, bool DOWN>
ECG_DEV FpR<Q> frs_mul_block_scan(const FpR<Q>& g, uint32_t (*wtot)[9]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  FpR<Q> v = g;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const FpR<Q> s = rr_mul(v, frs_shift<DOWN>(v, 1 << k));  // M x M
    v = frs_pick(DOWN ? lane + (1 << k) < 64 : lane >= (1 << k), s, v);
  }
  frs_put_limbs(wtot[wave], frs_bcast(v, DOWN ? 0 : 63));
  const FpR<Q> e = frs_shift<DOWN>(v, 1);
  __syncthreads();
  FpR<Q> w = FpR<Q>::one();
  for (int u = DOWN ? wave + 1 : 0; u < (DOWN ? NW : wave); u++) w = rr_mul(w, frs_limbs<Q>(wtot[u]));  // M x M
  const FpR<Q> x = rr_mul(w, e);
  __syncthreads();  // wtot may be written again
  return frs_pick(DOWN ? lane == 63 : lane == 0, w, x);
}

// ---------------------------------------------------------------------------
// host side: the R' form of the uniform multipliers (host_field.hpp), checks
// ---------------------------------------------------------------------------
template <class P, class Q>
static host::HFp<P> frs_from_limbs(const uint32_t* limbs) {  // sum limbs[i] 2^(BITS i), < 2^(64 N)
  host::HFp<P> r = host::HFp<P>::zero();
  for (int i = 0; i < Q::NL; i++) {
    const int bit = Q::BITS * i, w = bit >> 6, s = bit & 63;
    r.v[w] |= (uint64_t)limbs[i] << s;
    if (s + Q::BITS > 64 && w + 1 < P::N) r.v[w + 1] |= (uint64_t)limbs[i] >> (64 - s);
  }
  return r;
}
template <class P, class Q>
static void frs_to_limbs(const host::HFp<P>& x, uint32_t* limbs) {
  for (int i = 0; i < Q::NL; i++) {
    const int bit = Q::BITS * i, w = bit >> 6, s = bit & 63;
    uint64_t v = x.v[w] >> s;
    if (s + Q::BITS > 64 && w + 1 < P::N) v |= x.v[w + 1] << (64 - s);
    limbs[i] = (uint32_t)v & ((1u << Q::BITS) - 1);
  }
}
// x -> x R' / R: a Montgomery word v R becomes v R', the R' form of v (hmul(a, b) = a b / R)
template <class P, class Q>
static void frs_to_rr(const host::HFp<P>& x, uint32_t* limbs) {
  frs_to_limbs<P, Q>(host::hmul(x, frs_from_limbs<P, Q>(Q::ONE)), limbs);
}

template <class P>
static bool frs_below_r(const uint64_t* v) {
  for (int i = P::N - 1; i >= 0; i--)
    if (v[i] != P::P[i]) return v[i] < P::P[i];
  return false;
}

static uint32_t frs_lg_run(size_t ntiles) {  // smallest power-of-two run with which 1024 threads cover the tiles
  uint32_t lg = 0;
  while (((size_t)FRS_SCAN_THREADS << lg) < ntiles) lg++;
  return lg;
}

// shared argument checks; 1 = nothing to do (n == 0)
static int frs_check(const char* what, int field_id, const void* d_in, size_t n) {
  if (field_id != ECG_FIELD_BLS12_381_FR && field_id != ECG_FIELD_BN254_FR) {
    set_error("%s: field_id %d is not a scalar field (bls12_381_fr, bn254_fr)", what, field_id);
    return ECG_ERR_INVALID;
  }
  if (n == 0) return 1;
  if (!d_in) {
    set_error("%s: null pointer", what);
    return ECG_ERR_INVALID;
  }
  static_assert(32 - FRS_LOG_TILE - 10 <= FRS_MAX_LOG_RUN, "2^32 elements: 1024 threads x 2^FRS_MAX_LOG_RUN tiles");
  if (n >> 32) {
    set_error("%s: n = %zu is above 2^32", what, n);
    return ECG_ERR_INVALID;
  }
  return ECG_OK;
}

}  // namespace ecg
