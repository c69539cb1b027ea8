// Multilinear Fr on the device: evaluation tables on {0,1}^v,
// little-endian index i = sum x_j 2^j, arkworks' pairing of the entries 2b and
// 2b + 1 (the lowest variable goes first).
//   ecg_fr_sumcheck_round_dev   the round polynomial of a sum of products of
//                               tables, optionally fused with the bind of the
//                               previous round's challenge;
//   ecg_fr_mle_fix_dev          bind x_0 .. x_(m-1), up to the full evaluation;
//   ecg_fr_eq_table_dev         the eq(r, .) table.
//
// ---- the round kernel ------------------------------------------------------
// Tile.  SC_TILE = 512 consecutive elements per 256-thread workgroup: a lane
// owns one PAIR (lo, hi) = (col[2b], col[2b + 1]), a wave a 4-KB span of every
// column.  Global memory is only touched as consecutive uint4: lane l takes the
// uint4 l, 64 + l, 128 + l, 192 + l of the span and writes uint4 u to plane
// u & 3 (lo words 0-3, lo words 4-7, hi words 0-3, hi words 4-7), index u >> 2,
// of the wave's region, so a lane then reads its pair as four ds_read_b128 at
// unit stride.  Regions are wave-private, 16 KB per column and workgroup.
//   The columns keep their regions for the whole tile (dynamic LDS, k x 16 KB),
// as fr_vec.hip's vectors do, and NOT one image in turn as the grand product's:
// the products name their factors by run-time index, and a column set held in
// registers (8 x 18 limbs) could only be indexed through scratch.  Out of LDS a
// factor is four reads per use and the registers hold one product's chain.
//   Fold.  With fold_r a lane owns a QUAD of input elements (tile: 1024).  The
// columns go one at a time through the column's region (elements 0, 1 of the
// quad) and ONE extra 16-KB image (elements 2, 3): bind, canonical words back
// into the lane's own four slots -- now the pair layout above -- and the folded
// span leaves as consecutive uint4.  (k + 1) x 16 KB in all.
//   Grid.  Persistent, as fr_vec.hip: occupancy query x compute units, block b
// walks tiles b, b + G, ...  ECG_SC_GRID=<blocks> overrides G.
//
// Arithmetic: fieldrr.hpp's 9 x 29-bit form.  A word x R is re-read as limbs;
// rr_mul(a, b) = a b / R'.  Per pair and product of f factors, evaluated at
// t = 0 .. d (d = the largest f of the call):
//   step   hi - lo + 4 p, rr_reduce_q                          no product
//   v(0) = lo, v(1) = hi, v(t + 1) = v(t) + step (rr_add)      no product
//   chain  ((v_0(t) v_1(t)) v_2(t)) v_3(t)                     (f - 1)(d + 1)
//   c_p    K_p = c_p R'^f / R^(f-1) into lo and hi of factor 0  2
// so the chain's value is c_p prod x_j R, the word of the term.  When every
// product of the call has the same K (one product; equal counts and
// coefficients) the 2 are not spent: K goes into the fold launch, one product
// per t and call.  The fold's own bind is one product per folded element:
// (e1 - e0 + 4 p) x (r R').
//
// Operand classes (C canonical < p; M product output, exact limbs, < 1.5 p;
// N rr_reduce_q output < 1.1 p; Sk carried sum, QN, < k p):
//   lo, hi        C, or M after the coefficient;
//   step          (C | M) - (C | M) + 4 p < 5.5 p -> N;
//   v(t), t >= 2  hi + (t - 1) step: S4.3 from C, S4.8 from M (t = 4);
//   chain         first product S4.8 x S4.3 = 20.7 p^2, the widest, against the
//                 32 p^2 of BLS12-381 Fr; then M x S4.3;
//   bind          S5.1 x C -> M, lo + M = S2.6 -> N -> canonical.
// Totals: d + 1 carried sums per lane (rr_add: limbs stay QN).  A term is at
// most S4.8 (a one-factor product is its v(t)); rr_reduce_q after every
// `period` = max(1, 12 / n_products) tiles keeps a total below
// 1.1 p + 12 x 4.8 p = 58.7 p < 64 p.  Then six shuffle levels (N + N -> N),
// the four wave totals through LDS, one 48-B partial per workgroup and t in the
// workspace, and a one-workgroup launch that folds them and multiplies by the
// call's constant.  Pairs beyond the table read zero words: their terms are
// multiples of p, which the sums carry like any other value.
//
// ---- bind ------------------------------------------------------------------
// fr_scan.hpp's tile (2048 elements, a thread's run of 8 out of the LDS image).
// One launch binds up to 11 variables: three inside the run in registers
// (4 + 2 + 1 products), six by lane exchange (shuffle-xor; both lanes of a pair
// compute, every lane of a group holds the group's value), two through LDS
// across the four waves.  Level s takes its own challenge r_s R' from the kernel
// argument; the kernel stops after `levels` and writes what it holds, canonical
// words, through the image as consecutive uint4.  Later launches run on the
// workspace: 2^24 -> 2^13 -> 2^2 -> 1.  Every level is
//   lo + (hi - lo + 4 p) x (r R'):  (C | N) + S5.1 x C = S2.6 -> N.
//
// ---- eq --------------------------------------------------------------------
// i = lo + 2^h hi, h = ceil(log_n / 2): two factor tables of at most 2^16
// entries made on the host (one product per entry, host_field.hpp), the low one
// as words a R, the high one as b s R' (scale and the canonical exit folded in),
// so an output is ONE product C x C -> M -> canonical, staged out as in fr_vec.hip.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "fieldrr.hpp"
#include "fr_scan.hpp"
#include "host_field.hpp"

namespace ecg {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_TILE = 2 * SC_THREADS;                   // input elements per tile: a pair per lane
constexpr int SC_WAVE_SLOTS = 256;                        // uint4 per wave and column: four planes of 64
constexpr int SC_COL_SLOTS = SC_WAVES * SC_WAVE_SLOTS;    // 1024 uint4
constexpr size_t SC_COL_LDS = SC_COL_SLOTS * sizeof(uint4);  // 16 KB
constexpr int SC_FOLD_THREADS = 1024;
constexpr int SC_FOLD_WAVES = SC_FOLD_THREADS / 64;
constexpr uint32_t SC_MAX_GRID = 1u << 20;
constexpr int SC_TERM_BUDGET = 12;                        // terms (< 4.8 p each) between two rr_reduce_q
constexpr int MF_MAX_LEVELS = FRS_LOG_TILE;               // 3 in the run + 6 in the wave + 2 across waves
constexpr int EQ_TILE = 256;
static_assert(MF_MAX_LEVELS == 11 && FRS_WAVES == 4, "the bind kernel's level plan");

// Kernel argument of the round kernel (wave-uniform).  Limbs canonical (C).
struct ScArgs {
  const uint4* col[ECG_SC_MAX_COLS];
  uint4* folded[ECG_SC_MAX_COLS];
  uint32_t kcoef[ECG_SC_MAX_PRODUCTS][9];  // K_p = c_p R'^f / R^(f-1)
  uint32_t rk[9];                          // fold_r R'
  uint8_t nf[ECG_SC_MAX_PRODUCTS];
  uint8_t fc[ECG_SC_MAX_PRODUCTS][ECG_SC_MAX_FACTORS];
  uint32_t k, np, prescale, period;
};
// Indexed by wave-uniform run-time values (product, column): read through the
// kernel-argument segment itself (first parameter, offset 0), as FrvArgs is.
typedef const ScArgs __attribute__((address_space(4))) * ScArgsK;
struct ScFin {
  uint32_t fin[9];  // the fold launch's constant (C)
};

template <class Q, class PT>
ECG_DEV FpR<Q> ml_limbs(PT p) {
  static_assert(Q::NL == 9, "Fr layouts: 9 limbs");
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = p[i];
  return r;
}
template <class Q>
ECG_DEV FpR<Q> ml_xor(const FpR<Q>& a, int d) {
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = __shfl_xor(a.v[i], d, 64);
  return r;
}
template <class Q>
ECG_DEV FpR<Q> ml_unpack(const uint4& lo, const uint4& hi) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  FpR<Q> r;
  rr_unpack<Q, 8>(w, r.v);
  return r;
}
template <class Q>
ECG_DEV void ml_pack(const FpR<Q>& c, uint4& lo, uint4& hi) {
  uint32_t w[8];
  rr_pack<Q, 8>(c.v, w);
  lo = make_uint4(w[0], w[1], w[2], w[3]);
  hi = make_uint4(w[4], w[5], w[6], w[7]);
}
template <class Q>
ECG_DEV FpR<Q> ml_add_n(const FpR<Q>& a, const FpR<Q>& b) {  // N + N -> N
  return rr_reduce_q(rr_add(a, b));
}
// lo + (hi - lo) r for rk = r R':  (C | N) + S5.1 x C = S2.6 -> N
template <class Q>
ECG_DEV FpR<Q> ml_bind(const FpR<Q>& lo, const FpR<Q>& hi, const FpR<Q>& rk) {
  return rr_reduce_q(rr_add(lo, rr_mul(rr_sub<4>(hi, lo), rk)));
}
template <class Q>
ECG_DEV void ml_bind2(const FpR<Q>& lo0, const FpR<Q>& hi0, const FpR<Q>& lo1, const FpR<Q>& hi1, const FpR<Q>& rk,
                      FpR<Q>& o0, FpR<Q>& o1) {
  FpR<Q> m0, m1;
  rr_mul2(rr_sub<4>(hi0, lo0), rk, rr_sub<4>(hi1, lo1), rk, m0, m1);
  o0 = rr_reduce_q(rr_add(lo0, m0));
  o1 = rr_reduce_q(rr_add(lo1, m1));
}

// ---------------------------------------------------------------------------
// the round kernel
// ---------------------------------------------------------------------------
// the element whose two uint4 sit at s and s + 64: C
template <class Q>
ECG_DEV FpR<Q> sc_get(const uint4* lds, uint32_t s) {
  return ml_unpack<Q>(lds[s], lds[s + 64]);
}

// D = the degree of the round polynomial; n_in = the columns' length.
template <class Q, int D, bool FOLD>
__global__ void __launch_bounds__(SC_THREADS)
    sc_kernel(ScArgs args_by_value, size_t n_in, size_t ntiles, uint4* partial) {
  const ScArgsK args = (ScArgsK)__builtin_amdgcn_kernarg_segment_ptr();
  extern __shared__ uint4 lds[];
  __shared__ uint32_t wtot[SC_WAVES][9];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t wbase = wave * SC_WAVE_SLOTS;
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  const uint32_t k = args->k;

  FpR<Q> tot[D + 1];
#pragma unroll
  for (int t = 0; t <= D; t++) tot[t] = FpR<Q>::zero();
  uint32_t since = 0;

  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    if constexpr (FOLD) {
      // ---- a quad per lane: bind every column, store it, keep the pair ----
      const size_t ein = tile * (2 * SC_TILE) + wave * 256, eout = tile * SC_TILE + wave * 128;
      const size_t n_out = n_in >> 1;
      const uint32_t xbase = k * SC_COL_SLOTS + wbase;
      const FpR<Q> rk = ml_limbs<Q>(args->rk);
      for (uint32_t c = 0; c < k; c++) {
        const uint4* src = args->col[c];
        const uint32_t cbase = c * SC_COL_SLOTS + wbase;
        uint4 q[8];
#pragma unroll
        for (int h = 0; h < 8; h++) {
          const uint32_t u = lane + 64 * h;
          q[h] = zero4;
          if (ein + (u >> 1) < n_in) q[h] = src[2 * ein + u];
        }
#pragma unroll
        for (int h = 0; h < 8; h++) {
          const uint32_t u = lane + 64 * h;
          lds[((u & 4) ? xbase : cbase) + (u & 3) * 64 + (u >> 3)] = q[h];
        }
        __syncthreads();
        FpR<Q> f0, f1;
        ml_bind2(sc_get<Q>(lds, cbase + lane), sc_get<Q>(lds, cbase + 128 + lane), sc_get<Q>(lds, xbase + lane),
                 sc_get<Q>(lds, xbase + 128 + lane), rk, f0, f1);
        uint4 a0, a1, b0, b1;
        ml_pack(rr_canon_lt2p(f0), a0, a1);
        ml_pack(rr_canon_lt2p(f1), b0, b1);
        lds[cbase + lane] = a0, lds[cbase + 64 + lane] = a1;  // the lane's own slots
        lds[cbase + 128 + lane] = b0, lds[cbase + 192 + lane] = b1;
        __syncthreads();  // the extra image is free again; the folded span is complete
        uint4* dst = args->folded[c];
#pragma unroll
        for (int h = 0; h < 4; h++) {
          const uint32_t u = lane + 64 * h;
          if (eout + (u >> 1) < n_out) dst[2 * eout + u] = lds[cbase + (u & 3) * 64 + (u >> 2)];
        }
      }
    } else {
      // ---- stage in: consecutive uint4 of every column ----
      const size_t e0 = tile * SC_TILE + wave * 128;  // the wave's first element
      for (uint32_t c = 0; c < k; c++) {
        const uint4* src = args->col[c];
        uint4 q[4];
#pragma unroll
        for (int h = 0; h < 4; h++) {
          const uint32_t u = lane + 64 * h;
          q[h] = zero4;
          if (e0 + (u >> 1) < n_in) q[h] = src[2 * e0 + u];
        }
#pragma unroll
        for (int h = 0; h < 4; h++) {
          const uint32_t u = lane + 64 * h;
          lds[c * SC_COL_SLOTS + wbase + (u & 3) * 64 + (u >> 2)] = q[h];
        }
      }
      __syncthreads();
    }

    // ---- the products at t = 0 .. D ----
    for (uint32_t p = 0; p < args->np; p++) {
      FpR<Q> acc[D + 1];
#pragma unroll
      for (int t = 0; t <= D; t++) acc[t] = FpR<Q>::zero();
      const uint32_t nf = args->nf[p];
      for (uint32_t j = 0; j < nf; j++) {
        const uint32_t s = (uint32_t)args->fc[p][j] * SC_COL_SLOTS + wbase + lane;
        FpR<Q> lo = sc_get<Q>(lds, s), hi = sc_get<Q>(lds, s + 128);  // C
        if (j == 0 && args->prescale) {
          const FpR<Q> kk = ml_limbs<Q>(args->kcoef[p]);
          FpR<Q> l2, h2;
          rr_mul2(lo, kk, hi, kk, l2, h2);  // C x C -> M
          lo = l2, hi = h2;
        }
        const FpR<Q> step = rr_reduce_q(rr_sub<4>(hi, lo));  // < 5.5 p -> N
        FpR<Q> x[D + 1];
        x[0] = lo, x[1] = hi;
#pragma unroll
        for (int t = 2; t <= D; t++) x[t] = rr_add(x[t - 1], step);  // <= S4.8
        if (j == 0) {
#pragma unroll
          for (int t = 0; t <= D; t++) acc[t] = x[t];
        } else {
#pragma unroll
          for (int t = 0; t + 1 <= D; t += 2) {
            FpR<Q> y0, y1;
            rr_mul2(acc[t], x[t], acc[t + 1], x[t + 1], y0, y1);  // (S4.8 | M) x S4.3 -> M
            acc[t] = y0, acc[t + 1] = y1;
          }
          if constexpr ((D & 1) == 0) acc[D] = rr_mul(acc[D], x[D]);
        }
      }
#pragma unroll
      for (int t = 0; t <= D; t++) tot[t] = rr_add(tot[t], acc[t]);  // + (<= S4.8)
    }
    if (++since >= args->period) {  // < 1.1 p + SC_TERM_BUDGET x 4.8 p
      since = 0;
#pragma unroll
      for (int t = 0; t <= D; t++) tot[t] = rr_reduce_q(tot[t]);
    }
    __syncthreads();  // the next tile's stage-in writes the regions again
  }

#pragma unroll
  for (int t = 0; t <= D; t++) {
    FpR<Q> a = rr_reduce_q(tot[t]);
#pragma unroll
    for (int s = 0; s < 6; s++) a = ml_add_n(a, ml_xor(a, 1 << s));  // N + N -> N
    if (t) __syncthreads();
#pragma unroll
    for (int i = 0; i < 9; i++) wtot[wave][i] = a.v[i];
    __syncthreads();
    if (threadIdx.x == 0) {
      FpR<Q> w = ml_limbs<Q>(wtot[0]);
#pragma unroll
      for (int u = 1; u < SC_WAVES; u++) w = rr_add(w, ml_limbs<Q>(wtot[u]));  // S4.4
      w = rr_reduce_q(w);
      uint4* o = partial + 3 * ((size_t)blockIdx.x * (D + 1) + t);
      o[0] = make_uint4(w.v[0], w.v[1], w.v[2], w.v[3]);
      o[1] = make_uint4(w.v[4], w.v[5], w.v[6], w.v[7]);
      o[2] = make_uint4(w.v[8], 0, 0, 0);
    }
  }
}

// One workgroup: per t the partials (N, 3 uint4 each) -> the total times the
// call's constant, canonical, 2 uint4.
template <class Q>
__global__ void __launch_bounds__(SC_FOLD_THREADS)
    sc_fold_kernel(const uint4* __restrict__ partial, uint32_t nparts, uint32_t nt, ScFin f,
                   uint4* __restrict__ value) {
  __shared__ uint32_t wtot[SC_FOLD_WAVES][9];
  for (uint32_t t = 0; t < nt; t++) {
    FpR<Q> acc = FpR<Q>::zero();
    for (uint32_t i = threadIdx.x; i < nparts; i += SC_FOLD_THREADS) {
      const uint4* q = partial + 3 * ((size_t)i * nt + t);
      const uint4 a = q[0], b = q[1], c = q[2];
      FpR<Q> x;
      x.v[0] = a.x, x.v[1] = a.y, x.v[2] = a.z, x.v[3] = a.w;
      x.v[4] = b.x, x.v[5] = b.y, x.v[6] = b.z, x.v[7] = b.w;
      x.v[8] = c.x;
      acc = ml_add_n(acc, x);  // N + N -> N
    }
#pragma unroll
    for (int s = 0; s < 6; s++) acc = ml_add_n(acc, ml_xor(acc, 1 << s));
    __syncthreads();  // the previous t's readers are done
    frs_put_limbs(wtot[threadIdx.x >> 6], acc);
    __syncthreads();
    if (threadIdx.x == 0) {
      FpR<Q> s = frs_limbs<Q>(wtot[0]);
#pragma unroll
      for (int w = 1; w < SC_FOLD_WAVES; w++) s = rr_add(s, frs_limbs<Q>(wtot[w]));  // S17.6
      s = rr_canon_lt2p(rr_mul(s, frs_limbs<Q>(f.fin)));                               // S17.6 x C -> M
      ml_pack(s, value[2 * t], value[2 * t + 1]);
    }
  }
}

// ---------------------------------------------------------------------------
// the bind kernel
// ---------------------------------------------------------------------------
struct MfArgs {
  uint32_t r[MF_MAX_LEVELS][9];  // r_s R' of this launch's levels (C)
  uint32_t cst[9];               // R' / R (ECG_ML_OUT_CANONICAL)
  uint32_t levels, canon;
};

template <class Q>
ECG_DEV void mf_put(uint4* lds, uint32_t j, const FpR<Q>& x, const MfArgs& a) {
  // N -> canonical words of x, or of x / R
  const FpR<Q> c = rr_canon_lt2p(a.canon ? rr_mul(x, frs_limbs<Q>(a.cst)) : x);  // N x C -> M
  ml_pack(c, lds[2 * j], lds[2 * j + 1]);
}

// in: n elements; out: n_out = n >> levels elements, 2048 >> levels per tile.
template <class Q>
__global__ void __launch_bounds__(FRS_THREADS)
    mf_kernel(MfArgs a, const uint4* __restrict__ in, size_t n, uint4* __restrict__ out, size_t n_out) {
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wv[FRS_WAVES][9];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t L = a.levels;
  frs_stage_in(in, blockIdx.x, n, lds);
  __syncthreads();
  FpR<Q> v[FRS_E];
#pragma unroll
  for (int e = 0; e < FRS_E; e++) v[e] = frs_get<Q>(lds, e);  // C
  // levels 0..2: inside the run
#pragma unroll
  for (int s = 0; s < 3; s++)
    if ((int)L > s) {
      const FpR<Q> rk = frs_limbs<Q>(a.r[s]);
      if (s < 2) {
#pragma unroll
        for (int e = 0; e < (FRS_E >> (s + 1)); e += 2) {
          FpR<Q> o0, o1;
          ml_bind2(v[2 * e], v[2 * e + 1], v[2 * e + 2], v[2 * e + 3], rk, o0, o1);
          v[e] = o0, v[e + 1] = o1;
        }
      } else {
        v[0] = ml_bind(v[0], v[1], rk);
      }
    }
  // levels 3..8: lane exchange; every lane of a group ends with the group's value
  FpR<Q> x = v[0];
#pragma unroll
  for (int s = 0; s < 6; s++)
    if ((int)L > 3 + s) {
      const FpR<Q> y = ml_xor(x, 1 << s);
      const bool up = (lane >> s) & 1;
      x = ml_bind(frs_pick(up, y, x), frs_pick(up, x, y), frs_limbs<Q>(a.r[3 + s]));
    }
  // levels 9, 10: the four wave values through LDS
  FpR<Q> g0 = x, g1 = x;
  if (L > 9) {
    frs_put_limbs(wv[wave], x);
    __syncthreads();
    ml_bind2(frs_limbs<Q>(wv[0]), frs_limbs<Q>(wv[1]), frs_limbs<Q>(wv[2]), frs_limbs<Q>(wv[3]),
             frs_limbs<Q>(a.r[9]), g0, g1);
    if (L > 10) g0 = ml_bind(g0, g1, frs_limbs<Q>(a.r[10]));
  }
  __syncthreads();  // every run has left the image: it takes the outputs now
  if (L <= 3) {
    const uint32_t cnt = FRS_E >> L;
#pragma unroll
    for (int e = 0; e < FRS_E / 2; e++)
      if ((uint32_t)e < cnt) mf_put(lds, threadIdx.x * cnt + e, v[e], a);
  } else if (L <= 9) {
    if ((threadIdx.x & ((1u << (L - 3)) - 1)) == 0) mf_put(lds, threadIdx.x >> (L - 3), x, a);
  } else if (threadIdx.x == 0) {
    mf_put(lds, 0, g0, a);
    if (L == 10) mf_put(lds, 1, g1, a);
  }
  __syncthreads();
  const uint32_t oc = FRS_TILE >> L;  // outputs per tile
  const size_t obase = (size_t)blockIdx.x * oc;
  for (uint32_t i = threadIdx.x; i < 2 * oc; i += FRS_THREADS)
    if (obase + (i >> 1) < n_out) out[2 * obase + i] = lds[i];
}

// ---------------------------------------------------------------------------
// the eq kernel: out[i] = lo_tab[i mod 2^h] x hi_tab[i >> h]
// ---------------------------------------------------------------------------
template <class Q>
__global__ void __launch_bounds__(EQ_TILE)
    eq_kernel(const uint4* __restrict__ lo_tab, const uint4* __restrict__ hi_tab, uint32_t h, size_t n,
              size_t ntiles, uint4* __restrict__ out) {
  __shared__ uint4 lds[2 * EQ_TILE];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t wl = wave * 128 + lane;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t e0 = tile * EQ_TILE + wave * 64;
    const size_t i = e0 + lane < n ? e0 + lane : 0;
    const size_t il = i & (((size_t)1 << h) - 1), ih = i >> h;
    const FpR<Q> o = rr_canon_lt2p(rr_mul(ml_unpack<Q>(lo_tab[2 * il], lo_tab[2 * il + 1]),
                                          ml_unpack<Q>(hi_tab[2 * ih], hi_tab[2 * ih + 1])));  // C x C -> M
    ml_pack(o, lds[wl], lds[wl + 64]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const uint32_t u = lane + 64 * q;
      if (e0 + (u >> 1) < n) out[2 * e0 + u] = lds[wave * 128 + (u & 1) * 64 + (u >> 1)];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static bool ml_scalar_field(const char* what, int field_id) {
  if (field_id == ECG_FIELD_BLS12_381_FR || field_id == ECG_FIELD_BN254_FR) return true;
  set_error("%s: field_id %d is not a scalar field (bls12_381_fr, bn254_fr)", what, field_id);
  return false;
}
static bool ml_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const char *p = (const char*)a, *q = (const char*)b;
  return p < q + bbytes && q < p + abytes;
}

struct ScCall {
  uint32_t log_n, k;
  const void* const* cols;
  uint32_t np;
  const uint32_t* counts;
  const uint32_t* fcols;
  const uint64_t* coeffs;
  const uint64_t* fold_r;
  void* const* folded;
  uint64_t* evals_out;
  bool canonical;
  uint32_t d;
};

template <class Q, int D, bool FOLD>
static int sc_launch(ecg_ctx* ctx, const ScArgs& args, const ScFin& fin, const ScCall& c, hipStream_t s) {
  const size_t n_in = (size_t)1 << c.log_n;
  const size_t tile_in = FOLD ? 2 * SC_TILE : SC_TILE;
  const size_t ntiles = (n_in + tile_in - 1) / tile_in;
  const size_t lds_bytes = (c.k + (FOLD ? 1 : 0)) * SC_COL_LDS;
  void (*kern)(ScArgs, size_t, size_t, uint4*) = sc_kernel<Q, D, FOLD>;
  if (lds_bytes > 32768)
    ECG_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((ECG_SC_MAX_COLS + 1) * SC_COL_LDS)));
  size_t g = 0;
  if (const char* e = getenv("ECG_SC_GRID")) g = strtoull(e, nullptr, 10);
  if (!g) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kern, SC_THREADS, lds_bytes) != hipSuccess ||
        per_cu < 1)
      per_cu = 1;
    g = (size_t)per_cu * (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256);
  }
  if (g > SC_MAX_GRID) g = SC_MAX_GRID;
  const uint32_t grid = (uint32_t)(g < ntiles ? g : ntiles);

  void *part, *val, *h;
  ECG_TRY(ws_get(ctx, "fr_ml_partial", (size_t)grid * (D + 1) * 3 * sizeof(uint4), &part));
  ECG_TRY(ws_get(ctx, "fr_ml_evals", (D + 1) * 32, &val));
  ECG_TRY(hws_get(ctx, "fr_ml_evals_h", (ECG_SC_MAX_FACTORS + 1) * 32, &h));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(SC_THREADS), lds_bytes, s, args, n_in, ntiles, (uint4*)part);
  hipLaunchKernelGGL(sc_fold_kernel<Q>, dim3(1), dim3(SC_FOLD_THREADS), 0, s, (const uint4*)part, grid,
                     (uint32_t)(D + 1), fin, (uint4*)val);
  ECG_HIP(hipGetLastError());
  ECG_HIP(hipMemcpyAsync(h, val, (D + 1) * 32, hipMemcpyDeviceToHost, s));
  ECG_HIP(hipStreamSynchronize(s));
  memcpy(c.evals_out, h, (D + 1) * 32);
  return ECG_OK;
}

template <class Q, bool FOLD>
static int sc_launch_d(ecg_ctx* ctx, const ScArgs& args, const ScFin& fin, const ScCall& c, hipStream_t s) {
  switch (c.d) {
    case 1: return sc_launch<Q, 1, FOLD>(ctx, args, fin, c, s);
    case 2: return sc_launch<Q, 2, FOLD>(ctx, args, fin, c, s);
    case 3: return sc_launch<Q, 3, FOLD>(ctx, args, fin, c, s);
    default: return sc_launch<Q, 4, FOLD>(ctx, args, fin, c, s);
  }
}

template <class P, class Q>
static int sc_run_t(ecg_ctx* ctx, const ScCall& c, hipStream_t s) {
  using H = host::HFp<P>;
  for (uint32_t p = 0; c.coeffs && p < c.np; p++)
    if (!frs_below_r<P>(c.coeffs + 4 * p)) {
      set_error("fr_sumcheck_round: coefficient %u is not a reduced field element (>= r)", p);
      return ECG_ERR_INVALID;
    }
  if (c.fold_r && !frs_below_r<P>(c.fold_r)) {
    set_error("fr_sumcheck_round: fold_r is not a reduced field element (>= r)");
    return ECG_ERR_INVALID;
  }
  const H rp = frs_from_limbs<P, Q>(Q::ONE);  // R' mod r as an integer: hmul(x, rp) = x R' / R
  ScArgs args;
  memset(&args, 0, sizeof(args));
  args.k = c.k, args.np = c.np;
  args.period = SC_TERM_BUDGET / c.np ? SC_TERM_BUDGET / c.np : 1;
  for (uint32_t j = 0; j < c.k; j++) {
    args.col[j] = (const uint4*)c.cols[j];
    if (c.fold_r) args.folded[j] = (uint4*)c.folded[j];
  }
  H kp[ECG_SC_MAX_PRODUCTS];
  bool same = true;
  for (uint32_t p = 0, at = 0; p < c.np; at += c.counts[p], p++) {
    args.nf[p] = (uint8_t)c.counts[p];
    for (uint32_t j = 0; j < c.counts[p]; j++) args.fc[p][j] = (uint8_t)c.fcols[at + j];
    memcpy(kp[p].v, c.coeffs ? c.coeffs + 4 * p : P::ONE, sizeof(kp[p].v));
    for (uint32_t j = 0; j < c.counts[p]; j++) kp[p] = host::hmul(kp[p], rp);  // c R'^f / R^(f-1)
    frs_to_limbs<P, Q>(kp[p], args.kcoef[p]);
    same = same && memcmp(kp[p].v, kp[0].v, sizeof(kp[p].v)) == 0;
  }
  args.prescale = !same;
  // the fold launch's constant: K (no prescale) or R' (terms are words already);
  // canonical: one more factor 1 / R
  H f = same ? kp[0] : rp, one = H::zero();
  one.v[0] = 1;
  if (c.canonical) f = host::hmul(f, one);
  ScFin fin;
  frs_to_limbs<P, Q>(f, fin.fin);
  if (c.fold_r) {
    H r;
    memcpy(r.v, c.fold_r, sizeof(r.v));
    frs_to_rr<P, Q>(r, args.rk);
    return sc_launch_d<Q, true>(ctx, args, fin, c, s);
  }
  return sc_launch_d<Q, false>(ctx, args, fin, c, s);
}

struct MfCall {
  const void* in;
  uint32_t log_n, m;
  const uint64_t* point;
  void* out;
  uint64_t* value_out;
  bool canonical;
};

template <class P, class Q>
static int mf_run_t(ecg_ctx* ctx, const MfCall& c, hipStream_t s) {
  using H = host::HFp<P>;
  for (uint32_t j = 0; j < c.m; j++)
    if (!frs_below_r<P>(c.point + 4 * j)) {
      set_error("fr_mle_fix: point[%u] is not a reduced field element (>= r)", j);
      return ECG_ERR_INVALID;
    }
  MfArgs args;
  memset(&args, 0, sizeof(args));
  H one = H::zero();
  one.v[0] = 1;
  frs_to_rr<P, Q>(one, args.cst);  // R' / R
  const bool eval = c.m == c.log_n;
  void* final_out = c.out;
  if (!final_out) ECG_TRY(ws_get(ctx, "fr_ml_value", 32, &final_out));
  const void* cur = c.in;
  size_t n = (size_t)1 << c.log_n;
  for (uint32_t done = 0, pass = 0; done < c.m; pass++) {
    const uint32_t L = c.m - done < (uint32_t)MF_MAX_LEVELS ? c.m - done : (uint32_t)MF_MAX_LEVELS;
    const bool last = done + L == c.m;
    const size_t n_out = n >> L;
    void* dst = final_out;
    if (!last) ECG_TRY(ws_get(ctx, (pass & 1) ? "fr_ml_fix_b" : "fr_ml_fix_a", n_out * 32, &dst));
    for (uint32_t j = 0; j < L; j++) {
      H r;
      memcpy(r.v, c.point + 4 * (done + j), sizeof(r.v));
      frs_to_rr<P, Q>(r, args.r[j]);
    }
    args.levels = L, args.canon = last && c.canonical;
    const size_t ntiles = (n + FRS_TILE - 1) >> FRS_LOG_TILE;
    hipLaunchKernelGGL(mf_kernel<Q>, dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s, args, (const uint4*)cur, n,
                       (uint4*)dst, n_out);
    cur = dst, n = n_out, done += L;
  }
  ECG_HIP(hipGetLastError());
  if (eval && c.value_out) {
    void* h;
    ECG_TRY(hws_get(ctx, "fr_ml_value_h", 32, &h));
    ECG_HIP(hipMemcpyAsync(h, final_out, 32, hipMemcpyDeviceToHost, s));
    ECG_HIP(hipStreamSynchronize(s));
    memcpy(c.value_out, h, 32);
  }
  return ECG_OK;
}

// tab[x] = start prod_{j<nv} (x_j ? r_j : 1 - r_j) for x < 2^nv; one product per entry
template <class P>
static void eq_host_table(const host::HFp<P>& start, const uint64_t* point, uint32_t nv, host::HFp<P>* tab) {
  tab[0] = start;
  for (uint32_t j = 0; j < nv; j++) {
    host::HFp<P> r;
    memcpy(r.v, point + 4 * j, sizeof(r.v));
    for (size_t x = 0; x < ((size_t)1 << j); x++) {
      const host::HFp<P> hi = host::hmul(tab[x], r);
      tab[x + ((size_t)1 << j)] = hi;
      tab[x] = host::hsub(tab[x], hi);
    }
  }
}

template <class P, class Q>
static int eq_run_t(ecg_ctx* ctx, const uint64_t* point, uint32_t log_n, const uint64_t* scale, void* d_out,
                    bool canonical, hipStream_t s) {
  using H = host::HFp<P>;
  for (uint32_t j = 0; j < log_n; j++)
    if (!frs_below_r<P>(point + 4 * j)) {
      set_error("fr_eq_table: point[%u] is not a reduced field element (>= r)", j);
      return ECG_ERR_INVALID;
    }
  if (scale && !frs_below_r<P>(scale)) {
    set_error("fr_eq_table: scale is not a reduced field element (>= r)");
    return ECG_ERR_INVALID;
  }
  const uint32_t h = (log_n + 1) / 2;
  const size_t nlo = (size_t)1 << h, nhi = (size_t)1 << (log_n - h);
  static_assert(sizeof(H) == 32, "a table entry is an element's 32 bytes");
  void *hbuf, *dbuf;
  ECG_TRY(hws_get(ctx, "fr_ml_eq_h", (nlo + nhi) * sizeof(H), &hbuf));
  ECG_TRY(ws_get(ctx, "fr_ml_eq", (nlo + nhi) * sizeof(H), &dbuf));
  H* tab = (H*)hbuf;
  // low table: words a R.  High table: b s R' (canonical: b s R' / R), which the
  // table's products by the words r_j R keep.
  H st, one = H::zero();
  one.v[0] = 1;
  memcpy(st.v, scale ? scale : P::ONE, sizeof(st.v));
  st = host::hmul(st, frs_from_limbs<P, Q>(Q::ONE));
  if (canonical) st = host::hmul(st, one);
  eq_host_table<P>(H::one(), point, h, tab);
  eq_host_table<P>(st, point + 4 * h, log_n - h, tab + nlo);
  ECG_HIP(hipMemcpyAsync(dbuf, hbuf, (nlo + nhi) * sizeof(H), hipMemcpyHostToDevice, s));
  const size_t n = (size_t)1 << log_n;
  const size_t ntiles = (n + EQ_TILE - 1) / EQ_TILE;
  const uint32_t grid = (uint32_t)(ntiles < SC_MAX_GRID ? ntiles : SC_MAX_GRID);
  hipLaunchKernelGGL(eq_kernel<Q>, dim3(grid), dim3(EQ_TILE), 0, s, (const uint4*)dbuf, (const uint4*)dbuf + 2 * nlo, h,
                     n, ntiles, (uint4*)d_out);
  ECG_HIP(hipGetLastError());
  // the pinned staging buffer belongs to the next call once the copy has run
  ECG_HIP(hipStreamSynchronize(s));
  return ECG_OK;
}

}  // namespace ecg

using namespace ecg;

extern "C" size_t ecg_fr_sumcheck_tile(void) { return SC_TILE; }

extern "C" int ecg_fr_sumcheck_round_dev(ecg_ctx* ctx, int field_id, uint32_t log_n, uint32_t k,
                                         const void* const* d_cols, uint32_t n_products,
                                         const uint32_t* factor_counts, const uint32_t* factor_cols,
                                         const uint64_t* coeffs, const uint64_t* fold_r, void* const* d_folded,
                                         uint64_t* evals_out, uint32_t flags, void* stream) {
  ECG_ENTER(ctx);
  const char* what = "fr_sumcheck_round";
  if (!ml_scalar_field(what, field_id)) return ECG_ERR_INVALID;
  if (flags & ~(uint32_t)ECG_ML_OUT_CANONICAL) {
    set_error("%s: unknown flag bits 0x%x", what, flags);
    return ECG_ERR_INVALID;
  }
  if (log_n < (fold_r ? 2u : 1u) || log_n > 32) {
    set_error("%s: log_n = %u, expected %d to 32", what, log_n, fold_r ? 2 : 1);
    return ECG_ERR_INVALID;
  }
  if (k == 0 || k > ECG_SC_MAX_COLS || n_products == 0 || n_products > ECG_SC_MAX_PRODUCTS) {
    set_error("%s: k = %u columns, n_products = %u, expected 1 to %d and 1 to %d", what, k, n_products,
              ECG_SC_MAX_COLS, ECG_SC_MAX_PRODUCTS);
    return ECG_ERR_INVALID;
  }
  if (!d_cols || !factor_counts || !factor_cols || !evals_out || (fold_r && !d_folded)) {
    set_error("%s: null array or output%s", what, fold_r && !d_folded ? " (fold_r without d_folded)" : "");
    return ECG_ERR_INVALID;
  }
  uint32_t d = 0, nfac = 0;
  for (uint32_t p = 0; p < n_products; p++) {
    if (factor_counts[p] == 0 || factor_counts[p] > ECG_SC_MAX_FACTORS) {
      set_error("%s: product %u has %u factors, expected 1 to %d", what, p, factor_counts[p], ECG_SC_MAX_FACTORS);
      return ECG_ERR_INVALID;
    }
    d = factor_counts[p] > d ? factor_counts[p] : d;
    nfac += factor_counts[p];
  }
  for (uint32_t i = 0; i < nfac; i++)
    if (factor_cols[i] >= k) {
      set_error("%s: factor %u names column %u of %u", what, i, factor_cols[i], k);
      return ECG_ERR_INVALID;
    }
  const size_t in_bytes = ((size_t)1 << log_n) * 32, out_bytes = in_bytes / 2;
  for (uint32_t j = 0; j < k; j++) {
    if (!d_cols[j] || (fold_r && !d_folded[j])) {
      set_error("%s: null pointer (column %u)", what, j);
      return ECG_ERR_INVALID;
    }
    if (((uintptr_t)d_cols[j] & 15) || (fold_r && ((uintptr_t)d_folded[j] & 15))) {
      set_error("%s: column %u is not 16-byte aligned", what, j);
      return ECG_ERR_INVALID;
    }
  }
  for (uint32_t j = 0; fold_r && j < k; j++) {
    for (uint32_t i = 0; i < k; i++)
      if (ml_overlap(d_folded[j], out_bytes, d_cols[i], in_bytes) ||
          (i != j && ml_overlap(d_folded[j], out_bytes, d_folded[i], out_bytes))) {
        set_error("%s: d_folded[%u] overlaps an input or another output", what, j);
        return ECG_ERR_INVALID;
      }
  }
  const ScCall c = {log_n,  k,        d_cols,    n_products, factor_counts, factor_cols,
                    coeffs, fold_r,   d_folded,  evals_out,  (flags & ECG_ML_OUT_CANONICAL) != 0, d};
  hipStream_t s = pick_stream(ctx, stream);
  return field_id == ECG_FIELD_BLS12_381_FR ? sc_run_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, c, s)
                                            : sc_run_t<params::bn254_fr, params::bn254_fr_rr>(ctx, c, s);
}

extern "C" int ecg_fr_mle_fix_dev(ecg_ctx* ctx, int field_id, const void* d_in, uint32_t log_n, const uint64_t* point,
                                  uint32_t m, void* d_out, uint64_t* value_out, uint32_t flags, void* stream) {
  ECG_ENTER(ctx);
  const char* what = "fr_mle_fix";
  if (!ml_scalar_field(what, field_id)) return ECG_ERR_INVALID;
  if (flags & ~(uint32_t)ECG_ML_OUT_CANONICAL) {
    set_error("%s: unknown flag bits 0x%x", what, flags);
    return ECG_ERR_INVALID;
  }
  if (log_n < 1 || log_n > 32 || m < 1 || m > log_n) {
    set_error("%s: log_n = %u, m = %u, expected 1 <= m <= log_n <= 32", what, log_n, m);
    return ECG_ERR_INVALID;
  }
  if (!d_in || !point || (!d_out && (m < log_n || !value_out))) {
    set_error("%s: null pointer", what);
    return ECG_ERR_INVALID;
  }
  if (((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15)) {
    set_error("%s: a device pointer is not 16-byte aligned", what);
    return ECG_ERR_INVALID;
  }
  if (d_out && ml_overlap(d_out, ((size_t)1 << (log_n - m)) * 32, d_in, ((size_t)1 << log_n) * 32)) {
    set_error("%s: d_out overlaps d_in", what);
    return ECG_ERR_INVALID;
  }
  const MfCall c = {d_in, log_n, m, point, d_out, value_out, (flags & ECG_ML_OUT_CANONICAL) != 0};
  hipStream_t s = pick_stream(ctx, stream);
  return field_id == ECG_FIELD_BLS12_381_FR ? mf_run_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, c, s)
                                            : mf_run_t<params::bn254_fr, params::bn254_fr_rr>(ctx, c, s);
}

extern "C" int ecg_fr_eq_table_dev(ecg_ctx* ctx, int field_id, const uint64_t* point, uint32_t log_n,
                                   const uint64_t* scale, void* d_out, uint32_t flags, void* stream) {
  ECG_ENTER(ctx);
  const char* what = "fr_eq_table";
  if (!ml_scalar_field(what, field_id)) return ECG_ERR_INVALID;
  if (flags & ~(uint32_t)ECG_ML_OUT_CANONICAL) {
    set_error("%s: unknown flag bits 0x%x", what, flags);
    return ECG_ERR_INVALID;
  }
  if (log_n < 1 || log_n > 32) {
    set_error("%s: log_n = %u, expected 1 to 32", what, log_n);
    return ECG_ERR_INVALID;
  }
  if (!point || !d_out || ((uintptr_t)d_out & 15)) {
    set_error("%s: null or misaligned pointer", what);
    return ECG_ERR_INVALID;
  }
  hipStream_t s = pick_stream(ctx, stream);
  const bool canon = (flags & ECG_ML_OUT_CANONICAL) != 0;
  return field_id == ECG_FIELD_BLS12_381_FR
             ? eq_run_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, point, log_n, scale, d_out, canon, s)
             : eq_run_t<params::bn254_fr, params::bn254_fr_rr>(ctx, point, log_n, scale, d_out, canon, s);
}
