// Fused sums of products over device-resident Fr vectors:
//   ecg_fr_lincomb_dev   out[i] = sum_{j<k} c_j A_j[i] B_j[i] G_j(i),
//                        G_j(i) = g^(index0 + i) for the terms of geo_mask,
//                        and optionally sum_i out[i].
// What arkworks writes as the element-wise operators of DensePolynomial /
// Evaluations and as EvaluationDomain::distribute_powers, one pass over memory
// per call instead of one per operator.
//
// Memory first: at 2^24 the Hadamard product moves 1.5 GB for one product per
// element, so the kernel is laid out around its loads and stores.
//   Tile.  FRV_TILE = 256 consecutive elements, one per thread of a 256-thread
//   workgroup; a wave owns 64 of them, a 2-KB span of every vector.  Global
//   memory is only touched as consecutive uint4: lane l takes uint4 l and
//   64 + l of the span.  The two halves of an element go to two planes of the
//   wave's LDS region (uint4 u -> (u & 1) * 64 + (u >> 1)), so a lane then reads
//   its own element as two ds_read_b128 at unit stride, and the result returns
//   the same way.  Regions are wave-private; 8 KB of LDS per DISTINCT vector.
//   Load once.  The host lists the distinct operand pointers (<= 16); every
//   term names its operands by slot in that list, so a vector used twice (the
//   output among the inputs, a square, one vector in two terms) is fetched once
//   per tile.  All loads of up to four vectors are issued before the first LDS
//   write.
//   Grid.  Persistent: as many workgroups as the device holds at once for the
//   call's LDS size (occupancy query), block b walks tiles b, b + G, ...  The
//   running tiles are a contiguous window of G * 8 KB per vector and no two
//   tiles share a cache line, so the XCD remap of the NTT has nothing to gain
//   here.  ECG_FRV_GRID=<blocks> overrides G (A/B against one tile per block).
//
// Arithmetic: the 9 x 29-bit form of fieldrr.hpp; a word x R (R = 2^256) is
// re-read as 9 limbs, the reduced-radix form of x R / R' (R' = 2^261), and the
// output integer is out R, packed as it is.  rr_mul(x, y) = x y / R'.  Products
// per term (f = vector factors), the constant made on the host per term:
//   f = 0          0   the term is the constant c R itself;
//   f = 1, c = 1   0   the word is the term;
//   f = 1          1   a R x (c R')                     K = c R'
//   f = 2, c = 1   1   a R x b R = a b R / 32 (R^2 / R' = 2^251), then a 5-bit
//                      limb shift and rr_reduce_q: no second product;
//   f = 2          2   (a b R / 32) x (32 c R')          K = c R'^2 / R
// The geometric factor costs two products per element and call, paired in one
// rr_mul2: the terms of geo_mask are summed first and multiplied ONCE by the
// lane's running power g^i R', which a second product steps by g^(256 G) R' to
// the block's next tile.  The start power is made once per kernel from the
// host's table g^(2^m) R', m < 32: lane m of every wave takes entry m if bit m
// of the wave's first index is set (else 1) and a 5-level shuffle tree
// multiplies them (5 products instead of 32 per lane), then 6 select-products
// by g^(2^k) add the lane's own 6 bits.  ECG_FRV_OUT_CANONICAL is one product
// by R' / R on the sum.
//
// Operand classes at each product (first operand always quasi-normalised, so
// BLS12-381 keeps its ceil-carry form: AMAX = 0 everywhere):
//   C  canonical: exact limbs, value < p (inputs, constants, table entries);
//   M  product output: exact limbs, < 1.5 p;   N  rr_reduce_q output, < 1.1 p;
//   Sk carried sum (rr_add, QN) of value < k p.
// A term is C, M or N (< 1.5 p); the two sums of at most 8 terms are S12.  The
// widest product is S12 x M = 18 p^2 (geometric sum times power) against the
// 32 p^2 of BLS12-381 Fr's slack; the canonical exit is S13.5 x C.
//
// Total: every lane adds its stored values limb-wise with one carry step
// (rr_add), rr_reduce_q every 32 tiles (< 34 p); six shuffle levels, the four
// wave totals through LDS, one 48-B partial per workgroup in the workspace; a
// one-workgroup launch folds the partials into 4 words.  Field addition is
// exact, so the order does not show in the bits.  Every lane computes
// everything: lanes past n enter the total as zero by a select and only the
// global store is predicated.
#include <cstdlib>
#include <cstring>

#include "ctx.hpp"
#include "fieldrr.hpp"
#include "host_field.hpp"

namespace ecg {

constexpr int FRV_THREADS = 256;
constexpr int FRV_TILE = 256;                           // one element per thread
constexpr int FRV_WAVES = FRV_THREADS / 64;
constexpr int FRV_MAX_VEC = 2 * ECG_FRV_MAX_TERMS;      // distinct operand vectors
constexpr int FRV_WAVE_SLOTS = 128;                     // uint4 per wave and vector: two planes of 64
constexpr int FRV_VEC_SLOTS = FRV_WAVES * FRV_WAVE_SLOTS;
constexpr size_t FRV_VEC_LDS = FRV_VEC_SLOTS * sizeof(uint4);  // 8 KB
constexpr int FRV_FOLD_THREADS = 1024;
constexpr int FRV_FOLD_WAVES = FRV_FOLD_THREADS / 64;
constexpr int FRV_NPOW = 32;                            // g^(2^m), m < 32: index0 + n <= 2^32
constexpr uint32_t FRV_MAX_GRID = 1u << 20;
constexpr uint8_t FRV_A = 1, FRV_B = 2, FRV_GEO = 4, FRV_COEF = 8;
static_assert(FRV_TILE == FRV_THREADS, "one element per thread");

// Kernel argument (wave-uniform, scalar loads).  All limbs canonical (C).
struct FrvArgs {
  const uint4* src[FRV_MAX_VEC];              // the distinct operand vectors
  uint32_t pw[FRV_NPOW][9];                   // g^(2^m) R'
  uint32_t step[9];                           // g^(FRV_TILE gridDim) R'
  uint32_t cst[9];                            // R' / R (ECG_FRV_OUT_CANONICAL)
  uint32_t coef[ECG_FRV_MAX_TERMS][9];        // the term's constant, see the table above
  uint8_t kind[ECG_FRV_MAX_TERMS];            // FRV_A | FRV_B | FRV_GEO | FRV_COEF
  uint8_t sa[ECG_FRV_MAX_TERMS], sb[ECG_FRV_MAX_TERMS];  // slots of A_j, B_j in src
  uint32_t k, nvec, any_geo;
  uint64_t index0;
};

// PT: a generic pointer (LDS) or one into the kernel-argument segment
template <class Q, class PT>
ECG_DEV FpR<Q> frv_limbs(PT p) {
  static_assert(Q::NL == 9, "Fr layouts: 9 limbs");
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = p[i];
  return r;
}
// The kernels index the argument's arrays by wave-uniform run-time values (term,
// vector).  Through the by-value parameter the compiler answers that with a
// private copy of the whole struct (1.8 KB of scratch per lane); read through
// the kernel-argument segment itself (the struct is the first parameter, offset
// 0) they are scalar loads.
typedef const FrvArgs __attribute__((address_space(4))) * FrvArgsK;

template <class Q>
ECG_DEV FpR<Q> frv_pick(bool c, const FpR<Q>& a, const FpR<Q>& b) {
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}
template <class Q>
ECG_DEV FpR<Q> frv_xor(const FpR<Q>& a, int d) {
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = __shfl_xor(a.v[i], d, 64);
  return r;
}
template <class Q>
ECG_DEV FpR<Q> frv_unpack(const uint4& lo, const uint4& hi) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  FpR<Q> r;
  rr_unpack<Q, 8>(w, r.v);
  return r;
}
// the lane's element of vector `slot`: C
template <class Q>
ECG_DEV FpR<Q> frv_get(const uint4* lds, uint32_t slot, uint32_t wl) {
  const uint4* p = lds + slot * FRV_VEC_SLOTS + wl;
  return frv_unpack<Q>(p[0], p[64]);
}
// 32 a for exact limbs (M): exact limbs again, value < 48 p
template <class Q>
ECG_DEV FpR<Q> frv_shl5(const FpR<Q>& a) {
  constexpr int NL = Q::NL, B = Q::BITS;
  constexpr uint32_t MASK = (1u << B) - 1;
  FpR<Q> r;
  r.v[0] = (a.v[0] << 5) & MASK;
#pragma unroll
  for (int i = 1; i < NL - 1; i++) r.v[i] = ((a.v[i] << 5) & MASK) | (a.v[i - 1] >> (B - 5));
  r.v[NL - 1] = (a.v[NL - 1] << 5) | (a.v[NL - 2] >> (B - 5));
  return r;
}
// a + b with the sum brought back below 1.1 p (N)
template <class Q>
ECG_DEV FpR<Q> frv_add_n(const FpR<Q>& a, const FpR<Q>& b) {
  return rr_reduce_q(rr_add(a, b));
}

// g^(base + lane) R' for the lanes of a wave (base wave-uniform): M
template <class Q>
ECG_DEV FpR<Q> frv_start_power(FrvArgsK args, uint32_t base, uint32_t lane) {
  FpR<Q> v = FpR<Q>::one();
#pragma unroll
  for (int m = 0; m < FRV_NPOW; m++) v = frv_pick(lane == (uint32_t)m && ((base >> m) & 1), frv_limbs<Q>(args->pw[m]), v);
#pragma unroll
  for (int k = 0; k < 5; k++) v = rr_mul(v, frv_xor(v, 1 << k));  // (C | M) x (C | M); lanes 0..31 end with g^base
  FpR<Q> u;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) u.v[i] = __shfl(v.v[i], 0, 64);
#pragma unroll
  for (int k = 0; k < 6; k++) u = frv_pick((lane >> k) & 1, rr_mul(u, frv_limbs<Q>(args->pw[k])), u);  // M x C
  return u;
}

template <class Q, bool CANON>
__global__ void __launch_bounds__(FRV_THREADS)
    frv_kernel(FrvArgs args_by_value, size_t n, size_t ntiles, uint4* out, uint4* partial) {
  const FrvArgsK args = (FrvArgsK)__builtin_amdgcn_kernarg_segment_ptr();
  extern __shared__ uint4 lds[];
  __shared__ uint32_t wtot[FRV_WAVES][9];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t wl = wave * FRV_WAVE_SLOTS + lane;
  const uint4 zero4 = make_uint4(0, 0, 0, 0);

  FpR<Q> pwr = FpR<Q>::one();
  if (args->any_geo)
    pwr = frv_start_power<Q>(args, (uint32_t)(args->index0 + (uint64_t)blockIdx.x * FRV_TILE + wave * 64), lane);

  FpR<Q> acc = FpR<Q>::zero();
  uint32_t it = 0;
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, it++) {
    const size_t e0 = tile * FRV_TILE + wave * 64;  // the wave's first element
    // ---- stage in: consecutive uint4 of every distinct vector ----
    for (uint32_t v0 = 0; v0 < args->nvec; v0 += 4) {
      uint4 q[4][2];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool on = v0 + j < args->nvec;
        const uint4* s = args->src[on ? v0 + j : 0];
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const uint32_t u = lane + 64 * h;
          q[j][h] = zero4;
          if (on && e0 + (u >> 1) < n) q[j][h] = s[2 * e0 + u];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (v0 + j < args->nvec) {
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const uint32_t u = lane + 64 * h;
            lds[(v0 + j) * FRV_VEC_SLOTS + wave * FRV_WAVE_SLOTS + (u & 1) * 64 + (u >> 1)] = q[j][h];
          }
        }
    }
    __syncthreads();

    // ---- the terms: two carried sums, plain and geometric ----
    FpR<Q> sp = FpR<Q>::zero(), sg = FpR<Q>::zero();
    for (uint32_t j = 0; j < args->k; j++) {
      const uint32_t kind = args->kind[j];
      FpR<Q> t = frv_limbs<Q>(args->coef[j]);  // f = 0: C
      if (kind & FRV_A) {
        const FpR<Q> a = frv_get<Q>(lds, args->sa[j], wl);
        if (kind & FRV_B) {
          const FpR<Q> ab = rr_mul(a, frv_get<Q>(lds, args->sb[j], wl));  // C x C -> M
          if (kind & FRV_COEF)
            t = rr_mul(ab, t);  // M x C -> M
          else
            t = rr_reduce_q(frv_shl5(ab));  // 32 M < 48 p -> N
        } else if (kind & FRV_COEF) {
          t = rr_mul(a, t);  // C x C -> M
        } else {
          t = a;  // C
        }
      }
      const bool geo = kind & FRV_GEO;
      sg = rr_add(sg, frv_pick(geo, t, FpR<Q>::zero()));   // <= S12
      sp = rr_add(sp, frv_pick(geo, FpR<Q>::zero(), t));
    }
    FpR<Q> o = sp;
    if (args->any_geo) {
      FpR<Q> x, y;
      rr_mul2(sg, pwr, pwr, frv_limbs<Q>(args->step), x, y);  // S12 x M = 18 p^2 -> M;  M x C -> M
      pwr = y;
      o = rr_add(sp, x);  // S13.5
    }
    if constexpr (CANON)
      o = rr_canon_lt2p(rr_mul(o, frv_limbs<Q>(args->cst)));  // S13.5 x C -> M
    else
      o = rr_canon_lt2p(rr_reduce_q(o));

    if (partial) {
      const bool valid = tile * FRV_TILE + threadIdx.x < n;
      acc = rr_add(acc, frv_pick(valid, o, FpR<Q>::zero()));  // + C per tile
      if ((it & 31) == 31) acc = rr_reduce_q(acc);            // < 1.1 p + 32 p
    }
    // ---- stage out through the wave's region of vector 0 ----
    if (out) {
      uint32_t w[8];
      rr_pack<Q, 8>(o.v, w);
      __syncthreads();
      lds[wl] = make_uint4(w[0], w[1], w[2], w[3]);
      lds[wl + 64] = make_uint4(w[4], w[5], w[6], w[7]);
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t u = lane + 64 * h;
        if (e0 + (u >> 1) < n) out[2 * e0 + u] = lds[wave * FRV_WAVE_SLOTS + (u & 1) * 64 + (u >> 1)];
      }
    }
    __syncthreads();  // the next tile's stage-in writes the regions again
  }

  if (partial) {
    acc = rr_reduce_q(acc);
#pragma unroll
    for (int k = 0; k < 6; k++) acc = frv_add_n(acc, frv_xor(acc, 1 << k));  // N + N -> N
#pragma unroll
    for (int i = 0; i < 9; i++) wtot[wave][i] = acc.v[i];
    __syncthreads();
    FpR<Q> t = frv_limbs<Q>(wtot[0]);
#pragma unroll
    for (int w = 1; w < FRV_WAVES; w++) t = rr_add(t, frv_limbs<Q>(wtot[w]));  // S4.4
    t = rr_reduce_q(t);
    if (threadIdx.x == 0) {
      uint4* p = partial + 3 * (size_t)blockIdx.x;
      p[0] = make_uint4(t.v[0], t.v[1], t.v[2], t.v[3]);
      p[1] = make_uint4(t.v[4], t.v[5], t.v[6], t.v[7]);
      p[2] = make_uint4(t.v[8], 0, 0, 0);
    }
  }
}

// One workgroup: the partials (N, 3 uint4 each) -> the canonical total, 2 uint4.
template <class Q>
__global__ void __launch_bounds__(FRV_FOLD_THREADS)
    frv_fold_kernel(const uint4* __restrict__ partial, uint32_t nparts, uint4* __restrict__ value) {
  __shared__ uint32_t wtot[FRV_FOLD_WAVES][9];
  FpR<Q> acc = FpR<Q>::zero();
  for (uint32_t i = threadIdx.x; i < nparts; i += FRV_FOLD_THREADS) {
    const uint4 a = partial[3 * (size_t)i], b = partial[3 * (size_t)i + 1], c = partial[3 * (size_t)i + 2];
    FpR<Q> p;
    p.v[0] = a.x, p.v[1] = a.y, p.v[2] = a.z, p.v[3] = a.w;
    p.v[4] = b.x, p.v[5] = b.y, p.v[6] = b.z, p.v[7] = b.w;
    p.v[8] = c.x;
    acc = frv_add_n(acc, p);  // N + N -> N
  }
#pragma unroll
  for (int k = 0; k < 6; k++) acc = frv_add_n(acc, frv_xor(acc, 1 << k));
#pragma unroll
  for (int i = 0; i < 9; i++) wtot[threadIdx.x >> 6][i] = acc.v[i];
  __syncthreads();
  FpR<Q> t = frv_limbs<Q>(wtot[0]);
#pragma unroll
  for (int w = 1; w < FRV_FOLD_WAVES; w++) t = rr_add(t, frv_limbs<Q>(wtot[w]));  // S17.6
  if (threadIdx.x == 0) {
    t = rr_canon_lt2p(rr_reduce_q(t));
    uint32_t w[8];
    rr_pack<Q, 8>(t.v, w);
    value[0] = make_uint4(w[0], w[1], w[2], w[3]);
    value[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
}

// ---------------------------------------------------------------------------
// host side: the per-term constants and the power table (host_field.hpp)
// ---------------------------------------------------------------------------
template <class P, class Q>
static host::HFp<P> frv_from_limbs(const uint32_t* limbs) {  // sum limbs[i] 2^(BITS i), < 2^(64 N)
  host::HFp<P> r = host::HFp<P>::zero();
  for (int i = 0; i < Q::NL; i++) {
    const int bit = Q::BITS * i, w = bit >> 6, s = bit & 63;
    r.v[w] |= (uint64_t)limbs[i] << s;
    if (s + Q::BITS > 64 && w + 1 < P::N) r.v[w + 1] |= (uint64_t)limbs[i] >> (64 - s);
  }
  return r;
}
template <class P, class Q>
static void frv_to_limbs(const host::HFp<P>& x, uint32_t* limbs) {
  for (int i = 0; i < Q::NL; i++) {
    const int bit = Q::BITS * i, w = bit >> 6, s = bit & 63;
    uint64_t v = x.v[w] >> s;
    if (s + Q::BITS > 64 && w + 1 < P::N) v |= x.v[w + 1] << (64 - s);
    limbs[i] = (uint32_t)v & ((1u << Q::BITS) - 1);
  }
}
template <class P>
static bool frv_below_r(const uint64_t* v) {
  for (int i = P::N - 1; i >= 0; i--)
    if (v[i] != P::P[i]) return v[i] < P::P[i];
  return false;
}

static uint32_t frv_grid(ecg_ctx* ctx, const void* kern, size_t lds_bytes, size_t ntiles) {
  size_t g = 0;
  if (const char* e = getenv("ECG_FRV_GRID")) g = strtoull(e, nullptr, 10);
  if (!g) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, FRV_THREADS, lds_bytes) != hipSuccess || per_cu < 1)
      per_cu = 1;
    g = (size_t)per_cu * (size_t)(ctx->compute_units > 0 ? ctx->compute_units : 256);
  }
  if (g > FRV_MAX_GRID) g = FRV_MAX_GRID;
  return (uint32_t)(g < ntiles ? g : ntiles);
}

struct FrvCall {
  size_t n;
  uint32_t k;
  const void* const* a;
  const void* const* b;
  const uint64_t* coeffs;
  uint32_t geo_mask;
  const uint64_t* ratio;
  size_t index0;
  void* out;
  uint64_t* sum_out;
  bool canonical;
};

template <class P, class Q>
static int frv_run_t(ecg_ctx* ctx, const FrvCall& c, hipStream_t s) {
  using H = host::HFp<P>;
  static_assert(Q::NL * Q::BITS - 64 * P::N == 5, "R^2 / R' = R / 32: the shift of the c = 1 Hadamard term");
  const H rp = frv_from_limbs<P, Q>(Q::ONE);  // R' mod r as an integer: hmul(x, rp) = x R' / R
  FrvArgs args;
  memset(&args, 0, sizeof(args));
  args.k = c.k;
  args.index0 = c.index0;
  args.any_geo = c.geo_mask != 0;
  for (uint32_t j = 0; j < c.k; j++) {
    const void* ops[2] = {c.a ? c.a[j] : nullptr, c.b ? c.b[j] : nullptr};
    if (!ops[0]) ops[0] = ops[1], ops[1] = nullptr;
    uint8_t slot[2] = {0, 0};
    for (int o = 0; o < 2 && ops[o]; o++) {
      uint32_t v = 0;
      while (v < args.nvec && (const void*)args.src[v] != ops[o]) v++;
      if (v == args.nvec) args.src[args.nvec++] = (const uint4*)ops[o];
      slot[o] = (uint8_t)v;
    }
    H cw;
    memcpy(cw.v, c.coeffs ? c.coeffs + 4 * j : P::ONE, sizeof(cw.v));
    const bool unit = memcmp(cw.v, P::ONE, sizeof(cw.v)) == 0;
    uint8_t kind = (ops[0] ? FRV_A : 0) | (ops[1] ? FRV_B : 0) | (((c.geo_mask >> j) & 1) ? FRV_GEO : 0);
    if (ops[0] && !unit) kind |= FRV_COEF;
    if (ops[1]) cw = host::hmul(host::hmul(cw, rp), rp);  // c R'^2 / R
    else if (ops[0]) cw = host::hmul(cw, rp);             // c R'
    frv_to_limbs<P, Q>(cw, args.coef[j]);                 // f = 0: c R
    args.kind[j] = kind, args.sa[j] = slot[0], args.sb[j] = slot[1];
  }
  H one = H::zero();
  one.v[0] = 1;
  frv_to_limbs<P, Q>(host::hmul(one, rp), args.cst);  // R' / R

  const size_t ntiles = (c.n + FRV_TILE - 1) / FRV_TILE;
  const size_t lds_bytes = (args.nvec ? args.nvec : 1) * FRV_VEC_LDS;
  void (*kern)(FrvArgs, size_t, size_t, uint4*, uint4*) = c.canonical ? frv_kernel<Q, true> : frv_kernel<Q, false>;
  if (lds_bytes > 32768)
    ECG_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(FRV_MAX_VEC * FRV_VEC_LDS)));
  const uint32_t grid = frv_grid(ctx, (const void*)kern, lds_bytes, ntiles);

  if (args.any_geo) {  // g^(2^m) by squaring, each to the R' form; the step g^(FRV_TILE grid)
    H gp, st = H::one();
    memcpy(gp.v, c.ratio, sizeof(gp.v));
    const uint64_t e = (uint64_t)grid * FRV_TILE;  // < 2^28
    for (int m = 0; m < FRV_NPOW; m++) {
      frv_to_limbs<P, Q>(host::hmul(gp, rp), args.pw[m]);
      if ((e >> m) & 1) st = host::hmul(st, gp);
      gp = host::hmul(gp, gp);
    }
    frv_to_limbs<P, Q>(host::hmul(st, rp), args.step);
  }

  void *part = nullptr, *val = nullptr;
  if (c.sum_out) {
    ECG_TRY(ws_get(ctx, "fr_vec_partial", (size_t)grid * 3 * sizeof(uint4), &part));
    ECG_TRY(ws_get(ctx, "fr_vec_value", 32, &val));
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(FRV_THREADS), lds_bytes, s, args, c.n, ntiles, (uint4*)c.out, (uint4*)part);
  if (c.sum_out)
    hipLaunchKernelGGL(frv_fold_kernel<Q>, dim3(1), dim3(FRV_FOLD_THREADS), 0, s, (const uint4*)part, grid, (uint4*)val);
  ECG_HIP(hipGetLastError());
  if (c.sum_out) {
    void* h;
    ECG_TRY(hws_get(ctx, "fr_vec_value_h", 32, &h));
    ECG_HIP(hipMemcpyAsync(h, val, 32, hipMemcpyDeviceToHost, s));
    ECG_HIP(hipStreamSynchronize(s));
    memcpy(c.sum_out, h, 32);
  }
  return ECG_OK;
}

template <class P>
static int frv_check_scalars(const FrvCall& c) {
  for (uint32_t j = 0; c.coeffs && j < c.k; j++)
    if (!frv_below_r<P>(c.coeffs + 4 * j)) {
      set_error("fr_lincomb: coefficient %u is not a reduced field element (>= r)", j);
      return ECG_ERR_INVALID;
    }
  if (c.ratio && !frv_below_r<P>(c.ratio)) {
    set_error("fr_lincomb: ratio is not a reduced field element (>= r)");
    return ECG_ERR_INVALID;
  }
  return ECG_OK;
}

}  // namespace ecg

using namespace ecg;

extern "C" size_t ecg_fr_lincomb_tile(void) { return FRV_TILE; }

extern "C" int ecg_fr_lincomb_dev(ecg_ctx* ctx, int field_id, size_t n, uint32_t k, const void* const* d_a,
                                  const void* const* d_b, const uint64_t* coeffs, uint32_t geo_mask,
                                  const uint64_t* ratio, size_t index0, void* d_out, uint64_t* sum_out, uint32_t flags,
                                  void* stream) {
  ECG_ENTER(ctx);
  if (field_id != ECG_FIELD_BLS12_381_FR && field_id != ECG_FIELD_BN254_FR) {
    set_error("fr_lincomb: field_id %d is not a scalar field (bls12_381_fr, bn254_fr)", field_id);
    return ECG_ERR_INVALID;
  }
  if (flags & ~(uint32_t)ECG_FRV_OUT_CANONICAL) {
    set_error("fr_lincomb: unknown flag bits 0x%x", flags);
    return ECG_ERR_INVALID;
  }
  if (k == 0 || k > ECG_FRV_MAX_TERMS) {
    set_error("fr_lincomb: k = %u terms, expected 1 to %d", k, ECG_FRV_MAX_TERMS);
    return ECG_ERR_INVALID;
  }
  if (geo_mask >> k) {
    set_error("fr_lincomb: geo_mask 0x%x names a term at or above k = %u", geo_mask, k);
    return ECG_ERR_INVALID;
  }
  if (geo_mask && !ratio) {
    set_error("fr_lincomb: geo_mask without a ratio");
    return ECG_ERR_INVALID;
  }
  if (!d_out && !sum_out) {
    set_error("fr_lincomb: neither d_out nor sum_out");
    return ECG_ERR_INVALID;
  }
  const uint64_t lim = (uint64_t)1 << 32;
  if ((uint64_t)index0 > lim || (uint64_t)n > lim - (uint64_t)index0) {
    set_error("fr_lincomb: index0 + n = %zu + %zu is above 2^32", index0, n);
    return ECG_ERR_INVALID;
  }
  const FrvCall c = {n, k, d_a, d_b, coeffs, geo_mask, ratio, index0, d_out, sum_out,
                     (flags & ECG_FRV_OUT_CANONICAL) != 0};
  ECG_TRY(field_id == ECG_FIELD_BLS12_381_FR ? frv_check_scalars<params::bls12_381_fr>(c)
                                             : frv_check_scalars<params::bn254_fr>(c));
  const char* o = (const char*)d_out;
  if ((uintptr_t)o & 15) {
    set_error("fr_lincomb: d_out is not 16-byte aligned");
    return ECG_ERR_INVALID;
  }
  for (uint32_t j = 0; j < 2 * k; j++) {
    const void* const* ops = j < k ? d_a : d_b;
    const char* p = ops ? (const char*)ops[j % k] : nullptr;
    if (!p) continue;
    if ((uintptr_t)p & 15) {
      set_error("fr_lincomb: operand %c_%u is not 16-byte aligned", j < k ? 'a' : 'b', j % k);
      return ECG_ERR_INVALID;
    }
    if (o && p != o && p < o + n * 32 && o < p + n * 32) {
      set_error("fr_lincomb: d_out overlaps operand %c_%u (in place, d_out == operand, is allowed)", j < k ? 'a' : 'b',
                j % k);
      return ECG_ERR_INVALID;
    }
  }
  if (n == 0) {
    if (sum_out) memset(sum_out, 0, 32);
    return ECG_OK;
  }
  hipStream_t s = pick_stream(ctx, stream);
  return field_id == ECG_FIELD_BLS12_381_FR ? frv_run_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, c, s)
                                            : frv_run_t<params::bn254_fr, params::bn254_fr_rr>(ctx, c, s);
}
