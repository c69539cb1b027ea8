// Grand products over device-resident Fr columns:
//   ecg_fr_grand_product_dev   out_0 = init, out_(i+1) = out_i f_i,
//                              f_i = (prod_j num_j[i]) inv0(prod_j den_j[i]),
// the running product of permutation and lookup arguments.  inv0(0) = 0: a
// vanishing denominator gives the ratio 0 (batch inversion's "zeros kept").
//
// The scheme is the inversion's (fr_scan.hip): with N_i and D_i the column
// products of element i,
//   out_i = init (prod_{t<i} N_t) (prod_{t>=i} D_t) / (prod_all D_t),
// a prefix product of the numerators and a SUFFIX product of the denominators
// around one Fermat inversion, so no element is ever inverted.  Three launches,
// no waiting between workgroups:
//   reduce  every tile leaves prod N and prod D of its 2048 elements;
//   scan    ONE workgroup: per tile the exclusive prefix of the numerator
//           aggregates and the exclusive suffix of the denominator aggregates,
//           the latter times K / prod_all D (one rr_inv_fermat, wave 0), and the
//           total;
//   apply   every tile recomputes its elements and stores.
// Without denominators (k_den = 0) there is no denominator chain and no
// inversion: K goes into the tile prefixes instead.
//
// Tile and columns.  The tile, its LDS image and the consecutive-uint4 access
// to global memory are fr_scan.hpp's.  The k_num + k_den columns go through the
// ONE image one at a time (barrier, stage in, barrier, eight ds_read_b128
// pairs) and are multiplied into the thread's eight run values, which stay in
// registers: the denominators first (they decide the zeros), reduced to the
// eight suffix values Y_e before the numerators are staged, so the apply kernel
// holds 16 values (144 VGPRs) only across the numerators' block scan, and two
// workgroups per CU keep fitting (figures in DESIGN §4.1.2b).
//
// Zeros and padding.  A denominator word of zero is read as 1 and flags its
// element; a flagged element's numerator product is replaced by 0, so f_i = 0.
// Numerator zeros are ordinary zeros.  Positions at or beyond n (zero words in
// the image) are 1 in BOTH chains: the numerators' padding is selected to 1 by
// index, since a zero would clear the total.
//
// Powers of R / R'.  Words x R are re-read as limbs, i.e. as the R' form of
// x rho, rho = R / R' (R' = 2^261), and rr_mul keeps the R' form.  A product of
// k columns therefore carries rho^k, and element i of the output would carry
// rho^(i (k_num - k_den)): a power that grows with the index.  So every
// numerator product is multiplied once by the uniform constant
// rho^(k_den - k_num) (R' form, made on the host; skipped when the counts are
// equal), after which every element contributes rho^k_den to both chains and
// prefix x suffix / total cancels it exactly, at every index.  With k_den = 0 the
// same constant, rho^(-k_num), makes the numerators true R' forms.  What is
// left is index-independent: with P, S, A the prefix, suffix and total as
// integers (value R'), rr_inv_fermat(A) = R'^2 / A and two products give
// P S (R' K / A) / R'^2 = value K: K is init R (the caller's word as it is) or,
// with ECG_GP_OUT_CANONICAL, init.
//
// Operand classes as in fr_scan.hip (C canonical < p, M product output < 1.5 p):
// every product here is C | M by C | M, at most 2.25 p^2 against BLS12-381 Fr's
// 32 p^2.  Stores go through rr_canon_lt2p (M -> canonical).
#include <cstring>

#include "ctx.hpp"
#include "fieldrr.hpp"
#include "fieldrr_inv.hpp"
#include "fr_scan.hpp"
#include "host_field.hpp"

namespace ecg {

// Kernel argument (wave-uniform).  The columns are indexed by unrolled
// constants only, so the struct stays in scalar registers.
struct GpArgs {
  const uint4* num[ECG_GP_MAX_COLS];
  const uint4* den[ECG_GP_MAX_COLS];
  uint32_t kn, kd;
  uint32_t fold_on;   // k_num != k_den
  uint32_t fold[9];   // rho^(k_den - k_num), R' form: C
  uint32_t k[9];      // K = init R, or init (canonical): C
};

// The columns' product over the thread's run: v[e] = prod_j col_j[run e], each
// column staged through the image.  NZ: a zero word is read as 1 and sets bit e
// of the returned mask.  C, then M x C.
template <class Q, bool NZ>
ECG_DEV uint32_t gp_fold(const uint4* const (&col)[ECG_GP_MAX_COLS], uint32_t k, size_t n, uint4* lds,
                         FpR<Q> (&v)[FRS_E]) {
  uint32_t zmask = 0;
#pragma unroll
  for (int j = 0; j < ECG_GP_MAX_COLS; j++) {
    if (j >= (int)k) break;
    __syncthreads();  // the image's readers are done
    frs_stage_in(col[j], blockIdx.x, n, lds);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < FRS_E; e += 2) {
      bool z0, z1;
      FpR<Q> x0 = frs_get<Q>(lds, e, z0), x1 = frs_get<Q>(lds, e + 1, z1);
      if constexpr (NZ) {
        x0 = frs_pick(z0, FpR<Q>::one(), x0);
        x1 = frs_pick(z1, FpR<Q>::one(), x1);
        zmask |= ((uint32_t)z0 << e) | ((uint32_t)z1 << (e + 1));
      }
      if (j == 0) {
        v[e] = x0, v[e + 1] = x1;
      } else {
        FpR<Q> p0, p1;
        rr_mul2(v[e], x0, v[e + 1], x1, p0, p1);  // (C | M) x C twice
        v[e] = p0, v[e + 1] = p1;
      }
    }
  }
  return zmask;
}

// D'_e: the denominator product of run element e, 1 where it vanishes (mask
// bit e) and beyond n (all words zero there).
template <class Q>
ECG_DEV uint32_t gp_den_run(const GpArgs& a, size_t n, uint4* lds, FpR<Q> (&v)[FRS_E]) {
  const uint32_t zmask = gp_fold<Q, true>(a.den, a.kd, n, lds, v);
#pragma unroll
  for (int e = 0; e < FRS_E; e++) v[e] = frs_pick((zmask >> e) & 1, FpR<Q>::one(), v[e]);
  return zmask;
}

// N'_e: the numerator product times rho^(k_den - k_num); 0 where the
// denominator vanishes; 1 beyond n, whatever the mask says there.
template <class Q>
ECG_DEV void gp_num_run(const GpArgs& a, size_t n, uint32_t zmask, uint4* lds, FpR<Q> (&v)[FRS_E]) {
  gp_fold<Q, false>(a.num, a.kn, n, lds, v);
  if (a.fold_on) {
    const FpR<Q> c = frs_limbs<Q>(a.fold);
#pragma unroll
    for (int e = 0; e < FRS_E; e += 2) {
      FpR<Q> p0, p1;
      rr_mul2(v[e], c, v[e + 1], c, p0, p1);  // (C | M) x C twice
      v[e] = p0, v[e + 1] = p1;
    }
  }
  const size_t first = ((size_t)blockIdx.x << FRS_LOG_TILE) + (size_t)threadIdx.x * FRS_E;
#pragma unroll
  for (int e = 0; e < FRS_E; e++)
    v[e] = frs_pick(first + e >= n, FpR<Q>::one(), frs_pick((zmask >> e) & 1, FpR<Q>::zero(), v[e]));
}

// the product of the eight run values as a tree: three paired levels
template <class Q>
ECG_DEV FpR<Q> gp_run_product(const FpR<Q> (&v)[FRS_E]) {
  FpR<Q> a, b, c, d, p, q;
  rr_mul2(v[0], v[1], v[2], v[3], a, b);  // (C | M) x (C | M) everywhere
  rr_mul2(v[4], v[5], v[6], v[7], c, d);
  rr_mul2(a, b, c, d, p, q);
  return rr_mul(p, q);
}

template <class Q, bool DEN>
__global__ void __launch_bounds__(FRS_THREADS)
    gp_reduce_kernel(GpArgs a, size_t n, FpR<Q>* __restrict__ aggn, FpR<Q>* __restrict__ aggd) {
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wtot[2][FRS_WAVES][9];
  FpR<Q> v[FRS_E], gd = FpR<Q>::one();
  uint32_t zmask = 0;
  if constexpr (DEN) {
    zmask = gp_den_run<Q>(a, n, lds, v);
    gd = gp_run_product<Q>(v);
  }
  gp_num_run<Q>(a, n, zmask, lds, v);
  FpR<Q> gn = gp_run_product<Q>(v);
#pragma unroll
  for (int k = 0; k < 6; k++) {  // M x M; lane 0 ends with the wave's products
    if constexpr (DEN) {
      FpR<Q> pn, pd;
      rr_mul2(gn, frs_shift<true>(gn, 1 << k), gd, frs_shift<true>(gd, 1 << k), pn, pd);
      gn = pn, gd = pd;
    } else {
      gn = rr_mul(gn, frs_shift<true>(gn, 1 << k));
    }
  }
  frs_put_limbs(wtot[0][threadIdx.x >> 6], frs_bcast(gn, 0));
  if constexpr (DEN) frs_put_limbs(wtot[1][threadIdx.x >> 6], frs_bcast(gd, 0));
  __syncthreads();
  if (threadIdx.x == 0) {
    FpR<Q> t = frs_limbs<Q>(wtot[0][0]);
    for (int w = 1; w < FRS_WAVES; w++) t = rr_mul(t, frs_limbs<Q>(wtot[0][w]));
    store(&aggn[blockIdx.x], t);
    if constexpr (DEN) {
      t = frs_limbs<Q>(wtot[1][0]);
      for (int w = 1; w < FRS_WAVES; w++) t = rr_mul(t, frs_limbs<Q>(wtot[1][w]));
      store(&aggd[blockIdx.x], t);
    }
  }
}

// One workgroup: thread i owns the aggregates [i R, (i + 1) R) (1 beyond the
// last tile).  pfx[t] = the numerator product of the tiles before t; sfx[t] =
// (the denominator product of the tiles after t) K / (that of all tiles): ONE
// rr_inv_fermat, by wave 0.  Without denominators K goes into pfx.  Thread 0
// writes the total, (all numerators) K / (all denominators), canonical limbs.
template <class Q, bool DEN>
__global__ void __launch_bounds__(FRS_SCAN_THREADS)
    gp_scan_kernel(const FpR<Q>* __restrict__ aggn, const FpR<Q>* __restrict__ aggd, size_t ntiles, uint32_t lg_run,
                   GpArgs a, FpR<Q>* __restrict__ pfx, FpR<Q>* __restrict__ sfx, uint4* __restrict__ value) {
  __shared__ uint32_t wtot[FRS_SCAN_WAVES][9];
  __shared__ uint32_t kinv[9], ntot[9];
  const size_t i0 = (size_t)threadIdx.x << lg_run;
  const int run = 1 << lg_run;
  FpR<Q> gn = FpR<Q>::one(), gd = FpR<Q>::one();
  for (int k = 0; k < run; k++)
    if (i0 + k < ntiles) {
      gn = rr_mul(gn, load(&aggn[i0 + k]));  // M x M
      if constexpr (DEN) gd = rr_mul(gd, load(&aggd[i0 + k]));
    }
  FpR<Q> pre = frs_mul_block_scan<Q, FRS_SCAN_WAVES, false>(gn, wtot);
  if (threadIdx.x == FRS_SCAN_THREADS - 1) frs_put_limbs(ntot, rr_mul(pre, gn));  // all numerators
  FpR<Q> suf = FpR<Q>::one();
  if constexpr (DEN) {
    suf = frs_mul_block_scan<Q, FRS_SCAN_WAVES, true>(gd, wtot);
    if (threadIdx.x < 64) {  // wave 0, thread 0's values on every lane: all denominators = g_0 * (what follows thread 0)
      const FpR<Q> all = rr_mul(frs_bcast(gd, 0), frs_bcast(suf, 0));
      frs_put_limbs(kinv, rr_mul(rr_inv_fermat(all), frs_limbs<Q>(a.k)));  // M x C
    }
  }
  __syncthreads();
  const FpR<Q> kv = DEN ? frs_limbs<Q>(kinv) : frs_limbs<Q>(a.k);  // R' K / A (M), or K (C)
  if constexpr (DEN)
    suf = rr_mul(suf, kv);
  else
    pre = rr_mul(pre, kv);
  if (threadIdx.x == 0) {
    const FpR<Q> t = rr_canon_lt2p(rr_mul(frs_limbs<Q>(ntot), kv));  // M x (C | M)
    uint32_t w[8];
    rr_pack<Q, 8>(t.v, w);
    value[0] = make_uint4(w[0], w[1], w[2], w[3]);
    value[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
  for (int k = 0; k < run; k++) {
    if (i0 + k >= ntiles) break;
    store(&pfx[i0 + k], pre);
    pre = rr_mul(pre, load(&aggn[i0 + k]));
  }
  if constexpr (DEN)
    for (int k = run - 1; k >= 0; k--) {
      if (i0 + k >= ntiles) continue;
      store(&sfx[i0 + k], suf);
      suf = rr_mul(suf, load(&aggd[i0 + k]));
    }
}

// out may be one of the columns: a tile has read every column before it stores
// and reads only what it alone writes.  Y_e = D'_e .. D'_7 x (the runs and tiles
// after) x K / (all D') by a backward sweep; then the forward sweep pairs
// out_e = c Y_e with c = c N'_e from c = the prefix before the run.
template <class Q, bool DEN>
__global__ void __launch_bounds__(FRS_THREADS)
    gp_apply_kernel(GpArgs a, size_t n, const FpR<Q>* __restrict__ pfx, const FpR<Q>* __restrict__ sfx, uint4* out) {
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wtot[FRS_WAVES][9];
  FpR<Q> y[FRS_E], x[FRS_E];
  uint32_t zmask = 0;
  if constexpr (DEN) {
    zmask = gp_den_run<Q>(a, n, lds, y);
    const FpR<Q> after = frs_mul_block_scan<Q, FRS_WAVES, true>(gp_run_product<Q>(y), wtot);
    FpR<Q> s = rr_mul(after, load(&sfx[blockIdx.x]));  // M x M
#pragma unroll
    for (int e = FRS_E - 1; e >= 0; e--) y[e] = s = rr_mul(y[e], s);  // (C | M) x M
  }
  gp_num_run<Q>(a, n, zmask, lds, x);
  const FpR<Q> before = frs_mul_block_scan<Q, FRS_WAVES, false>(gp_run_product<Q>(x), wtot);
  FpR<Q> c = rr_mul(before, load(&pfx[blockIdx.x]));  // M x M
#pragma unroll
  for (int e = 0; e < FRS_E; e++) {
    FpR<Q> o = c;
    if constexpr (DEN) {
      FpR<Q> next;
      rr_mul2(c, y[e], c, x[e], o, next);  // M x M, M x (C | M)
      c = next;
    } else {
      c = rr_mul(c, x[e]);
    }
    frs_put(lds, e, rr_canon_lt2p(o));  // the thread's own slots: its reads of the image are done
  }
  __syncthreads();
  frs_stage_out(out, blockIdx.x, n, lds);
}

// ---------------------------------------------------------------------------
// host side: the two constants (host_field.hpp), workspace, launches
// ---------------------------------------------------------------------------
struct GpCall {
  size_t n;
  uint32_t kn, kd;
  const void* const* num;
  const void* const* den;
  const uint64_t* init;
  void* out;
  uint64_t* total_out;
  bool canonical;
};

template <class Q, bool DEN>
static void gp_launch(const GpArgs& args, const GpCall& c, size_t ntiles, FpR<Q>* aggn, FpR<Q>* aggd, FpR<Q>* pfx,
                      FpR<Q>* sfx, uint4* val, hipStream_t s) {
  using F = FpR<Q>;
  hipLaunchKernelGGL((gp_reduce_kernel<Q, DEN>), dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s, args, c.n, aggn, aggd);
  hipLaunchKernelGGL((gp_scan_kernel<Q, DEN>), dim3(1), dim3(FRS_SCAN_THREADS), 0, s, (const F*)aggn, (const F*)aggd,
                     ntiles, frs_lg_run(ntiles), args, pfx, sfx, val);
  hipLaunchKernelGGL((gp_apply_kernel<Q, DEN>), dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s, args, c.n,
                     (const F*)pfx, (const F*)sfx, (uint4*)c.out);
}

template <class P, class Q>
static int gp_run_t(ecg_ctx* ctx, const GpCall& c, hipStream_t s) {
  using F = FpR<Q>;
  using H = host::HFp<P>;
  if (c.init && !frs_below_r<P>(c.init)) {
    set_error("fr_grand_product: init is not a reduced field element (>= r)");
    return ECG_ERR_INVALID;
  }
  // K: the word init R as it is, or init = hmul(init R, 1)
  H k, one = H::zero();
  one.v[0] = 1;
  memcpy(k.v, c.init ? c.init : P::ONE, sizeof(k.v));
  if (c.canonical) k = host::hmul(k, one);
  if (c.n == 0) {
    if (c.total_out) memcpy(c.total_out, k.v, 32);
    return ECG_OK;
  }
  GpArgs args;
  memset(&args, 0, sizeof(args));
  for (uint32_t j = 0; j < c.kn; j++) args.num[j] = (const uint4*)c.num[j];
  for (uint32_t j = 0; j < c.kd; j++) args.den[j] = (const uint4*)c.den[j];
  args.kn = c.kn, args.kd = c.kd, args.fold_on = c.kn != c.kd;
  frs_to_limbs<P, Q>(k, args.k);
  // rho^(k_den - k_num) in the R' form.  rp = R' mod r is the Montgomery word of
  // 1 / rho and hinv(rp) that of rho; frs_to_rr turns the word v R into v R'.
  const H rp = frs_from_limbs<P, Q>(Q::ONE);
  const H step = c.kd > c.kn ? host::hinv(rp) : rp;
  H f = H::one();
  for (uint32_t j = 0; j < (c.kd > c.kn ? c.kd - c.kn : c.kn - c.kd); j++) f = host::hmul(f, step);
  frs_to_rr<P, Q>(f, args.fold);

  const size_t ntiles = (c.n + FRS_TILE - 1) >> FRS_LOG_TILE;
  void *aggn, *aggd = nullptr, *pfx, *sfx = nullptr, *val;
  ECG_TRY(ws_get(ctx, "fr_scan_agg", ntiles * sizeof(F), &aggn));
  ECG_TRY(ws_get(ctx, "fr_scan_pfx", ntiles * sizeof(F), &pfx));
  ECG_TRY(ws_get(ctx, "fr_scan_value", 32, &val));
  if (c.kd) {
    ECG_TRY(ws_get(ctx, "fr_scan_agg_den", ntiles * sizeof(F), &aggd));
    ECG_TRY(ws_get(ctx, "fr_scan_inv", ntiles * sizeof(F), &sfx));
    gp_launch<Q, true>(args, c, ntiles, (F*)aggn, (F*)aggd, (F*)pfx, (F*)sfx, (uint4*)val, s);
  } else {
    gp_launch<Q, false>(args, c, ntiles, (F*)aggn, (F*)aggd, (F*)pfx, (F*)sfx, (uint4*)val, s);
  }
  ECG_HIP(hipGetLastError());
  if (c.total_out) {
    void* h;
    ECG_TRY(hws_get(ctx, "fr_scan_value_h", 32, &h));
    ECG_HIP(hipMemcpyAsync(h, val, 32, hipMemcpyDeviceToHost, s));
    ECG_HIP(hipStreamSynchronize(s));
    memcpy(c.total_out, h, 32);
  }
  return ECG_OK;
}

}  // namespace ecg

using namespace ecg;

extern "C" int ecg_fr_grand_product_dev(ecg_ctx* ctx, int field_id, size_t n, uint32_t k_num,
                                        const void* const* d_num, uint32_t k_den, const void* const* d_den,
                                        const uint64_t* init, void* d_out, uint64_t* total_out, uint32_t flags,
                                        void* stream) {
  ECG_ENTER(ctx);
  if (flags & ~(uint32_t)ECG_GP_OUT_CANONICAL) {
    set_error("fr_grand_product: unknown flag bits 0x%x", flags);
    return ECG_ERR_INVALID;
  }
  if (k_num == 0 || k_num > ECG_GP_MAX_COLS || k_den > ECG_GP_MAX_COLS) {
    set_error("fr_grand_product: k_num = %u, k_den = %u columns, expected 1 to %d and 0 to %d", k_num, k_den,
              ECG_GP_MAX_COLS, ECG_GP_MAX_COLS);
    return ECG_ERR_INVALID;
  }
  // field and size as the other scans; d_out and the two arrays stand in for d_in
  const bool arrays = d_num && (d_den || !k_den);
  const int rc = frs_check("fr_grand_product", field_id, arrays ? d_out : nullptr, n);
  if (rc < 0) return rc;
  const GpCall c = {n, k_num, k_den, d_num, d_den, init, d_out, total_out, (flags & ECG_GP_OUT_CANONICAL) != 0};
  if (rc == ECG_OK) {
    const char* o = (const char*)d_out;
    for (uint32_t j = 0; j < k_num + k_den; j++) {
      const char* p = (const char*)(j < k_num ? d_num[j] : d_den[j - k_num]);
      if (!p) {
        set_error("fr_grand_product: null pointer (column %u)", j);
        return ECG_ERR_INVALID;
      }
      if (p != o && p < o + n * 32 && o < p + n * 32) {
        set_error("fr_grand_product: d_out overlaps column %u (in place, d_out == a column, is allowed)", j);
        return ECG_ERR_INVALID;
      }
    }
  }
  hipStream_t s = pick_stream(ctx, stream);
  return field_id == ECG_FIELD_BLS12_381_FR ? gp_run_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, c, s)
                                            : gp_run_t<params::bn254_fr, params::bn254_fr_rr>(ctx, c, s);
}
