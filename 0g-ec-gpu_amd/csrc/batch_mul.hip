// Variable-base batch scalar multiplication on G1:
// out_i = s_i P_i for n resident points and n resident scalars (or ONE scalar).
//   ecg_batch_mul_dev   one launch: GLV split, per-lane table, joint windowed
//                       chain, normalisation and the packed records.
//
// The product.  k = k1 + k2 LAMBDA with 128-bit halves (glv_split.hpp: BLS12-381
// by division, BN254 by the signed lattice split) and phi(x, y) = (BETA x, y) =
// LAMBDA P, so k P = k1 P + k2 phi(P): both halves ride ONE doubling chain
// (Straus-Shamir).  Each half is recoded into signed 4-bit digits with no carry
// pass, K = |k_h| + sum_{i<32} 8 16^i + 8 16^32 and digit i = nibble i of K
// minus 8, in [-8, 7] (digit 32 is 0 or 1).  Per digit position, top down:
// 4 doublings, then one addition per half.  ONE table per point, m P for
// m = 1..8; the phi half reads the same record and multiplies its X by BETA,
// and a half's sign (the digit's, times the lattice half's on BN254) selects
// Y or -Y limb by limb.  33 positions: 128 doublings that do work (the first
// four meet the identity) and 66 additions, after 4 doublings + 3 additions
// for the table.
//
// Every addition is the complete rr_add_xyzz (identity operands, P = Q,
// P = -Q behind a test waves almost never pass): small and structured scalars
// (k1 = k2, k = LAMBDA +- 1, repeated points, identity inputs) do meet
// acc = +-entry and acc = O mid-chain.  No wave diverges on digits: a zero
// digit adds entry 1 and a limb select keeps the accumulator.
//
// The kernel.  256 threads, one point per thread and tile, BM_TILES tiles per
// normalisation group, a PERSISTENT grid (the resident workgroups of the
// device, host-side) that loops over the groups: the table slots belong to the
// resident lanes, so the workspace does not grow with n.  A lane's 8 XYZZ
// records are contiguous ([lane][entry], 8 x 4 NL words = 1664 B on the
// 13-limb layout): a lane reads one whole record per addition, whichever
// entry its digit names, so every 128-B line it touches is used in full;
// [entry][lane] would coalesce only when the wave's digits agree (16 B used
// of each line otherwise, 8 lines per lane and vector).  Normalisation and
// the store are the fixed-base kernel's (norm_group.hpp): one Fermat
// inversion per 512 outputs, the records through an LDS transposition; the
// Jacobian form (x, y, 1) / (0, 1, 0) leaves the same stage with three
// coordinates per record.  In place works because a group reads its 512 inputs
// before it writes its 512 outputs, and groups do not share records.
#include "ctx.hpp"
#include "glv_split.hpp"
#include "norm_group.hpp"

namespace ecg {

constexpr int BM_TAB = 8;    // table entries per lane (m P, m = 1..8)
constexpr int BM_TILES = 2;  // tiles of 256 outputs per inversion, as the fixed-base kernel
constexpr int BM_DIGITS = 33;  // signed nibbles of a recoded 128-bit half

template <class C>
using BmQ = typename RR1of<typename C::FqParams>::Q;

// k = k1 + k2 LAMBDA for canonical k < r (BN254: signed halves, the sign in bit 127)
template <class C>
ECG_DEV void bm_split(const uint32_t* k, uint32_t* k1, uint32_t* k2) {
  if constexpr (C::Gen::GLV == 2)
    glv_lattice_split<C>(k, k1, k2);
  else
    glv_split<C>(k, k1, k2);
}

// ECG_BM_ONE_SCALAR: the one scalar is split here, once; the product kernel reads the halves.
template <class C>
__global__ void bm_split_kernel(const uint4* __restrict__ scalar, uint32_t mont, uint4* __restrict__ halves) {
  uint32_t s[8], k1[4], k2[4];
  fb_load_scalar<typename C::FrParams>(scalar, 0, 1, mont, s);
  bm_split<C>(s, k1, k2);
  halves[0] = make_uint4(k1[0], k1[1], k1[2], k1[3]);
  halves[1] = make_uint4(k2[0], k2[1], k2[2], k2[3]);
}

// K = k + 0x88...8 (32 nibbles) with digit 32 = carry + 8: nibble i of K minus 8 is the signed digit i
ECG_DEV void bm_recode(const uint32_t* k, uint32_t* K) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    c += (uint64_t)k[i] + 0x88888888u;
    K[i] = (uint32_t)c;
    c >>= 32;
  }
  K[4] = (uint32_t)c + 8u;
}
// The next digit, top down (the low nibble of K[4]); K moves up by one nibble.
ECG_DEV int bm_digit(uint32_t* K) {
  const int d = (int)(K[4] & 15u) - 8;
#pragma unroll
  for (int j = 4; j > 0; j--) K[j] = (K[j] << 4) | (K[j - 1] >> 28);
  K[0] <<= 4;
  return d;
}

// Point i as XYZZ limbs (the identity beyond n): an [x, y] record, all-zero =
// identity, or a Jacobian (X, Y, Z) with any Z, Z = 0 = identity (as ecfft_load_kernel).
template <class C, bool JAC>
ECG_DEV XYZZ<FpR<BmQ<C>>> bm_load_point(const typename C::Fq* pts, size_t i, size_t n) {
  using F = typename C::Fq;
  using Q = BmQ<C>;
  using R = FpR<Q>;
  XYZZ<R> r = xyzz_zero<R>();
  if (i < n) {
    if constexpr (JAC) {
      Jac<F> j;
      j.X = load(&pts[3 * i]);
      j.Y = load(&pts[3 * i + 1]);
      j.Z = load(&pts[3 * i + 2]);
      const bool id = fis_zero(j.Z);
      const XYZZ<R> p = pa_from_std_rr<Q>(xyzz_from_jac(j));
      rr_sel(r, !id, p);
    } else {
      const Affine<F> a = load_affine(&pts[2 * i]);
      XYZZ<R> p;
      p.X = rr_from_std<Q>(a.x);
      p.Y = rr_from_std<Q>(a.y);
      p.ZZ = R::one();
      p.ZZZ = R::one();
      rr_sel(r, !aff_is_identity(a), p);
    }
  }
  return r;
}

// k P_i for one tile: table in the lane's slot, then the joint chain.
template <class C, bool JAC>
ECG_DEV XYZZ<FpR<BmQ<C>>> bm_product(const typename C::Fq* pts, const uint4* __restrict__ scalars,
                                     const uint4* __restrict__ halves, size_t i, size_t n, uint32_t mont,
                                     XYZZ<FpR<BmQ<C>>>* __restrict__ tab, const uint32_t* beta) {
  using Q = BmQ<C>;
  using R = FpR<Q>;
  uint32_t k1[4], k2[4], K1[5], K2[5];
  if (halves) {  // uniform
    const uint4 lo = halves[0], hi = halves[1];
    k1[0] = lo.x; k1[1] = lo.y; k1[2] = lo.z; k1[3] = lo.w;
    k2[0] = hi.x; k2[1] = hi.y; k2[2] = hi.z; k2[3] = hi.w;
  } else {
    uint32_t s[8];
    fb_load_scalar<typename C::FrParams>(scalars, i, n, mont, s);
    bm_split<C>(s, k1, k2);
  }
  const bool n1 = glv_take_sign<C>(k1), n2 = glv_take_sign<C>(k2);
  bm_recode(k1, K1);
  bm_recode(k2, K2);

  {  // m P, m = 1..8: four levels (2P; 3P, 4P; 5P, 6P, 8P; 7P)
    const XYZZ<R> P = bm_load_point<C, JAC>(pts, i, n);
    store_xyzz(&tab[0], P);
    const XYZZ<R> P2 = pa_dbl(P);
    store_xyzz(&tab[1], P2);
    const XYZZ<R> P3 = pa_add(P2, P);
    store_xyzz(&tab[2], P3);
    const XYZZ<R> P4 = pa_dbl(P2);
    store_xyzz(&tab[3], P4);
    store_xyzz(&tab[4], pa_add(P4, P));
    const XYZZ<R> P6 = pa_dbl(P3);
    store_xyzz(&tab[5], P6);
    store_xyzz(&tab[6], pa_add(P6, P));
    store_xyzz(&tab[7], pa_dbl(P4));
  }

  XYZZ<R> acc = xyzz_zero<R>();
#pragma unroll 1
  for (int pos = 0; pos < BM_DIGITS; pos++) {
#pragma unroll 1
    for (int b = 0; b < 4; b++) acc = pa_dbl(acc);
#pragma unroll 1
    for (int h = 0; h < 2; h++) {  // half 0: k1 on P, half 1: k2 on phi(P)
      const int d = h ? bm_digit(K2) : bm_digit(K1);
      const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
      XYZZ<R> T = load_xyzz(&tab[mag ? mag - 1 : 0]);
      if (h) T.X = rr_mul(T.X, fb_limbs<Q>(beta));  // phi(x, y) = (BETA x, y)
      T.Y = rr_pick((d < 0) != (h ? n2 : n1), pa_neg(T).Y, T.Y);
      const XYZZ<R> r = pa_add(acc, T);
      rr_sel(acc, mag != 0, r);
    }
  }
  return acc;
}

template <class C, bool JAC>
__global__ void __launch_bounds__(FB_THREADS) __attribute__((amdgpu_waves_per_eu(fb_waves<BmQ<C>>())))
    bm_mul_kernel(const typename C::Fq* points, const uint4* __restrict__ scalars, const uint4* __restrict__ halves,
                  size_t n, uint32_t mont, XYZZ<FpR<BmQ<C>>>* __restrict__ tabs, uint4* out) {
  using Q = BmQ<C>;
  using F = FpR<Q>;
  using S = typename C::Fq;
  constexpr int NL = Q::NL, T = BM_TILES;
  constexpr int L = S::L;                    // 32-bit words per boundary coordinate
  constexpr int RV = (JAC ? 3 : 2) * L / 4;  // uint4 per output record
  static_assert(L % 4 == 0, "a coordinate is whole uint4");
  __shared__ uint4 stage[FB_THREADS * (RV + 1)];
  __shared__ uint32_t stash[T - 1][2 * NL][FB_THREADS];  // word k of thread t at [k][t]: no bank met twice
  __shared__ uint32_t wtot[FB_WAVES][NL];
  __shared__ uint32_t tot[T][NL], kinv[T][NL];
  __shared__ uint32_t beta[NL];

  if (threadIdx.x < 64) {  // every lane of wave 0 writes the same limbs
    S bs;
    from_u64_words(bs, C::Gen::BETA);
    fb_put_limbs(beta, rr_from_std<Q>(bs));
  }
  __syncthreads();
  XYZZ<F>* tab = tabs + ((size_t)blockIdx.x * FB_THREADS + threadIdx.x) * BM_TAB;
  const size_t per = (size_t)FB_THREADS * T, groups = (n + per - 1) / per;

  for (size_t g = blockIdx.x; g < groups; g += gridDim.x) {
    F a, b;            // the last tile's pair stays in registers
    uint32_t ids = 0;  // bit t: this thread's output of tile t is the identity
    for (int t = 0; t < T; t++) {
      const size_t i = (g * T + t) * FB_THREADS + threadIdx.x;
      const XYZZ<F> acc = bm_product<C, JAC>(points, scalars, halves, i, n, mont, tab, beta);
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
      const bool id = (ids >> t) & 1;
      uint32_t wd[4 * RV];
      rr_pack<Q, L>(rr_canon_lt2p(x).v, wd);
      rr_pack<Q, L>(rr_canon_lt2p(y).v, wd + L);
#pragma unroll
      for (int k = 0; k < 2 * L; k++) wd[k] = id ? 0u : wd[k];
      if constexpr (JAC) {  // (x, y, 1) or (0, 1, 0), 1 the boundary's Montgomery one
#pragma unroll
        for (int k = 0; k < L; k++) {
          wd[L + k] = id ? S::one32(k) : wd[L + k];
          wd[2 * L + k] = id ? 0u : S::one32(k);
        }
      }
      __syncthreads();  // the stage is read by the previous tile's stores
#pragma unroll
      for (int j = 0; j < RV; j++)
        stage[(RV + 1) * threadIdx.x + j] = make_uint4(wd[4 * j], wd[4 * j + 1], wd[4 * j + 2], wd[4 * j + 3]);
      __syncthreads();
      const size_t base = (g * T + t) * FB_THREADS;
#pragma unroll
      for (int q = 0; q < RV; q++) {
        const uint32_t J = q * FB_THREADS + threadIdx.x, owner = J / RV;
        if (base + owner < n) out[base * RV + J] = stage[J + owner];  // (RV + 1) owner + J % RV
      }
    }
  }
}

// the largest persistent grid of the kernel on this device: its resident workgroups
template <class C, bool JAC>
static int bm_resident(ecg_ctx* ctx, uint32_t* blocks) {
  int per_cu = 0;
  ECG_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bm_mul_kernel<C, JAC>, FB_THREADS, 0));
  if (per_cu < 1 || ctx->compute_units < 1) {
    set_error("batch_mul: the kernel does not fit a compute unit");
    return ECG_ERR_HIP;
  }
  *blocks = (uint32_t)per_cu * (uint32_t)ctx->compute_units;
  return ECG_OK;
}

template <class C, bool JAC>
static int bm_run(ecg_ctx* ctx, const void* d_points, const void* d_scalars, size_t n, uint32_t flags, void* d_out,
                  hipStream_t s) {
  using X = XYZZ<FpR<BmQ<C>>>;
  uint32_t resident = 0;
  ECG_TRY((bm_resident<C, JAC>(ctx, &resident)));
  const size_t per = (size_t)FB_THREADS * BM_TILES, groups = (n + per - 1) / per;
  const uint32_t grid = (uint32_t)(groups < resident ? groups : resident);
  void *tabs, *halves = nullptr;
  ECG_TRY(ws_get(ctx, "batch_mul_tab", (size_t)grid * FB_THREADS * BM_TAB * sizeof(X), &tabs));
  const uint32_t mont = flags & ECG_BM_SCALARS_MONTGOMERY ? 1u : 0u;
  if (flags & ECG_BM_ONE_SCALAR) {
    ECG_TRY(ws_get(ctx, "batch_mul_halves", 2 * sizeof(uint4), &halves));
    hipLaunchKernelGGL(bm_split_kernel<C>, dim3(1), dim3(1), 0, s, (const uint4*)d_scalars, mont, (uint4*)halves);
    ECG_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL((bm_mul_kernel<C, JAC>), dim3(grid), dim3(FB_THREADS), 0, s, (const typename C::Fq*)d_points,
                     (const uint4*)d_scalars, (const uint4*)halves, n, mont, (X*)tabs, (uint4*)d_out);
  ECG_HIP(hipGetLastError());
  return ECG_OK;
}

static bool bm_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace ecg

using namespace ecg;

extern "C" int ecg_batch_mul_dev(ecg_ctx* ctx, int curve_id, const void* d_points, const void* d_scalars, size_t n,
                                 uint32_t flags, void* d_out, void* stream) {
  ECG_ENTER(ctx);
  if (curve_id != ECG_CURVE_BLS12_381 && curve_id != ECG_CURVE_BN254) {
    const char* name = ecg_curve_name(curve_id);
    set_error("batch_mul: curve %s (id %d) has no batch multiplication kernel (G1 of bls12_381 and bn254 only)",
              name ? name : "?", curve_id);
    return ECG_ERR_INVALID;
  }
  if (flags & ~(uint32_t)(ECG_BM_SCALARS_MONTGOMERY | ECG_BM_ONE_SCALAR | ECG_BM_JACOBIAN)) {
    set_error("batch_mul: unknown flag bits 0x%x", flags);
    return ECG_ERR_INVALID;
  }
  if (n == 0) return ECG_OK;
  if (!d_points || !d_scalars || !d_out) {
    set_error("batch_mul: null pointer");
    return ECG_ERR_INVALID;
  }
  if (n > ((size_t)1 << 32)) {
    set_error("batch_mul: n = %zu is above 2^32", n);
    return ECG_ERR_INVALID;
  }
  const bool jac = flags & ECG_BM_JACOBIAN;
  const size_t pts_bytes = n * (jac ? 3 : 2) * fq_limbs64(curve_id) * 8;
  const size_t sc_bytes = (flags & ECG_BM_ONE_SCALAR ? 1 : n) * 32;
  if ((d_out != d_points && bm_overlap(d_out, pts_bytes, d_points, pts_bytes)) ||
      bm_overlap(d_out, pts_bytes, d_scalars, sc_bytes)) {
    set_error("batch_mul: d_out overlaps an input (only d_out == d_points, in place, is allowed)");
    return ECG_ERR_INVALID;
  }
  hipStream_t s = pick_stream(ctx, stream);
  if (curve_id == ECG_CURVE_BLS12_381)
    ECG_TRY(jac ? (bm_run<BLS12_381, true>(ctx, d_points, d_scalars, n, flags, d_out, s))
                : (bm_run<BLS12_381, false>(ctx, d_points, d_scalars, n, flags, d_out, s)));
  else
    ECG_TRY(jac ? (bm_run<BN254, true>(ctx, d_points, d_scalars, n, flags, d_out, s))
                : (bm_run<BN254, false>(ctx, d_points, d_scalars, n, flags, d_out, s)));
  if (!stream) ECG_HIP(hipStreamSynchronize(s));
  return ECG_OK;
}
