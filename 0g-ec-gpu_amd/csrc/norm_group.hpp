// Workgroup routines shared by the fixed-base kernel (fixed_base.hip) and the
// batch scalar multiplication (batch_mul.hip): the scalar load (Montgomery ->
// canonical, then mod r) and the normalisation of 256-point tiles of
// reduced-radix XYZZ points around ONE Fermat inversion per workgroup
// (DESIGN.md §4.7).  256 threads per workgroup.
#pragma once
#include "curve_rr.hpp"
#include "fieldrr_inv.hpp"

namespace ecg {

constexpr int FB_THREADS = 256;
constexpr int FB_WAVES = FB_THREADS / 64;

template <bool DOWN, class Q>
ECG_DEV FpR<Q> fb_shift(const FpR<Q>& a, int d) {  // lane + d (DOWN) / lane - d; no partner: itself
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = DOWN ? __shfl_down(a.v[i], d, 64) : __shfl_up(a.v[i], d, 64);
  return r;
}
template <class Q>
ECG_DEV FpR<Q> fb_bcast(const FpR<Q>& a, int lane) {
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = __shfl(a.v[i], lane, 64);
  return r;
}
template <class Q>
ECG_DEV FpR<Q> fb_limbs(const uint32_t* p) {
  FpR<Q> r;
#pragma unroll
  for (int i = 0; i < Q::NL; i++) r.v[i] = p[i];
  return r;
}
template <class Q>
ECG_DEV void fb_put_limbs(uint32_t* p, const FpR<Q>& a) {
#pragma unroll
  for (int i = 0; i < Q::NL; i++) p[i] = a.v[i];
}

// Exclusive product scan over the workgroup: the product of the g of every
// earlier (UP) / later (DOWN) thread, 1 at the edge (fr_scan.hip's scheme).
template <bool DOWN, class Q>
ECG_DEV FpR<Q> fb_mul_block_scan(const FpR<Q>& g, uint32_t (*wtot)[Q::NL]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  FpR<Q> v = g;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const FpR<Q> s = rr_mul(v, fb_shift<DOWN>(v, 1 << k));
    v = rr_pick(DOWN ? lane + (1 << k) < 64 : lane >= (1 << k), s, v);
  }
  fb_put_limbs(wtot[wave], fb_bcast(v, DOWN ? 0 : 63));
  const FpR<Q> e = fb_shift<DOWN>(v, 1);
  __syncthreads();
  FpR<Q> w = FpR<Q>::one();
  for (int u = DOWN ? wave + 1 : 0; u < (DOWN ? FB_WAVES : wave); u++) w = rr_mul(w, fb_limbs<Q>(wtot[u]));
  const FpR<Q> x = rr_mul(w, e);
  __syncthreads();  // wtot may be written again
  return rr_pick(DOWN ? lane == 63 : lane == 0, w, x);
}

// Normalisation of 256-point tiles around ONE inversion per workgroup.
// fb_norm_tile: a = X ZZZ q and b = Y ZZ q, q the product of the other 255
// points' u = ZZ ZZZ (1 for an identity: id), so that (x, y) = (a, b) / total;
// wave 0 leaves total, the product of all 256 u, in tot.  Product outputs.
template <class Q>
ECG_DEV void fb_norm_tile(const XYZZ<FpR<Q>>& p, uint32_t (*wtot)[Q::NL], uint32_t* tot, FpR<Q>& a, FpR<Q>& b,
                          bool& id) {
  using F = FpR<Q>;
  id = xyzz_is_zero_rr(p);
  const F zz = rr_pick(id, F::one(), p.ZZ), zzz = rr_pick(id, F::one(), p.ZZZ);
  const F u = rr_mul(zz, zzz);
  rr_mul2(p.X, zzz, p.Y, zz, a, b);
  const F before = fb_mul_block_scan<false>(u, wtot);
  const F after = fb_mul_block_scan<true>(u, wtot);
  if (threadIdx.x < 64)  // wave 0, thread 0's values on every lane: total = u_0 (what follows thread 0)
    fb_put_limbs(tot, rr_mul(fb_bcast(u, 0), fb_bcast(after, 0)));
  const F q = rr_mul(before, after), a0 = a, b0 = b;
  rr_mul2(a0, q, b0, q, a, b);
}
// fb_norm_invert: kinv[t] = K / total_t for the T tiles' totals, by wave 0 (a
// barrier before and after is the caller's).  K = R mod p (TO_STD: the products
// by kinv land in the boundary's Montgomery form) or 1 (the limbs stay).
template <bool TO_STD, int T, class Q>
ECG_DEV void fb_norm_invert(uint32_t (*tot)[Q::NL], uint32_t (*kinv)[Q::NL]) {
  using F = FpR<Q>;
  if (threadIdx.x >= 64) return;
  F K, pre[T];  // pre[t]: the product of the totals before t
#pragma unroll
  for (int i = 0; i < Q::NL; i++) K.v[i] = TO_STD ? Q::FROM_RR[i] : Q::ONE[i];
  F all = fb_limbs<Q>(tot[0]);
#pragma unroll
  for (int t = 1; t < T; t++) {
    pre[t] = all;
    all = rr_mul(all, fb_limbs<Q>(tot[t]));
  }
  F inv = rr_mul(rr_inv_fermat(all), K);
#pragma unroll
  for (int t = T - 1; t >= 1; t--) {
    fb_put_limbs(kinv[t], rr_mul(inv, pre[t]));
    inv = rr_mul(inv, fb_limbs<Q>(tot[t]));
  }
  fb_put_limbs(kinv[0], inv);
}

// Scalar i (zero beyond n) as eight canonical words below r.
template <class FrP>
ECG_DEV void fb_load_scalar(const uint4* __restrict__ scalars, size_t i, size_t n, uint32_t mont, uint32_t* s) {
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  if (i < n) {
    lo = scalars[2 * i];
    hi = scalars[2 * i + 1];
  }
  s[0] = lo.x; s[1] = lo.y; s[2] = lo.z; s[3] = lo.w;
  s[4] = hi.x; s[5] = hi.y; s[6] = hi.z; s[7] = hi.w;
  if (mont) {  // PrimeFieldRepr::to_bigint on the device, as the MSM's digit kernel
    Fp<FrP> m;
#pragma unroll
    for (int k = 0; k < 8; k++) m.v[k] = s[k];
    m = from_mont(m);
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = m.v[k];
  }
  for (int it = 0; it < 8; it++) {  // any 256-bit word: at most 2^256 / r subtractions
    uint32_t t[8];
    int64_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      c = (int64_t)s[k] - Fp<FrP>::p32(k) + (c >> 32);
      t[k] = (uint32_t)c;
    }
    if ((c >> 32) & 1) break;  // s < r
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = t[k];
  }
}

// Register budget: 2 waves per SIMD on the 13-limb layout (256 registers), 3 on the 9-limb one (168).
template <class Q>
constexpr int fb_waves() {
  return Q::NL > 9 ? 2 : 3;
}

}  // namespace ecg
