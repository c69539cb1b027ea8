// Radix-2^DEG Stockham NTT over the scalar fields (BLS12-381 Fr, BN254 Fr).
//
// Replaces FIELD_radix_fft (ag-build/cl/fft.cl:4-68) and its host driver
// SingleFftKernel::radix_fft (ec-gpu-proxy/src/fft.rs:50-135).  Same
// decomposition (Stockham autosort: natural order in and out, each pass a
// batch of independent 2^deg-point DFTs between a strided gather and a
// scatter), re-designed for gfx950:
//
//  * v2 (default): ceil(log n / 10) balanced passes of radix up to 2^10
//    (2^24 is three passes of 2^8; ECG_NTT_MAXDEG up to 12 for A/B).  A
//    pass's groups are packed into 1024-element tiles in LDS worked by
//    256-thread workgroups, so every global read is a G*32-byte run.  Each
//    thread runs TWO DIF rounds per LDS round trip on 4 register-resident
//    elements (radix-2^2 step), halving LDS traffic and barriers.
//  * The butterflies run in the reduced-radix form (ntt_pass_rr_kernel in
//    ntt_pass.hpp, see its header) whenever the full per-pass twiddle tables fit (log n <= 28):
//    ~1/3 fewer VALU instructions per product.  ECG_NTT_RR=0 keeps the
//    32-bit-limb passes below for A/B.
//  * No per-thread exponentiation (the reference's FIELD_pow_lookup + FIELD_pow
//    per thread, fft.cl:39-45, ~4x the butterfly work): inter-pass twiddles
//    w^e (e < n) = T_hi[e >> 12] * T_lo[e & 4095] from L2-resident tables;
//    in-group roots from a 2^(maxdeg-1) table.  Tables are built on the device
//    once per (omega, log n) and cached in the context.
//  * Values stay fully reduced (< r): output bytes equal serial_fft's.
//  * v1 (ECG_NTT_VARIANT=1): radix-2^8 passes, one DIF round per LDS round
//    trip -- kept for A/B measurement.
#include <cstdlib>
#include <cstring>

#include "ntt_pass.hpp"

namespace ecg {

template <class F>
struct LdsPlanes {
  uint4* p0;
  uint4* p1;
  ECG_DEV F get(uint32_t i) const {
    uint4 a = p0[i], b = p1[i];
    F r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
  }
  ECG_DEV void put(uint32_t i, const F& v) const {
    p0[i] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    p1[i] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
  }
};

// ---------------------------------------------------------------------------
// shared load / store phases of a Stockham pass
//   u[i] = x[g + i*t] * w^((n >> (lgp+DEG)) * k * i),  k = g mod 2^lgp, t = n >> DEG
//   y[(g - k)*2^DEG + k + j*2^lgp] = v[j]   (v = DFT of u, natural order)
// ---------------------------------------------------------------------------
template <class F, int DEG>
ECG_DEV void pass_load(const F* __restrict__ x, const F* __restrict__ tw_lo, const F* __restrict__ tw_hi,
                       const F* __restrict__ twf, const LdsPlanes<F>& U, uint32_t log_n, uint32_t lgp,
                       uint32_t log_g, uint32_t E) {
  const uint32_t G = 1u << log_g;
  const uint64_t t = (1ull << log_n) >> DEG;
  const uint64_t p = 1ull << lgp;
  const uint64_t g0 = (uint64_t)blockIdx.x << log_g;
  const uint32_t s_tw_log = log_n - lgp - DEG;  // n >> (lgp + DEG) = 2^s_tw_log
  F v[NTT_EPT], w[NTT_EPT];
  bool mul[NTT_EPT];
#pragma unroll
  for (int q = 0; q < NTT_EPT; q++) {
    const uint32_t f = threadIdx.x + q * blockDim.x;
    mul[q] = false;
    if (f < E) {
      const uint32_t gi = f & (G - 1), i = f >> log_g;
      const uint64_t g = g0 + gi;
      v[q] = load(&x[g + (uint64_t)i * t]);
      if (lgp != 0) {
        const uint64_t k = g & (p - 1);
        const uint64_t e = (k * i) << s_tw_log;  // < n
        if (e != 0) {
          // full per-pass table twf[i * p + k] (one load, k contiguous across
          // lanes) or the split tables (two loads + one product)
          mul[q] = true;
          w[q] = twf ? load(&twf[(uint64_t)i * p + k]) : twiddle(tw_lo, tw_hi, e);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NTT_EPT; q++) {
    const uint32_t f = threadIdx.x + q * blockDim.x;
    if (f < E) {
      if (mul[q]) v[q] = fmul(v[q], w[q]);
      U.put(((f & (G - 1)) << DEG) + (f >> log_g), v[q]);
    }
  }
}

template <class F, int DEG>
ECG_DEV void pass_store(F* __restrict__ y, const LdsPlanes<F>& U, uint32_t lgp, uint32_t log_g, uint32_t E) {
  constexpr uint32_t R = 1u << DEG;
  const uint64_t p = 1ull << lgp;
  const uint64_t g0 = (uint64_t)blockIdx.x << log_g;
  const uint32_t lpp = lgp < log_g ? lgp : log_g;  // lanes walk min(p, G) fastest -> contiguous runs
  const uint32_t pp = 1u << lpp;
#pragma unroll
  for (int q = 0; q < NTT_EPT; q++) {
    const uint32_t f = threadIdx.x + q * blockDim.x;
    if (f >= E) break;
    const uint32_t kk = f & (pp - 1);
    const uint32_t j = (f >> lpp) & (R - 1);
    const uint32_t gh = f >> (lpp + DEG);
    const uint32_t gi = (gh << lpp) + kk;
    const uint64_t g = g0 + gi;
    const uint64_t k = g & (p - 1);
    store(&y[((g - k) << DEG) + k + (uint64_t)j * p], U.get((gi << DEG) + bitrev(j, DEG)));
  }
}

// ---------------------------------------------------------------------------
// v2 pass: DEG <= 12, two DIF rounds per LDS round trip
// ---------------------------------------------------------------------------
// threads per workgroup = max(2^DEG, 1024) / 4 (see launch_pass)
template <class P, int DEG>
__global__ void __launch_bounds__(1024)
    ntt_pass_kernel(const Fp<P>* __restrict__ x, Fp<P>* __restrict__ y, const Fp<P>* __restrict__ pq,
                    uint32_t pq_shift, const Fp<P>* __restrict__ tw_lo, const Fp<P>* __restrict__ tw_hi,
                    const Fp<P>* __restrict__ twf, uint32_t log_n, uint32_t lgp, uint32_t log_g) {
  using F = Fp<P>;
  static_assert(F::L == 8, "NTT tiles assume 32-byte scalar-field elements");
  constexpr uint32_t R = 1u << DEG;
  extern __shared__ uint4 smem[];
  const uint32_t E = R << log_g;
  LdsPlanes<F> U{smem, smem + E};

  pass_load<F, DEG>(x, tw_lo, tw_hi, twf, U, log_n, lgp, log_g, E);
  __syncthreads();

  // radix-2^2 steps: rounds r and r+1 of the DIF network on quartets
  // {j, j+h, j+2h, j+3h} (h = bit/2, bit = R/2 >> r); root w = w_{2^DEG}.
  int r = 0;
  constexpr uint32_t RQ = R >= 4 ? R / 4 : 1;  // quartets per group
#pragma unroll 1
  for (; r + 1 < DEG; r += 2) {
    const uint32_t bit = (R / 2) >> r, h = bit >> 1;
    for (uint32_t f = threadIdx.x; f < E / 4; f += blockDim.x) {
      const uint32_t gi = f / RQ, q = f % RQ;
      const uint32_t qm = q & (h - 1);
      const uint32_t j = (gi << DEG) + ((q / h) * (2 * bit)) + qm;
      F e0 = U.get(j), e1 = U.get(j + h), e2 = U.get(j + bit), e3 = U.get(j + bit + h);
      // round r: (e0, e2) twiddle w^(qm << r), (e1, e3) twiddle w^((qm + h) << r)
      F s0 = fadd(e0, e2), d0 = fsub(e0, e2);
      F s1 = fadd(e1, e3), d1 = fsub(e1, e3);
      if (qm != 0) d0 = fmul(d0, load(&pq[(uint64_t)(qm << r) << pq_shift]));
      d1 = fmul(d1, load(&pq[(uint64_t)((qm + h) << r) << pq_shift]));
      // round r+1: pairs (s0, s1) and (d0, d1), both twiddle w^(qm << (r+1))
      F a0 = fadd(s0, s1), a1 = fsub(s0, s1);
      F b0 = fadd(d0, d1), b1 = fsub(d0, d1);
      if (qm != 0) {
        const F w2 = load(&pq[(uint64_t)(qm << (r + 1)) << pq_shift]);
        a1 = fmul(a1, w2);
        b1 = fmul(b1, w2);
      }
      U.put(j, a0);
      U.put(j + h, a1);
      U.put(j + bit, b0);
      U.put(j + bit + h, b1);
    }
    __syncthreads();
  }
  if (r < DEG) {  // odd DEG: last radix-2 round (bit = 1, all twiddles trivial)
    for (uint32_t f = threadIdx.x; f < E / 2; f += blockDim.x) {
      const uint32_t i0 = 2 * f;
      F u0 = U.get(i0), u1 = U.get(i0 + 1);
      U.put(i0, fadd(u0, u1));
      U.put(i0 + 1, fsub(u0, u1));
    }
    __syncthreads();
  }
  pass_store<F, DEG>(y, U, lgp, log_g, E);
}

// ---------------------------------------------------------------------------
// v1 pass (A/B): radix-2^8, one radix-2 round per LDS round trip, 256 threads
// ---------------------------------------------------------------------------
template <class P, int DEG>
__global__ void __launch_bounds__(256)
    ntt_pass_v1_kernel(const Fp<P>* __restrict__ x, Fp<P>* __restrict__ y, const Fp<P>* __restrict__ pq,
                       uint32_t pq_shift, const Fp<P>* __restrict__ tw_lo, const Fp<P>* __restrict__ tw_hi,
                       const Fp<P>* __restrict__ twf, uint32_t log_n, uint32_t lgp, uint32_t log_g) {
  using F = Fp<P>;
  constexpr uint32_t R = 1u << DEG;
  extern __shared__ uint4 smem[];
  const uint32_t E = R << log_g;
  LdsPlanes<F> U{smem, smem + E};
  pass_load<F, DEG>(x, tw_lo, tw_hi, twf, U, log_n, lgp, log_g, E);
  __syncthreads();
#pragma unroll 1
  for (int rnd = 0; rnd < DEG; rnd++) {
    const uint32_t bit = (R / 2) >> rnd;
    for (uint32_t f = threadIdx.x; f < E / 2; f += blockDim.x) {
      const uint32_t gi = f >> (DEG - 1), b = f & (R / 2 - 1);
      const uint32_t di = b & (bit - 1);
      const uint32_t i0 = (gi << DEG) + (b << 1) - di, i1 = i0 + bit;
      F u0 = U.get(i0), u1 = U.get(i1);
      F s = fadd(u0, u1);
      F d = fsub(u0, u1);
      if (di != 0) d = fmul(d, load(&pq[(uint64_t)(di << rnd) << pq_shift]));
      U.put(i0, s);
      U.put(i1, d);
    }
    __syncthreads();
  }
  pass_store<F, DEG>(y, U, lgp, log_g, E);
}

// Full inter-pass twiddle table of one pass: out[i * p + k] = w^((k i) << s),
// i < 2^deg, k < p = 2^lgp, s = log n - lgp - deg.
template <class P>
__global__ void ntt_fulltw_kernel(const Fp<P>* __restrict__ tw_lo, const Fp<P>* __restrict__ tw_hi, uint32_t lgp,
                                  uint32_t deg, uint32_t log_n, Fp<P>* __restrict__ out) {
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >> (lgp + deg)) return;
  const uint64_t k = idx & ((1ull << lgp) - 1), i = idx >> lgp;
  const uint64_t e = (k * i) << (log_n - lgp - deg);
  store(&out[idx], e ? twiddle(tw_lo, tw_hi, e) : Fp<P>::one());
}

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------
template <class P, int DEG, bool V1>
static hipError_t launch_pass(const PassArgs& a, hipStream_t s) {
  using F = Fp<P>;
  const uint32_t tile_log = V1 ? 10 : (DEG > ntt_tile_log() ? DEG : ntt_tile_log());  // elements per workgroup
  uint32_t log_g = tile_log - DEG;
  const uint32_t log_groups = a.log_n - DEG;
  if (log_g > log_groups) log_g = log_groups;
  const uint32_t E = 1u << (DEG + log_g);
  const uint64_t blocks = 1ull << (log_groups - log_g);
  const size_t lds = (size_t)2 * E * sizeof(uint4);
  uint32_t threads;
  if (V1) {
    threads = 256;
  } else {
    threads = E / NTT_EPT;
    if (threads < 64) threads = 64;
    if (threads > 1024) threads = 1024;
  }
  auto kern = V1 ? ntt_pass_v1_kernel<P, DEG> : ntt_pass_kernel<P, DEG>;
  static bool attr_set = false;  // > 64 KiB dynamic LDS needs an explicit opt-in
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(threads), lds, s, (const F*)a.x, (F*)a.y, (const F*)a.pq,
                     a.pq_shift, (const F*)a.tw_lo, (const F*)a.tw_hi, (const F*)a.twf, a.log_n, a.lgp, log_g);
  return hipGetLastError();
}


template <class Q, int DEG>
static hipError_t launch_pass_rr_io(bool in_rr, bool out_rr, const PassArgs& a, const RrTables& t, hipStream_t s) {
  if (in_rr) return out_rr ? launch_pass_rr<Q, DEG, true, true>(a, t, s) : launch_pass_rr<Q, DEG, true, false>(a, t, s);
  return out_rr ? launch_pass_rr<Q, DEG, false, true>(a, t, s) : launch_pass_rr<Q, DEG, false, false>(a, t, s);
}

template <class Q>
static hipError_t launch_pass_rr_deg(int deg, bool in_rr, bool out_rr, const PassArgs& a, const RrTables& t,
                                     hipStream_t s) {
  switch (deg) {
    case 1: return launch_pass_rr_io<Q, 1>(in_rr, out_rr, a, t, s);
    case 2: return launch_pass_rr_io<Q, 2>(in_rr, out_rr, a, t, s);
    case 3: return launch_pass_rr_io<Q, 3>(in_rr, out_rr, a, t, s);
    case 4: return launch_pass_rr_io<Q, 4>(in_rr, out_rr, a, t, s);
    case 5: return launch_pass_rr_io<Q, 5>(in_rr, out_rr, a, t, s);
    case 6: return launch_pass_rr_io<Q, 6>(in_rr, out_rr, a, t, s);
    case 7: return launch_pass_rr_io<Q, 7>(in_rr, out_rr, a, t, s);
    case 8: return launch_pass_rr_io<Q, 8>(in_rr, out_rr, a, t, s);
    case 9: return launch_pass_rr_io<Q, 9>(in_rr, out_rr, a, t, s);
    case 10: return launch_pass_rr_io<Q, 10>(in_rr, out_rr, a, t, s);
    case 11: return launch_pass_rr_io<Q, 11>(in_rr, out_rr, a, t, s);
    case 12: return launch_pass_rr_io<Q, 12>(in_rr, out_rr, a, t, s);
    default: return hipErrorInvalidValue;
  }
}

static bool ntt_rr_enabled() {  // reduced-radix butterflies (A/B: ECG_NTT_RR=0 keeps the 32-bit-limb passes)
  static bool v = [] {
    const char* e = getenv("ECG_NTT_RR");
    return !(e && e[0] == '0');
  }();
  return v;
}

template <class P, bool V1>
static hipError_t launch_pass_deg(int deg, const PassArgs& a, hipStream_t s) {
  switch (deg) {
    case 1: return launch_pass<P, 1, V1>(a, s);
    case 2: return launch_pass<P, 2, V1>(a, s);
    case 3: return launch_pass<P, 3, V1>(a, s);
    case 4: return launch_pass<P, 4, V1>(a, s);
    case 5: return launch_pass<P, 5, V1>(a, s);
    case 6: return launch_pass<P, 6, V1>(a, s);
    case 7: return launch_pass<P, 7, V1>(a, s);
    case 8: return launch_pass<P, 8, V1>(a, s);
    case 9: return V1 ? hipErrorInvalidValue : launch_pass<P, 9, false>(a, s);
    case 10: return V1 ? hipErrorInvalidValue : launch_pass<P, 10, false>(a, s);
    case 11: return V1 ? hipErrorInvalidValue : launch_pass<P, 11, false>(a, s);
    case 12: return V1 ? hipErrorInvalidValue : launch_pass<P, 12, false>(a, s);
    default: return hipErrorInvalidValue;
  }
}

static int ntt_variant() {
  static int v = [] {
    const char* e = getenv("ECG_NTT_VARIANT");
    return (e && e[0] == '1') ? 1 : 2;
  }();
  return v;
}

static bool ntt_full_twiddles() {  // per-pass full twiddle tables (A/B: ECG_NTT_FULLTW=0)
  static bool v = [] {
    const char* e = getenv("ECG_NTT_FULLTW");
    return !(e && e[0] == '0');
  }();
  return v;
}

static uint32_t ntt_max_deg() {  // largest radix exponent per pass (v2), tunable for A/B
  static uint32_t d = [] {
    const char* e = getenv("ECG_NTT_MAXDEG");
    int v = e ? atoi(e) : 10;
    return (uint32_t)(v < 2 ? 2 : v > 12 ? 12 : v);
  }();
  return d;
}

// Pass degrees: v2 splits log n into ceil(log n / maxdeg) balanced passes;
// v1 uses radix-2^8 passes like the reference (fft.rs:101-102).
static int plan_passes(uint32_t log_n, int variant, uint32_t* degs) {
  if (variant == 1) {
    int np = 0;
    for (uint32_t lgp = 0; lgp < log_n;) {
      const uint32_t d = log_n - lgp < 8 ? log_n - lgp : 8;
      degs[np++] = d;
      lgp += d;
    }
    return np;
  }
  const uint32_t md = ntt_max_deg();
  const int np = (int)((log_n + md - 1) / md);
  for (int k = 0; k < np; k++) degs[k] = log_n / np + ((uint32_t)k < log_n % np ? 1 : 0);
  return np;
}

template <class P, class Q>
static int ntt_run_t(ecg_ctx* ctx, int field_id, void* d_data, const uint64_t* omega, uint32_t log_n,
                     hipStream_t s, ecg_abort_cb abort_cb, void* user, uint32_t batch = 1) {
  using F = Fp<P>;
  const int variant = ntt_variant();
  uint32_t degs[40];
  const int np = plan_passes(log_n, variant, degs);
  uint32_t max_deg = 0;
  for (int k = 0; k < np; k++) max_deg = degs[k] > max_deg ? degs[k] : max_deg;

  const uint64_t n = 1ull << log_n;
  const uint64_t lo_cnt = 1ull << NTT_LO_BITS;
  const uint64_t hi_cnt = n > lo_cnt ? (n >> NTT_LO_BITS) : 1;
  const uint64_t pq_cnt = max_deg > 1 ? 1ull << (max_deg - 1) : 1;

  // full per-pass tables (passes after the first): sum of 2^(lgp + deg) <= 2n entries
  const bool full = ntt_full_twiddles() && log_n <= 28 && np > 1;
  // reduced-radix passes need the full tables (their twiddles are one load each)
  const bool rr = ntt_rr_enabled() && variant == 2 && (np == 1 || full) && (1u << (max_deg > ntt_tile_log() ? max_deg : ntt_tile_log())) <= 4 * NTT_RR_THREADS;
  // bytes per element between passes: the plane layout for the reduced-radix
  // passes, the boundary layout otherwise
  const size_t elem = rr ? RR_PLANE_BYTES : sizeof(F);
  if (batch > 1 && !rr) {  // batched launches are a reduced-radix feature: one transform at a time
    for (uint32_t b = 0; b < batch; b++)
      ECG_TRY((ntt_run_t<P, Q>(ctx, field_id, (F*)d_data + b * n, omega, log_n, s, abort_cb, user, 1)));
    return ECG_OK;
  }

  void *scratch = nullptr, *scratch2 = nullptr, *tables;
  if (np > 1 || variant == 1) ECG_TRY(ws_get(ctx, "ntt_scratch", batch * n * elem, &scratch));
  // odd pass counts (> 1) rotate through a second scratch buffer so the last
  // pass writes d_data directly (no copy back; HBM is plentiful); the
  // reduced-radix inner passes always rotate two (planes do not fit d_data)
  if (np > 1 && ((np & 1) || (rr && np > 2))) ECG_TRY(ws_get(ctx, "ntt_scratch2", batch * n * elem, &scratch2));
  ECG_TRY(ws_get(ctx, "ntt_tables", (pq_cnt + lo_cnt + hi_cnt) * sizeof(F), &tables));
  F* pq = (F*)tables;
  F* tw_lo = pq + pq_cnt;
  F* tw_hi = tw_lo + lo_cnt;

  F* twf[40] = {nullptr};
  uint64_t twf_off[40] = {0}, twf_tot = 0;
  if (full) {
    uint32_t lg = 0;
    for (int k = 0; k < np; k++) {
      if (k > 0) {
        twf_off[k] = twf_tot;
        twf_tot += 1ull << (lg + degs[k]);
      }
      lg += degs[k];
    }
    void* t;
    ECG_TRY(ws_get(ctx, "ntt_twf", twf_tot * sizeof(F), &t));
    for (int k = 1; k < np; k++) twf[k] = (F*)t + twf_off[k];
  }
  // the reduced-radix passes' twiddles: w R' as planes of exact canonical limbs
  void *pq_rr = nullptr, *twf_rr = nullptr;
  if (rr) {
    ECG_TRY(ws_get(ctx, "ntt_pq_rr", pq_cnt * RR_PLANE_BYTES, &pq_rr));
    if (full) ECG_TRY(ws_get(ctx, "ntt_twf_rr", twf_tot * RR_PLANE_BYTES, &twf_rr));
  }

  const bool cached = ctx->tw_fid == field_id && ctx->tw_log_n == log_n && ctx->tw_variant == variant &&
                      ctx->tw_full == (int)full + 2 * (int)rr &&
                      memcmp(ctx->tw_omega, omega, sizeof(ctx->tw_omega)) == 0;
  if (!cached) {
    F w;
    memcpy(w.v, omega, sizeof(w.v));
    // pq[j] = w^(j * (n >> max_deg)) (fft.rs:68-78); tw_lo[j] = w^j; tw_hi[j] = w^(j << 12)
    hipLaunchKernelGGL(ntt_powers_kernel<P>, dim3((uint32_t)((pq_cnt + 255) / 256)), dim3(256), 0, s, w,
                       log_n - max_deg, pq_cnt, pq);
    hipLaunchKernelGGL(ntt_powers_kernel<P>, dim3((uint32_t)((lo_cnt + 255) / 256)), dim3(256), 0, s, w, 0u,
                       lo_cnt, tw_lo);
    hipLaunchKernelGGL(ntt_powers_kernel<P>, dim3((uint32_t)((hi_cnt + 255) / 256)), dim3(256), 0, s, w,
                       (uint32_t)NTT_LO_BITS, hi_cnt, tw_hi);
    if (full) {
      uint32_t lg = 0;
      for (int k = 0; k < np; k++) {
        if (k > 0) {
          const uint64_t cnt = 1ull << (lg + degs[k]);
          hipLaunchKernelGGL(ntt_fulltw_kernel<P>, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, s, tw_lo,
                             tw_hi, lg, degs[k], log_n, twf[k]);
        }
        lg += degs[k];
      }
    }
    if (rr) {
      hipLaunchKernelGGL(ntt_tab_to_rr_kernel<Q>, dim3((uint32_t)((pq_cnt + 255) / 256)), dim3(256), 0, s, pq,
                         pq_cnt, (uint4*)pq_rr);
      if (full)
        hipLaunchKernelGGL(ntt_tab_to_rr_kernel<Q>, dim3((uint32_t)((twf_tot + 255) / 256)), dim3(256), 0, s,
                           twf[1], twf_tot, (uint4*)twf_rr);
    }
    ECG_HIP(hipGetLastError());
    ctx->tw_fid = field_id;
    ctx->tw_log_n = log_n;
    ctx->tw_variant = variant;
    ctx->tw_full = (int)full + 2 * (int)rr;
    memcpy(ctx->tw_omega, omega, sizeof(ctx->tw_omega));
  }

  kt_reset(ctx, "ntt_pass");
  // Single-pass v2 transforms (log n <= 12) have one workgroup reading every
  // element before any write: safe in place.  Otherwise ping-pong, arranged so
  // the last pass lands in d_data whenever the pass count is even.
  void* bufs[41];
  bufs[0] = d_data;
  for (int k = 1; k <= np; k++) {
    if (variant == 1) bufs[k] = (k & 1) ? scratch : d_data;       // ping-pong + copy back (fft.rs:126)
    else if (np == 1) bufs[k] = d_data;                            // one workgroup: in place
    else if (k == np) bufs[k] = d_data;                            // last pass lands in place
    else if (rr) bufs[k] = (k & 1) ? scratch : scratch2;           // planes: two scratches
    else if (np & 1) bufs[k] = (k & 1) ? scratch : scratch2;       // odd: rotate two scratches
    else bufs[k] = (k & 1) ? scratch : d_data;                     // even: ping-pong
  }
  uint32_t lgp = 0;
  for (int k = 0; k < np; k++) {
    if (abort_cb && abort_cb(user)) return ECG_ABORTED;  // fft.rs:94-98
    const PassArgs a{bufs[k], bufs[k + 1], pq, max_deg - degs[k], tw_lo, tw_hi, twf[k], log_n, lgp, batch};
    ECG_TRY(kt_begin(ctx, "ntt_pass", s));
    hipError_t e;
    if (rr) {
      const RrTables t{pq_rr, (uint32_t)pq_cnt, twf_rr, twf_tot, twf_off[k]};
      e = launch_pass_rr_deg<Q>((int)degs[k], k > 0, k + 1 < np, a, t, s);
    }
    else
      e = variant == 1 ? launch_pass_deg<P, true>((int)degs[k], a, s) : launch_pass_deg<P, false>((int)degs[k], a, s);
    ECG_HIP(e);
    ECG_TRY(kt_end(ctx, "ntt_pass", s));
    lgp += degs[k];
  }
  if (bufs[np] != d_data)
    ECG_HIP(hipMemcpyAsync(d_data, bufs[np], batch * n * sizeof(F), hipMemcpyDeviceToDevice, s));
  return ECG_OK;
}

// The conditions under which ntt_run_t takes the reduced-radix passes.
int ntt_rr_plan(uint32_t log_n, uint32_t* degs) {
  if (!ntt_rr_enabled() || ntt_variant() != 2) return 0;
  const int np = plan_passes(log_n, 2, degs);
  uint32_t max_deg = 0;
  for (int k = 0; k < np; k++) max_deg = degs[k] > max_deg ? degs[k] : max_deg;
  if (np > 1 && !(ntt_full_twiddles() && log_n <= 28)) return 0;
  if ((1u << (max_deg > ntt_tile_log() ? max_deg : ntt_tile_log())) > 4 * NTT_RR_THREADS) return 0;
  return np;
}

hipError_t ntt_launch_plain_rr(int field_id, int deg, bool in_rr, bool out_rr, const PassArgs& a, const RrTables& t,
                               hipStream_t s) {
  return field_id == ECG_FIELD_BLS12_381_FR ? launch_pass_rr_deg<params::bls12_381_fr_rr>(deg, in_rr, out_rr, a, t, s)
                                            : launch_pass_rr_deg<params::bn254_fr_rr>(deg, in_rr, out_rr, a, t, s);
}

int ntt_validate(int field_id, uint32_t log_n) {
  uint32_t adic;
  switch (field_id) {
    case ECG_FIELD_BLS12_381_FR: adic = params::bls12_381_fr::TWO_ADICITY; break;
    case ECG_FIELD_BN254_FR: adic = params::bn254_fr::TWO_ADICITY; break;
    default:
      set_error("radix_fft: field_id %d is not an FFT-friendly scalar field", field_id);
      return ECG_ERR_INVALID;
  }
  if (log_n == 0) {
    set_error("radix_fft: log_n must be >= 1");  // the reference panics (fft.rs:68-70)
    return ECG_ERR_INVALID;
  }
  if (log_n > adic || log_n > 32) {
    set_error("radix_fft: log_n %u exceeds the field's two-adicity %u", log_n, adic);
    return ECG_ERR_INVALID;
  }
  return ECG_OK;
}

int ntt_run(ecg_ctx* ctx, int field_id, void* d_data, const uint64_t* omega, uint32_t log_n, hipStream_t s,
            ecg_abort_cb abort_cb, void* user, uint32_t batch) {
  ECG_TRY(ntt_validate(field_id, log_n));
  if (batch == 0) return ECG_OK;
  switch (field_id) {
    case ECG_FIELD_BLS12_381_FR:
      return ntt_run_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, field_id, d_data, omega, log_n, s,
                                                                       abort_cb, user, batch);
    default:
      return ntt_run_t<params::bn254_fr, params::bn254_fr_rr>(ctx, field_id, d_data, omega, log_n, s, abort_cb,
                                                               user, batch);
  }
}

}  // namespace ecg
