// Shared templates of the Stockham NTT (ntt.hip: the plain transform;
// ntt_ext.hip: the shifted / scaled transform): the reduced-radix pass kernel,
// its plane layout, the table kernels and the launch helper.
#pragma once
#include <cstdlib>

#include "ctx.hpp"
#include "field.hpp"
#include "fieldrr.hpp"

namespace ecg {

constexpr int NTT_LO_BITS = 12;  // twiddle split table size 2^12

ECG_DEV uint32_t bitrev(uint32_t x, int bits) { return __builtin_bitreverse32(x) >> (32 - bits); }

// twiddle w^e for e < n from the split tables
template <class F>
ECG_DEV F twiddle(const F* __restrict__ tw_lo, const F* __restrict__ tw_hi, uint64_t e) {
  return fmul(load(&tw_hi[e >> NTT_LO_BITS]), load(&tw_lo[e & ((1u << NTT_LO_BITS) - 1)]));
}

// A thread owns at most NTT_EPT elements of the tile (launch: threads >= E /
// NTT_EPT).  Every global load of the tile -- elements and twiddles -- is
// issued before the first product, so a tile waits for one HBM latency, not
// one per element (the strided loop over a runtime bound could not unroll).
constexpr int NTT_EPT = 4;

// ---------------------------------------------------------------------------
// Reduced-radix pass (default for both scalar fields): the same Stockham
// schedule, with the butterflies in the 9 x 29-bit form of fieldrr.hpp.  An
// Fr product is then 162 v_mad_u64_u32 and no carry instructions (the 32-bit
// form of ntt.hip issues 128 mads + 128 addc + the final subtraction), and
// sums / differences are limb-wise with no carry chain.
//
// No conversion product anywhere: the caller's word x R (< r) is re-read as a
// 9-limb integer, i.e. as the reduced-radix form of x R / R' (R' = 2^261).
// The transform is linear, so the output integers are y R / R' * R' = y R --
// exactly the boundary form -- once packed back into 8 words.  Twiddles are
// stored in the R' form (converted once when the tables are built).
//
// Values between butterfly rounds ("E-form"): exact limbs, value <= 2.5 r.
// A radix-2^2 step on e0..e3 (r / R' <= 2^-6.1; products take one operand
// with un-carried limbs -- NttLimbs<Q> (fieldrr.hpp) derives their bounds from
// the K p rows: up to 2 (2^29 - 1) + max(16p row) = 2.5 x 2^30 = 2^31.33 --
// against an exact twiddle and return < r (1 + K 2^-6.1)).  Eight such limbs
// against a twiddle's eight limbs of up to 2^29 - 1 put 1.20 x 2^63 into
// column 7 (s0 + 16r - s1; 1.16 x 2^63 for s0 + s1), which BLS12-381's signed
// ceil-carry chains misread, so every product of an un-carried operand names
// its limb bound (rr_mul2<NttLimbs<Q>::PF>) and runs in the unsigned general
// column form (tests/test_rr_contracts.py replays each call site):
//   s0 = e0 + e2, d0 = (e0 + 8r - e2) w0        (<= 5 r,  <= 1.15 r)
//   s1 = e1 + e3, d1 = (e1 + 8r - e3) w1
//   a0 = reduce_q(s0 + s1)                      (<= 1.1 r)
//   a1 = (s0 + 16r - s1) w2                     (<= 1.3 r)
//   b0 = carry(d0 + d1)                         (<= 2.3 r)
//   b1 = (d0 + 4r - d1) w2                      (<= 1.1 r)
// The last step of a pass (h = 1: three of its four twiddles are 1, or the
// radix-2 round of an odd DEG) leaves its outputs unreduced ("P-form": limbs
// <= NttLimbs<Q>::PF < 2^31.4, value <= 21 r): they meet a product next -- the
// following pass multiplies every element by its twiddle first, and a product
// of such an operand with an exact twiddle is < r (1 + 21 * 2^-6.1) < 1.4 r
// with exact limbs (column sums < 9 2^60.4 + 9 2^58 < 2^64, unsigned: the
// general column form, see above) -- or rr_store_std's
// reduce_q (limbs < 2^31.4, value < 64 r).  The first pass reads canonical
// input and has no twiddle product, so P-form values never enter a sum.
//
// HBM layout: the transform's input and output are the boundary layout
// (canonical, 8 packed words).  Between passes the elements stay in the
// P-form as three planes (limbs 0-3 | 4-7 | 8: 36 B per element, coalesced
// 16-B / 4-B accesses), so an inner pass boundary costs no unpacking,
// reduction, canonicalisation or packing (~125 VALU instructions per element
// saved for 4 more bytes).  The twiddle tables are planes of exact canonical
// limbs for the same reason.
//
// Shifted / scaled transform (ntt_ext.hip, DESIGN.md "Inverse and coset NTT"):
// y[k] = c t^k sum_j s^j a[j] w^(jk).  Every factor but two small ones is
// folded into the full per-pass tables; what is left is
//   MUL_IN  (first pass only, lgp = 0): u[i] = x[g + i t] * IN0[i],
//           IN0[i] = s^(i << s_0), read where later passes read TW (the
//           table index i p + k is i for p = 1).  Canonical input times an
//           exact canonical entry: < r (1 + 2^-6.1), exact limbs -- inside
//           the E-form, as the canonical input itself is.
//   MUL_OUT (last pass only): y[..] = v[jj] * OUT[jj] before rr_store_std,
//           OUT[jj] = c t^(jj << lgp), stored right behind the pass's own
//           table (entry 2^(lgp + DEG) of TW).  v is in the P-form (limbs <
//           2^31.4, value <= 21 r), the same operand the next pass's twiddle
//           product takes: the product is < 1.4 r with exact limbs, and
//           rr_store_std's reduce_q (limbs < 2^31.4, value < 64 r) takes it.
// Both are compile-time flags: the plain instantiations keep their code.
// ---------------------------------------------------------------------------
template <class Q>
struct RrPlanes {  // limbs 0-3 | 4-7 | 8 of element i (NL = 9)
  uint4* a;
  uint4* b;
  uint32_t* c;
  ECG_HD static RrPlanes over(void* base, size_t n) {
    uint4* p = reinterpret_cast<uint4*>(base);
    return RrPlanes{p, p + n, reinterpret_cast<uint32_t*>(p + 2 * n)};
  }
  ECG_HD RrPlanes at(size_t off) const { return RrPlanes{a + off, b + off, c + off}; }
  ECG_DEV FpR<Q> get(size_t i) const {
    static_assert(Q::NL == 9, "three planes hold 9 limbs");
    const uint4 x = a[i], y = b[i];
    FpR<Q> r;
    r.v[0] = x.x; r.v[1] = x.y; r.v[2] = x.z; r.v[3] = x.w;
    r.v[4] = y.x; r.v[5] = y.y; r.v[6] = y.z; r.v[7] = y.w;
    r.v[8] = c[i];
    return r;
  }
  ECG_DEV void put(size_t i, const FpR<Q>& v) const {
    a[i] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
    b[i] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
    c[i] = v.v[8];
  }
};
constexpr size_t RR_PLANE_BYTES = 36;  // bytes per element in the plane layout

template <class Q>
ECG_DEV FpR<Q> rr_load_std(const uint4* __restrict__ x, size_t i) {  // 8 words x R -> 9 exact limbs
  const uint4 lo = x[2 * i], hi = x[2 * i + 1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  FpR<Q> r;
  rr_unpack<Q, 8>(w, r.v);
  return r;
}

template <class Q>
ECG_DEV void rr_store_std(uint4* __restrict__ y, size_t i, const FpR<Q>& v) {  // E-form -> canonical 8 words
  const FpR<Q> c = rr_canon_lt2p(rr_reduce_q(v));
  uint32_t w[8];
  rr_pack<Q, 8>(c.v, w);
  y[2 * i] = make_uint4(w[0], w[1], w[2], w[3]);
  y[2 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// LDS layout: the three planes, unswizzled.  A linear XOR swizzle of the
// element slots (found by a bank simulation of every access pattern of the
// 1024-element tiles) cut SQ_LDS_BANK_CONFLICT from 1354 to 96 cycles per wave
// but left the pass time unchanged and added ~3% VALU instructions for the
// slot arithmetic: the pass is VALU-issue-bound (SQ_INSTS_VALU x 4 cycles ~
// 0.94 of the wave cycles at 4 waves/SIMD), not LDS-bound
// (profiles/r02b/ntt_lds_swizzle.txt).
ECG_HD constexpr uint32_t lds_phys(uint32_t j) { return j; }

// Up to 1024 threads (4096-element tiles, 147 KB of LDS: the 2-pass 2^24
// schedule of ECG_NTT_MAXDEG=12); 4 waves/SIMD bound the kernel to 128 VGPRs
// either way.
constexpr uint32_t NTT_RR_THREADS = 1024;

#ifndef ECG_NTT_RR_WAVES
#define ECG_NTT_RR_WAVES 4
#endif
// IN_RR / OUT_RR: the pass reads / writes the plane layout (inner pass
// boundaries) instead of the boundary layout.  MUL_IN / MUL_OUT: the load-side
// / store-side product of the shifted transform (see the header above).
template <class Q, int DEG, bool IN_RR, bool OUT_RR, bool MUL_IN = false, bool MUL_OUT = false>
__global__ void __launch_bounds__(NTT_RR_THREADS) __attribute__((amdgpu_waves_per_eu(ECG_NTT_RR_WAVES)))
    ntt_pass_rr_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, const uint4* __restrict__ pq_base,
                       uint32_t pq_cnt, uint32_t pq_shift, const uint4* __restrict__ twf_base, uint64_t twf_cnt,
                       uint64_t twf_off, uint32_t log_n, uint32_t lgp, uint32_t log_g, uint32_t xcd_runs,
                       uint32_t log_tiles) {
  static_assert(!(MUL_IN && IN_RR) && !(MUL_OUT && OUT_RR), "the shift products sit at the transform's boundary");
  using F = FpR<Q>;
  constexpr uint32_t R = 1u << DEG;
  // limb bounds of the products' first operands: the P-form (and, below it,
  // every un-carried butterfly difference); a first pass loads canonical limbs
  constexpr uint32_t PF = NttLimbs<Q>::PF, AIN = IN_RR ? PF : 0;
  extern __shared__ uint4 smem[];
  const uint32_t E = R << log_g;
  const RrPlanes<Q> U = RrPlanes<Q>::over(smem, E);
  const uint32_t G = 1u << log_g;
  const size_t n = (size_t)1 << log_n;
  // XCD-aware tile order (xcd_runs): blocks b and b + 8 share an XCD (round-robin
  // dispatch), so XCD b % 8 takes a contiguous run of tiles.  Neighbouring tiles
  // share the 128-B lines of the planes (4 columns of 16 + 16 + 4 B per tile
  // row) and now meet in one L2 instead of fetching each line once per XCD.
  const uint32_t tile_all = xcd_runs ? (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  // batched transforms (radix_fft_many): transform tile_all >> log_tiles of the
  // batch, stored back to back in the input's and the output's layout
  const uint32_t tile = tile_all & ((1u << log_tiles) - 1);
  const size_t tix = tile_all >> log_tiles;
  x += tix * (IN_RR ? ((size_t)9 << log_n) / 4 : (size_t)2 << log_n);  // 36 B or 32 B per element, in uint4
  y += tix * (OUT_RR ? ((size_t)9 << log_n) / 4 : (size_t)2 << log_n);
  const uint64_t g0 = (uint64_t)tile << log_g;
  const RrPlanes<Q> PQ = RrPlanes<Q>::over(const_cast<uint4*>(pq_base), pq_cnt);

  // ---- load: u[i] = x[g + i t] * w^((n >> (lgp + DEG)) k i) (full per-pass table)
  {
    const uint64_t t = n >> DEG;
    const uint64_t p = 1ull << lgp;
    F v[NTT_EPT];
#pragma unroll
    for (int q = 0; q < NTT_EPT; q++) {
      const uint32_t f = threadIdx.x + q * blockDim.x;
      v[q] = F::zero();
      if (f < E) {
        const uint64_t src = g0 + (f & (G - 1)) + (uint64_t)(f >> log_g) * t;
        if constexpr (IN_RR)
          v[q] = RrPlanes<Q>::over(const_cast<uint4*>(x), n).get(src);
        else
          v[q] = rr_load_std<Q>(x, src);
      }
    }
    // every element times its twiddle (w^0 = 1 is a table entry too: no
    // divergence); MUL_IN: the first pass (p = 1) reads IN0[i] at the same index
    if (MUL_IN || lgp != 0) {
      const RrPlanes<Q> TW = RrPlanes<Q>::over(const_cast<uint4*>(twf_base), twf_cnt).at(twf_off);
      F w[NTT_EPT];
#pragma unroll
      for (int q = 0; q < NTT_EPT; q++) {
        const uint32_t f = threadIdx.x + q * blockDim.x;
        const uint64_t g = g0 + (f & (G - 1));
        w[q] = f < E ? TW.get((uint64_t)(f >> log_g) * p + (g & (p - 1))) : F::one();
      }
#pragma unroll
      for (int q = 0; q + 1 < NTT_EPT; q += 2) {
        F p0, p1;
        rr_mul2<AIN>(v[q], w[q], v[q + 1], w[q + 1], p0, p1);
        v[q] = p0;
        v[q + 1] = p1;
      }
    }
#pragma unroll
    for (int q = 0; q < NTT_EPT; q++) {
      const uint32_t f = threadIdx.x + q * blockDim.x;
      if (f < E) U.put(lds_phys(((f & (G - 1)) << DEG) + (f >> log_g)), v[q]);
    }
  }
  __syncthreads();

  // ---- radix-2^2 steps (rounds r, r+1 of the DIF network)
  int r = 0;
  constexpr uint32_t RQ = R >= 4 ? R / 4 : 1;
#pragma unroll 1
  for (; r + 1 < DEG; r += 2) {
    const uint32_t bit = (R / 2) >> r, h = bit >> 1;
    // slots of the quartet offsets h, bit, bit + h (disjoint from j's bits)
    const uint32_t oh = lds_phys(h), ob = lds_phys(bit), obh = lds_phys(bit + h);
    for (uint32_t f = threadIdx.x; f < E / 4; f += blockDim.x) {
      const uint32_t gi = f / RQ, q = f % RQ;
      const uint32_t qm = q & (h - 1);
      const uint32_t j = (gi << DEG) + ((q / h) * (2 * bit)) + qm;
      const uint32_t pj = lds_phys(j);
      const F e0 = U.get(pj), e1 = U.get(pj ^ oh), e2 = U.get(pj ^ ob), e3 = U.get(pj ^ obh);
      const F s0 = rr_add_nc(e0, e2), s1 = rr_add_nc(e1, e3);
      F a0, a1, b0, b1;
      if (h > 1) {
        F d0, d1, a1p, b1p;
        rr_mul2<PF>(rr_sub_nc<8>(e0, e2), PQ.get((size_t)(qm << r) << pq_shift), rr_sub_nc<8>(e1, e3),
                PQ.get((size_t)((qm + h) << r) << pq_shift), d0, d1);
        a0 = rr_reduce_q(rr_add_nc(s0, s1));
        b0 = rr_carry_seq(rr_add_nc(d0, d1));
        const F w2 = PQ.get((size_t)(qm << (r + 1)) << pq_shift);
        rr_mul2<PF>(rr_sub_nc<16>(s0, s1), w2, rr_sub_nc<4>(d0, d1), w2, a1p, b1p);
        a1 = a1p;
        b1 = b1p;
      } else {  // h = 1 (the pass's last step): qm = 0, only d1's twiddle w^(1 << r) is non-trivial
        const F d0 = rr_reduce_q(rr_sub_nc<8>(e0, e2));
        const F d1 = rr_mul<PF>(rr_sub_nc<8>(e1, e3), PQ.get((size_t)(1u << r) << pq_shift));
        // Left unreduced ("P-form", see the header): every consumer -- the
        // next pass's twiddle product or rr_store_std's reduce_q -- takes
        // limbs < 2^31.4 and values < 64 r.
        a0 = rr_add_nc(s0, s1);      // <= 10 r, limbs <= NttLimbs::A0 = 2^31 - 4
        a1 = rr_sub_nc<16>(s0, s1);  // <= 21 r, limbs <= NttLimbs::A1 = 2^30 - 2 + max(16p row) < 2.5 x 2^30
        b0 = rr_add_nc(d0, d1);      // <= 2.3 r, limbs <= NttLimbs::S
        b1 = rr_sub_nc<4>(d0, d1);   // <= 5.2 r, limbs <= NttLimbs::B1 = 2^29 - 1 + max(4p row) < 2^31
      }
      U.put(pj, a0);
      U.put(pj ^ oh, a1);
      U.put(pj ^ ob, b0);
      U.put(pj ^ obh, b1);
    }
    __syncthreads();
  }
  if (r < DEG) {  // odd DEG: last radix-2 round (bit = 1, trivial twiddles), outputs in the P-form
    for (uint32_t f = threadIdx.x; f < E / 2; f += blockDim.x) {
      const uint32_t p0 = lds_phys(2 * f);  // phys(2f + 1) = phys(2f) ^ 1
      const F u0 = U.get(p0), u1 = U.get(p0 ^ 1);
      U.put(p0, rr_add_nc(u0, u1));           // <= 5 r
      U.put(p0 ^ 1, rr_sub_nc<8>(u0, u1));    // <= 10.5 r, limbs <= NttLimbs::D < 2^31
    }
    __syncthreads();
  }

  // ---- store: y[(g - k) 2^DEG + k + j 2^lgp] = v[j] (natural order)
  {
    const uint64_t p = 1ull << lgp;
    const uint32_t lpp = lgp < log_g ? lgp : log_g;
    const uint32_t pp = 1u << lpp;
    // element f of the tile: its LDS slot, output digit jj and destination
    auto place = [&](uint32_t f, uint32_t& slot, uint32_t& jj, size_t& dst) {
      const uint32_t kk = f & (pp - 1);
      jj = (f >> lpp) & (R - 1);
      const uint32_t gh = f >> (lpp + DEG);
      const uint32_t gi = (gh << lpp) + kk;
      const uint64_t g = g0 + gi;
      const uint64_t k = g & (p - 1);
      dst = ((g - k) << DEG) + k + (uint64_t)jj * p;
      slot = lds_phys((gi << DEG) + bitrev(jj, DEG));
    };
    if constexpr (MUL_OUT) {
      // v (P-form: limbs < 2^31.4, <= 21 r) times the exact OUT[jj]: < 1.4 r,
      // exact limbs -- inside rr_store_std's reduce_q bound (< 64 r)
      const RrPlanes<Q> OUT =
          RrPlanes<Q>::over(const_cast<uint4*>(twf_base), twf_cnt).at(twf_off + ((uint64_t)R << lgp));
      F v[NTT_EPT], w[NTT_EPT];
      size_t dst[NTT_EPT];
#pragma unroll
      for (int q = 0; q < NTT_EPT; q++) {
        const uint32_t f = threadIdx.x + q * blockDim.x;
        v[q] = F::zero();
        w[q] = F::one();
        dst[q] = 0;
        if (f < E) {
          uint32_t slot, jj;
          place(f, slot, jj, dst[q]);
          v[q] = U.get(slot);
          w[q] = OUT.get(jj);
        }
      }
#pragma unroll
      for (int q = 0; q + 1 < NTT_EPT; q += 2) {
        F p0, p1;
        rr_mul2<PF>(v[q], w[q], v[q + 1], w[q + 1], p0, p1);
        v[q] = p0;
        v[q + 1] = p1;
      }
#pragma unroll
      for (int q = 0; q < NTT_EPT; q++) {
        const uint32_t f = threadIdx.x + q * blockDim.x;
        if (f < E) rr_store_std<Q>(y, dst[q], v[q]);
      }
    } else {
#pragma unroll
      for (int q = 0; q < NTT_EPT; q++) {
        const uint32_t f = threadIdx.x + q * blockDim.x;
        if (f >= E) break;
        uint32_t slot, jj;
        size_t dst;
        place(f, slot, jj, dst);
        const F v = U.get(slot);
        if constexpr (OUT_RR)
          RrPlanes<Q>::over(y, n).put(dst, v);  // P-form: the next pass multiplies it by its twiddle first
        else
          rr_store_std<Q>(y, dst, v);
      }
    }
  }
}

// boundary-form table entries w R -> w R' as planes of exact canonical limbs
template <class Q>
__global__ void ntt_tab_to_rr_kernel(const Fp<typename Q::Base>* __restrict__ in, uint64_t cnt, uint4* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  RrPlanes<Q>::over(out, cnt).put(i, rr_canon_lt2p(rr_reduce_q(rr_from_std<Q>(load(&in[i])))));
}

// out[j] = w^(j << shift), j < count  (w given by value, Montgomery)
template <class P>
__global__ void ntt_powers_kernel(Fp<P> w, uint32_t shift, uint64_t count, Fp<P>* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  Fp<P> base = w;
  for (uint32_t s = 0; s < shift; s++) base = fsqr(base);  // base = w^(2^shift)
  Fp<P> r = Fp<P>::one();
  uint64_t e = j;
  while (e) {
    if (e & 1) r = fmul(r, base);
    e >>= 1;
    if (e) base = fsqr(base);
  }
  store(&out[j], r);
}

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------
struct PassArgs {
  const void* x;
  void* y;
  const void* pq;
  uint32_t pq_shift;
  const void* tw_lo;
  const void* tw_hi;
  const void* twf;  // full table of this pass, or null
  uint32_t log_n, lgp;
  uint32_t batch = 1;  // transforms back to back (reduced-radix passes only)
};

// A/B knob: log2 elements per workgroup (ECG_NTT_TILE, default 10)
static uint32_t ntt_tile_log() {
  static uint32_t v = [] {
    const char* e = getenv("ECG_NTT_TILE");
    return e ? (uint32_t)atoi(e) : 10u;
  }();
  return v;
}

static bool ntt_xcd_runs() {  // XCD-aware tile order (A/B: ECG_NTT_XCD=0 keeps blockIdx order)
  static bool v = [] {
    const char* e = getenv("ECG_NTT_XCD");
    return !(e && e[0] == '0');
  }();
  return v;
}

// Tables of the reduced-radix passes (planes): pq (cnt entries) and the full
// per-pass twiddles (twf_cnt entries over all passes, this pass at twf_off).
struct RrTables {
  const void* pq;
  uint32_t pq_cnt;
  const void* twf;
  uint64_t twf_cnt, twf_off;
};

template <class Q, int DEG, bool IN_RR, bool OUT_RR, bool MUL_IN = false, bool MUL_OUT = false>
static hipError_t launch_pass_rr(const PassArgs& a, const RrTables& t, hipStream_t s) {
  const uint32_t tile_log = DEG > ntt_tile_log() ? DEG : ntt_tile_log();
  uint32_t log_g = tile_log - DEG;
  const uint32_t log_groups = a.log_n - DEG;
  if (log_g > log_groups) log_g = log_groups;
  const uint32_t E = 1u << (DEG + log_g);
  const uint64_t blocks = 1ull << (log_groups - log_g);
  const size_t lds = (size_t)E * RR_PLANE_BYTES;
  uint32_t threads = E / NTT_EPT;
  if (threads < 64) threads = 64;
  if (threads > NTT_RR_THREADS) return hipErrorInvalidValue;  // tiles of <= 4096 elements only
  auto kern = ntt_pass_rr_kernel<Q, DEG, IN_RR, OUT_RR, MUL_IN, MUL_OUT>;
  static bool attr_set = false;  // > 64 KiB dynamic LDS needs an explicit opt-in
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const uint64_t grid = blocks * a.batch;
  uint32_t log_tiles = 0;
  while ((1ull << log_tiles) < blocks) log_tiles++;
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(threads), lds, s, (const uint4*)a.x, (uint4*)a.y,
                     (const uint4*)t.pq, t.pq_cnt, a.pq_shift, (const uint4*)t.twf, t.twf_cnt, t.twf_off, a.log_n,
                     a.lgp, log_g, (uint32_t)(ntt_xcd_runs() && grid >= 8 && grid % 8 == 0), log_tiles);
  return hipGetLastError();
}

// ntt.hip, for ntt_ext.hip: the pass degrees of a 2^log_n transform when the
// reduced-radix passes serve it (returns the pass count), 0 otherwise; and
// the launch of a plain reduced-radix pass (the instantiations live in ntt.hip).
int ntt_rr_plan(uint32_t log_n, uint32_t* degs);
hipError_t ntt_launch_plain_rr(int field_id, int deg, bool in_rr, bool out_rr, const PassArgs& a, const RrTables& t,
                               hipStream_t s);

}  // namespace ecg
