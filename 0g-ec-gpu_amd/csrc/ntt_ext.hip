// Shifted / scaled NTT: y[k] = c t^k sum_j s^j a[j] w^(jk)  (s = in_shift,
// t = out_shift, c = scale) -- the inverse (w^-1, c = 1/n), the coset
// evaluation (s = g) and its inverse (w^-1, t = 1/g, c = 1/n) -- fused into
// the reduced-radix Stockham passes of ntt_pass.hpp.
//
// Folding.  Pass k (radix 2^deg_k, L_k = sum of the earlier degrees, p =
// 2^L_k, s_k = log n - L_k - deg_k) loads x[g + i t] and multiplies it by its
// full table entry twf_k[i p + kk], kk = g mod p.
//  * The load digits i_k are the digits of the input index j = sum_k i_k
//    2^s_k, so s^j = prod_k (s^(2^s_k))^(i_k): pass k >= 1 takes its factor
//    into twf_k[i p + kk] *= s^(i << s_k) at no cost.  Pass 0 has no table
//    (p = 1); it reads IN0[i] = s^(i << s_0) in its place (MUL_IN): one
//    product per element.
//  * The store digit jj of pass k is digit L_k of the output index, and every
//    later pass sees it inside its kk.  The last pass's kk is therefore the
//    whole output index below its own digit: twf_last[i p + kk] *= t^kk.  Its
//    own digit is left: OUT[jj] = c t^(jj << L_last), one product per element
//    in the store phase (MUL_OUT).
//  * c alone (the plain inverse) goes into the last pass's table: no kernel
//    change and no product.  A single-pass transform (log n <= 10) has no
//    table; there c goes into IN0 if there is an input shift, else into OUT.
// The bounds of the two products are stated at the kernel (ntt_pass.hpp).
//
// Tables are built on the device in the boundary form and converted once to
// planes of exact canonical limbs, like the plain tables.  One plane array per
// table set: [twf_1 | ... | twf_last | OUT (2^deg_last) | IN0 (2^deg_0)], or
// [IN0 (n) | OUT (n)] for a single pass, so that OUT always sits right behind
// the last pass's table and the pass kernel needs no further argument.
//
// Cache: three slots in the context (ctx.hpp NttExtSlot), keyed by (field,
// log n, w, s, t, c), least recently used replaced first; the plain
// transform's slot (ctx->tw_*) and buffers are never touched.  Memory per
// slot: (2n + 2^deg_0 + 2^deg_last) x 36 B of planes ("ntt_ext_twf<i>", 1.2 GB
// at 2^24) plus the in-group roots ("ntt_ext_pq<i>", < 20 KB).  Shared by the
// slots and used only while a set is built: the boundary-form image of the
// planes ("ntt_ext_tmp", 2n x 32 B) and the split power tables of w, s and t
// ("ntt_ext_pw", 3 x (2^12 + n / 2^12) x 32 B).
//
// Unfused path (ntt_scale_kernel before / after the plain transform): where
// the reduced-radix passes are not used (log n > 28, ECG_NTT_RR=0,
// ECG_NTT_VARIANT=1) or after ecg_fft_set_fused(0).
#include <atomic>
#include <cstdio>
#include <cstring>

#include "ntt_pass.hpp"

namespace ecg {

// A/B and test knob (ecg_fft_set_fused); results never depend on it.
static std::atomic<int> g_ntt_fused{1};

// out[j] = c * w^(j << shift), j < count
template <class P>
__global__ void ntt_cpowers_kernel(Fp<P> w, Fp<P> c, uint32_t shift, uint64_t count, Fp<P>* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  Fp<P> base = w;
  for (uint32_t s = 0; s < shift; s++) base = fsqr(base);
  Fp<P> r = c;
  for (uint64_t e = j; e; e >>= 1) {
    if (e & 1) r = fmul(r, base);
    base = fsqr(base);
  }
  store(&out[j], r);
}

// Full table of pass k >= 1 with the folded factors:
//   out[i p + kk] = w^((kk i) << s) * a^(i << s) * b^kk * c
// a (in_shift) and b (out_shift) by their split tables, null = 1; b and c
// are given for the last pass only.  All exponents are < n.
template <class P>
__global__ void ntt_fulltw_ex_kernel(const Fp<P>* __restrict__ w_lo, const Fp<P>* __restrict__ w_hi,
                                     const Fp<P>* __restrict__ a_lo, const Fp<P>* __restrict__ a_hi,
                                     const Fp<P>* __restrict__ b_lo, const Fp<P>* __restrict__ b_hi, Fp<P> c,
                                     uint32_t has_c, uint32_t lgp, uint32_t deg, uint32_t log_n,
                                     Fp<P>* __restrict__ out) {
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >> (lgp + deg)) return;
  const uint64_t kk = idx & ((1ull << lgp) - 1), i = idx >> lgp;
  const uint32_t s = log_n - lgp - deg;
  const uint64_t e = (kk * i) << s;
  Fp<P> t = e ? twiddle(w_lo, w_hi, e) : Fp<P>::one();
  if (a_lo && i) t = fmul(t, twiddle(a_lo, a_hi, i << s));
  if (b_lo && kk) t = fmul(t, twiddle(b_lo, b_hi, kk));
  if (has_c) t = fmul(t, c);
  store(&out[idx], t);
}

// x[j] *= c s^j: lo[j] = c s^j (j < 2^12), hi[j] = s^(j << 12); lo null: x[j] *= c
template <class P>
__global__ void ntt_scale_kernel(Fp<P>* __restrict__ x, uint64_t n, const Fp<P>* __restrict__ lo,
                                 const Fp<P>* __restrict__ hi, Fp<P> c) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const Fp<P> f = lo ? twiddle(lo, hi, j) : c;
  store(&x[j], fmul(load(&x[j]), f));
}

template <class P>
static Fp<P> host_fp(const uint64_t* v) {  // null = 1
  Fp<P> r;
  memcpy(r.v, v ? v : P::ONE, sizeof(r.v));
  return r;
}

static uint32_t blocks256(uint64_t cnt) { return (uint32_t)((cnt + 255) / 256); }

// split tables of w at tab: lo (2^12 entries, times c) then hi
template <class P>
static void split_tables(const uint64_t* w, const uint64_t* c, uint64_t hi_cnt, Fp<P>* tab, hipStream_t s) {
  const uint64_t lo_cnt = 1ull << NTT_LO_BITS;
  hipLaunchKernelGGL(ntt_cpowers_kernel<P>, dim3(blocks256(lo_cnt)), dim3(256), 0, s, host_fp<P>(w), host_fp<P>(c),
                     0u, lo_cnt, tab);
  hipLaunchKernelGGL(ntt_powers_kernel<P>, dim3(blocks256(hi_cnt)), dim3(256), 0, s, host_fp<P>(w),
                     (uint32_t)NTT_LO_BITS, hi_cnt, tab + lo_cnt);
}

// ---------------------------------------------------------------------------
// unfused: x[j] *= c s^j around the plain transform
// ---------------------------------------------------------------------------
template <class P>
static int ntt_scale_run(ecg_ctx* ctx, void* d_data, uint32_t log_n, const uint64_t* shift, const uint64_t* c,
                         hipStream_t s) {
  using F = Fp<P>;
  const uint64_t n = 1ull << log_n, lo_cnt = 1ull << NTT_LO_BITS;
  const uint64_t hi_cnt = n > lo_cnt ? (n >> NTT_LO_BITS) : 1;
  F* tab = nullptr;
  if (shift) {  // 2^12 + n / 2^12 powers by square-and-multiply: rebuilt per call
    void* t;
    ECG_TRY(ws_get(ctx, "ntt_scale_tab", (lo_cnt + hi_cnt) * sizeof(F), &t));
    tab = (F*)t;
    split_tables<P>(shift, c, hi_cnt, tab, s);
  }
  hipLaunchKernelGGL(ntt_scale_kernel<P>, dim3(blocks256(n)), dim3(256), 0, s, (F*)d_data, n, tab,
                     tab ? tab + lo_cnt : nullptr, host_fp<P>(c));
  ECG_HIP(hipGetLastError());
  return ECG_OK;
}

template <class P>
static int ntt_ex_unfused_t(ecg_ctx* ctx, int field_id, void* d_data, const uint64_t* omega, uint32_t log_n,
                            const uint64_t* in_s, const uint64_t* out_s, const uint64_t* scale, hipStream_t s,
                            ecg_abort_cb abort_cb, void* user) {
  const bool c_before = in_s && !out_s;  // one scaling kernel where one is enough
  if (in_s) ECG_TRY(ntt_scale_run<P>(ctx, d_data, log_n, in_s, c_before ? scale : nullptr, s));
  ECG_TRY(ntt_run(ctx, field_id, d_data, omega, log_n, s, abort_cb, user));
  if (out_s || (scale && !c_before)) ECG_TRY(ntt_scale_run<P>(ctx, d_data, log_n, out_s, scale, s));
  return ECG_OK;
}

// ---------------------------------------------------------------------------
// fused: the extra products inside the first / last pass
// ---------------------------------------------------------------------------
template <class Q, int DEG>
static hipError_t launch_ext(bool in_rr, bool out_rr, bool mul_in, bool mul_out, const PassArgs& a, const RrTables& t,
                             hipStream_t s) {
  if (mul_in && mul_out) return launch_pass_rr<Q, DEG, false, false, true, true>(a, t, s);  // single pass
  if (mul_in)
    return out_rr ? launch_pass_rr<Q, DEG, false, true, true, false>(a, t, s)
                  : launch_pass_rr<Q, DEG, false, false, true, false>(a, t, s);
  return in_rr ? launch_pass_rr<Q, DEG, true, false, false, true>(a, t, s)
               : launch_pass_rr<Q, DEG, false, false, false, true>(a, t, s);
}

template <class Q>
static hipError_t launch_ext_deg(int deg, bool in_rr, bool out_rr, bool mul_in, bool mul_out, const PassArgs& a,
                                 const RrTables& t, hipStream_t s) {
  switch (deg) {
    case 1: return launch_ext<Q, 1>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 2: return launch_ext<Q, 2>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 3: return launch_ext<Q, 3>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 4: return launch_ext<Q, 4>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 5: return launch_ext<Q, 5>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 6: return launch_ext<Q, 6>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 7: return launch_ext<Q, 7>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 8: return launch_ext<Q, 8>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 9: return launch_ext<Q, 9>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 10: return launch_ext<Q, 10>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 11: return launch_ext<Q, 11>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    case 12: return launch_ext<Q, 12>(in_rr, out_rr, mul_in, mul_out, a, t, s);
    default: return hipErrorInvalidValue;
  }
}

template <class P, class Q>
static int ntt_ex_fused_t(ecg_ctx* ctx, int field_id, void* d_data, const uint64_t* omega, uint32_t log_n,
                          const uint64_t* in_s, const uint64_t* out_s, const uint64_t* scale, hipStream_t s,
                          ecg_abort_cb abort_cb, void* user, const uint32_t* degs, int np) {
  using F = Fp<P>;
  uint32_t max_deg = 0;
  for (int k = 0; k < np; k++) max_deg = degs[k] > max_deg ? degs[k] : max_deg;
  const uint64_t n = 1ull << log_n;
  const uint64_t lo_cnt = 1ull << NTT_LO_BITS;
  const uint64_t hi_cnt = n > lo_cnt ? (n >> NTT_LO_BITS) : 1;
  const uint64_t pq_cnt = max_deg > 1 ? 1ull << (max_deg - 1) : 1;
  const uint32_t d0 = degs[0], dl = degs[np - 1];

  // plane array: per-pass tables (as the plain transform lays them out), OUT, IN0
  uint64_t twf_off[40] = {0}, twf_tot = 0;
  {
    uint32_t lg = 0;
    for (int k = 0; k < np; k++) {
      if (k > 0) {
        twf_off[k] = twf_tot;
        twf_tot += 1ull << (lg + degs[k]);
      }
      lg += degs[k];
    }
  }
  const uint64_t in_off = np > 1 ? twf_tot + (1ull << dl) : 0;
  const uint64_t out_off = np > 1 ? twf_tot : n;  // = the last pass's table offset + n
  const uint64_t cnt = np > 1 ? in_off + (1ull << d0) : 2 * n;
  // where c goes: the last pass's table, or a small table when there is none
  const bool c_in0 = scale && np == 1 && in_s;
  const bool c_out = scale && !c_in0 && (out_s || np == 1);
  const bool c_twf = scale && !c_in0 && !c_out;
  const bool mul_in = in_s != nullptr, mul_out = out_s || c_out;

  // ---- slot
  uint64_t key[16] = {0};
  memcpy(key, omega, 32);
  if (in_s) memcpy(key + 4, in_s, 32);
  if (out_s) memcpy(key + 8, out_s, 32);
  if (scale) memcpy(key + 12, scale, 32);
  const int present = (in_s ? 1 : 0) | (out_s ? 2 : 0) | (scale ? 4 : 0);
  int slot = -1;
  for (int i = 0; i < 3; i++) {
    const auto& e = ctx->tw_ext[i];
    if (e.fid == field_id && e.log_n == log_n && e.present == present && memcmp(e.key, key, sizeof(key)) == 0) slot = i;
  }
  const bool cached = slot >= 0;
  if (!cached) {
    slot = 0;  // an empty slot (used = 0), else the least recently used
    for (int i = 1; i < 3; i++)
      if (ctx->tw_ext[i].used < ctx->tw_ext[slot].used) slot = i;
    ctx->tw_ext[slot].fid = -1;  // not valid until built (a failed allocation leaves it empty)
    ctx->tw_ext[slot].used = 0;
  }
  char name_twf[32], name_pq[32];
  snprintf(name_twf, sizeof(name_twf), "ntt_ext_twf%d", slot);
  snprintf(name_pq, sizeof(name_pq), "ntt_ext_pq%d", slot);
  void *twf_rr, *pq_rr;
  ECG_TRY(ws_get(ctx, name_twf, cnt * RR_PLANE_BYTES, &twf_rr));
  ECG_TRY(ws_get(ctx, name_pq, pq_cnt * RR_PLANE_BYTES, &pq_rr));

  void *scratch = nullptr, *scratch2 = nullptr;
  if (np > 1) ECG_TRY(ws_get(ctx, "ntt_scratch", n * RR_PLANE_BYTES, &scratch));
  if (np > 2) ECG_TRY(ws_get(ctx, "ntt_scratch2", n * RR_PLANE_BYTES, &scratch2));

  if (!cached) {
    void *tmp_v, *pw_v;
    ECG_TRY(ws_get(ctx, "ntt_ext_tmp", cnt * sizeof(F), &tmp_v));
    ECG_TRY(ws_get(ctx, "ntt_ext_pw", (pq_cnt + 3 * (lo_cnt + hi_cnt)) * sizeof(F), &pw_v));
    F* tmp = (F*)tmp_v;
    F* pq = (F*)pw_v;
    F* w_tab = pq + pq_cnt;
    F* a_tab = w_tab + lo_cnt + hi_cnt;
    F* b_tab = a_tab + lo_cnt + hi_cnt;
    hipLaunchKernelGGL(ntt_powers_kernel<P>, dim3(blocks256(pq_cnt)), dim3(256), 0, s, host_fp<P>(omega),
                       log_n - max_deg, pq_cnt, pq);
    if (np > 1) {
      split_tables<P>(omega, nullptr, hi_cnt, w_tab, s);
      if (in_s) split_tables<P>(in_s, nullptr, hi_cnt, a_tab, s);
      if (out_s) split_tables<P>(out_s, nullptr, hi_cnt, b_tab, s);
      uint32_t lg = degs[0];
      for (int k = 1; k < np; k++) {
        const bool last = k == np - 1;
        const uint64_t c = 1ull << (lg + degs[k]);
        hipLaunchKernelGGL(ntt_fulltw_ex_kernel<P>, dim3(blocks256(c)), dim3(256), 0, s, w_tab, w_tab + lo_cnt,
                           in_s ? a_tab : nullptr, a_tab + lo_cnt, last && out_s ? b_tab : nullptr, b_tab + lo_cnt,
                           host_fp<P>(scale), (uint32_t)(last && c_twf), lg, degs[k], log_n, tmp + twf_off[k]);
        lg += degs[k];
      }
    }
    // OUT[jj] = c t^(jj << L_last), IN0[i] = c s^(i << s_0) (all ones where unused)
    hipLaunchKernelGGL(ntt_cpowers_kernel<P>, dim3(blocks256(1ull << dl)), dim3(256), 0, s, host_fp<P>(out_s),
                       host_fp<P>(c_out ? scale : nullptr), log_n - dl, 1ull << dl, tmp + out_off);
    hipLaunchKernelGGL(ntt_cpowers_kernel<P>, dim3(blocks256(1ull << d0)), dim3(256), 0, s, host_fp<P>(in_s),
                       host_fp<P>(c_in0 ? scale : nullptr), log_n - d0, 1ull << d0, tmp + in_off);
    hipLaunchKernelGGL(ntt_tab_to_rr_kernel<Q>, dim3(blocks256(pq_cnt)), dim3(256), 0, s, pq, pq_cnt, (uint4*)pq_rr);
    hipLaunchKernelGGL(ntt_tab_to_rr_kernel<Q>, dim3(blocks256(cnt)), dim3(256), 0, s, tmp, cnt, (uint4*)twf_rr);
    ECG_HIP(hipGetLastError());
    auto& e = ctx->tw_ext[slot];
    e.fid = field_id;
    e.log_n = log_n;
    e.present = present;
    memcpy(e.key, key, sizeof(key));
  }
  ctx->tw_ext[slot].used = ++ctx->tw_ext_clock;

  // ---- passes: the plain transform's schedule (ntt_run_t)
  kt_reset(ctx, "ntt_pass");
  void* bufs[41];
  bufs[0] = d_data;
  for (int k = 1; k <= np; k++) bufs[k] = k == np ? d_data : (k & 1) ? scratch : scratch2;
  uint32_t lgp = 0;
  for (int k = 0; k < np; k++) {
    if (abort_cb && abort_cb(user)) return ECG_ABORTED;
    const PassArgs a{bufs[k], bufs[k + 1], nullptr, max_deg - degs[k], nullptr, nullptr, nullptr, log_n, lgp, 1};
    const RrTables t{pq_rr, (uint32_t)pq_cnt, twf_rr, cnt, k == 0 ? in_off : twf_off[k]};
    const bool mi = mul_in && k == 0, mo = mul_out && k == np - 1;
    ECG_TRY(kt_begin(ctx, "ntt_pass", s));
    ECG_HIP(mi || mo ? launch_ext_deg<Q>((int)degs[k], k > 0, k + 1 < np, mi, mo, a, t, s)
                     : ntt_launch_plain_rr(field_id, (int)degs[k], k > 0, k + 1 < np, a, t, s));
    ECG_TRY(kt_end(ctx, "ntt_pass", s));
    lgp += degs[k];
  }
  return ECG_OK;
}

template <class P>
static bool fr_param_ok(const uint64_t* v, bool nonzero, const char* what) {
  if (!v) return true;
  bool zero = true, lt = false;
  for (int i = P::N - 1; i >= 0; i--) {
    if (v[i] != P::P[i]) {
      lt = v[i] < P::P[i];
      break;
    }
  }
  if (!lt) {
    set_error("radix_fft_ex: %s is not a reduced field element (>= r)", what);
    return false;
  }
  for (int i = 0; i < P::N; i++) zero = zero && v[i] == 0;
  if (zero && nonzero) {
    set_error("radix_fft_ex: %s must be non-zero", what);
    return false;
  }
  return true;
}

int ntt_ex_validate(int field_id, uint32_t log_n, const uint64_t* in_shift, const uint64_t* out_shift,
                    const uint64_t* scale) {
  ECG_TRY(ntt_validate(field_id, log_n));
  const bool ok = field_id == ECG_FIELD_BLS12_381_FR
                      ? fr_param_ok<params::bls12_381_fr>(in_shift, true, "in_shift") &&
                            fr_param_ok<params::bls12_381_fr>(out_shift, true, "out_shift") &&
                            fr_param_ok<params::bls12_381_fr>(scale, false, "scale")
                      : fr_param_ok<params::bn254_fr>(in_shift, true, "in_shift") &&
                            fr_param_ok<params::bn254_fr>(out_shift, true, "out_shift") &&
                            fr_param_ok<params::bn254_fr>(scale, false, "scale");
  return ok ? ECG_OK : ECG_ERR_INVALID;
}

int ntt_run_ex(ecg_ctx* ctx, int field_id, void* d_data, const uint64_t* omega, uint32_t log_n,
               const uint64_t* in_shift, const uint64_t* out_shift, const uint64_t* scale, hipStream_t s,
               ecg_abort_cb abort_cb, void* user) {
  if (!in_shift && !out_shift && !scale) return ntt_run(ctx, field_id, d_data, omega, log_n, s, abort_cb, user);
  ECG_TRY(ntt_ex_validate(field_id, log_n, in_shift, out_shift, scale));
  uint32_t degs[40];
  const int np = g_ntt_fused.load() ? ntt_rr_plan(log_n, degs) : 0;
  const bool bls = field_id == ECG_FIELD_BLS12_381_FR;
  if (np == 0)
    return bls ? ntt_ex_unfused_t<params::bls12_381_fr>(ctx, field_id, d_data, omega, log_n, in_shift, out_shift,
                                                         scale, s, abort_cb, user)
               : ntt_ex_unfused_t<params::bn254_fr>(ctx, field_id, d_data, omega, log_n, in_shift, out_shift, scale,
                                                    s, abort_cb, user);
  return bls ? ntt_ex_fused_t<params::bls12_381_fr, params::bls12_381_fr_rr>(
                   ctx, field_id, d_data, omega, log_n, in_shift, out_shift, scale, s, abort_cb, user, degs, np)
             : ntt_ex_fused_t<params::bn254_fr, params::bn254_fr_rr>(ctx, field_id, d_data, omega, log_n, in_shift,
                                                                      out_shift, scale, s, abort_cb, user, degs, np);
}

}  // namespace ecg

extern "C" int ecg_fft_set_fused(int on) {
  ecg::g_ntt_fused.store(on ? 1 : 0);
  return ECG_OK;
}
