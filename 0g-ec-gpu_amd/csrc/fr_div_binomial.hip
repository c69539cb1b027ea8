// Division of resident Fr coefficients by X^m - c, m = 2^log_m (DESIGN.md
// §4.1.2a): d_out[j] = s_j with s_j = p_j + c s_(j+m), s_j = 0 for j >= n, i.e.
// d_out[0..m) = p mod (X^m - c) and d_out[m + j] = q_j.
//
// The vector is a matrix of ceil(n / m) rows by m columns, element j = row m +
// col, and the recurrence runs up every column with the uniform multiplier c:
// m interleaved Horner chains.  Two layouts, chosen by fdb_plan:
//
//  strided (1 <= log_m <= FDB_MAX_STRIDED): the chains are long and each one is
//    a scan.  The tile of fr_scan.hip (2048 consecutive elements = 2048 / m
//    whole rows, global memory as consecutive uint4 through LDS), but a
//    thread's run is 8 consecutive ROWS of one column, and the 256 / m threads
//    of one column are a contiguous group.  The wave reduce and the block scan
//    become segmented: log2(group) shuffle levels with a select at the group
//    edge, the carry-in injected at the group's last lane, and a cross-wave
//    step only where a group spans waves (m = 2).  A tile leaves m aggregates,
//    one per column; the middle kernel runs one workgroup per column over the
//    strided aggregates (multiplier c^(2048 / m)); the apply kernel recomputes
//    from the column's carry-in and stores.
//    LDS: slot j of the tile's uint4 image sits at j + j / (16 m), one uint4 of
//    padding per 8 rows.  A thread's run starts at (16 m + 1) g + 2 col (g its
//    place in the group), so the lanes of one column are 16 m + 1 slots apart
//    in every ds_read_b128 and spread over the banks as in the linear kernel
//    (17 there); the 8 reads of a run are 2 m slots apart and stay inside the
//    run's own padding interval.
//
//  columns (log_m > FDB_MAX_STRIDED): 64 columns are one contiguous 2 KB of a
//    row, so a thread owns a column: 32 B per row and lane, consecutive across
//    the lanes, no LDS and no shuffles.  The rows are cut into segments so the
//    grid fills the device (fdb_plan: a power-of-two number of rows each, so
//    c^(rows per segment) is a table entry) and the three phases run across
//    segments: a Horner aggregate per (segment, column) cell; a pass per column
//    over the segments that leaves each cell its carry-in in place of its
//    aggregate -- one thread per column walking them where they are few (up
//    to FDB_SEQ_SEGMENTS), else the strided layout's middle kernel, a workgroup
//    per column; and an apply that walks the cell again.  One segment: the
//    apply alone, one read and one write.  A cell loads four rows ahead of the
//    four whose dependent products it runs.
//
// In place is safe in both: a tile / a cell reads only what it alone writes.
// Arithmetic and operand classes (C, M, Sk, N) as in fr_scan.hip: the caller's
// word re-read as the R' form, c^(2^k) and c^L made on the host in the true R'
// form, every product a plain rr_mul of two QN operands, aggregates and
// carries stored through rr_reduce_q.
#include <algorithm>
#include <cstring>

#include "ctx.hpp"
#include "fieldrr.hpp"
#include "fr_scan.hpp"
#include "host_field.hpp"

namespace ecg {

constexpr uint32_t FDB_MAX_STRIDED = 5;       // log_m of the widest strided layout: groups of 8 threads
constexpr int FDB_COL_THREADS = 256;
constexpr int FDB_COL_BATCH = 4;              // rows loaded ahead per cell
constexpr size_t FDB_TARGET_CELLS = 1 << 19;  // (segment, column) cells that fill 256 CUs x 4 SIMDs x 8 waves
constexpr size_t FDB_MIN_SEG_ROWS = 16;       // aggregates stay below 36 / (16 x 32) = 7 % of the input
constexpr uint32_t FDB_SEQ_SEGMENTS = 128;    // up to here one thread per column walks the segments

struct FdbPlan {
  int path;
  uint32_t segments;
  size_t rows_per_segment;
  size_t cols_p;  // columns path: the columns that hold data, rounded up to whole waves
};

// The split along a chain.  Strided: tiles, 2048 / m rows each.  Columns: as
// many segments as bring the grid to FDB_TARGET_CELLS cells, none shorter than
// FDB_MIN_SEG_ROWS rows (but one).
static FdbPlan fdb_plan(size_t n, uint32_t log_m) {
  FdbPlan pl{};
  const size_t ntiles = (n + FRS_TILE - 1) >> FRS_LOG_TILE;
  if (log_m <= FDB_MAX_STRIDED) {
    pl.path = log_m == 0 ? ECG_DIVB_PATH_LINEAR : ECG_DIVB_PATH_STRIDED;
    pl.segments = (uint32_t)ntiles;
    pl.rows_per_segment = (size_t)FRS_TILE >> log_m;
    return pl;
  }
  const size_t m = (size_t)1 << log_m, rows = (n + m - 1) >> log_m;
  pl.path = ECG_DIVB_PATH_COLUMNS;
  pl.cols_p = (std::min(m, n) + 63) & ~(size_t)63;
  if (rows == 0) return pl;
  const size_t want = std::max<size_t>(1, FDB_TARGET_CELLS >> log_m);
  pl.rows_per_segment = FDB_MIN_SEG_ROWS;  // a power of two: c^L is an entry of the table
  while (pl.rows_per_segment * want < rows) pl.rows_per_segment <<= 1;
  pl.segments = (uint32_t)((rows + pl.rows_per_segment - 1) / pl.rows_per_segment);
  return pl;
}

// two uint4 of a boundary-form element -> limbs: C
template <class Q>
ECG_DEV FpR<Q> fdb_unpack(const uint4& lo, const uint4& hi) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  FpR<Q> r;
  rr_unpack<Q, 8>(w, r.v);
  return r;
}
template <class Q>
ECG_DEV void fdb_pack(const FpR<Q>& c, uint4& lo, uint4& hi) {
  uint32_t w[8];
  rr_pack<Q, 8>(c.v, w);
  lo = make_uint4(w[0], w[1], w[2], w[3]);
  hi = make_uint4(w[4], w[5], w[6], w[7]);
}

// ---------------------------------------------------------------------------
// strided layout: LM = log_m, groups of G = 256 / m threads per column
// ---------------------------------------------------------------------------
template <int LM>
ECG_DEV uint32_t fdb_slot(uint32_t j) {
  return j + (j >> (4 + LM));
}
template <int LM>
ECG_DEV void fdb_stage_in(const uint4* src, size_t tile, size_t n, uint4* lds) {
  const size_t base = tile << FRS_LOG_TILE;
#pragma unroll
  for (int q = 0; q < 2 * FRS_E; q++) {
    const uint32_t j = q * FRS_THREADS + threadIdx.x;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (base + (j >> 1) < n) w = src[2 * base + j];
    lds[fdb_slot<LM>(j)] = w;
  }
}
template <int LM>
ECG_DEV void fdb_stage_out(uint4* dst, size_t tile, size_t n, const uint4* lds) {
  const size_t base = tile << FRS_LOG_TILE;
#pragma unroll
  for (int q = 0; q < 2 * FRS_E; q++) {
    const uint32_t j = q * FRS_THREADS + threadIdx.x;
    if (base + (j >> 1) < n) dst[2 * base + j] = lds[fdb_slot<LM>(j)];
  }
}
// the slot of row k of this thread's run: thread = col G + g holds the rows
// 8 g .. 8 g + 7 of column col, element (8 g + k) m + col of the tile
template <int LM>
ECG_DEV uint32_t fdb_run_slot(int k) {
  constexpr int LG = 8 - LM;
  const uint32_t col = threadIdx.x >> LG, g = threadIdx.x & ((1u << LG) - 1);
  return (g << (4 + LM)) + g + 2 * col + ((uint32_t)k << (LM + 1));
}
template <class Q, int LM>
ECG_DEV FpR<Q> fdb_get(const uint4* lds, int k) {
  const uint32_t s = fdb_run_slot<LM>(k);
  return fdb_unpack<Q>(lds[s], lds[s + 1]);
}
// Horner value of the run, sum_k p_k c^k: S2.5
template <class Q, int LM>
ECG_DEV FpR<Q> fdb_run(const uint4* lds, const FpR<Q>& c) {
  FpR<Q> h = fdb_get<Q, LM>(lds, FRS_E - 1);
#pragma unroll
  for (int k = FRS_E - 2; k >= 0; k--) h = rr_add(fdb_get<Q, LM>(lds, k), rr_mul(h, c));  // (C | S2.5) x C -> C + M
  return h;
}

// Segmented reduce: the first lane of every group of 2^LW lanes (LW <= 6) ends
// with sum_l g_l M^l over its group, M = c^8 = pw[3].  No select: a group's
// first lane never reads past its group.  g S2.5 on entry, at most S13.1.
template <class Q, int LW>
ECG_DEV FpR<Q> fdb_group_reduce(FpR<Q> g, const FrsTable& tab) {
#pragma unroll
  for (int k = 0; k < LW; k++) {
    const FpR<Q> o = frs_shift<true>(g, 1 << k);
    g = rr_add(g, rr_mul(o, frs_limbs<Q>(tab.pw[3 + k])));  // S13.1 x C -> M
  }
  return g;
}

// Segmented block scan: the value that follows this thread's run in its column,
// X_i = sum_{j > i in the group} g_j M^(j-i-1) + M^(G-1-i) carry_in, M = c^8.
// g S2.5; carry_in N, the column's (the same on every thread of a group).
// LG <= 6: the carry enters at the group's last lane (g + M c: S4.1), then LG
// levels of the inclusive suffix scan with a select at the group's edge.
// LG > 6 (m = 2: a group is two waves): first the wave totals through LDS and
// the wave's own carry by Horner over the group's later waves (c^512), as in
// frs_div_block_scan, with the group's last wave in the place of the block's.
template <class Q, int LG>
ECG_DEV FpR<Q> fdb_group_scan(FpR<Q> g, const FpR<Q>& carry_in, const FrsTable& tab, uint32_t (*wagg)[9]) {
  constexpr int LW = LG < 6 ? LG : 6, W = 1 << LW;
  const int pos = threadIdx.x & (W - 1);  // place in the group's part of this wave
  FpR<Q> c = carry_in;
  if constexpr (LG > 6) {
    const int wave = threadIdx.x >> 6, last = wave | ((1 << (LG - 6)) - 1);
    frs_put_limbs(wagg[wave], rr_reduce_q(frs_bcast(fdb_group_reduce<Q, 6>(g, tab), 0)));  // N
    __syncthreads();
    for (int u = last; u > wave; u--)
      c = rr_add(frs_limbs<Q>(wagg[u]), rr_mul(c, frs_limbs<Q>(tab.pw[9])));  // N + (N | S2.6) x C
  }
  const FpR<Q> gi = rr_add(g, rr_mul(c, frs_limbs<Q>(tab.pw[3])));  // S2.5 + S2.6 x C
  g = frs_pick(pos == W - 1, gi, g);
#pragma unroll
  for (int k = 0; k < LW; k++) {
    const FpR<Q> o = frs_shift<true>(g, 1 << k);
    const FpR<Q> s = rr_add(g, rr_mul(o, frs_limbs<Q>(tab.pw[3 + k])));  // S13.1 x C -> M
    g = frs_pick(pos + (1 << k) < W, s, g);
  }
  const FpR<Q> x = frs_shift<true>(g, 1);
  if constexpr (LG > 6) __syncthreads();  // wagg may be written again
  return frs_pick(pos == W - 1, c, x);
}

// agg[tile m + col] = the Horner value of the tile's rows of column col: N
template <class Q, int LM>
__global__ void __launch_bounds__(FRS_THREADS)
    fdb_str_reduce_kernel(const uint4* __restrict__ p, size_t n, FrsTable tab, FpR<Q>* __restrict__ agg) {
  constexpr int LG = 8 - LM, LW = LG < 6 ? LG : 6;
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wagg[FRS_WAVES][9];
  fdb_stage_in<LM>(p, blockIdx.x, n, lds);
  __syncthreads();
  FpR<Q> h = fdb_group_reduce<Q, LW>(fdb_run<Q, LM>(lds, frs_limbs<Q>(tab.pw[0])), tab);
  const uint32_t col = threadIdx.x >> LG, g = threadIdx.x & ((1u << LG) - 1);
  if constexpr (LG > 6) {
    const int wave = threadIdx.x >> 6, last = wave | ((1 << (LG - 6)) - 1);
    frs_put_limbs(wagg[wave], rr_reduce_q(frs_bcast(h, 0)));
    __syncthreads();
    if (g == 0) {
      h = frs_limbs<Q>(wagg[last]);
      for (int w = last - 1; w >= wave; w--)
        h = rr_add(frs_limbs<Q>(wagg[w]), rr_mul(h, frs_limbs<Q>(tab.pw[9])));  // N + (N | S2.6) x C
    }
  }
  if (g == 0) store(&agg[((size_t)blockIdx.x << LM) + col], rr_reduce_q(h));
}

// One workgroup per column (both layouts): thread i owns the column's
// aggregates of the tiles / segments [i R, (i + 1) R), R = 2^lg_run, `stride`
// entries apart; each is replaced by its carry-in
// carry[t] = sum_{u > t} A_u (c^rows)^(u-t-1), N; c^rows = pw[lt].
template <class Q>
__global__ void __launch_bounds__(FRS_SCAN_THREADS)
    fdb_chain_scan_kernel(FpR<Q>* agg, size_t ntiles, uint32_t lg_run, size_t stride, int lt, FrsTable tab) {
  __shared__ uint32_t wagg[FRS_SCAN_WAVES][9];
  const size_t i0 = (size_t)threadIdx.x << lg_run;
  const int run = 1 << lg_run;
  FpR<Q>* col = agg + blockIdx.x;
  const FpR<Q> ct = frs_limbs<Q>(tab.pw[lt]);
  FpR<Q> h = FpR<Q>::zero();
  for (int k = run - 1; k >= 0; k--)
    if (i0 + k < ntiles) h = rr_add(load(&col[(i0 + k) * stride]), rr_mul(h, ct));  // N + S2.6 x C
  FpR<Q> c = frs_div_block_scan<Q, FRS_SCAN_WAVES>(h, FpR<Q>::zero(), tab, lt + (int)lg_run, wagg);
  for (int k = run - 1; k >= 0; k--) {
    if (i0 + k >= ntiles) continue;
    const FpR<Q> a = load(&col[(i0 + k) * stride]);
    store(&col[(i0 + k) * stride], rr_reduce_q(c));
    c = rr_add(a, rr_mul(c, ct));  // N + (S13.1 | S2.6) x C
  }
}

// p and out may be the same buffer: a tile reads only what it alone writes.
template <class Q, int LM, bool CANON>
__global__ void __launch_bounds__(FRS_THREADS)
    fdb_str_apply_kernel(const uint4* p, size_t n, FrsTable tab, const FpR<Q>* __restrict__ carry, uint4* out) {
  constexpr int LG = 8 - LM;
  __shared__ uint4 lds[FRS_SLOTS];
  __shared__ uint32_t wagg[FRS_WAVES][9];
  fdb_stage_in<LM>(p, blockIdx.x, n, lds);
  __syncthreads();
  const FpR<Q> z = frs_limbs<Q>(tab.pw[0]);
  const FpR<Q> cin = load(&carry[((size_t)blockIdx.x << LM) + (threadIdx.x >> LG)]);
  FpR<Q> c = fdb_group_scan<Q, LG>(fdb_run<Q, LM>(lds, z), cin, tab, wagg);
#pragma unroll
  for (int k = FRS_E - 1; k >= 0; k--) {
    c = rr_add(fdb_get<Q, LM>(lds, k), rr_mul(c, z));  // C + (S13.1 | S2.5) x C = S2.5
    const uint32_t s = fdb_run_slot<LM>(k);
    fdb_pack(frs_div_out<Q, CANON>(c, tab), lds[s], lds[s + 1]);
  }
  __syncthreads();
  fdb_stage_out<LM>(out, blockIdx.x, n, lds);
}

// ---------------------------------------------------------------------------
// column layout: cell t = seg cols_p + col, rows [seg L, (seg + 1) L) of col
// ---------------------------------------------------------------------------
struct FdbColTable {
  uint32_t c[9];    // c, R' form
  uint32_t cl[9];   // c^L, L = rows per segment
  uint32_t cst[9];  // R' / R
};

struct FdbRows {
  uint4 w[FDB_COL_BATCH][2];
};
// the rows row .. row + 3 of column col
ECG_DEV void fdb_col_load(FdbRows& b, const uint4* p, size_t row, uint32_t log_m, size_t col) {
#pragma unroll
  for (int k = 0; k < FDB_COL_BATCH; k++) {
    const size_t j = ((row + k) << log_m) + col;
    b.w[k][0] = p[2 * j];
    b.w[k][1] = p[2 * j + 1];
  }
}

// APPLY = false: aux[t] = the Horner value of the cell (N; zero for a cell
// without rows).  APPLY = true: s = p + c s down the cell from its carry-in
// aux[t] (zero with CARRY = false: one segment), every s stored.  The ragged
// top (rows mod 4) goes row by row, the rest in batches of four with the next
// batch's loads issued before the current batch's four dependent products.
template <class Q, bool APPLY, bool CARRY, bool CANON>
__global__ void __launch_bounds__(FDB_COL_THREADS)
    fdb_col_kernel(const uint4* p, size_t n, uint32_t log_m, size_t cols_p, uint32_t segments, size_t seg_rows,
                   FdbColTable tab, FpR<Q>* aux, uint4* out) {
  const size_t t = (size_t)blockIdx.x * FDB_COL_THREADS + threadIdx.x;
  const size_t seg = t / cols_p, col = t - seg * cols_p;
  if (seg >= segments || col >= n) return;  // col < cols_p <= m whenever col < n
  const size_t rows_col = ((n - 1 - col) >> log_m) + 1;  // rows of this column below n
  const size_t lo = seg * seg_rows, hi = std::min(lo + seg_rows, rows_col);
  const FpR<Q> c = frs_limbs<Q>(tab.c);
  FpR<Q> h = FpR<Q>::zero();
  if constexpr (APPLY && CARRY) h = load(&aux[t]);  // N
  auto step = [&](const uint4& wlo, const uint4& whi, size_t row) {
    h = rr_add(fdb_unpack<Q>(wlo, whi), rr_mul(h, c));  // C + (N | S2.5) x C = S2.5
    if constexpr (APPLY) {
      FpR<Q> o;
      if constexpr (CANON)
        o = rr_canon_lt2p(rr_mul(h, frs_limbs<Q>(tab.cst)));  // S2.5 x C -> M
      else
        o = frs_canon(h);
      const size_t j = (row << log_m) + col;
      fdb_pack(o, out[2 * j], out[2 * j + 1]);
    }
  };
  size_t row = hi > lo ? hi : lo;
  while ((row - lo) & (FDB_COL_BATCH - 1)) {
    row--;
    const size_t j = (row << log_m) + col;
    step(p[2 * j], p[2 * j + 1], row);
  }
  if (row > lo) {
    FdbRows cur;
    fdb_col_load(cur, p, row - FDB_COL_BATCH, log_m, col);
    while (row > lo) {
      FdbRows nxt = cur;
      row -= FDB_COL_BATCH;
      if (row > lo) fdb_col_load(nxt, p, row - FDB_COL_BATCH, log_m, col);
#pragma unroll
      for (int k = FDB_COL_BATCH - 1; k >= 0; k--) step(cur.w[k][0], cur.w[k][1], row + k);
      cur = nxt;
    }
  }
  if constexpr (!APPLY) store(&aux[t], rr_reduce_q(h));
}

// One thread per column: aux[seg cols_p + col] from the cell's aggregate to its
// carry-in, carry[seg] = sum_{u > seg} A_u (c^L)^(u-seg-1): N.
template <class Q>
__global__ void __launch_bounds__(FDB_COL_THREADS)
    fdb_col_scan_kernel(FpR<Q>* aux, size_t n, size_t cols_p, uint32_t segments, FdbColTable tab) {
  const size_t col = (size_t)blockIdx.x * FDB_COL_THREADS + threadIdx.x;
  if (col >= cols_p || col >= n) return;
  const FpR<Q> cl = frs_limbs<Q>(tab.cl);
  FpR<Q> s = FpR<Q>::zero();
  for (uint32_t seg = segments; seg-- > 0;) {
    FpR<Q>* cell = &aux[(size_t)seg * cols_p + col];
    const FpR<Q> a = load(cell);
    store(cell, rr_reduce_q(s));
    s = rr_add(a, rr_mul(s, cl));  // N + S2.6 x C
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <class Q, int LM>
static void fdb_str_launch(const void* d_coeffs, size_t n, const FrsTable& tab, FpR<Q>* agg, void* d_out,
                           bool canonical, hipStream_t s) {
  using F = FpR<Q>;
  const size_t ntiles = (n + FRS_TILE - 1) >> FRS_LOG_TILE;
  hipLaunchKernelGGL((fdb_str_reduce_kernel<Q, LM>), dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s,
                     (const uint4*)d_coeffs, n, tab, agg);
  hipLaunchKernelGGL(fdb_chain_scan_kernel<Q>, dim3(1u << LM), dim3(FRS_SCAN_THREADS), 0, s, agg, ntiles,
                     frs_lg_run(ntiles), (size_t)1 << LM, FRS_LOG_TILE - LM, tab);
  if (canonical)
    hipLaunchKernelGGL((fdb_str_apply_kernel<Q, LM, true>), dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s,
                       (const uint4*)d_coeffs, n, tab, (const F*)agg, (uint4*)d_out);
  else
    hipLaunchKernelGGL((fdb_str_apply_kernel<Q, LM, false>), dim3((uint32_t)ntiles), dim3(FRS_THREADS), 0, s,
                       (const uint4*)d_coeffs, n, tab, (const F*)agg, (uint4*)d_out);
}

template <class Q, bool CARRY>
static void fdb_col_apply(const FdbPlan& pl, uint32_t blocks, const void* d_coeffs, size_t n, uint32_t log_m,
                          const FdbColTable& ct, FpR<Q>* aux, void* d_out, bool canonical, hipStream_t s) {
  if (canonical)
    hipLaunchKernelGGL((fdb_col_kernel<Q, true, CARRY, true>), dim3(blocks), dim3(FDB_COL_THREADS), 0, s,
                       (const uint4*)d_coeffs, n, log_m, pl.cols_p, pl.segments, pl.rows_per_segment, ct, aux,
                       (uint4*)d_out);
  else
    hipLaunchKernelGGL((fdb_col_kernel<Q, true, CARRY, false>), dim3(blocks), dim3(FDB_COL_THREADS), 0, s,
                       (const uint4*)d_coeffs, n, log_m, pl.cols_p, pl.segments, pl.rows_per_segment, ct, aux,
                       (uint4*)d_out);
}

template <class P, class Q>
static int fdb_div_t(ecg_ctx* ctx, const void* d_coeffs, size_t n, uint32_t log_m, const uint64_t* c, void* d_out,
                     bool canonical, hipStream_t s) {
  using F = FpR<Q>;
  using H = host::HFp<P>;
  if (!frs_below_r<P>(c)) {
    set_error("poly_div_binomial: c is not a reduced field element (>= r)");
    return ECG_ERR_INVALID;
  }
  const FdbPlan pl = fdb_plan(n, log_m);
  H cp, one = H::zero();
  memcpy(cp.v, c, sizeof(cp.v));
  one.v[0] = 1;
  FrsTable tab;
  for (int k = 0; k < FRS_NPOW; k++) {  // c^(2^k) R by squaring, each to the R' form
    frs_to_rr<P, Q>(cp, tab.pw[k]);
    cp = host::hmul(cp, cp);
  }
  frs_to_rr<P, Q>(one, tab.cst);  // R' / R
  if (pl.path == ECG_DIVB_PATH_STRIDED) {
    void* agg;
    ECG_TRY(ws_get(ctx, "fr_scan_agg", ((size_t)pl.segments << log_m) * sizeof(F), &agg));
    switch (log_m) {
      case 1: fdb_str_launch<Q, 1>(d_coeffs, n, tab, (F*)agg, d_out, canonical, s); break;
      case 2: fdb_str_launch<Q, 2>(d_coeffs, n, tab, (F*)agg, d_out, canonical, s); break;
      case 3: fdb_str_launch<Q, 3>(d_coeffs, n, tab, (F*)agg, d_out, canonical, s); break;
      case 4: fdb_str_launch<Q, 4>(d_coeffs, n, tab, (F*)agg, d_out, canonical, s); break;
      default: fdb_str_launch<Q, 5>(d_coeffs, n, tab, (F*)agg, d_out, canonical, s); break;
    }
    static_assert(FDB_MAX_STRIDED == 5, "one instantiation per strided log_m");
  } else {
    int lt = 0;  // rows per segment = 2^lt <= 2^26: c^L = pw[lt]
    while (((size_t)1 << lt) < pl.rows_per_segment) lt++;
    FdbColTable ct;
    memcpy(ct.c, tab.pw[0], sizeof(ct.c));
    memcpy(ct.cl, tab.pw[lt], sizeof(ct.cl));
    memcpy(ct.cst, tab.cst, sizeof(ct.cst));
    const size_t cells = pl.segments * pl.cols_p;
    const uint32_t blocks = (uint32_t)((cells + FDB_COL_THREADS - 1) / FDB_COL_THREADS);
    if (pl.segments == 1) {
      fdb_col_apply<Q, false>(pl, blocks, d_coeffs, n, log_m, ct, (F*)nullptr, d_out, canonical, s);
    } else {
      void* aux;
      ECG_TRY(ws_get(ctx, "fr_scan_agg", cells * sizeof(F), &aux));
      hipLaunchKernelGGL((fdb_col_kernel<Q, false, false, false>), dim3(blocks), dim3(FDB_COL_THREADS), 0, s,
                         (const uint4*)d_coeffs, n, log_m, pl.cols_p, pl.segments, pl.rows_per_segment, ct, (F*)aux,
                         (uint4*)nullptr);
      // few segments: a thread per column walks them; many (small m): a workgroup per column scans them
      if (pl.segments <= FDB_SEQ_SEGMENTS)
        hipLaunchKernelGGL(fdb_col_scan_kernel<Q>,
                           dim3((uint32_t)((pl.cols_p + FDB_COL_THREADS - 1) / FDB_COL_THREADS)),
                           dim3(FDB_COL_THREADS), 0, s, (F*)aux, n, pl.cols_p, pl.segments, ct);
      else
        hipLaunchKernelGGL(fdb_chain_scan_kernel<Q>, dim3((uint32_t)std::min((size_t)1 << log_m, n)),
                           dim3(FRS_SCAN_THREADS), 0, s, (F*)aux, (size_t)pl.segments, frs_lg_run(pl.segments),
                           pl.cols_p, lt, tab);
      fdb_col_apply<Q, true>(pl, blocks, d_coeffs, n, log_m, ct, (F*)aux, d_out, canonical, s);
    }
  }
  ECG_HIP(hipGetLastError());
  return ECG_OK;
}

}  // namespace ecg

using namespace ecg;

extern "C" int ecg_poly_div_binomial_plan(size_t n, uint32_t log_m, int* path, uint32_t* segments,
                                          size_t* rows_per_segment) {
  if (!path || !segments || !rows_per_segment) {
    set_error("poly_div_binomial_plan: null pointer");
    return ECG_ERR_INVALID;
  }
  if (log_m > 31 || n > ((size_t)1 << 32)) {
    set_error("poly_div_binomial_plan: log_m = %u above 31 or n = %zu above 2^32", log_m, n);
    return ECG_ERR_INVALID;
  }
  const FdbPlan pl = fdb_plan(n, log_m);
  *path = pl.path;
  *segments = pl.segments;
  *rows_per_segment = pl.rows_per_segment;
  return ECG_OK;
}

extern "C" int ecg_poly_div_binomial_dev(ecg_ctx* ctx, int field_id, const void* d_coeffs, size_t n, uint32_t log_m,
                                         const uint64_t* c, void* d_out, uint32_t flags, void* stream) {
  ECG_ENTER(ctx);
  if (flags & ~(uint32_t)ECG_POLY_OUT_CANONICAL) {
    set_error("poly_div_binomial: unknown flag bits 0x%x", flags);
    return ECG_ERR_INVALID;
  }
  if (log_m > 31) {
    set_error("poly_div_binomial: log_m = %u is above 31", log_m);
    return ECG_ERR_INVALID;
  }
  const int rc = frs_check("poly_div_binomial", field_id, d_coeffs, n);
  if (rc != ECG_OK) return rc < 0 ? rc : ECG_OK;
  if (!c || !d_out) {
    set_error("poly_div_binomial: null pointer (c and d_out are required)");
    return ECG_ERR_INVALID;
  }
  const char *a = (const char*)d_coeffs, *b = (const char*)d_out;
  if (b != a && b < a + n * 32 && a < b + n * 32) {
    set_error("poly_div_binomial: d_out overlaps d_coeffs (in place, d_out == d_coeffs, is allowed)");
    return ECG_ERR_INVALID;
  }
  if (log_m == 0) return ecg_poly_div_linear_dev(ctx, field_id, d_coeffs, n, c, d_out, nullptr, flags, stream);
  const bool canonical = flags & ECG_POLY_OUT_CANONICAL;
  hipStream_t s = pick_stream(ctx, stream);
  return field_id == ECG_FIELD_BLS12_381_FR
             ? fdb_div_t<params::bls12_381_fr, params::bls12_381_fr_rr>(ctx, d_coeffs, n, log_m, c, d_out, canonical, s)
             : fdb_div_t<params::bn254_fr, params::bn254_fr_rr>(ctx, d_coeffs, n, log_m, c, d_out, canonical, s);
}
