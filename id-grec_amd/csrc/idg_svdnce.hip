// LightGCL's SVD-view contrastive terms (Cai et al. ICLR'23: models/LightGCL.py:58-120 of the reference) and the two
// tall-skinny rank-q products they need, forward and backward, without the [B, N] score matrix and without an [n, d] view
// panel.
//
// The reference's view rows are, per layer, g^l = (A S)(A'^T E'^(l-1)) summed over the layers (A, A' the two factor
// panels).  By linearity G = E^0 + (A S) P with P = A'^T T', T = sum_{l < K} E^l: two projections to [q, d] per step, and
// only the batch's rows of G are ever read — they are formed in the operand packing below.
//
//   g_b  = ego[row0 + id_b] + AS[id_b] P                       (the query rows; AS [N, q], P [q, d])
//   s_bj = <g_b, F_j> / tau,  F_j = final[row0 + j], j < N     (RAW dot products: no normalisation)
//   loss[0] = (1/B) sum_b log(sum_j exp(s_bj) + 1e-8)
//   loss[1] = (1/B) sum_b clamp(<F_id_b, g_b> / tau, -5, 5)
// Raw scores have no bound, so the log-sum-exp carries a true running maximum:
//   m_b = max_j s_bj,  S_b = sum_j exp(s_bj - m_b),  L_b = m_b + log(S_b + 1e-8 exp(-m_b))
// which is finite where exp(s) overflows fp32 and keeps the 1e-8 where every score is far below zero.
//   w_bj = up0 / (B tau) exp(s_bj - m_b) / (S_b + 1e-8 exp(-m_b)),   c_b = up1 / (B tau) [-5 <= pos_b <= 5]
//   gQ_b = sum_j w_bj F_j + c_b F_id_b,   gF_j += sum_b w_bj g_b,   gF_id_b += c_b g_b,   dP = sum_b AS[id_b]^T gQ_b
//
// Layout, as idg_tnce.hip: the operands are copied once into the workspace, rows padded with zero rows to a multiple of
// 128 and columns with zero columns to a multiple of 32; every product is v_mfma_f32_32x32x2_f32, and a score's features are
// summed 32 at a time (score_tile_chunked below).
//   prep    one wave per row: the padded table copy; the query rows g_b (the rank-q expansion, k ascending).
//   sums    grid (batch tile, table chunk): a workgroup owns 128 query rows and walks the 128-row table tiles of its
//           chunk.  Per tile: the raw scores into the 128 x 128 LDS tile (-inf past row N), the row maxima, the new running
//           maximum m', E = exp((s - m') / tau) in place, rsum = rsum exp((m - m') / tau) + sum E and — with gradients —
//           acc = acc exp((m - m') / tau) + E F, the [128, d] accumulator in registers across the tiles.  (m, rsum, acc)
//           are stored per chunk.
//   rows    one wave per query row: the chunks' (m_c, S_c, acc_c) meet in chunk order under the row's maximum; L_b, the
//           positive's dot product, the clamp, the coefficients and gQ_b; the largest term's score is taken once more in
//           double (its table row travels with the maximum) and its fp32 rounding removed from L_b to first order.  A one-workgroup fixed tree gives each loss.
//   table   grid (table tile, split): a workgroup owns 128 table rows and walks the batch tiles (the second recompute of
//           the score tile): w_bj from the stored m_b and coefficient of each column, acc += W^T Q, one store per split.
//   finish  the splits added in order into the gradient panel; the positives' part per distinct id, its occurrences in
//           batch order; gQ into the ego gradient's rows the same way; dP by the projection below with a row-id list.
// A batch below one tile (B <= 127) takes the direct form instead of the two tile passes: the scores [B, N] in double in the
// workspace (at most 127 rows), each row's maximum, sum and E F by one workgroup, the table gradient by one wave per table
// row — the same statistics, coefficients and finishing kernels, no fp32 rounding in the weights.
// The projection out = A^T X is a tall reduction: every workgroup owns a fixed run of rows and stores one [q, d] partial,
// the partials meet in the library's one slice reduction.  No float atomics, every sum in a fixed order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "idg_common.h"
#include "idg_tile128.h"

namespace {

using namespace idg::tile128;  // BLOCK, T = 128 rows of a tile, LG the row stride of the E tile, LDS_FLOATS
using idg::align256;
using idg::f32x16;
using idg::mfma_c_row;
using idg::round_up;
using idg::WAVE;
using idg::wave_sum;

constexpr int MAX_NDT = 8;  // d <= 256
constexpr int MAX_Q = 16;
constexpr int MAX_CHUNKS = 64;
constexpr int TARGET_WGS = 512;  // two 80 KB workgroups per CU
constexpr double LOG_GUARD = -18.420680743952367;  // log(1e-8)
// A batch that does not fill one 128-row score tile takes the direct form: scores, row statistics and weights in double.
// With few rows nothing averages — a gradient entry is one weight times one row, and the weight exp((s_j - m) / tau) /
// denom carries the fp32 rounding of two 1 / tau-amplified dot products — and the matrix cores would run mostly empty.
constexpr int SMALL_B = 127;

// ---------------------------------------------------------------------------------------------------------------
// The rank-q products.  A workgroup of 256 threads is cw columns (the power of two >= d, at least 32) x 256 / cw row lanes.
struct LrGeo {
  int cw_shift, lanes, slices;
  int64_t rows_per;
};

constexpr int LR_MAX_SLICES = 1024;
constexpr int LR_MIN_ROWS = 64;

LrGeo lr_geo(int64_t n, int64_t d) {
  LrGeo g;
  g.cw_shift = d <= 32 ? 5 : d <= 64 ? 6 : d <= 128 ? 7 : 8;
  g.lanes = BLOCK >> g.cw_shift;
  int64_t per = (n + LR_MAX_SLICES - 1) / LR_MAX_SLICES;
  per = per < LR_MIN_ROWS ? LR_MIN_ROWS : per;
  g.rows_per = round_up(per, g.lanes);
  g.slices = (int)((n + g.rows_per - 1) / g.rows_per);
  return g;
}

// part[slice][k][c] = sum over the slice's rows r of A[row(r)][k] X[r][c]: each row lane adds its rows ascending, the row
// lanes are added in lane order.
template <int QB>
__global__ __launch_bounds__(BLOCK) void lr_project_kernel(const float* __restrict__ A, int64_t lda,
                                                           const int64_t* __restrict__ a_rows, const float* __restrict__ X,
                                                           int64_t ldx, int64_t n, int q, int d, int cw_shift, int64_t rows_per,
                                                           int64_t a_limit, float* __restrict__ part) {
  __shared__ float s[BLOCK * QB];
  const int tid = threadIdx.x, cw = 1 << cw_shift, c = tid & (cw - 1), rl = tid >> cw_shift, lanes = BLOCK >> cw_shift;
  const int64_t lo = (int64_t)blockIdx.x * rows_per, hi = lo + rows_per < n ? lo + rows_per : n;
  const bool col = c < d;
  float acc[QB];
#pragma unroll
  for (int k = 0; k < QB; ++k) acc[k] = 0.f;
#pragma unroll 4
  for (int64_t r = lo + rl; r < hi; r += lanes) {
    const float x = col ? X[r * ldx + c] : 0.f;
    int64_t ar = a_rows ? a_rows[r] : r;
    if (a_limit > 0) ar = ar < 0 ? 0 : ar >= a_limit ? a_limit - 1 : ar;  // idg_svd_nce_f32's reading of a stray id
    const float* a = A + ar * lda;
#pragma unroll
    for (int k = 0; k < QB; ++k)
      if (k < q) acc[k] = fmaf(a[k], x, acc[k]);
  }
#pragma unroll
  for (int k = 0; k < QB; ++k) s[(rl * QB + k) * cw + c] = acc[k];
  __syncthreads();
  for (int e = tid; e < q * cw; e += BLOCK) {
    const int k = e >> cw_shift, cc = e & (cw - 1);
    float v = 0.f;
    for (int l = 0; l < lanes; ++l) v += s[(l * QB + k) * cw + cc];
    if (cc < d) part[((int64_t)blockIdx.x * q + k) * d + cc] = v;
  }
}

// Y[r] (+)= scale A[row(r)] P, k ascending.
template <int QB>
__global__ __launch_bounds__(BLOCK) void lr_expand_kernel(const float* __restrict__ A, int64_t lda,
                                                          const int64_t* __restrict__ a_rows, const float* __restrict__ P,
                                                          int64_t n, int q, int d, int cw_shift, float scale, int accumulate,
                                                          float* __restrict__ Y, int64_t ldy) {
  const int tid = threadIdx.x, cw = 1 << cw_shift, c = tid & (cw - 1), rl = tid >> cw_shift, lanes = BLOCK >> cw_shift;
  if (c >= d) return;
  float p[QB];
#pragma unroll
  for (int k = 0; k < QB; ++k) p[k] = k < q ? P[(int64_t)k * d + c] : 0.f;
  for (int64_t r = (int64_t)blockIdx.x * lanes + rl; r < n; r += (int64_t)gridDim.x * lanes) {
    const float* a = A + (a_rows ? a_rows[r] : r) * lda;
    float y = 0.f;
#pragma unroll
    for (int k = 0; k < QB; ++k)
      if (k < q) y = fmaf(a[k], p[k], y);
    float* o = Y + r * ldy + c;
    *o = accumulate ? *o + scale * y : scale * y;
  }
}

size_t lr_project_bytes(int64_t n, int64_t q, int64_t d) { return align256((size_t)lr_geo(n, d).slices * (size_t)(q * d) * 4); }

int lr_project(const float* A, int64_t lda, const int64_t* a_rows, int64_t a_limit, const float* X, int64_t ldx, int64_t n, int64_t q,
               int64_t d, float* out, bool accumulate, void* ws, hipStream_t st) {
  const LrGeo g = lr_geo(n, d);
  float* part = reinterpret_cast<float*>(ws);
#define IDG_LR_CASE(QB)                                                                                                     \
  hipLaunchKernelGGL((lr_project_kernel<QB>), dim3((unsigned)g.slices), dim3(BLOCK), 0, st, A, lda, a_rows, X, ldx, n, (int)q, \
                     (int)d, g.cw_shift, g.rows_per, a_limit, part)
  if (q <= 4) IDG_LR_CASE(4);
  else if (q <= 8) IDG_LR_CASE(8);
  else IDG_LR_CASE(16);
#undef IDG_LR_CASE
  IDG_HIP(hipGetLastError());
  return idg::slices_reduce(part, g.slices, q * d, out, accumulate, st);
}

// ---------------------------------------------------------------------------------------------------------------
// The contrastive call.
enum { MODE_SUMS = 0, MODE_SUMS_ACC = 1, MODE_TABLE = 2 };

struct Geo {
  int64_t dp, Np, Bp;
  int nt, nbt, chunks, per, splits, sper;
};

Geo geo_of(int64_t B, int64_t N, int64_t d) {
  Geo g;
  g.dp = round_up(d, 32);
  g.Np = round_up(N, T);
  g.Bp = round_up(B, T);
  g.nt = (int)(g.Np / T);
  g.nbt = (int)(g.Bp / T);
  int want = (TARGET_WGS + g.nbt - 1) / g.nbt;
  want = want < 1 ? 1 : want > MAX_CHUNKS ? MAX_CHUNKS : want;
  want = want > g.nt ? g.nt : want;
  if (B <= SMALL_B) want = 1;  // the direct form keeps one set of statistics per row
  g.per = (g.nt + want - 1) / want;
  g.chunks = (g.nt + g.per - 1) / g.per;
  // table pass: one workgroup per table tile fills the chip when there are many tiles; otherwise the batch tiles are split
  int sw = g.nt >= TARGET_WGS / 2 ? 1 : (TARGET_WGS + g.nt - 1) / g.nt;
  sw = sw > g.nbt ? g.nbt : sw;
  sw = sw > MAX_CHUNKS ? MAX_CHUNKS : sw;
  if (B <= SMALL_B) sw = 1;
  g.sper = (g.nbt + sw - 1) / sw;
  g.splits = (g.nbt + g.sper - 1) / g.sper;
  return g;
}

struct Ws {
  size_t Fp, Qp, cm, cj, rs, acc, m, a, c, lrow, dq, dT, proj, sc, stats, ad, total;
};

Ws layout(int64_t B, int64_t N, int64_t d, int64_t q) {
  const Geo g = geo_of(B, N, d);
  Ws w;
  size_t o = 0;
  const size_t rows = (size_t)g.Bp;
  w.Fp = o, o += align256((size_t)g.Np * g.dp * 4);
  w.Qp = o, o += align256(rows * g.dp * 4);
  w.cm = o, o += align256((size_t)g.chunks * rows * 4);
  w.cj = o, o += align256((size_t)g.chunks * rows * 4);
  w.rs = o, o += align256((size_t)g.chunks * rows * 4);
  w.acc = o, o += align256((size_t)g.chunks * rows * g.dp * 4);
  w.m = o, o += align256(rows * 4);
  w.a = o, o += align256(rows * 4);
  w.c = o, o += align256(rows * 4);
  w.lrow = o, o += align256(2 * rows * 8);  // doubles
  w.dq = o, o += align256(rows * g.dp * 4);
  w.dT = o, o += align256((size_t)g.splits * g.Np * g.dp * 4);
  w.proj = o, o += lr_project_bytes(B, q, d);
  w.sc = o, o += align256(B <= SMALL_B ? (size_t)B * g.Np * 8 : 0);  // the direct form: scores [B][Np], (m, S) [Bp][2],
  w.stats = o, o += align256(2 * rows * 8);                          // the coefficients [Bp], all double
  w.ad = o, o += align256(rows * 8);
  w.total = o;
  return w;
}

// An id outside [0, N) reads as the nearest row of the side: no call reads or writes outside its panels.
__device__ __forceinline__ int64_t side_id(const int64_t* __restrict__ ids, int64_t b, int64_t N) {
  const int64_t id = ids[b];
  return id < 0 ? 0 : id >= N ? N - 1 : id;
}

// Where else does the id of batch position b occur?  (an earlier position holds it, a later one does), on every lane.
__device__ __forceinline__ void occurrences(const int64_t* __restrict__ ids, int64_t B, int64_t N, int64_t b, int64_t id, int lane,
                                            bool& earlier, bool& later) {
  bool e = false, l = false;
#pragma unroll 4
  for (int64_t o = 0; o < B; o += WAVE) {
    const int64_t i = o + lane;
    const bool hit = i < B && side_id(ids, i, N) == id;
    e |= hit && i < b;
    l |= hit && i > b;
  }
  earlier = __ballot(e) != 0;
  later = __ballot(l) != 0;
}

// One wave per row of the padded operands: rows [0, Np) the table copy, then Bp query rows g_b.  Rows past N / B and columns
// past d are zero; the per-row coefficients and maxima of the padding rows are cleared.
__global__ __launch_bounds__(BLOCK) void svd_prep_kernel(const float* __restrict__ table, const float* __restrict__ ego,
                                                         const float* __restrict__ AS, const float* __restrict__ P,
                                                         const int64_t* __restrict__ ids, int64_t N, int64_t B, int64_t d, int q,
                                                         int64_t dp, int64_t Np, int64_t Bp, float* __restrict__ Fp,
                                                         float* __restrict__ Qp, float* __restrict__ m, float* __restrict__ a,
                                                         float* __restrict__ c) {
  const int64_t r = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (r >= Np + Bp) return;
  if (r < Np) {
    const float* src = r < N ? table + r * d : nullptr;
    for (int64_t f = lane; f < dp; f += WAVE) Fp[r * dp + f] = (src && f < d) ? src[f] : 0.f;
    return;
  }
  const int64_t b = r - Np;
  if (lane == 0) m[b] = a[b] = c[b] = 0.f;
  if (b >= B) {
    for (int64_t f = lane; f < dp; f += WAVE) Qp[b * dp + f] = 0.f;
    return;
  }
  const int64_t id = side_id(ids, b, N);
  const float* e = ego + id * d;
  const float* as = AS + id * q;
  for (int64_t f = lane; f < dp; f += WAVE) {
    float v = 0.f;
    if (f < d) {
      for (int k = 0; k < q; ++k) v = fmaf(as[k], P[(int64_t)k * d + f], v);
      v = e[f] + v;
    }
    Qp[b * dp + f] = v;
  }
}

// S = X Y^T as tile128::score_tile_128 lays it out, with the features added 32 at a time: each 32-column chunk is summed in
// an accumulator of its own (ascending, exact fp32 products) and the chunks' sums are added in ascending order.  The raw
// scores here are divided by tau inside an exponent, so a weight carries 1 / tau times a score's rounding; one chain of d
// terms left g_ego 3.7e-6 of its largest entry from float64 at d = 224, tau = 0.2 (plain float32 torch: 1.6e-6), the
// chains of 32 leave about a third of that.  One chunk (d <= 32) is the shared tile itself, bit for bit.  Ends behind a
// barrier, as the shared tile does.
template <int NDT>
__device__ __forceinline__ void score_tile_chunked(const float* X, const float* Y, float* s_x, float* s_y, f32x16 (&s)[2][2]) {
  if constexpr (NDT == 1) {
    score_tile_128<1>(X, Y, s_x, s_y, s);
  } else {
    constexpr int64_t dp = 32 * NDT;
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, i = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[m][n][r] = 0.f;
    // Unrolled for two chunks (d <= 64), rolled above: unrolled, the chunks' operand loads are hoisted over one another and
    // the two accumulator sets spill from d = 96 on (152 .. 752 bytes a lane at NDT 3 .. 5)
    constexpr int CHUNKS_UNROLLED = NDT <= 2 ? NDT : 1;
#pragma unroll CHUNKS_UNROLLED
    for (int kc = 0; kc < NDT; ++kc) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = tid + BLOCK * j, rr = e >> 3, c4 = (e & 7) * 4;
        *reinterpret_cast<float4*>(s_x + rr * LK + c4) = *reinterpret_cast<const float4*>(X + rr * dp + kc * KC + c4);
        *reinterpret_cast<float4*>(s_y + rr * LK + c4) = *reinterpret_cast<const float4*>(Y + rr * dp + kc * KC + c4);
      }
      __syncthreads();
      f32x16 c[2][2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) c[m][n][r] = 0.f;
      const float* pa = s_x + (64 * wr + i) * LK + 16 * h;
      const float* pb = s_y + (64 * wc + i) * LK + 16 * h;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const float4 a0 = *reinterpret_cast<const float4*>(pa + 4 * q4);
        const float4 a1 = *reinterpret_cast<const float4*>(pa + 32 * LK + 4 * q4);
        const float4 b0 = *reinterpret_cast<const float4*>(pb + 4 * q4);
        const float4 b1 = *reinterpret_cast<const float4*>(pb + 32 * LK + 4 * q4);
#define IDG_SVD_SCORE_STEP(F)                                                       \
  c[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.F, b0.F, c[0][0], 0, 0, 0);     \
  c[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.F, b1.F, c[0][1], 0, 0, 0);     \
  c[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.F, b0.F, c[1][0], 0, 0, 0);     \
  c[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.F, b1.F, c[1][1], 0, 0, 0);
        IDG_SVD_SCORE_STEP(x) IDG_SVD_SCORE_STEP(y) IDG_SVD_SCORE_STEP(z) IDG_SVD_SCORE_STEP(w)
#undef IDG_SVD_SCORE_STEP
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[m][n][r] += c[m][n][r];
      __syncthreads();
    }
  }
}

// The tile pass in its three forms.  X: the 128 rows the workgroup owns (rows of the LDS tile); Y: the tiles it walks (columns
// of the LDS tile), tile p at Y + p * 128 * dp.
//   MODE_SUMS / MODE_SUMS_ACC  X = a query tile, Y = the table tiles [lo, hi) of chunk blockIdx.y: the running maximum, the
//                              rescaled row sums and (ACC) the rescaled acc += E Y.
//   MODE_TABLE                 X = a table tile, Y = the query tiles [lo, hi) of split blockIdx.y; w_bj^T into LDS from the
//                              stored maximum and coefficient of each column, acc += that . Y.
// Wave w computes the 64 x 64 quarter (w >> 1, w & 1) of the score tile, and rows [32 w, 32 w + 32) x all columns of the second
// product, whose A operand (the tile) comes from LDS and whose B operand (Y) straight from memory (idg_tnce.hip).
// The score tile comes from score_tile_chunked: above d = 32 two sets of 64 score registers are live inside a chunk (the
// chunk's own sums and the running total), one set after it.
// Two workgroups per CU up to d = 128, except the accumulating sums form at 96 < d <= 128: its 64 accumulator registers,
// the 128 of the two score sets and the staged operands do not fit 256 registers without spilling, so it takes one.
template <int NDT, int MODE>
__global__ __launch_bounds__(BLOCK, (NDT <= 3 || (NDT == 4 && MODE != MODE_SUMS_ACC)) ? 2 : 1) void svd_tile_kernel(
    const float* __restrict__ Xall, const float* __restrict__ Yall, int per, int n_y, int64_t n_valid, float scale2,
    const float* __restrict__ ca, const float* __restrict__ cmax, float* __restrict__ out_acc, float* __restrict__ out_rs,
    float* __restrict__ out_max, int32_t* __restrict__ out_arg, int64_t out_rows) {
  constexpr int64_t dp = 32 * NDT;
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS + 4 * T];
  float* s_x = lds;            // [128][LK]   (score phase)
  float* s_y = lds + T * LK;   // [128][LK]
  float* s_g = lds;            // [128][LG]   (after the score phase)
  float* s_f = lds + LDS_FLOATS;  // [128] the rows' rescale factors of this tile
  float* s_m = s_f + T;           // [128] the rows' running maxima and [128] their running sums: in LDS, since the d = 128
  float* s_r = s_m + T;           // form with the accumulator has no two registers to spare across the score phase
  int* s_j = reinterpret_cast<int*>(s_r + T);  // [128] the table row of each running maximum (the lowest on a tie)
  const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, i = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t x0 = (int64_t)blockIdx.x * T;
  const float* X = Xall + x0 * dp;
  const int lo = blockIdx.y * per, hi = lo + per < n_y ? lo + per : n_y;

  f32x16 acc[MODE == MODE_SUMS ? 1 : NDT];
  if (MODE != MODE_SUMS) {
#pragma unroll
    for (int ct = 0; ct < NDT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  }
  // sums forms: the statistics of row x0 + tid / 2, kept by the even thread of the pair
  if (MODE != MODE_TABLE && (tid & 1) == 0) {
    s_m[tid >> 1] = -INFINITY;
    s_r[tid >> 1] = 0.f;
    s_j[tid >> 1] = 0;
  }

  for (int p = lo; p < hi; ++p) {
    const int64_t y0 = (int64_t)p * T;
    const float* Y = Yall + y0 * dp;
    f32x16 s[2][2];
    score_tile_chunked<NDT>(X, Y, s_x, s_y, s);  // ---- S = X Y^T
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = 64 * wc + 32 * n + i;
      float a_b = 0.f, m_b = 0.f;
      bool col_ok = true;
      if (MODE == MODE_TABLE) {
        a_b = ca[y0 + col];
        m_b = cmax[y0 + col];
      } else {
        col_ok = y0 + col < n_valid;
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 64 * wr + 32 * m + mfma_c_row(r, h);
          float v;
          if (MODE == MODE_TABLE) {
            v = x0 + row < n_valid ? a_b * __builtin_amdgcn_exp2f((s[m][n][r] - m_b) * scale2) : 0.f;
          } else {
            v = col_ok ? s[m][n][r] : -INFINITY;
          }
          s_g[row * LG + col] = v;
        }
    }
    __syncthreads();
    if (MODE != MODE_TABLE) {
      // thread t owns 64 columns of row t / 2: their maximum, the pair's, the running one; E in place and its sum in order
      const int row = tid >> 1, hh = tid & 1;
      float* g = s_g + row * LG + 64 * hh;
      float mx = g[0];
      int ix = 0;
#pragma unroll 8
      for (int k = 1; k < 64; ++k) {
        const float v = g[k];
        if (v > mx) mx = v, ix = k;
      }
      int jx = (int)y0 + 64 * hh + ix;
      {
        const float omx = __shfl_xor(mx, 1, WAVE);
        const int ojx = __shfl_xor(jx, 1, WAVE);
        if (omx > mx || (omx == mx && ojx < jx)) mx = omx, jx = ojx;
      }
      const float m_run = s_m[row];
      const float m_new = fmaxf(m_run, mx);  // finite: every tile holds a valid column
      float v = 0.f;
#pragma unroll 8
      for (int k = 0; k < 64; ++k) {
        const float e = __builtin_amdgcn_exp2f((g[k] - m_new) * scale2);
        g[k] = e;
        v += e;
      }
      const float o = __shfl_xor(v, 1, WAVE);
      const float f = __builtin_amdgcn_exp2f((m_run - m_new) * scale2);  // 0 at the first tile (m_run = -inf)
      __builtin_amdgcn_wave_barrier();  // both threads of the pair have read s_m[row]
      if (hh == 0) {
        s_r[row] = s_r[row] * f + (v + o);
        s_m[row] = m_new;
        s_f[row] = f;
        if (mx > m_run) s_j[row] = jx;
      }
      if (MODE == MODE_SUMS_ACC) __syncthreads();
    }
    if (MODE != MODE_SUMS) {
      if (MODE == MODE_SUMS_ACC) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float f = s_f[32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h];
#pragma unroll
          for (int ct = 0; ct < NDT; ++ct) acc[ct][r] *= f;
        }
      }
      // ---- acc += tile . Y: A = tile[32 wave + i][k] from LDS, B = Y[k][32 ct + i] from memory; lane half h feeds
      // k in [64 h, 64 h + 64)
      const float* ga = s_g + (32 * wave + i) * LG + 64 * h;
      const float* yb = Y + (int64_t)(64 * h) * dp + i;
#pragma unroll
      for (int ct = 0; ct < NDT; ++ct) {
#pragma unroll 8
        for (int k = 0; k < 64; ++k)
          acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[k], yb[k * dp + 32 * ct], acc[ct], 0, 0, 0);
      }
    }
    __syncthreads();  // the tile is overwritten by the next tile's operands
  }

  if (MODE != MODE_SUMS) {
    float* out = out_acc + ((int64_t)blockIdx.y * out_rows + x0) * dp;
#pragma unroll
    for (int ct = 0; ct < NDT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
        out[(int64_t)row * dp + 32 * ct + i] = acc[ct][r];
      }
  }
  if (MODE != MODE_TABLE && (tid & 1) == 0) {
    out_rs[(int64_t)blockIdx.y * out_rows + x0 + (tid >> 1)] = s_r[tid >> 1];
    out_max[(int64_t)blockIdx.y * out_rows + x0 + (tid >> 1)] = s_m[tid >> 1];
    out_arg[(int64_t)blockIdx.y * out_rows + x0 + (tid >> 1)] = s_j[tid >> 1];
  }
}

// ---- The direct form (B <= SMALL_B), in place of the two tile passes.
// One wave per table row j: sc[b][j] = <Q_b, F_j> in double, the features added lane-strided then by the wave's butterfly.
__global__ __launch_bounds__(BLOCK) void svd_small_scores_kernel(const float* __restrict__ Fp, const float* __restrict__ Qp,
                                                                 int64_t N, int64_t Np, int64_t B, int64_t dp,
                                                                 double* __restrict__ sc) {
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (j >= N) return;
  double t[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) t[u] = lane + WAVE * u < dp ? (double)Fp[j * dp + lane + WAVE * u] : 0.;
  for (int64_t b = 0; b < B; ++b) {
    double v = 0.;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (lane + WAVE * u < dp) v += t[u] * (double)Qp[b * dp + lane + WAVE * u];
    v = wave_sum(v);
    if (lane == 0) sc[b * Np + j] = v;
  }
}

// One workgroup per batch row b: the maximum (the lowest table row on a tie) and S = sum_j exp((s_j - m) / tau) by fixed
// trees, and with gradients acc[f] = sum_j exp((s_j - m) / tau) F_j[f], j ascending, thread f.
__global__ __launch_bounds__(BLOCK) void svd_small_stats_kernel(const float* __restrict__ Fp, const double* __restrict__ sc,
                                                                int64_t N, int64_t Np, int64_t dp, double inv_tau, int grads,
                                                                double* __restrict__ stats, int32_t* __restrict__ cj,
                                                                float* __restrict__ pacc) {
  __shared__ double sd[BLOCK];
  __shared__ int si[BLOCK];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* s = sc + b * Np;
  double mx = -INFINITY;
  int ix = 0;
  for (int64_t j = tid; j < N; j += BLOCK) {
    const double v = s[j];
    if (v > mx) mx = v, ix = (int)j;
  }
  sd[tid] = mx;
  si[tid] = ix;
  __syncthreads();
  for (int o = BLOCK / 2; o > 0; o >>= 1) {
    if (tid < o && (sd[tid + o] > sd[tid] || (sd[tid + o] == sd[tid] && si[tid + o] < si[tid]))) {
      sd[tid] = sd[tid + o];
      si[tid] = si[tid + o];
    }
    __syncthreads();
  }
  const double m = sd[0];
  const int jm = si[0];
  __syncthreads();
  double part = 0.;
  for (int64_t j = tid; j < N; j += BLOCK) part += exp((s[j] - m) * inv_tau);
  const double S = idg::block_tree_sum<BLOCK>(part, sd);
  if (tid == 0) {
    stats[2 * b] = m;
    stats[2 * b + 1] = S;
    cj[b] = jm;
  }
  if (!grads) return;
  double a = 0.;
  for (int64_t j0 = 0; j0 < N; j0 += BLOCK) {
    __syncthreads();
    sd[tid] = j0 + tid < N ? exp((s[j0 + tid] - m) * inv_tau) : 0.;
    __syncthreads();
    if (tid < dp) {
      const int lim = N - j0 < BLOCK ? (int)(N - j0) : BLOCK;
      for (int k = 0; k < lim; ++k) a += sd[k] * (double)Fp[(j0 + k) * dp + tid];
    }
  }
  if (tid < dp) pacc[b * dp + tid] = (float)a;
}

// One wave per table row j: dT[j] = sum_b a_b exp((s_bj - m_b) / tau) Q_b, b ascending, in double; rounded once.
__global__ __launch_bounds__(BLOCK) void svd_small_table_kernel(const float* __restrict__ Qp, const double* __restrict__ sc,
                                                                const double* __restrict__ stats, const double* __restrict__ a_d,
                                                                int64_t N, int64_t Np, int64_t B, int64_t dp, double inv_tau,
                                                                float* __restrict__ dT) {
  __shared__ double sw[BLOCK / WAVE][SMALL_B + 1];
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / WAVE) + wave;
  const bool live = j < N;
  for (int b = lane; b <= SMALL_B; b += WAVE)
    sw[wave][b] = live && b < B ? a_d[b] * exp((sc[(int64_t)b * Np + j] - stats[2 * b]) * inv_tau) : 0.;
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < dp) {
      double v = 0.;
      for (int64_t b = 0; b < B; ++b) v += sw[wave][b] * (double)Qp[b * dp + f];
      dT[j * dp + f] = (float)v;
    }
  }
}

// One wave per query row b: the chunks meet under the row's maximum (chunk order), L_b, the positive, the clamp, and with
// gradients the coefficients and gQ_b (dq: [Bp][dp], the first d columns used).  The scalars in double.
__global__ __launch_bounds__(BLOCK) void svd_rows_kernel(const float* __restrict__ Fp, const float* __restrict__ Qp,
                                                         const float* __restrict__ ego, const float* __restrict__ AS,
                                                         const float* __restrict__ P, int64_t d, int q,
                                                         const int64_t* __restrict__ ids, int64_t B, int64_t N, int64_t Bp,
                                                         int64_t dp, int chunks, const float* __restrict__ cm,
                                                         const int32_t* __restrict__ cj, const float* __restrict__ rs, const float* __restrict__ pacc,
                                                         double inv_tau, const float* __restrict__ upstream, int grads,
                                                         double* __restrict__ lrow, float* __restrict__ m_out,
                                                         float* __restrict__ a, float* __restrict__ c, float* __restrict__ dq,
                                                         const double* __restrict__ small_stats, double* __restrict__ a_d) {
  const int64_t b = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (b >= B) return;
  double m, S = 0.;
  int64_t jmax = cj[b];
  if (small_stats) {  // the direct form: (m, S) in double, one chunk
    m = small_stats[2 * b];
    S = small_stats[2 * b + 1];
  } else {
    float mf = cm[b];
    for (int ch = 1; ch < chunks; ++ch) {
      const float mc = cm[(int64_t)ch * Bp + b];
      if (mc > mf) mf = mc, jmax = cj[(int64_t)ch * Bp + b];  // chunks ascend: the lowest row on a tie
    }
    for (int ch = 0; ch < chunks; ++ch)
      S += (double)rs[(int64_t)ch * Bp + b] * exp((double)(cm[(int64_t)ch * Bp + b] - mf) * inv_tau);
    m = (double)mf;
  }
  // log(S e^m' + 1e-8) = m' + log(S + e^t), t = log(1e-8) - m'; S >= 1 (the maximum's own term)
  const double mt = m * inv_tau, t = LOG_GUARD - mt;
  const bool guard_only = t > 600.;  // every score below -580: the sum is 1e-8 to all places
  const double denom = guard_only ? 1. : S + exp(t);
  double L = guard_only ? LOG_GUARD : mt + log(denom);
  const int64_t id = side_id(ids, b, N);
  // The row's two scalar scores — the positive's and the largest term's — once more in double, from the view row formed in
  // double (the operand copy Qp carries the fp32 rounding of ego + AS P, which 1 / tau multiplies).  d L / d s_max =
  // 1 / denom, so (s*_max - s_max) / (tau denom) takes the fp32 rounding of that one dot product out of L: all of L's error
  // where one score dominates (a one-row table, a batch of one id), where no averaging over terms or rows hides it.
  const float* t_pos = Fp + id * dp;
  const float* t_max = Fp + jmax * dp;
  float tp[4];
  double dot = 0., dm = 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    tp[u] = 0.f;
    if (f < dp) tp[u] = t_pos[f];
    if (f < d) {
      double gd = 0.;
      for (int k = 0; k < q; ++k) gd += (double)AS[id * q + k] * (double)P[(int64_t)k * d + f];
      gd += (double)ego[id * d + f];
      dot += (double)tp[u] * gd;
      dm += (double)t_max[f] * gd;
    }
  }
  dot = wave_sum(dot);
  dm = wave_sum(dm);
  if (!guard_only) L += (dm - m) * inv_tau / denom;
  const double pos = dot * (double)inv_tau;
  const bool inside = pos >= -5. && pos <= 5.;
  if (lane == 0) {
    lrow[b] = L;
    lrow[Bp + b] = pos < -5. ? -5. : pos > 5. ? 5. : pos;
  }
  if (!grads) return;
  const double up0 = upstream ? (double)upstream[0] : 1., up1 = upstream ? (double)upstream[1] : 1.;
  const float ab = guard_only ? 0.f : (float)(up0 * (double)inv_tau / ((double)B * denom));
  const float cb = inside ? (float)(up1 * (double)inv_tau / (double)B) : 0.f;
  float g[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ch = 0; ch < chunks; ++ch) {
    const float fc = small_stats ? 1.f : (float)exp(((double)cm[(int64_t)ch * Bp + b] - m) * inv_tau);
    const float* pa = pacc + ((int64_t)ch * Bp + b) * dp;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t f = lane + WAVE * u;
      if (f < dp) g[u] = fmaf(fc, pa[f], g[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < dp) dq[b * dp + f] = fmaf(cb, tp[u], ab * g[u]);
  }
  if (lane == 0) {
    m_out[b] = (float)m;
    a[b] = ab;
    c[b] = cb;
    if (a_d) a_d[b] = guard_only ? 0. : up0 * inv_tau / ((double)B * denom);
  }
}

// loss[k] = (1/B) sum_b lrow[k][b] by a fixed tree of 1024 leaves, in double (the rows' terms are of one size and sign: in
// fp32 the mean would carry the sum's rounding, a few units in the last place); one workgroup per entry.
__global__ __launch_bounds__(1024) void svd_loss_kernel(const double* __restrict__ lrow, int64_t B, int64_t Bp, float* __restrict__ loss) {
  __shared__ double s[1024];
  const int tid = threadIdx.x, k = blockIdx.x;
  double acc = 0.;
  for (int64_t b = tid; b < B; b += 1024) acc += lrow[(int64_t)k * Bp + b];
  const double sum = idg::block_tree_sum<1024>(acc, s);
  if (tid == 0) loss[k] = (float)(sum / (double)B);
}

// One wave per table row: the splits added in order, then added to the gradient panel.
__global__ __launch_bounds__(BLOCK) void svd_table_finish_kernel(const float* __restrict__ dT, int64_t N, int64_t Np, int64_t d,
                                                                 int64_t dp, int splits, float* __restrict__ g_table) {
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (j >= N) return;
  for (int64_t f = lane; f < d; f += WAVE) {
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += dT[((int64_t)sp * Np + j) * dp + f];
    g_table[j * d + f] += s;
  }
}

// One wave per batch position b: if no earlier position holds the same id, coef[bb] src[bb] (coef NULL: 1) of every occurrence
// bb of the id is added in batch order and the sum added to row id of the panel.
__global__ __launch_bounds__(BLOCK) void svd_scatter_kernel(const int64_t* __restrict__ ids, const float* __restrict__ src,
                                                            const float* __restrict__ coef, int64_t B, int64_t N, int64_t d,
                                                            int64_t dp, float* __restrict__ g_panel) {
  const int64_t b = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (b >= B) return;
  const int64_t id = side_id(ids, b, N);
  bool earlier, later;
  occurrences(ids, B, N, b, id, lane, earlier, later);
  if (earlier) return;
  const int64_t end = later ? B : 0;
  // the running total starts from the panel's value: one rounding per occurrence, none for a separate final addition
  const float c0 = coef ? coef[b] : 1.f;
  float g[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    g[u] = lane + WAVE * u < d ? fmaf(c0, src[b * dp + lane + WAVE * u], g_panel[id * d + lane + WAVE * u]) : 0.f;
  for (int64_t o = b + 1 - ((b + 1) % WAVE); o < end; o += WAVE) {
    const bool hit = o + lane > b && o + lane < end && side_id(ids, o + lane, N) == id;
    unsigned long long mk = __ballot(hit);
    while (mk) {
      const int64_t bb = o + __builtin_ctzll(mk);
      mk &= mk - 1;
      const float cc = coef ? coef[bb] : 1.f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (lane + WAVE * u < d) g[u] = fmaf(cc, src[bb * dp + lane + WAVE * u], g[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (lane + WAVE * u < d) g_panel[id * d + lane + WAVE * u] = g[u];
}

template <int MODE>
void launch_tile(int ndt, dim3 grid, hipStream_t st, const float* X, const float* Y, int per, int n_y, int64_t n_valid,
                 float scale2, const float* ca, const float* cmax, float* out_acc, float* out_rs, float* out_max,
                 int32_t* out_arg, int64_t out_rows) {
  switch (ndt) {
#define IDG_SVD_CASE(NN)                                                                                                  \
  case NN:                                                                                                                \
    hipLaunchKernelGGL((svd_tile_kernel<NN, MODE>), grid, dim3(BLOCK), 0, st, X, Y, per, n_y, n_valid, scale2, ca, cmax,   \
                       out_acc, out_rs, out_max, out_arg, out_rows);                                                      \
    break;
    IDG_SVD_CASE(1) IDG_SVD_CASE(2) IDG_SVD_CASE(3) IDG_SVD_CASE(4)
    IDG_SVD_CASE(5) IDG_SVD_CASE(6) IDG_SVD_CASE(7) IDG_SVD_CASE(8)
#undef IDG_SVD_CASE
  }
}

bool lr_sizes_ok(int64_t n, int64_t q, int64_t d) { return n >= 1 && q >= 1 && q <= MAX_Q && d >= 1 && d <= 32 * MAX_NDT; }

}  // namespace

extern "C" {

size_t idg_lowrank_project_workspace_bytes(int64_t n, int64_t q, int64_t d) {
  if (!lr_sizes_ok(n, q, d)) return 0;
  return lr_project_bytes(n, q, d);
}

int idg_lowrank_project_f32(const float* A, int64_t lda, const int64_t* a_rows, const float* X, int64_t ldx, int64_t n,
                            int64_t q, int64_t d, float* out, int accumulate, void* ws, void* stream) {
  IDG_REQUIRE(A && X && out && ws, "idg_lowrank_project_f32: NULL argument");
  IDG_REQUIRE(lr_sizes_ok(n, q, d), "idg_lowrank_project_f32: n = %lld, q = %lld, d = %lld (n >= 1, 1 <= q <= %d, 1 <= d <= %d)",
              (long long)n, (long long)q, (long long)d, MAX_Q, 32 * MAX_NDT);
  IDG_REQUIRE(lda >= q && ldx >= d, "idg_lowrank_project_f32: a leading dimension below its row's width");
  IDG_REQUIRE((uintptr_t)ws % 256 == 0, "idg_lowrank_project_f32: the workspace must be 256-byte aligned");
  return lr_project(A, lda, a_rows, 0, X, ldx, n, q, d, out, accumulate != 0, ws, (hipStream_t)stream);
}

int idg_lowrank_expand_f32(const float* A, int64_t lda, const int64_t* a_rows, const float* P, int64_t n, int64_t q, int64_t d,
                           float scale, int accumulate, float* Y, int64_t ldy, void* stream) {
  IDG_REQUIRE(A && P && Y, "idg_lowrank_expand_f32: NULL argument");
  IDG_REQUIRE(lr_sizes_ok(n, q, d), "idg_lowrank_expand_f32: n = %lld, q = %lld, d = %lld (n >= 1, 1 <= q <= %d, 1 <= d <= %d)",
              (long long)n, (long long)q, (long long)d, MAX_Q, 32 * MAX_NDT);
  IDG_REQUIRE(lda >= q && ldy >= d, "idg_lowrank_expand_f32: a leading dimension below its row's width");
  const LrGeo g = lr_geo(n, d);
  int64_t wgs = (n + g.lanes - 1) / g.lanes;
  wgs = wgs > 4096 ? 4096 : wgs;
  hipStream_t st = (hipStream_t)stream;
#define IDG_LR_CASE(QB)                                                                                                  \
  hipLaunchKernelGGL((lr_expand_kernel<QB>), dim3((unsigned)wgs), dim3(BLOCK), 0, st, A, lda, a_rows, P, n, (int)q, (int)d, \
                     g.cw_shift, scale, accumulate ? 1 : 0, Y, ldy)
  if (q <= 4) IDG_LR_CASE(4);
  else if (q <= 8) IDG_LR_CASE(8);
  else IDG_LR_CASE(16);
#undef IDG_LR_CASE
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

size_t idg_svd_nce_workspace_bytes(int64_t B, int64_t N, int64_t d, int64_t q) {
  if (B <= 0 || N <= 0 || d <= 0 || d > 32 * MAX_NDT || q < 1 || q > MAX_Q) return 0;
  if (N >= ((int64_t)1 << 31) - T || B >= ((int64_t)1 << 31) - T) return 0;
  return layout(B, N, d, q).total;
}

int idg_svd_nce_f32(const float* final_panel, const float* ego_panel, int64_t row0, int64_t N, int64_t d, const float* AS,
                    int64_t q, const float* P, const int64_t* ids, int64_t B, float temperature, float* loss,
                    const float* upstream, float* g_final_panel, float* g_ego_panel, float* dP, void* ws, void* stream) {
  IDG_REQUIRE(final_panel && ego_panel && AS && P && ids && ws, "idg_svd_nce_f32: NULL argument");
  IDG_REQUIRE(B >= 1 && N >= 1 && row0 >= 0, "idg_svd_nce_f32: bad sizes (B = %lld, N = %lld, row0 = %lld)", (long long)B,
              (long long)N, (long long)row0);
  IDG_REQUIRE(d >= 1 && d <= 32 * MAX_NDT, "idg_svd_nce_f32: d = %lld (1 .. %d are built)", (long long)d, 32 * MAX_NDT);
  IDG_REQUIRE(q >= 1 && q <= MAX_Q, "idg_svd_nce_f32: q = %lld (1 .. %d are built)", (long long)q, MAX_Q);
  IDG_REQUIRE(N < ((int64_t)1 << 31) - T && B < ((int64_t)1 << 31) - T, "idg_svd_nce_f32: sizes exceed int32 positions");
  IDG_REQUIRE(temperature > 0.f && std::isfinite(temperature), "idg_svd_nce_f32: temperature must be positive");
  const bool grads = g_final_panel || g_ego_panel || dP;
  IDG_REQUIRE(!grads || (g_final_panel && g_ego_panel && dP), "idg_svd_nce_f32: the gradient outputs go together");
  IDG_REQUIRE(grads || loss, "idg_svd_nce_f32: nothing to compute");
  IDG_REQUIRE((uintptr_t)ws % 256 == 0, "idg_svd_nce_f32: the workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Geo g = geo_of(B, N, d);
  const Ws w = layout(B, N, d, q);
  char* base = reinterpret_cast<char*>(ws);
  float* Fp = reinterpret_cast<float*>(base + w.Fp);
  float* Qp = reinterpret_cast<float*>(base + w.Qp);
  float* cm = reinterpret_cast<float*>(base + w.cm);
  int32_t* cj = reinterpret_cast<int32_t*>(base + w.cj);
  float* rs = reinterpret_cast<float*>(base + w.rs);
  float* pacc = reinterpret_cast<float*>(base + w.acc);
  float* rm = reinterpret_cast<float*>(base + w.m);
  float* ca = reinterpret_cast<float*>(base + w.a);
  float* cc = reinterpret_cast<float*>(base + w.c);
  double* lrow = reinterpret_cast<double*>(base + w.lrow);
  float* dq = reinterpret_cast<float*>(base + w.dq);
  float* dT = reinterpret_cast<float*>(base + w.dT);
  const float* table = final_panel + row0 * d;
  const float* ego = ego_panel + row0 * d;
  const int ndt = (int)(g.dp / 32);
  const int wpb = BLOCK / WAVE;
  const double inv_tau = 1. / (double)temperature;  // one rounding in scale2, none in the rows kernel's scalars
  const float scale2 = (float)(inv_tau * 1.4426950408889634);

  hipLaunchKernelGGL(svd_prep_kernel, dim3((unsigned)((g.Np + g.Bp + wpb - 1) / wpb)), dim3(BLOCK), 0, st, table, ego, AS, P, ids,
                     N, B, d, (int)q, g.dp, g.Np, g.Bp, Fp, Qp, rm, ca, cc);
  const bool small = B <= SMALL_B;
  double* sc = reinterpret_cast<double*>(base + w.sc);
  double* stats = reinterpret_cast<double*>(base + w.stats);
  double* ad = reinterpret_cast<double*>(base + w.ad);
  const dim3 grid1((unsigned)g.nbt, (unsigned)g.chunks);
  if (small) {
    hipLaunchKernelGGL(svd_small_scores_kernel, dim3((unsigned)((N + wpb - 1) / wpb)), dim3(BLOCK), 0, st, Fp, Qp, N, g.Np, B, g.dp, sc);
    hipLaunchKernelGGL(svd_small_stats_kernel, dim3((unsigned)B), dim3(BLOCK), 0, st, Fp, sc, N, g.Np, g.dp, inv_tau, grads ? 1 : 0,
                       stats, cj, pacc);
  } else if (grads)
    launch_tile<MODE_SUMS_ACC>(ndt, grid1, st, Qp, Fp, g.per, g.nt, N, scale2, nullptr, nullptr, pacc, rs, cm, cj, g.Bp);
  else
    launch_tile<MODE_SUMS>(ndt, grid1, st, Qp, Fp, g.per, g.nt, N, scale2, nullptr, nullptr, nullptr, rs, cm, cj, g.Bp);
  hipLaunchKernelGGL(svd_rows_kernel, dim3((unsigned)((B + wpb - 1) / wpb)), dim3(BLOCK), 0, st, Fp, Qp, ego, AS, P, d, (int)q, ids, B, N, g.Bp, g.dp,
                     g.chunks, cm, cj, rs, pacc, inv_tau, upstream, grads ? 1 : 0, lrow, rm, ca, cc, dq, small ? stats : nullptr,
                     small ? ad : nullptr);
  if (loss) hipLaunchKernelGGL(svd_loss_kernel, dim3(2), dim3(1024), 0, st, lrow, B, g.Bp, loss);
  if (grads) {
    const dim3 grid2((unsigned)g.nt, (unsigned)g.splits);
    if (small)
      hipLaunchKernelGGL(svd_small_table_kernel, dim3((unsigned)((N + wpb - 1) / wpb)), dim3(BLOCK), 0, st, Qp, sc, stats, ad, N, g.Np,
                         B, g.dp, inv_tau, dT);
    else
      launch_tile<MODE_TABLE>(ndt, grid2, st, Fp, Qp, g.sper, g.nbt, N, scale2, ca, rm, dT, nullptr, nullptr, nullptr, g.Np);
    float* g_table = g_final_panel + row0 * d;
    hipLaunchKernelGGL(svd_table_finish_kernel, dim3((unsigned)((N + wpb - 1) / wpb)), dim3(BLOCK), 0, st, dT, N, g.Np, d, g.dp,
                       g.splits, g_table);
    const dim3 gb((unsigned)((B + wpb - 1) / wpb));
    hipLaunchKernelGGL(svd_scatter_kernel, gb, dim3(BLOCK), 0, st, ids, Qp, cc, B, N, d, g.dp, g_table);
    hipLaunchKernelGGL(svd_scatter_kernel, gb, dim3(BLOCK), 0, st, ids, dq, nullptr, B, N, d, g.dp, g_ego_panel + row0 * d);
    IDG_HIP(hipGetLastError());
    // dP = sum_b AS[id_b]^T gQ_b
    return lr_project(AS, q, ids, N, dq, g.dp, B, q, d, dP, false, base + w.proj, st);
  }
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
