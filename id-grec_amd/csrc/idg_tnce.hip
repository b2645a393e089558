// Full-table contrastive loss (CGCL, He et al. SIGIR'23: models/CGCL.py:95-215 of the reference; the same expression as
// losses.get_InfoNCE_loss_all and NCL's structural term): every batch row scored against a whole normalised embedding
// table, forward and backward, without the [B, N] score matrix.
//
//   Th = normalize(table rows [row0, row0 + N)),  Qh_k = normalize(panel_k[ids_k]),  s_bj = <Qh_b, Th_j>,  p = pos_ids[b]
//   r_b = exp(s_bp / tau) / sum_j exp(s_bj / tau),      loss[k] = -w_k sum_b log(r_b + 1e-7)
//   G_bj = c_b (e_bj / S_b - [j = p]),  c_b = up_k w_k r_b / (r_b + 1e-7) / tau,  dQh = G Th,  dTh = G^T Qh
// Scores are cosines, so e_bj = exp((s_bj - 1) / tau) <= 1 needs no running maximum (the common factor exp(-1 / tau)
// cancels in r_b); S_b = sum_j e_bj.
//
// Layout.  The normalised operands are copied once into the workspace, rows padded with zero rows to a multiple of 128
// and columns with zero columns to a multiple of 32 (so d = 48 or 100 run the same matrix-core tiles as 64 and 128, and no
// tile needs a bounds check on its loads).  Every product is v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums.
//   prep      one wave per row: norms, the normalised copies, cleared per-row coefficients.
//   sums      grid (batch tile x query block, table chunk): a workgroup owns 128 query rows and walks the 128-row table
//             tiles of its chunk.  Per tile: S = Q T^T from 32-column LDS chunks, E = exp((S - 1) / tau) (0 past row N)
//             into a 128 x 128 LDS tile (row stride 129), its row sums, and — when gradients are wanted — acc += E Th with the
//             [128, d] accumulator in registers across the tiles.  acc and the row sums are stored per chunk.  E carries
//             no per-row coefficient, so this one pass is both the statistics pass and the batch-major gradient pass:
//             dQh_b = a_b sum_chunks acc_b - c_b Th_p with a_b = c_b / S_b, applied by the rows kernel.
//   rows      one wave per query row: S_b (chunk order), r_b from the positive's own e (picked out of its tile), the loss term, a_b, c_b, dQh_b in chunk
//             order, back through the normalisation.  A one-workgroup fixed tree per block gives loss[k].
//   table     grid (table tile, split): a workgroup owns 128 table rows and walks the batch tiles of every query block
//             (the second recompute of the score tile): a_b E^T into the LDS tile, acc += (a E)^T Qh in registers across
//             all batch tiles, one store per split.  The positives' part -c_b Qh_b of row p is not in this sum.
//   finish    one wave per table row: splits added in order, back through the normalisation, ADDED to the gradient
//             panel; then the positives' part, one wave per distinct positive, its occurrences in batch order.  Query rows: one wave per batch position, the first occurrence of an id adds every occurrence in
//             batch order into the panel row (an ordered sum; the blocks one launch after the other).
// No float atomics, every sum in a fixed order: the same bits every run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "idg_common.h"
#include "idg_tile128.h"

namespace {

using namespace idg::tile128;  // T = 128 rows of a query / table tile, LG the row stride of the E / G tile, LDS_FLOATS
using idg::align256;
using idg::f32x16;
using idg::mfma_c_row;
using idg::round_up;
using idg::WAVE;
using idg::wave_sum;

constexpr int MAX_NDT = 8;    // d <= 256
constexpr int MAX_NQ = IDG_TNCE_MAX_QUERY_BLOCKS;
constexpr int MAX_CHUNKS = 64;
constexpr int TARGET_WGS = 512;  // two 80 KB workgroups per CU
constexpr float NORM_EPS = 1e-12f;
constexpr float GUARD = 1e-7f;   // the reference's 10e-8

enum { MODE_SUMS = 0, MODE_SUMS_ACC = 1, MODE_TABLE = 2 };

// Where else does the id of batch position b occur?  One pass over the list with independent loads: (an earlier position
// holds it, a later one does) — the same on every lane.
__device__ __forceinline__ void occurrences(const int64_t* __restrict__ ids, int64_t B, int64_t b, int64_t id, int lane,
                                            bool& earlier, bool& later) {
  bool e = false, l = false;
#pragma unroll 4
  for (int64_t o = 0; o < B; o += WAVE) {
    const int64_t i = o + lane;
    const bool hit = i < B && ids[i] == id;
    e |= hit && i < b;
    l |= hit && i > b;
  }
  earlier = __ballot(e) != 0;
  later = __ballot(l) != 0;
}

struct Geo {
  int64_t dp, Np, Bp;
  int nt, nbt, chunks, per, splits, sper;
};

Geo geo_of(int64_t B, int64_t N, int64_t d, int nq) {
  Geo g;
  g.dp = round_up(d, 32);
  g.Np = round_up(N, T);
  g.Bp = round_up(B, T);
  g.nt = (int)(g.Np / T);
  g.nbt = (int)(g.Bp / T);
  const int owners = g.nbt * nq;
  int want = (TARGET_WGS + owners - 1) / owners;
  want = want < 1 ? 1 : want > MAX_CHUNKS ? MAX_CHUNKS : want;
  want = want > g.nt ? g.nt : want;
  g.per = (g.nt + want - 1) / want;
  g.chunks = (g.nt + g.per - 1) / g.per;
  // table pass: one workgroup per table tile fills the chip when there are many tiles; otherwise the batch tiles are split
  int sw = g.nt >= TARGET_WGS / 2 ? 1 : (TARGET_WGS + g.nt - 1) / g.nt;
  sw = sw > owners ? owners : sw;
  sw = sw > MAX_CHUNKS ? MAX_CHUNKS : sw;
  g.sper = (owners + sw - 1) / sw;
  g.splits = (owners + g.sper - 1) / g.sper;
  return g;
}

struct Ws {
  size_t Th, tinv, Qh, qinv, rs, acc, S, a, c, lrow, dq, dT, total;
};

Ws layout(int64_t B, int64_t N, int64_t d, int nq) {
  const Geo g = geo_of(B, N, d, nq);
  Ws w;
  size_t o = 0;
  const size_t rows = (size_t)nq * g.Bp;
  w.Th = o, o += align256((size_t)g.Np * g.dp * 4);
  w.tinv = o, o += align256((size_t)g.Np * 4);
  w.Qh = o, o += align256(rows * g.dp * 4);
  w.qinv = o, o += align256(rows * 4);
  w.rs = o, o += align256((size_t)g.chunks * rows * 4);
  w.acc = o, o += align256((size_t)g.chunks * rows * g.dp * 4);
  w.S = o, o += align256(rows * 4);
  w.a = o, o += align256(rows * 4);
  w.c = o, o += align256(rows * 4);
  w.lrow = o, o += align256(rows * 4);
  w.dq = o, o += align256(rows * g.dp * 4);
  w.dT = o, o += align256((size_t)g.splits * g.Np * g.dp * 4);
  w.total = o;
  return w;
}

struct QueryArgs {
  const float* panel[MAX_NQ];
  const int64_t* ids[MAX_NQ];
  float weight[MAX_NQ];
};

// One wave per row of the padded operands: rows [0, Np) the table, then nq blocks of Bp query rows.  Rows past N / B and
// columns past d are zero.  inv = 1 / max(||x||, 1e-12) (F.normalize), 0 for a padding row.
__global__ __launch_bounds__(BLOCK) void tnce_prep_kernel(const float* __restrict__ table, QueryArgs q, int64_t N, int64_t B,
                                                          int64_t d, int64_t dp, int64_t Np, int64_t Bp, int nq,
                                                          float* __restrict__ Th, float* __restrict__ tinv,
                                                          float* __restrict__ Qh, float* __restrict__ qinv,
                                                          float* __restrict__ a, float* __restrict__ c) {
  const int64_t r = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (r >= Np + (int64_t)nq * Bp) return;
  const float* src = nullptr;
  float *dst, *inv;
  if (r < Np) {
    if (r < N) src = table + r * d;
    dst = Th + r * dp;
    inv = tinv + r;
  } else {
    const int64_t e = r - Np;
    const int k = (int)(e / Bp);
    const int64_t b = e - (int64_t)k * Bp;
    if (b < B) src = q.panel[k] + q.ids[k][b] * d;
    dst = Qh + e * dp;
    inv = qinv + e;
    if (lane == 0) {
      a[e] = 0.f;
      c[e] = 0.f;
    }
  }
  float ss = 0.f;
  if (src)
    for (int64_t f = lane; f < d; f += WAVE) ss = fmaf(src[f], src[f], ss);
  ss = wave_sum(ss);
  const float iv = src ? 1.f / fmaxf(sqrtf(ss), NORM_EPS) : 0.f;
  for (int64_t f = lane; f < dp; f += WAVE) dst[f] = (src && f < d) ? src[f] * iv : 0.f;
  if (lane == 0) *inv = iv;
}

// The tile pass in its three forms.  X: the 128 rows the workgroup owns (rows of the LDS tile); Y: the tiles it walks
// (columns of the LDS tile), tile p at Y + p * 128 * dp.
//   MODE_SUMS / MODE_SUMS_ACC  X = a query tile, Y = the table tiles [lo, hi) of chunk blockIdx.y; E into LDS, row sums,
//                              and (ACC) acc += E Y.
//   MODE_TABLE                 X = a table tile, Y = the query tiles [lo, hi) of split blockIdx.y (all blocks, 128 rows
//                              each); (a_b e_bj)^T into LDS from the per-row coefficient of each column, acc += that . Y.
// Wave w computes the 64 x 64 quarter (w >> 1, w & 1) of the score tile as 2 x 2 MFMA blocks, and rows [32 w, 32 w + 32) x all
// columns of the second product.  C/D map of a block: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
// The second product takes its A operand (the tile) from LDS and its B operand (Y) straight from memory, 128-byte row
// pieces that all four waves share through the L1: no barrier inside it.
template <int NDT, int MODE>
__global__ __launch_bounds__(BLOCK, NDT <= 4 ? 2 : 1) void tnce_tile_kernel(
    const float* __restrict__ Xall, const float* __restrict__ Yall, int per, int n_y, int64_t n_valid, float scale2,
    const float* __restrict__ ca, float* __restrict__ out_acc,
    float* __restrict__ out_rs, int64_t out_rows, const int64_t* __restrict__ pos_ids, int64_t B, int64_t Bp,
    float* __restrict__ out_epos) {
  constexpr int64_t dp = 32 * NDT;
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  float* s_x = lds;            // [128][LK]   (score phase)
  float* s_y = lds + T * LK;   // [128][LK]
  float* s_g = lds;            // [128][LG]   (after the score phase)
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
  float rsum = 0.f;
  // sums forms: the positive of the row whose sums this thread adds (row x0 + tid / 2 of block (x0 + tid / 2) / Bp)
  int64_t my_pos = -1;
  if (MODE != MODE_TABLE) {
    const int64_t b = (x0 + (tid >> 1)) % Bp;
    if (b < B) my_pos = pos_ids[b];
  }

  for (int p = lo; p < hi; ++p) {
    const int64_t y0 = (int64_t)p * T;
    const float* Y = Yall + y0 * dp;
    f32x16 s[2][2];
    score_tile_128<NDT>(X, Y, s_x, s_y, s);  // ---- S = X Y^T
    // ---- the E / G^T tile
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = 64 * wc + 32 * n + i;
      float a_b = 0.f;
      bool col_ok = true;
      if (MODE == MODE_TABLE) {
        a_b = ca[y0 + col];
      } else {
        col_ok = y0 + col < n_valid;
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 64 * wr + 32 * m + mfma_c_row(r, h);
          const float e = __builtin_amdgcn_exp2f((s[m][n][r] - 1.f) * scale2);
          float v;
          if (MODE == MODE_TABLE) v = a_b * e;
          else v = col_ok ? e : 0.f;
          s_g[row * LG + col] = v;
        }
    }
    __syncthreads();
    if (MODE != MODE_TABLE) {
      // row sums: thread t adds 64 columns of row t / 2 in order, then the pair meets
      const int row = tid >> 1, hh = tid & 1;
      const float* g = s_g + row * LG + 64 * hh;
      float v = 0.f;
#pragma unroll 8
      for (int k = 0; k < 64; ++k) v += g[k];
      const float o = __shfl_xor(v, 1, WAVE);
      rsum += hh == 0 ? v + o : o + v;
      // the positive's own term, taken from the tile so that pos / ttl is formed from one arithmetic (exactly 1 for N = 1)
      const int64_t pl = my_pos - y0 - 64 * hh;
      if (pl >= 0 && pl < 64) out_epos[x0 + row] = g[pl];
    }
    if (MODE != MODE_SUMS) {
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
        // idg::mfma_c_row written out: through the helper the compiler forms these 16 NDT store addresses another way and
        // the kernels of d = 64 .. 128 take two more registers
        const int row = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
        out[(int64_t)row * dp + 32 * ct + i] = acc[ct][r];
      }
  }
  if (MODE != MODE_TABLE && (tid & 1) == 0) out_rs[(int64_t)blockIdx.y * out_rows + x0 + (tid >> 1)] = rsum;
}

// One wave per query row (k, b): S_b, r_b, log(r_b + 1e-7), and with gradients a_b, c_b and the row's gradient before the
// scatter (dq: [nq][Bp][dp], the first d columns used).  dQh_b = a_b sum_chunks acc_b - c_b Th_p: the two parts go back
// through the normalisation SEPARATELY, v - x (x . v) / (x . x) with the dot products in double.  Where the positive
// dominates and is nearly parallel to the row (its part is then almost all projected away) the sum of the parts would
// carry the large part's rounding into the small remainder.
__global__ __launch_bounds__(BLOCK) void tnce_rows_kernel(const float* __restrict__ Th, const float* __restrict__ Qh,
                                                          const float* __restrict__ qinv, const int64_t* __restrict__ pos_ids,
                                                          int64_t B, int64_t Bp, int64_t dp, int nq, int chunks,
                                                          const float* __restrict__ rs, const float* __restrict__ epos,
                                                          const float* __restrict__ pacc, QueryArgs q, float inv_tau,
                                                          const float* __restrict__ upstream, int grads,
                                                          float* __restrict__ lrow, float* __restrict__ a,
                                                          float* __restrict__ c, float* __restrict__ dq) {
  const int64_t w = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (w >= (int64_t)nq * B) return;
  const int k = (int)(w / B);
  const int64_t b = w - (int64_t)k * B, e = (int64_t)k * Bp + b, rows = (int64_t)nq * Bp;
  float S = 0.f;
  for (int ch = 0; ch < chunks; ++ch) S += rs[(int64_t)ch * rows + e];
  const float* x = Qh + e * dp;
  const float* t = Th + pos_ids[b] * dp;
  const float r = epos[e] / S;
  // near r = 1 (a table of few rows) r + 1e-7 does not exist in fp32: r - 1 is exact there, and log1p takes the rest
  if (lane == 0) lrow[e] = r > 0.5f ? log1pf((r - 1.f) + GUARD) : logf(r + GUARD);
  if (!grads) return;
  const float cb = (upstream ? upstream[k] : 1.f) * q.weight[k] * (r / (r + GUARD)) * inv_tau;
  const float ab = cb / S;
  // the dense part in chunk order (dp <= 256: at most four features per lane)
  float g[4], tp[4], xv[4];
  double dg = 0., dt = 0., xx = 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    g[u] = tp[u] = xv[u] = 0.f;
    if (f < dp) {
      float s = 0.f;
      for (int ch = 0; ch < chunks; ++ch) s += pacc[((int64_t)ch * rows + e) * dp + f];
      g[u] = ab * s;
      tp[u] = t[f];
      xv[u] = x[f];
      dg += (double)xv[u] * g[u];
      dt += (double)xv[u] * tp[u];
      xx += (double)xv[u] * xv[u];
    }
  }
  dg = wave_sum(dg);
  dt = wave_sum(dt);
  xx = wave_sum(xx);
  const float iv = qinv[e];
  const bool proj = iv < 1.f / NORM_EPS && xx > 0.;  // a row shorter than eps is divided by the constant: no projection
  const double pg = proj ? dg / xx : 0., pt = proj ? dt / xx : 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < dp) dq[e * dp + f] = (float)((((double)g[u] - xv[u] * pg) - (double)cb * ((double)tp[u] - xv[u] * pt)) * (double)iv);
  }
  if (lane == 0) {
    a[e] = ab;
    c[e] = cb;
  }
}

// loss[k] = -w_k sum_b lrow[k][b] by a fixed tree of 1024 leaves; one workgroup per block.
__global__ __launch_bounds__(1024) void tnce_loss_kernel(const float* __restrict__ lrow, int64_t B, int64_t Bp, QueryArgs q,
                                                         float* __restrict__ loss) {
  __shared__ float s[1024];
  const int tid = threadIdx.x, k = blockIdx.x;
  float acc = 0.f;
  for (int64_t b = tid; b < B; b += 1024) acc += lrow[(int64_t)k * Bp + b];
  const float sum = idg::block_tree_sum<1024>(acc, s);
  if (tid == 0) loss[k] = -q.weight[k] * sum;
}

// One wave per table row: the dense part sum_b a_b e_bj Qh_b, its splits added in order, back through the normalisation,
// added to the gradient panel.
__global__ __launch_bounds__(BLOCK) void tnce_table_finish_kernel(const float* __restrict__ Th, const float* __restrict__ tinv,
                                                                  const float* __restrict__ dT, int64_t N, int64_t Np, int64_t d,
                                                                  int64_t dp, int splits, float* __restrict__ g_table) {
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (j >= N) return;
  const float* x = Th + j * dp;
  float g[4], xv[4];
  double dot = 0., xx = 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    g[u] = xv[u] = 0.f;
    if (f < dp) {
      float s = 0.f;
      for (int sp = 0; sp < splits; ++sp) s += dT[((int64_t)sp * Np + j) * dp + f];
      g[u] = s;
      xv[u] = x[f];
      dot += (double)xv[u] * s;
      xx += (double)xv[u] * xv[u];
    }
  }
  dot = wave_sum(dot);
  xx = wave_sum(xx);
  const float iv = tinv[j];
  const bool proj = iv < 1.f / NORM_EPS && xx > 0.;
  const double pg = proj ? dot / xx : 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < d) g_table[j * d + f] += (float)(((double)g[u] - xv[u] * pg) * (double)iv);
  }
}

// The positives' part of the table gradient, -sum over (k, b) with pos_ids[b] = j of c_kb Qh_kb, kept out of the matrix
// pass (one large term inside a long fp32 sum would cost the small ones their last places).  One wave per batch position:
// if no earlier position has the same positive, every occurrence in batch order, the blocks in order inside each, each
// term back through the normalisation on its own, then one addition into the panel row.
__global__ __launch_bounds__(BLOCK) void tnce_table_pos_kernel(const int64_t* __restrict__ pos_ids, const float* __restrict__ Th,
                                                               const float* __restrict__ tinv, const float* __restrict__ Qh,
                                                               const float* __restrict__ c, int64_t B, int64_t Bp, int nq,
                                                               int64_t d, int64_t dp, float* __restrict__ g_table) {
  const int64_t b = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (b >= B) return;
  const int64_t id = pos_ids[b];
  bool earlier, later;
  occurrences(pos_ids, B, b, id, lane, earlier, later);
  if (earlier) return;
  const int64_t end = later ? B : b + 1;
  const float* x = Th + id * dp;
  float xv[4];
  double acc[4];
  double xx = 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    xv[u] = f < dp ? x[f] : 0.f;
    acc[u] = 0.;
    xx += (double)xv[u] * xv[u];
  }
  xx = wave_sum(xx);
  const float iv = tinv[id];
  const bool proj = iv < 1.f / NORM_EPS && xx > 0.;
  for (int64_t o = b - (b % WAVE); o < end; o += WAVE) {
    const bool hit = o + lane >= b && o + lane < end && pos_ids[o + lane] == id;
    unsigned long long m = __ballot(hit);
    while (m) {
      const int64_t bb = o + __builtin_ctzll(m);
      m &= m - 1;
      for (int k = 0; k < nq; ++k) {
        const int64_t e = (int64_t)k * Bp + bb;
        const float* qr = Qh + e * dp;
        float qv[4];
        double dot = 0.;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t f = lane + WAVE * u;
          qv[u] = f < dp ? qr[f] : 0.f;
          dot += (double)xv[u] * qv[u];
        }
        dot = wave_sum(dot);
        const double pq = proj ? dot / xx : 0., ck = (double)c[e];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] -= ck * ((double)qv[u] - xv[u] * pq);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < d) g_table[id * d + f] += (float)(acc[u] * (double)iv);
  }
}

// One wave per batch position b of one query block: if no earlier position holds the same id, every occurrence of the id is
// added in batch order and the sum added to the panel row.
__global__ __launch_bounds__(BLOCK) void tnce_query_scatter_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dq,
                                                                   int64_t B, int64_t d, int64_t dp,
                                                                   float* __restrict__ g_panel) {
  const int64_t b = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (b >= B) return;
  const int64_t id = ids[b];
  bool earlier, later;
  occurrences(ids, B, b, id, lane, earlier, later);
  if (earlier) return;
  const int64_t end = later ? B : 0;
  float g[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) g[u] = lane + WAVE * u < d ? dq[b * dp + lane + WAVE * u] : 0.f;
  for (int64_t o = b + 1 - ((b + 1) % WAVE); o < end; o += WAVE) {
    const bool hit = o + lane > b && o + lane < end && ids[o + lane] == id;
    unsigned long long m = __ballot(hit);
    while (m) {
      const int64_t bb = o + __builtin_ctzll(m);
      m &= m - 1;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (lane + WAVE * u < d) g[u] += dq[bb * dp + lane + WAVE * u];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (lane + WAVE * u < d) g_panel[id * d + lane + WAVE * u] += g[u];
}

template <int MODE>
void launch_tile(int ndt, dim3 grid, hipStream_t st, const float* X, const float* Y, int per, int n_y, int64_t n_valid,
                 float scale2, const float* ca, float* out_acc, float* out_rs,
                 int64_t out_rows, const int64_t* pos_ids, int64_t B, int64_t Bp, float* out_epos) {
  switch (ndt) {
#define IDG_TNCE_CASE(NN)                                                                                                    \
  case NN:                                                                                                                   \
    hipLaunchKernelGGL((tnce_tile_kernel<NN, MODE>), grid, dim3(BLOCK), 0, st, X, Y, per, n_y, n_valid, scale2, ca,           \
                       out_acc, out_rs, out_rows, pos_ids, B, Bp, out_epos);                                                 \
    break;
    IDG_TNCE_CASE(1) IDG_TNCE_CASE(2) IDG_TNCE_CASE(3) IDG_TNCE_CASE(4)
    IDG_TNCE_CASE(5) IDG_TNCE_CASE(6) IDG_TNCE_CASE(7) IDG_TNCE_CASE(8)
#undef IDG_TNCE_CASE
  }
}

}  // namespace

extern "C" {

size_t idg_table_nce_workspace_bytes(int64_t B, int64_t N, int64_t d, int nq) {
  if (B <= 0 || N <= 0 || d <= 0 || d > 32 * MAX_NDT || nq < 1 || nq > MAX_NQ) return 0;
  return layout(B, N, d, nq).total;
}

int idg_table_nce_f32(const float* table_panel, int64_t row0, int64_t N, int64_t d, int nq, const float* const* query_panels,
                      const int64_t* const* query_ids, int64_t B, const int64_t* pos_ids, const float* weights,
                      float temperature, float* loss, const float* upstream, float* g_table_panel,
                      float* const* g_query_panels, void* ws, void* stream) {
  IDG_REQUIRE(table_panel && query_panels && query_ids && pos_ids && weights && ws, "idg_table_nce_f32: NULL argument");
  IDG_REQUIRE(nq >= 1 && nq <= MAX_NQ, "idg_table_nce_f32: nq = %d query blocks (1 .. %d are built)", nq, MAX_NQ);
  IDG_REQUIRE(B >= 1 && N >= 1 && row0 >= 0, "idg_table_nce_f32: bad sizes (B = %lld, N = %lld, row0 = %lld)", (long long)B,
              (long long)N, (long long)row0);
  IDG_REQUIRE(d >= 1 && d <= 32 * MAX_NDT, "idg_table_nce_f32: d = %lld (1 .. %d are built)", (long long)d, 32 * MAX_NDT);
  IDG_REQUIRE(N < ((int64_t)1 << 31) - T && (int64_t)nq * B < ((int64_t)1 << 31) - T,
              "idg_table_nce_f32: sizes exceed int32 positions");
  IDG_REQUIRE(temperature > 0.f && std::isfinite(temperature), "idg_table_nce_f32: temperature must be positive");
  const bool grads = g_table_panel || g_query_panels;
  IDG_REQUIRE(!grads || (g_table_panel && g_query_panels), "idg_table_nce_f32: the gradient panels go together");
  IDG_REQUIRE(grads || loss, "idg_table_nce_f32: nothing to compute");
  IDG_REQUIRE(((uintptr_t)table_panel | (uintptr_t)g_table_panel) % 4 == 0 && (uintptr_t)ws % 256 == 0,
              "idg_table_nce_f32: misaligned panel or workspace (panels 4 bytes, ws 256 bytes)");
  QueryArgs q;
  for (int k = 0; k < MAX_NQ; ++k) {
    q.panel[k] = nullptr;
    q.ids[k] = nullptr;
    q.weight[k] = 0.f;
  }
  for (int k = 0; k < nq; ++k) {
    IDG_REQUIRE(query_panels[k] && query_ids[k] && (!grads || g_query_panels[k]), "idg_table_nce_f32: NULL query block %d", k);
    IDG_REQUIRE(((uintptr_t)query_panels[k] | (uintptr_t)(grads ? g_query_panels[k] : nullptr)) % 4 == 0,
                "idg_table_nce_f32: misaligned query panel %d", k);
    q.panel[k] = query_panels[k];
    q.ids[k] = query_ids[k];
    q.weight[k] = weights[k];
  }
  hipStream_t st = (hipStream_t)stream;
  const Geo g = geo_of(B, N, d, nq);
  const Ws w = layout(B, N, d, nq);
  char* base = reinterpret_cast<char*>(ws);
  float* Th = reinterpret_cast<float*>(base + w.Th);
  float* tinv = reinterpret_cast<float*>(base + w.tinv);
  float* Qh = reinterpret_cast<float*>(base + w.Qh);
  float* qinv = reinterpret_cast<float*>(base + w.qinv);
  float* rs = reinterpret_cast<float*>(base + w.rs);
  float* epos = reinterpret_cast<float*>(base + w.S);
  float* pacc = reinterpret_cast<float*>(base + w.acc);
  float* ca = reinterpret_cast<float*>(base + w.a);
  float* cc = reinterpret_cast<float*>(base + w.c);
  float* lrow = reinterpret_cast<float*>(base + w.lrow);
  float* dq = reinterpret_cast<float*>(base + w.dq);
  float* dT = reinterpret_cast<float*>(base + w.dT);
  const float* table = table_panel + row0 * d;
  const int ndt = (int)(g.dp / 32);
  const int64_t rows = (int64_t)nq * g.Bp;
  const int wpb = BLOCK / WAVE;
  const float inv_tau = 1.f / temperature;
  const float scale2 = inv_tau * 1.4426950408889634f;

  hipLaunchKernelGGL(tnce_prep_kernel, dim3((unsigned)((g.Np + rows + wpb - 1) / wpb)), dim3(BLOCK), 0, st, table, q, N, B, d,
                     g.dp, g.Np, g.Bp, nq, Th, tinv, Qh, qinv, ca, cc);
  const dim3 grid1((unsigned)(g.nbt * nq), (unsigned)g.chunks);
  if (grads)
    launch_tile<MODE_SUMS_ACC>(ndt, grid1, st, Qh, Th, g.per, g.nt, N, scale2, nullptr, pacc, rs, rows, pos_ids,
                               B, g.Bp, epos);
  else
    launch_tile<MODE_SUMS>(ndt, grid1, st, Qh, Th, g.per, g.nt, N, scale2, nullptr, nullptr, rs, rows, pos_ids, B,
                           g.Bp, epos);
  hipLaunchKernelGGL(tnce_rows_kernel, dim3((unsigned)(((int64_t)nq * B + wpb - 1) / wpb)), dim3(BLOCK), 0, st, Th, Qh, qinv,
                     pos_ids, B, g.Bp, g.dp, nq, g.chunks, rs, epos, pacc, q, inv_tau, upstream, grads ? 1 : 0, lrow, ca, cc, dq);
  if (loss) hipLaunchKernelGGL(tnce_loss_kernel, dim3(nq), dim3(1024), 0, st, lrow, B, g.Bp, q, loss);
  if (grads) {
    const dim3 grid2((unsigned)g.nt, (unsigned)g.splits);
    launch_tile<MODE_TABLE>(ndt, grid2, st, Th, Qh, g.sper, g.nbt * nq, 0, scale2, ca, dT, nullptr, g.Np, nullptr, 0, 1,
                            nullptr);
    hipLaunchKernelGGL(tnce_table_finish_kernel, dim3((unsigned)((N + wpb - 1) / wpb)), dim3(BLOCK), 0, st, Th, tinv, dT, N, g.Np,
                       d, g.dp, g.splits, g_table_panel + row0 * d);
    hipLaunchKernelGGL(tnce_table_pos_kernel, dim3((unsigned)((B + wpb - 1) / wpb)), dim3(BLOCK), 0, st, pos_ids, Th, tinv, Qh, cc,
                       B, g.Bp, nq, d, g.dp, g_table_panel + row0 * d);
    for (int k = 0; k < nq; ++k)
      hipLaunchKernelGGL(tnce_query_scatter_kernel, dim3((unsigned)((B + wpb - 1) / wpb)), dim3(BLOCK), 0, st, q.ids[k],
                         dq + (int64_t)k * g.Bp * g.dp, B, d, g.dp, g_query_panels[k]);
  }
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
