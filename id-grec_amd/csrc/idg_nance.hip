// LightCCF (Zhang et al., SIGIR'25; models/LightCCF.py:81-94 of the reference) and LightCSCF (models/LightCSCF.py:93-104):
// the neighbour-aggregation loss over a batch's (user, positive item) rows and its gradient, without an autograd graph or
// a [B, B] matrix.
//
//   a_i = normalize(final[users[i]]),  b_i = normalize(final[num_users + pos[i]]),  p_i = a_i.b_i      (F.normalize, eps 1e-12)
//   total_score[i, j] = a_i.b_j + a_i.a_j = a_i.c_j,  c_j = a_j + b_j        (the SUM of the two matrices is inside exp)
//   T_i = sum_j f(a_i.c_j)   (all j, the diagonal included),   r_i = f(p_i) / T_i
//   loss = grad_scale (1 / B) sum_i -log(r_i + 1e-5)                                          (the reference's `10e-6`)
//   LightCCF:  f(s) = exp(s / T)            LightCSCF:  f(s) = exp(s / T) + exp(relu(s - m) / T)
// so the term is ONE rectangular Gram problem A C^T over the batch rows as they come, scores in [-2, 2].  The diagonal makes
// r_i <= exp(-1 / T), the order of the 1e-5 at small T: row i's gradient carries w_i = r_i / (r_i + 1e-5), which exists only
// once T_i is complete, so the score tiles are formed again after a row-sum pass:
//   d loss = sum_i sum_j P_ij d(a_i.c_j) - sum_i q_i d(a_i.b_i),
//   P_ij = w_i f'(s_ij) / (T_i B),  q_i = (w_i / B) f'(p_i) / f(p_i),  f'(s) = (exp(s / T) + [s > m] exp((s - m) / T)) / T
//   G_a[i] = sum_j P_ij c_j + G_c[i] - q_i b_i,   G_b[i] = G_c[i] - q_i a_i,   G_c[j] = sum_i P_ij a_i     (c_j = a_j + b_j)
// and only then back through normalize().  Every exponential carries the fixed shift -2 / T (scores <= 2, relu(s - m) <= 2
// for m >= 0): f~ = f exp(-2 / T) <= 2.  The shift cancels in r_i, w_i, P_ij and q_i, so nothing goes back into the log here.
//
// WHY DOUBLE.  The diagonal score is 1 + p_i, and so is every column j that repeats row i's user: at a low temperature those
// columns hold nearly all of T_i, sum_j P_ij c_j is then nearly q_i (a_i + b_i), its b-part cancels against -q_i b_i and its
// a-part is removed by normalize()'s projection.  What remains — the gradient — is 1e2 (T = 0.1, one user repeated) to 1e5
// (LightCCF at T = 0.05) times smaller than the parts it is the difference of, so operands, scores or products rounded to
// float32 (6e-8 of the PARTS) leave it wrong by up to percents: the reference's own expressions in float32 sit 3e-2 of the
// largest entry from their float64 value there (tests/test_na_host.py).  The whole term therefore runs in double: the
// normalised rows, the 64 x 64 score tiles and both products on the matrix cores' fp64 form (v_mfma_f64_16x16x4_f64), the
// exponentials and every sum.  idg_tile128.h's fp32 tile is not used here (DESIGN.md section 4 has the figures).
//
//   prep     one wave per (padded) batch position: a, c and b into zero-padded double [Bp, 32 NDT] operand copies, the raw
//            norms, f~(p_i) and (T f' / f)(p_i).
//   rowsum   grid (row tile, split): the workgroup walks its split's column tiles in ascending order; per tile the 64 x 64
//            scores, f~ into the LDS tile (columns >= B as zeros), every row summed over the tile's columns in a fixed order and
//            added to the row's running sum: rowpart[split][Bp], each element written by exactly one workgroup.
//   rows     one workgroup: T~_i (splits in order), r_i, w_i, the loss (a fixed tree), the row coefficient w_i / (T~_i B T), q_i.
//   grad     twice, with the same kernel: (row tile, split) walking column tiles — the tile again, P_ij = coefficient_i T f~'(s_ij)
//            into the LDS tile, then tile . C-rows accumulated in registers across the walk — and (column tile, split) walking
//            row tiles, the transposed tile . A-rows (G_c).  part[side][split][Bp][dp].
//   slot     one wave per (side, i): the splits added in order, G_a / G_b, back through normalize().
//   scatter  one wave per distinct row of the plan: occurrences added in batch order and rounded once to float, then ADDED
//            into or STORED to g_final.
// The split count is a function of B alone.  idg_reg_rows_f32 (below) is the regulariser of LightCSCF's LightGCN form, which
// has no BPR call to carry it.  No atomics, every sum in a fixed order: the same bits every run, and the same loss bits with or
// without gradients.
#include <hip/hip_runtime.h>

#include <cmath>

#include "idg_common.h"
#include "idg_device.h"

namespace {

using idg::align256;
using idg::round_up;
using idg::WAVE;
using idg::wave_sum;
using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int BLOCK = 256;
constexpr int TD = 64;        // rows / columns of a score tile
constexpr int KC = 32;        // feature chunk staged through LDS
constexpr int LKD = KC + 1;   // its row stride (doubles)
constexpr int LGD = TD + 1;   // row stride of the 64 x 64 tile written from the scores
constexpr int MAX_NDT = 8;    // d <= 256
constexpr int MAX_SPLITS = 8;
constexpr int WPB = BLOCK / WAVE;
constexpr double NORM_EPS = 1e-12;
constexpr double LOG_EPS = 1e-5;    // the reference's 10e-6
constexpr float MIN_TAU = 0.01f;    // exp(-4 / T), the smallest shifted term, is a normal double far below this

struct Geo {
  int64_t dp, Bp;
  int nbt, tps, splits;  // tiles per edge, tiles per split, splits
};

Geo geo_of(int64_t B, int64_t d) {
  Geo g;
  g.dp = round_up(d, 32);
  g.Bp = round_up(B, TD);
  g.nbt = (int)(g.Bp / TD);
  // enough workgroups for the chip at the models' batch sizes (B = 4096: 64 tiles x 8 splits), one split below 64 tiles' work
  int want = (512 + g.nbt - 1) / g.nbt;
  want = want < 1 ? 1 : (want > MAX_SPLITS ? MAX_SPLITS : want);
  if (want > g.nbt) want = g.nbt;
  g.tps = (g.nbt + want - 1) / want;
  g.splits = (g.nbt + g.tps - 1) / g.tps;
  return g;
}

// Offsets (bytes) into the workspace.  H: [3][Bp][dp] doubles (a, c, b); rowpart: [splits][Bp]; part: [2][splits][Bp][dp].
struct Ws {
  size_t plan, H, nrm, fp, dpos, rowpart, coef, q, part, gx, regp, scal, total;
};

Ws layout(int64_t B, int64_t d) {
  const Geo g = geo_of(B, d);
  Ws w;
  size_t o = 0;
  const size_t P = (size_t)g.Bp * (size_t)g.dp * 8;
  w.plan = o, o += align256(idg_bpr_workspace_bytes(B, d));
  w.H = o, o += align256(3 * P);
  w.nrm = o, o += align256((size_t)2 * g.Bp * 8);
  w.fp = o, o += align256((size_t)g.Bp * 8);
  w.dpos = o, o += align256((size_t)g.Bp * 8);
  w.rowpart = o, o += align256((size_t)g.splits * g.Bp * 8);
  w.coef = o, o += align256((size_t)g.Bp * 8);
  w.q = o, o += align256((size_t)g.Bp * 8);
  w.part = o, o += align256((size_t)2 * g.splits * P);
  w.gx = o, o += align256((size_t)2 * B * d * 8);
  w.regp = o, o += align256((size_t)3 * B * 8);
  w.scal = o, o += 256;
  w.total = o;
  return w;
}

// The four features a lane holds of a row of at most 256 values (0 past `lim`).
template <typename V>
__device__ __forceinline__ void load4(const V* __restrict__ row, int64_t lim, int lane, double (&v)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    v[u] = f < lim ? (double)row[f] : 0.;
  }
}

__device__ __forceinline__ double dot4(const double (&x)[4], const double (&y)[4]) {
  double s = 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) s = fma(x[u], y[u], s);
  return wave_sum(s);
}

// ---- prep.  One wave per padded batch position.  margin < 0: LightCCF's f.
__global__ __launch_bounds__(BLOCK) void na_prep_kernel(const float* __restrict__ fin, const int64_t* __restrict__ users,
                                                        const int64_t* __restrict__ pos, int64_t B, int64_t Bp, int64_t d,
                                                        int64_t dp, int64_t num_users, double inv_tau, double margin,
                                                        double* __restrict__ H, double* __restrict__ nrm,
                                                        double* __restrict__ fp, double* __restrict__ dpos) {
  const int64_t i = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (i >= Bp) return;
  double* ha = H + i * dp;
  double* hc = H + (Bp + i) * dp;
  double* hb = H + (2 * Bp + i) * dp;
  if (i >= B) {
    for (int64_t f = lane; f < dp; f += WAVE) ha[f] = 0., hc[f] = 0., hb[f] = 0.;
    if (lane == 0) nrm[i] = 0., nrm[Bp + i] = 0., fp[i] = 0., dpos[i] = 0.;
    return;
  }
  double x[4], y[4];
  load4(fin + users[i] * d, d, lane, x);
  load4(fin + (num_users + pos[i]) * d, d, lane, y);
  const double n0 = sqrt(dot4(x, x)), n1 = sqrt(dot4(y, y));
  const double den0 = fmax(n0, NORM_EPS), den1 = fmax(n1, NORM_EPS);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    x[u] = f < d ? x[u] / den0 : 0.;
    y[u] = f < d ? y[u] / den1 : 0.;
    if (f < dp) ha[f] = x[u], hc[f] = x[u] + y[u], hb[f] = y[u];
  }
  const double p = dot4(x, y);
  if (lane == 0) {
    const bool has_margin = margin >= 0.;
    const double e1 = exp((p - 2.) * inv_tau);
    const double e2 = has_margin ? exp((fmax(p - margin, 0.) - 2.) * inv_tau) : 0.;
    nrm[i] = n0;
    nrm[Bp + i] = n1;
    fp[i] = e1 + e2;                                              // f~(p_i)
    dpos[i] = (e1 + (has_margin && p > margin ? e2 : 0.)) / (e1 + e2);  // (T f' / f)(p_i)
  }
}

// ---- the tile walk.  Workgroup (t, s): the FIXED tile t — 64 rows of X — against the tiles [s tps, s tps + tps) of Y, in
// ascending order.  Wave w computes the 32 x 32 quarter (w >> 1, w & 1) of a score tile as 2 x 2 blocks of
// v_mfma_f64_16x16x4_f64 (A: lane l holds X[l & 15][k = l >> 4], B: Y[l & 15][k = l >> 4]; D: column l & 15, rows
// (l >> 4) + 4 r), the features staged through LDS 32 at a time.
//   MODE 0 (X = a rows, Y = c rows): f~(s) into the LDS tile, columns >= B as zeros; thread t sums columns [16 (t >> 6), + 16)
//           of row t & 63 in ascending order, the four quarters are added pairwise and join the row's running sum.
//   MODE 1 (X = a rows, Y = c rows): coefficient[fixed row] T f~'(s) into the LDS tile, then wave w's 16 rows x all features
//           of tile . Y-rows join its accumulators: sum_j P_ij c_j.
//   MODE 2 (X = c rows, Y = a rows): the transposed tile, coefficient[walking index] T f~'(s); tile . Y-rows is G_c[j].
template <int NDT, int MODE>
__global__ __launch_bounds__(BLOCK) void na_tile_kernel(const double* __restrict__ Xall, const double* __restrict__ Yall,
                                                        int64_t Bp, int64_t B, int nbt, int tps, double inv_tau, double margin,
                                                        int has_margin, const double* __restrict__ coef,
                                                        double* __restrict__ out) {
  constexpr int64_t dp = 32 * NDT;
  constexpr int NF = MODE == 0 ? 1 : 2 * NDT;  // 16-feature blocks of a product row
  __shared__ double s_x[TD * LKD];
  __shared__ double s_y[TD * LKD];
  __shared__ double s_g[TD * LGD];
  __shared__ double s_r[BLOCK];
  const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, li = lane & 15, lk = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t x0 = (int64_t)blockIdx.x * TD;
  const double* X = Xall + x0 * dp;
  const int t_begin = (int)blockIdx.y * tps, t_end = t_begin + tps < nbt ? t_begin + tps : nbt;

  f64x4 acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = f64x4{0., 0., 0., 0.};
  double rowacc = 0.;

#pragma unroll 1
  for (int yt = t_begin; yt < t_end; ++yt) {
    const int64_t y0 = (int64_t)yt * TD;
    const double* Y = Yall + y0 * dp;
    f64x4 s[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) s[m][n] = f64x4{0., 0., 0., 0.};
#pragma unroll 1
    for (int kc = 0; kc < NDT; ++kc) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = tid + BLOCK * j, rr = e >> 5, cc = e & 31;
        s_x[rr * LKD + cc] = X[rr * dp + kc * KC + cc];
        s_y[rr * LKD + cc] = Y[rr * dp + kc * KC + cc];
      }
      __syncthreads();
      const double* pa = s_x + (32 * wr + li) * LKD + lk;
      const double* pb = s_y + (32 * wc + li) * LKD + lk;
#pragma unroll
      for (int ks = 0; ks < KC / 4; ++ks) {
        const double a0 = pa[4 * ks], a1 = pa[16 * LKD + 4 * ks];
        const double b0 = pb[4 * ks], b1 = pb[16 * LKD + 4 * ks];
        s[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, s[0][0], 0, 0, 0);
        s[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, s[0][1], 0, 0, 0);
        s[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, s[1][0], 0, 0, 0);
        s[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, s[1][1], 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = 32 * wc + 16 * n + li;
      const bool col_ok = y0 + col < B;  // the walking index past the batch: no term
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 32 * wr + 16 * m + lk + 4 * r;
          const double sc = s[m][n][r];
          const double e1 = exp((sc - 2.) * inv_tau);
          const double e2 = has_margin ? exp((fmax(sc - margin, 0.) - 2.) * inv_tau) : 0.;
          double v;
          if (MODE == 0) v = e1 + e2;
          else v = (MODE == 1 ? coef[x0 + row] : coef[y0 + col]) * (e1 + (has_margin && sc > margin ? e2 : 0.));
          s_g[row * LGD + col] = col_ok ? v : 0.;
        }
    }
    __syncthreads();
    if (MODE == 0) {
      const double* g = s_g + (tid & (TD - 1)) * LGD + 16 * (tid >> 6);
      double part = 0.;
#pragma unroll
      for (int k = 0; k < 16; ++k) part += g[k];
      s_r[tid] = part;
      __syncthreads();
      if (tid < TD) rowacc += (s_r[tid] + s_r[tid + TD]) + (s_r[tid + 2 * TD] + s_r[tid + 3 * TD]);
    } else {
      const double* ga = s_g + (16 * wave + li) * LGD + lk;
      const double* yb = Y + (int64_t)lk * dp + li;
#pragma unroll 2
      for (int ks = 0; ks < TD / 4; ++ks) {
        const double a = ga[4 * ks];
#pragma unroll
        for (int f = 0; f < NF; ++f)
          acc[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[(int64_t)(4 * ks) * dp + 16 * f], acc[f], 0, 0, 0);
      }
    }
    // (the next tile's staging barriers come before its writes to s_g and s_r: no wave is still reading them then)
  }
  if (MODE == 0) {
    if (tid < TD) out[(int64_t)blockIdx.y * Bp + x0 + tid] = rowacc;
  } else {
    double* o = out + ((int64_t)blockIdx.y * Bp + x0 + 16 * wave + lk) * dp + li;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(int64_t)(4 * r) * dp + 16 * f] = acc[f][r];
  }
}

// ---- rows.  One workgroup.  Per row: T~_i, r_i, w_i, its loss term, the coefficient of its tile entries and q_i; then the loss
// by a fixed tree of 1024 leaves.  scal[0] = grad_scale * upstream.
__global__ __launch_bounds__(1024) void na_rows_kernel(const double* __restrict__ rowpart, int splits, int64_t B, int64_t Bp,
                                                       const double* __restrict__ fp, const double* __restrict__ dpos,
                                                       double inv_tau, float grad_scale, const float* __restrict__ upstream,
                                                       double* __restrict__ coef, double* __restrict__ q,
                                                       float* __restrict__ loss, double* __restrict__ scal) {
  __shared__ double s[1024];
  const int tid = threadIdx.x;
  double acc = 0.;
  for (int64_t b = tid; b < Bp; b += 1024) {
    if (b >= B) {
      coef[b] = 0., q[b] = 0.;
      continue;
    }
    double t = 0.;
    for (int j = 0; j < splits; ++j) t += rowpart[(int64_t)j * Bp + b];
    const double r = fp[b] / t, w = r / (r + LOG_EPS);
    acc += -log(r + LOG_EPS);
    coef[b] = w * inv_tau / (t * (double)B);
    q[b] = w * dpos[b] * inv_tau / (double)B;
  }
  const double total = idg::block_tree_sum<1024>(acc, s);
  if (tid == 0) {
    loss[0] = (float)((double)grad_scale * total / (double)B);
    scal[0] = (double)grad_scale * (double)(upstream ? upstream[0] : 1.f);
  }
}

// ---- slot.  One wave per (side, i), side 0 = a_i, side 1 = b_i: G_a = rowside_i + G_c[i] - q_i b_i, G_b = G_c[i] - q_i a_i
// (the splits added in order), times grad_scale * upstream, back through normalize(): (g - <g, h> h) / ||x|| for
// ||x|| >= eps, g / eps below.  Into gx[side][i] (row stride d).
__global__ __launch_bounds__(BLOCK) void na_slot_kernel(const double* __restrict__ H, const double* __restrict__ nrm,
                                                        const double* __restrict__ q, const double* __restrict__ part,
                                                        int splits, const double* __restrict__ scal, int64_t B, int64_t Bp,
                                                        int64_t d, int64_t dp, double* __restrict__ gx) {
  const int64_t idx = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (idx >= 2 * B) return;
  const int side = idx >= B ? 1 : 0;
  const int64_t i = idx - side * B;
  double hx[4], ho[4], gr[4] = {0., 0., 0., 0.}, gc[4] = {0., 0., 0., 0.}, t[4];
  load4(H + ((side ? 2 : 0) * Bp + i) * dp, dp, lane, hx);
  load4(H + ((side ? 0 : 2) * Bp + i) * dp, dp, lane, ho);
  for (int s = 0; s < splits; ++s) {
    if (!side) {
      load4(part + ((int64_t)s * Bp + i) * dp, dp, lane, t);
#pragma unroll
      for (int u = 0; u < 4; ++u) gr[u] += t[u];
    }
    load4(part + ((int64_t)(splits + s) * Bp + i) * dp, dp, lane, t);
#pragma unroll
    for (int u = 0; u < 4; ++u) gc[u] += t[u];
  }
  const double up = scal[0], qi = q[i];
  double g[4];
  double dot = 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    g[u] = up * (gr[u] + gc[u] - qi * ho[u]);
    dot += g[u] * hx[u];
  }
  dot = wave_sum(dot);
  const double n = nrm[side * Bp + i];
  const bool proj = n >= NORM_EPS;
  const double den = proj ? n : NORM_EPS;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < d) gx[idx * d + f] = (g[u] - (proj ? dot * hx[u] : 0.)) / den;
  }
}

// ---- scatter.  One wave per distinct row of the sorted plan (slot 3i: users[i] <- gx[0][i]; 3i + 1: num_users + pos[i] <-
// gx[1][i]; 3i + 2: the plan's third id, a negative or a copy of the positive, which has no term here), occurrences added in
// batch order in double, rounded once.  Store mode writes every row of the plan (zeros where only third slots name it).
__global__ __launch_bounds__(BLOCK) void na_scatter_kernel(const int32_t* __restrict__ skeys, const int32_t* __restrict__ sslots,
                                                           const double* __restrict__ gx, int64_t B, int64_t d,
                                                           float* __restrict__ g_final, int accumulate) {
  const int64_t j = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int64_t n3 = 3 * B;
  if (j >= n3) return;
  const int32_t row = skeys[j];
  if (j > 0 && skeys[j - 1] == row) return;
  int64_t e = j + 1;
  while (e < n3 && skeys[e] == row) ++e;
  for (int64_t f = lane; f < d; f += WAVE) {
    double sum = 0.;
    for (int64_t t = j; t < e; ++t) {
      const int32_t s = sslots[t];
      const int64_t i = s / 3;
      const int kind = s - 3 * (int32_t)i;
      if (kind == 2) continue;
      sum += gx[((int64_t)kind * B + i) * d + f];
    }
    const float acc = (float)sum;
    const int64_t o = (int64_t)row * d + f;
    g_final[o] = accumulate ? g_final[o] + acc : acc;
  }
}

// ---- the regulariser alone.  One wave per distinct row of the sorted three-slot plan: the row's occurrences added in batch
// order in double and rounded once into g_ego (STORED), zeros STORED to the row of g_final, and the row's share of
// sum ||e||^2 (occurrences times its squared norm, double) into sq[head position]; positions that head no run hold 0.
__global__ __launch_bounds__(BLOCK) void reg_rows_kernel(const float* __restrict__ ego, const int32_t* __restrict__ skeys,
                                                         int64_t B, int64_t d, double reg_scale, float* __restrict__ g_ego,
                                                         float* __restrict__ g_final, double* __restrict__ sq) {
  const int64_t j = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int64_t n3 = 3 * B;
  if (j >= n3) return;
  const int32_t row = skeys[j];
  if (j > 0 && skeys[j - 1] == row) {
    if (lane == 0) sq[j] = 0.;
    return;
  }
  int64_t e = j + 1;
  while (e < n3 && skeys[e] == row) ++e;
  double nn = 0.;
  for (int64_t f = lane; f < d; f += WAVE) {
    const int64_t o = (int64_t)row * d + f;
    const double v = (double)ego[o];
    double sum = 0.;
    for (int64_t t = j; t < e; ++t) sum += v;
    nn += v * v;
    if (g_ego) g_ego[o] = (float)(reg_scale * sum);
    if (g_final) g_final[o] = 0.f;
  }
  nn = wave_sum(nn);
  if (lane == 0) sq[j] = nn * (double)(e - j);
}

__global__ __launch_bounds__(1024) void reg_reduce_kernel(const double* __restrict__ sq, int64_t n3, float reg_lambda, int64_t B,
                                                          float* __restrict__ loss) {
  __shared__ double s[1024];
  double acc = 0.;
  for (int64_t t = threadIdx.x; t < n3; t += 1024) acc += sq[t];
  const double total = idg::block_tree_sum<1024>(acc, s);
  if (threadIdx.x == 0) loss[0] = (float)((double)reg_lambda * 0.5 * total / (double)B);
}

template <int MODE>
void launch_tile(int ndt, dim3 grid, hipStream_t st, const double* X, const double* Y, int64_t Bp, int64_t B, const Geo& g,
                 double inv_tau, double margin, int has_margin, const double* coef, double* out) {
  switch (ndt) {
#define IDG_NA_CASE(NN)                                                                                                       \
  case NN:                                                                                                                    \
    hipLaunchKernelGGL((na_tile_kernel<NN, MODE>), grid, dim3(BLOCK), 0, st, X, Y, Bp, B, g.nbt, g.tps, inv_tau, margin,      \
                       has_margin, coef, out);                                                                                \
    break;
    IDG_NA_CASE(1) IDG_NA_CASE(2) IDG_NA_CASE(3) IDG_NA_CASE(4)
    IDG_NA_CASE(5) IDG_NA_CASE(6) IDG_NA_CASE(7) IDG_NA_CASE(8)
#undef IDG_NA_CASE
  }
}

}  // namespace

extern "C" {

size_t idg_na_nce_workspace_bytes(int64_t B, int64_t d) {
  if (B <= 0 || B >= ((int64_t)1 << 22) || d <= 0 || d > 32 * MAX_NDT) return 0;
  return layout(B, d).total;
}

int idg_na_nce_f32(const float* final_panel, int64_t n, int64_t d, const int64_t* users, const int64_t* pos, int64_t B,
                   int64_t num_users, float temperature, float margin, float grad_scale, float* loss, const float* upstream,
                   float* g_final, int accumulate, const void* plan_ws, void* ws, void* stream) {
  IDG_REQUIRE(final_panel && users && pos && loss && ws, "idg_na_nce_f32: NULL argument");
  IDG_REQUIRE(B >= 1 && B < ((int64_t)1 << 22), "idg_na_nce_f32: B = %lld (1 .. 2^22 - 1)", (long long)B);
  IDG_REQUIRE(d >= 1 && d <= 32 * MAX_NDT, "idg_na_nce_f32: d = %lld (1 .. %d are built)", (long long)d, 32 * MAX_NDT);
  IDG_REQUIRE(num_users >= 1 && n > num_users && n < ((int64_t)1 << 31),
              "idg_na_nce_f32: bad panel (n = %lld rows, %lld of them users)", (long long)n, (long long)num_users);
  IDG_REQUIRE(std::isfinite(temperature) && temperature >= MIN_TAU, "idg_na_nce_f32: temperature must be at least %g",
              (double)MIN_TAU);
  IDG_REQUIRE(std::isfinite(margin) && margin <= 2.f, "idg_na_nce_f32: margin must be in [0, 2], or negative for none");
  IDG_REQUIRE(std::isfinite(grad_scale), "idg_na_nce_f32: grad_scale must be finite");
  IDG_REQUIRE(!idg::overlap(g_final, idg::extent(n, d, d), final_panel, idg::extent(n, d, d)),
              "idg_na_nce_f32: the gradient panel overlaps the input");
  IDG_REQUIRE((uintptr_t)ws % 256 == 0, "idg_na_nce_f32: ws must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Geo g = geo_of(B, d);
  const Ws w = layout(B, d);
  char* base = reinterpret_cast<char*>(ws);
  auto atd = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  double *H = atd(w.H), *nrm = atd(w.nrm), *fp = atd(w.fp), *dpos = atd(w.dpos), *rowpart = atd(w.rowpart);
  double *coef = atd(w.coef), *q = atd(w.q), *part = atd(w.part), *scal = atd(w.scal), *gx = atd(w.gx);
  const double *Ha = H, *Hc = H + g.Bp * g.dp;
  const bool grads = g_final != nullptr;
  if (grads && !plan_ws) {  // the plan of (users, pos, pos) in-call: only the scatter reads it
    const int rc = idg_bpr_plan_f32(users, pos, pos, B, num_users, n, base + w.plan, stream);
    if (rc != IDG_OK) return rc;
  }
  const double inv_tau = 1. / (double)temperature;
  const int has_margin = margin >= 0.f ? 1 : 0;
  const double mg = has_margin ? (double)margin : -1.;
  auto blocks = [](int64_t waves) { return dim3((unsigned)((waves + WPB - 1) / WPB)); };
  hipLaunchKernelGGL(na_prep_kernel, blocks(g.Bp), dim3(BLOCK), 0, st, final_panel, users, pos, B, g.Bp, d, g.dp, num_users,
                     inv_tau, mg, H, nrm, fp, dpos);
  const dim3 grid((unsigned)g.nbt, (unsigned)g.splits);
  const int ndt = (int)(g.dp / 32);
  launch_tile<0>(ndt, grid, st, Ha, Hc, g.Bp, B, g, inv_tau, mg, has_margin, nullptr, rowpart);
  hipLaunchKernelGGL(na_rows_kernel, dim3(1), dim3(1024), 0, st, rowpart, g.splits, B, g.Bp, fp, dpos, inv_tau, grad_scale,
                     upstream, coef, q, loss, scal);
  if (grads) {
    const int32_t *skeys = nullptr, *sslots = nullptr;
    idg::bpr_plan_lists(plan_ws ? plan_ws : base + w.plan, B, &skeys, &sslots);
    launch_tile<1>(ndt, grid, st, Ha, Hc, g.Bp, B, g, inv_tau, mg, has_margin, coef, part);
    launch_tile<2>(ndt, grid, st, Hc, Ha, g.Bp, B, g, inv_tau, mg, has_margin, coef, part + (int64_t)g.splits * g.Bp * g.dp);
    hipLaunchKernelGGL(na_slot_kernel, blocks(2 * B), dim3(BLOCK), 0, st, H, nrm, q, part, g.splits, scal, B, g.Bp, d, g.dp, gx);
    hipLaunchKernelGGL(na_scatter_kernel, blocks(3 * B), dim3(BLOCK), 0, st, skeys, sslots, gx, B, d, g_final,
                       accumulate ? 1 : 0);
  }
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int idg_reg_rows_f32(const float* ego_panel, int64_t n, int64_t d, const int64_t* users, const int64_t* pos,
                     const int64_t* neg, int64_t B, int64_t num_users, float reg_lambda, float* loss, float* g_ego,
                     float* g_final, const void* plan_ws, void* ws, void* stream) {
  IDG_REQUIRE(ego_panel && loss && ws, "idg_reg_rows_f32: NULL argument");
  IDG_REQUIRE(plan_ws || (users && pos && neg), "idg_reg_rows_f32: the id lists or a plan built from them");
  IDG_REQUIRE(B >= 1 && B < ((int64_t)1 << 22), "idg_reg_rows_f32: B = %lld (1 .. 2^22 - 1)", (long long)B);
  IDG_REQUIRE(d >= 1 && d <= 32 * MAX_NDT, "idg_reg_rows_f32: d = %lld (1 .. %d are built)", (long long)d, 32 * MAX_NDT);
  IDG_REQUIRE(num_users >= 1 && n > num_users && n < ((int64_t)1 << 31),
              "idg_reg_rows_f32: bad panel (n = %lld rows, %lld of them users)", (long long)n, (long long)num_users);
  IDG_REQUIRE(std::isfinite(reg_lambda), "idg_reg_rows_f32: reg_lambda must be finite");
  IDG_REQUIRE(!g_final || g_final != g_ego, "idg_reg_rows_f32: g_final must be distinct from g_ego");
  IDG_REQUIRE(!idg::overlap(g_final, idg::extent(n, d, d), ego_panel, idg::extent(n, d, d)) &&
                  !idg::overlap(g_ego, idg::extent(n, d, d), ego_panel, idg::extent(n, d, d)) &&
                  !idg::overlap(g_ego, idg::extent(n, d, d), g_final, idg::extent(n, d, d)),
              "idg_reg_rows_f32: gradient panels overlap the input or each other");
  IDG_REQUIRE((uintptr_t)ws % 256 == 0, "idg_reg_rows_f32: ws must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Ws w = layout(B, d);
  char* base = reinterpret_cast<char*>(ws);
  if (!plan_ws) {
    const int rc = idg_bpr_plan_f32(users, pos, neg, B, num_users, n, base + w.plan, stream);
    if (rc != IDG_OK) return rc;
  }
  const int32_t *skeys = nullptr, *sslots = nullptr;
  idg::bpr_plan_lists(plan_ws ? plan_ws : base + w.plan, B, &skeys, &sslots);
  double* sq = reinterpret_cast<double*>(base + w.regp);
  hipLaunchKernelGGL(reg_rows_kernel, dim3((unsigned)((3 * B + WPB - 1) / WPB)), dim3(BLOCK), 0, st, ego_panel, skeys, B, d,
                     (double)reg_lambda / (double)B, g_ego, g_final, sq);
  hipLaunchKernelGGL(reg_reduce_kernel, dim3(1), dim3(1024), 0, st, sq, 3 * B, reg_lambda, B, loss);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
