// MixRec's in-batch mixing contrastive terms (Zhang et al., WWW'25: models/MixRec.py:94-154 of the reference, every term a
// losses.get_InfoNCE_loss_all whose positive is NOT a row of its negative set), forward and backward in one call, without
// a [B, B] matrix.  The math is stated at idg_mix_nce_f32 in include/idgrec.h; in short, with x the gathered batch rows
// of one side (users, or positives), pi its permutation, beta its mixing weight, h = normalize(x),
//   c_i = beta x_i + (1 - beta) x_pi(i),  ch = normalize(c),   m = sum_j nu_j x_j,  mh = normalize(m)
//   D_i = sum_j exp(h_i.h_j / T) + exp(h_i.mh / T)                      (ONE symmetric Gram matrix serves both halves)
//   side = (1/B) sum_i [-beta log(exp(ch_i.h_i / T) / D_i + 1e-7) - (1 - beta) log(exp(ch_i.h_pi(i) / T) / D_pi(i) + 1e-7)]
// and the rectangular term -(1/B) sum_i log(exp(a_i.ph_i) / sum_j exp(a_i.s_j) + 1e-7), a = normalize(users' rows),
// ph = normalize(positives' rows), s = normalize(Mn), Mn_j = beta_I n_j + (1 - beta_I) n_piI(j).
// Scores are cosines: e = exp((s - 1) / T) <= 1 needs no running maximum, the common factor cancels in every ratio.
//
// Three "problems" share every launch: 0 the user Gram (X = Y = H0), 1 the item Gram (X = Y = H1), 2 users x Mn
// (X = H0, Y = H2).  Operands are normalised copies in the workspace, zero-padded to 128 rows x 32 columns
// (idg_tile128.h); every product is v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 sums).
//   prep     one wave per row and problem: gathers, mixes and normalises h / ch / Mn-hat, finds the inverse permutation by a
//            scan (no scatter: a list that is no permutation stays memory-safe, rows nobody points at get no second half),
//            clears the per-row coefficients; 2 x 16 more waves add the rows of m in 16 ordered slices.
//   tile 1   grid (row tile, column chunk, problem): E = exp((X Y^T - 1) / T) tile by tile in LDS, its row sums and
//            acc += E Y with the [128, d] accumulator in registers.  E carries no coefficient, so the pass is both the
//            statistics pass and the first gradient pass (kappa_k sum_j e_kj h_j).
//   rows     one wave per row and problem: D (chunk order + the mix row's own dot product), both ratios, the loss terms,
//            kappa_k = d side / d D_k, the positives' coefficients q1, q2, and the transposed pass's column coefficient.
//   tile 2   the same tile with a per-COLUMN coefficient: sum_j e_kj kappa_j h_j for the two Gram problems (E is
//            symmetric: no transposed pass), and for problem 2 the transposed product sum_i (q_i / S_i) e_ij a_i.
//   mixcol   2 x 16 waves: sum_k kappa_k e_km h_k (the mix row's gradient) in 16 ordered slices.
//   finish   one wave per row and problem: everything that reaches h_i, back through its normalisation; the parts through
//            c_i and c_pi^-1(i), through m, through Mn_j and Mn_piI^-1(j), each back through its own normalisation
//            (projections with double dot products); one row of d loss / d x per gathered row.
//   scatter  users, positives, negatives, one launch each in that order: the first occurrence of an id adds every
//            occurrence in batch order and ADDS the sum to the panel row.
// No float atomics, every sum in a fixed order: the same bits every run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "idg_common.h"
#include "idg_tile128.h"

namespace {

using namespace idg::tile128;  // BLOCK, T = 128, LK, LG, LDS_FLOATS
using idg::align256;
using idg::f32x16;
using idg::mfma_c_row;
using idg::round_up;
using idg::WAVE;
using idg::wave_sum;

constexpr int MAX_NDT = 8;  // d <= 256
constexpr int MAX_CHUNKS = 64;
constexpr int TARGET_WGS = 512;  // two 66 KB workgroups per CU
constexpr int NPROB = 3;
constexpr int SLICES = 16;  // ordered slices of the two column sums (m, and its gradient)
constexpr int WPB = BLOCK / WAVE;
constexpr float NORM_EPS = 1e-12f;
constexpr float GUARD = 1e-7f;  // the reference's 10e-8
constexpr float LOG2E = 1.4426950408889634f;

enum { MODE_SUMS = 0, MODE_SUMS_ACC = 1, MODE_COEF = 2 };

struct Geo {
  int64_t dp, Bp;
  int nbt, chunks, per;
};

Geo geo_of(int64_t B, int64_t d) {
  Geo g;
  g.dp = round_up(d, 32);
  g.Bp = round_up(B, T);
  g.nbt = (int)(g.Bp / T);
  const int owners = g.nbt * NPROB;
  int want = (TARGET_WGS + owners - 1) / owners;
  want = want < 1 ? 1 : want > MAX_CHUNKS ? MAX_CHUNKS : want;
  want = want > g.nbt ? g.nbt : want;
  g.per = (g.nbt + want - 1) / want;
  g.chunks = (g.nbt + g.per - 1) / g.per;
  return g;
}

// Offsets (bytes) into the workspace.  Per-row arrays are [problem][Bp]; panels [problem][Bp][dp].
struct Ws {
  size_t H, hinv, CH, cinv, pinv, mpart, rs, acc1, kap, q1, q2, kem, qr, lrow, acc2, dmpart, dX, total;
};

Ws layout(int64_t B, int64_t d) {
  const Geo g = geo_of(B, d);
  Ws w;
  size_t o = 0;
  const size_t R = (size_t)g.Bp, P = R * (size_t)g.dp * 4;
  w.H = o, o += align256(NPROB * P);
  w.hinv = o, o += align256(NPROB * R * 4);
  w.CH = o, o += align256(2 * P);
  w.cinv = o, o += align256(2 * R * 4);
  w.pinv = o, o += align256(2 * R * 4);
  w.mpart = o, o += align256((size_t)2 * SLICES * g.dp * 4);
  w.rs = o, o += align256((size_t)NPROB * g.chunks * R * 4);
  w.acc1 = o, o += align256((size_t)NPROB * g.chunks * P);
  w.kap = o, o += align256(NPROB * R * 4);  // [0], [1]: kappa; [2]: q_i / S_i of the rectangular term
  w.q1 = o, o += align256(2 * R * 4);
  w.q2 = o, o += align256(2 * R * 4);
  w.kem = o, o += align256(2 * R * 4);
  w.qr = o, o += align256(R * 4);
  w.lrow = o, o += align256(NPROB * R * 4);
  w.acc2 = o, o += align256((size_t)NPROB * g.chunks * P);
  w.dmpart = o, o += align256((size_t)2 * SLICES * g.dp * 4);
  w.dX = o, o += align256(NPROB * P);
  w.total = o;
  return w;
}

struct Args {
  const float* panel;
  int64_t d, dp, U, B, Bp;
  const int64_t* ids[NPROB];   // users, pos, neg
  const int64_t* perm[2];      // user_perm, item_perm
  const float* nu;
  float beta[2];               // user_beta, item_beta
  float inv_tau, scale2;       // 1 / T and log2(e) / T of the Gram problems (problem 2: T = 1)
  float ssl_weight;
  const float* upstream;
  int chunks;
  float *H, *hinv, *CH, *cinv;
  int32_t* pinv;
  float *mpart, *rs, *acc1, *kap, *q1, *q2, *kem, *qr, *lrow, *acc2, *dmpart, *dX;
};

// pi(i), or i where the list holds no position of the batch (memory safety for a list that is no permutation)
__device__ __forceinline__ int64_t perm_at(const int64_t* __restrict__ perm, int64_t i, int64_t B) {
  const int64_t p = perm[i];
  return (uint64_t)p < (uint64_t)B ? p : i;
}

__device__ __forceinline__ int64_t row_off(const Args& a, int p) { return p == 0 ? 0 : a.U; }

// The four features a lane holds of a row of dp <= 256 floats (0 past `lim`).
__device__ __forceinline__ void load4(const float* __restrict__ row, int64_t lim, int lane, float (&v)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    v[u] = (row && f < lim) ? row[f] : 0.f;
  }
}

__device__ __forceinline__ float dot4(const float (&x)[4], const float (&y)[4]) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) s = fmaf(x[u], y[u], s);
  return wave_sum(s);
}

// v * inv with inv = 1 / max(||v||, 1e-12) (F.normalize) into dst[0, dp), zero past d; returns inv.
__device__ __forceinline__ float store_normalized(const float (&v)[4], int64_t d, int64_t dp, int lane, float* __restrict__ dst) {
  const float iv = 1.f / fmaxf(sqrtf(dot4(v, v)), NORM_EPS);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < dp) dst[f] = f < d ? v[u] * iv : 0.f;
  }
  return iv;
}

// The mix row of side g from its 16 slices (slice order), normalised: mh and 1 / max(||m||, 1e-12).
__device__ __forceinline__ float mix_row(const Args& a, int g, int lane, float (&mh)[4]) {
  const float* part = a.mpart + (int64_t)g * SLICES * a.dp;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    float s = 0.f;
    if (f < a.dp)
      for (int sl = 0; sl < SLICES; ++sl) s += part[sl * a.dp + f];
    mh[u] = s;
  }
  const float iv = 1.f / fmaxf(sqrtf(dot4(mh, mh)), NORM_EPS);
#pragma unroll
  for (int u = 0; u < 4; ++u) mh[u] *= iv;
  return iv;
}

// Back through y = x / max(||x||, 1e-12) given the normalised row xh and inv: (g - xh (xh.g) / (xh.xh)) inv, the dot
// products in double; a row shorter than the floor is divided by the constant (no projection), as torch does.
__device__ __forceinline__ void normalize_bwd(const double (&g)[4], const float (&xh)[4], float iv, double (&out)[4]) {
  double dot = 0., xx = 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    dot += (double)xh[u] * g[u];
    xx += (double)xh[u] * xh[u];
  }
  dot = wave_sum(dot);
  xx = wave_sum(xx);
  const bool proj = iv < 1.f / NORM_EPS && xx > 0.;
  const double pg = proj ? dot / xx : 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) out[u] = (g[u] - xh[u] * pg) * (double)iv;
}

// ---- prep.  Waves [0, 3 Bp): row r of problem p; then 2 x SLICES waves: slice sl of the mix row of side g.
__global__ __launch_bounds__(BLOCK) void mix_prep_kernel(Args a) {
  const int64_t w = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int64_t B = a.B, Bp = a.Bp, d = a.d, dp = a.dp;
  if (w >= NPROB * Bp) {
    const int64_t e = w - NPROB * Bp;
    if (e >= 2 * SLICES) return;
    const int g = (int)(e / SLICES), sl = (int)(e % SLICES);
    const int64_t per = (B + SLICES - 1) / SLICES, lo = sl * per, hi = lo + per < B ? lo + per : B;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t j = lo; j < hi; ++j) {
      const float c = a.nu[j];
      const float* x = a.panel + (row_off(a, g) + a.ids[g][j]) * d;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t f = lane + WAVE * u;
        if (f < d) s[u] = fmaf(c, x[f], s[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t f = lane + WAVE * u;
      if (f < dp) a.mpart[(e * dp) + f] = s[u];
    }
    return;
  }
  const int p = (int)(w / Bp);
  const int64_t r = w - (int64_t)p * Bp, e = w;
  float* h = a.H + e * dp;
  if (lane == 0) a.kap[e] = 0.f;
  if (r >= B) {
    for (int64_t f = lane; f < dp; f += WAVE) h[f] = 0.f;
    if (lane == 0) a.hinv[e] = 0.f;
    if (p < 2) {
      for (int64_t f = lane; f < dp; f += WAVE) a.CH[e * dp + f] = 0.f;
      if (lane == 0) a.cinv[e] = 0.f, a.pinv[e] = -1;
    }
    return;
  }
  const int side = p == 0 ? 0 : 1;  // whose permutation and weight: problem 2 mixes the negatives with the items'
  const float beta = a.beta[side];
  const int64_t rp = perm_at(a.perm[side], r, B);
  float x[4], y[4], c[4];
  load4(a.panel + (row_off(a, p) + a.ids[p][r]) * d, d, lane, x);
  load4(a.panel + (row_off(a, p) + a.ids[p][rp]) * d, d, lane, y);
#pragma unroll
  for (int u = 0; u < 4; ++u) c[u] = beta * x[u] + (1.f - beta) * y[u];
  if (p == 2) {
    const float iv = store_normalized(c, d, dp, lane, h);
    if (lane == 0) a.hinv[e] = iv;
    return;
  }
  const float iv = store_normalized(x, d, dp, lane, h);
  const float ic = store_normalized(c, d, dp, lane, a.CH + e * dp);
  // the position pointing at r (the first, should the list hold r twice)
  int64_t found = -1;
  for (int64_t o = 0; o < B && found < 0; o += WAVE) {
    const bool hit = o + lane < B && a.perm[side][o + lane] == r;
    const unsigned long long m = __ballot(hit);
    if (m) found = o + __builtin_ctzll(m);
  }
  if (lane == 0) {
    a.hinv[e] = iv;
    a.cinv[e] = ic;
    a.pinv[e] = (int32_t)found;
  }
}

// ---- the tile pass.  X: the 128 rows the workgroup owns; Y: the column tiles [lo, hi) of chunk blockIdx.y.
//   MODE_SUMS / MODE_SUMS_ACC  E into LDS (0 past column B), row sums, and (ACC) acc += E Y.
//   MODE_COEF                  coef_col * E into LDS (coef is 0 past column B), acc += that . Y.
// Wave w computes the 64 x 64 quarter (w >> 1, w & 1) of the score tile, and rows [32 w, 32 w + 32) x all columns of the second
// product: its A operand (the tile) from LDS, its B operand (Y) from memory (idg_tnce.hip's tile kernel).
template <int NDT, int MODE>
__global__ __launch_bounds__(BLOCK, NDT <= 4 ? 2 : 1) void mix_tile_kernel(const float* __restrict__ H, int64_t Bp, int64_t B, int per,
                                                                           int n_y, float scale2_gram, const float* __restrict__ coef,
                                                                           float* __restrict__ out_acc, float* __restrict__ out_rs) {
  constexpr int64_t dp = 32 * NDT;
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  float* s_x = lds;
  float* s_y = lds + T * LK;
  float* s_g = lds;
  const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, i = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int p = blockIdx.z;
  // pass 1: (X, Y) = (H0, H0), (H1, H1), (H0, H2); pass 2: (H0, H0), (H1, H1), (H2, H0)
  const int px = MODE == MODE_COEF ? p : (p == 2 ? 0 : p);
  const int py = MODE == MODE_COEF ? (p == 2 ? 0 : p) : p;
  const float scale2 = p == 2 ? LOG2E : scale2_gram;
  const int64_t x0 = (int64_t)blockIdx.x * T;
  const float* X = H + ((int64_t)px * Bp + x0) * dp;
  const float* Yall = H + (int64_t)py * Bp * dp;
  const float* ca = MODE == MODE_COEF ? coef + (int64_t)p * Bp : nullptr;
  const int lo = blockIdx.y * per, hi = lo + per < n_y ? lo + per : n_y;

  f32x16 acc[MODE == MODE_SUMS ? 1 : NDT];
  if (MODE != MODE_SUMS) {
#pragma unroll
    for (int ct = 0; ct < NDT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  }
  float rsum = 0.f;

  for (int t = lo; t < hi; ++t) {
    const int64_t y0 = (int64_t)t * T;
    const float* Y = Yall + y0 * dp;
    f32x16 s[2][2];
    score_tile_128<NDT>(X, Y, s_x, s_y, s);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = 64 * wc + 32 * n + i;
      float a_b = 0.f;
      bool col_ok = true;
      if (MODE == MODE_COEF) a_b = ca[y0 + col];
      else col_ok = y0 + col < B;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 64 * wr + 32 * m + mfma_c_row(r, h);
          const float e = __builtin_amdgcn_exp2f((s[m][n][r] - 1.f) * scale2);
          s_g[row * LG + col] = MODE == MODE_COEF ? a_b * e : (col_ok ? e : 0.f);
        }
    }
    __syncthreads();
    if (MODE != MODE_COEF) {
      // row sums: thread t adds 64 columns of row t / 2 in order, then the pair meets
      const int row = tid >> 1, hh = tid & 1;
      const float* g = s_g + row * LG + 64 * hh;
      float v = 0.f;
#pragma unroll 8
      for (int k = 0; k < 64; ++k) v += g[k];
      const float o = __shfl_xor(v, 1, WAVE);
      rsum += hh == 0 ? v + o : o + v;
    }
    if (MODE != MODE_SUMS) {
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

  const int64_t slab = ((int64_t)p * gridDim.y + blockIdx.y) * Bp + x0;  // [problem][chunk][Bp]
  if (MODE != MODE_SUMS) {
    float* out = out_acc + slab * dp;
#pragma unroll
    for (int ct = 0; ct < NDT; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h;
        out[(int64_t)row * dp + 32 * ct + i] = acc[ct][r];
      }
  }
  if (MODE != MODE_COEF && (tid & 1) == 0) out_rs[slab + (tid >> 1)] = rsum;
}

// ---- rows.  One wave per (problem, row).
__global__ __launch_bounds__(BLOCK) void mix_rows_kernel(Args a, int grads) {
  const int64_t w = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int64_t B = a.B, Bp = a.Bp, dp = a.dp;
  if (w >= NPROB * B) return;
  const int p = (int)(w / B);
  const int64_t k = w - (int64_t)p * B, e = (int64_t)p * Bp + k;
  float S = 0.f;
  for (int ch = 0; ch < a.chunks; ++ch) S += a.rs[((int64_t)p * a.chunks + ch) * Bp + k];
  const float inv_B = 1.f / (float)B;
  float hk[4];
  load4(a.H + k * dp, dp, lane, hk);  // problem 2's anchors are the users' rows: H0
  if (p == 2) {
    float ph[4];
    load4(a.H + (Bp + k) * dp, dp, lane, ph);
    const float r = __builtin_amdgcn_exp2f((dot4(hk, ph) - 1.f) * LOG2E) / S;
    if (lane == 0) {
      a.lrow[e] = -logf(r + GUARD);
      if (grads) {
        const float q = (a.upstream ? a.upstream[0] : 1.f) * (1.f - a.beta[1]) * inv_B * (r / (r + GUARD));
        a.qr[k] = q;
        a.kap[e] = q / S;
      }
    }
    return;
  }
  if (p == 1) load4(a.H + e * dp, dp, lane, hk);
  const float beta = a.beta[p];
  const int64_t ip = a.pinv[e];  // the row whose second half has h_k as its anchor (-1: none)
  float mh[4], c1[4], c2[4];
  mix_row(a, p, lane, mh);
  load4(a.CH + e * dp, dp, lane, c1);
  load4(ip >= 0 ? a.CH + ((int64_t)p * Bp + ip) * dp : nullptr, dp, lane, c2);
  const float em = __builtin_amdgcn_exp2f((dot4(hk, mh) - 1.f) * a.scale2);
  const float D = S + em;
  const float r1 = __builtin_amdgcn_exp2f((dot4(hk, c1) - 1.f) * a.scale2) / D;
  const float r2 = __builtin_amdgcn_exp2f((dot4(hk, c2) - 1.f) * a.scale2) / D;
  if (lane != 0) return;
  float l = -beta * logf(r1 + GUARD);
  if (ip >= 0) l -= (1.f - beta) * logf(r2 + GUARD);
  a.lrow[e] = l;
  if (!grads) return;
  const float wgt = (a.upstream ? a.upstream[1] : 1.f) * a.ssl_weight * inv_B;
  const float q1 = wgt * beta * (r1 / (r1 + GUARD));
  const float q2 = ip >= 0 ? wgt * (1.f - beta) * (r2 / (r2 + GUARD)) : 0.f;
  const float kappa = (q1 + q2) / D;
  a.q1[e] = q1;
  if (ip >= 0) a.q2[(int64_t)p * Bp + ip] = q2;
  a.kap[e] = kappa;
  a.kem[e] = kappa * em;
}

// loss[0] = (1 - item_beta) / B sum_i lrow[2][i];  loss[1] = ssl_weight / B (sum lrow[0] + sum lrow[1]): fixed trees of 1024
// leaves, one workgroup per entry.
__global__ __launch_bounds__(1024) void mix_loss_kernel(Args a, float* __restrict__ loss) {
  __shared__ float s[1024];
  const int tid = threadIdx.x;
  const float inv_B = 1.f / (float)a.B;
  if (blockIdx.x == 0) {
    float acc = 0.f;
    for (int64_t b = tid; b < a.B; b += 1024) acc += a.lrow[2 * a.Bp + b];
    const float sum = idg::block_tree_sum<1024>(acc, s);
    if (tid == 0) loss[0] = (1.f - a.beta[1]) * (sum * inv_B);
  } else {
    float acc = 0.f;
    for (int64_t b = tid; b < a.B; b += 1024) acc += a.lrow[b];
    const float su = idg::block_tree_sum<1024>(acc, s);
    __syncthreads();
    acc = 0.f;
    for (int64_t b = tid; b < a.B; b += 1024) acc += a.lrow[a.Bp + b];
    const float si = idg::block_tree_sum<1024>(acc, s);
    if (tid == 0) loss[1] = a.ssl_weight * (su * inv_B + si * inv_B);
  }
}

// ---- mixcol.  Wave (g, slice): sum over the slice's rows k of kappa_k e_km h_k, rows ascending.
__global__ __launch_bounds__(BLOCK) void mix_col_kernel(Args a) {
  const int64_t e = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (e >= 2 * SLICES) return;
  const int g = (int)(e / SLICES), sl = (int)(e % SLICES);
  const int64_t B = a.B, dp = a.dp;
  const int64_t per = (B + SLICES - 1) / SLICES, lo = sl * per, hi = lo + per < B ? lo + per : B;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t k = lo; k < hi; ++k) {
    const float c = a.kem[(int64_t)g * a.Bp + k];
    const float* h = a.H + ((int64_t)g * a.Bp + k) * dp;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t f = lane + WAVE * u;
      if (f < dp) s[u] = fmaf(c, h[f], s[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < dp) a.dmpart[e * dp + f] = s[u];
  }
}

// d loss / d c_i of side g, back through c's normalisation: d ch_i = -(1 / T)(q1_i h_i + q2_i h_pi(i)).
__device__ __forceinline__ void mixed_row_grad(const Args& a, int g, int64_t i, int lane, double (&out)[4]) {
  const int64_t base = (int64_t)g * a.Bp, e = base + i;
  const int64_t ip = perm_at(a.perm[g], i, a.B);
  float h1[4], h2[4], ch[4];
  load4(a.H + e * a.dp, a.dp, lane, h1);
  load4(a.H + (base + ip) * a.dp, a.dp, lane, h2);
  load4(a.CH + e * a.dp, a.dp, lane, ch);
  // q2_i was written by the row pi(i) whose inverse is i; a row that is not the FIRST to point at pi(i) has no second half
  const bool second = a.pinv[base + ip] == (int32_t)i;
  const double q1 = a.q1[e], q2 = second ? (double)a.q2[e] : 0.;
  double g4[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) g4[u] = -(double)a.inv_tau * (q1 * h1[u] + q2 * h2[u]);
  normalize_bwd(g4, ch, a.cinv[e], out);
}

// ---- finish.  One wave per (problem, row): d loss / d x of the gathered row into dX.
__global__ __launch_bounds__(BLOCK) void mix_finish_kernel(Args a) {
  const int64_t w = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int64_t B = a.B, Bp = a.Bp, dp = a.dp;
  if (w >= NPROB * B) return;
  const int p = (int)(w / B);
  const int64_t k = w - (int64_t)p * B, e = (int64_t)p * Bp + k;
  double dx[4] = {0., 0., 0., 0.};
  if (p == 2) {
    // through Mn_k and Mn_j, j the first position with piI(j) = k
    const float bI = a.beta[1];
    for (int half = 0; half < 2; ++half) {
      int64_t j = k;
      if (half == 1) {
        j = a.pinv[Bp + k];
        if (j < 0) break;
      }
      const int64_t ej = 2 * Bp + j;
      float sh[4];
      load4(a.H + ej * dp, dp, lane, sh);
      double g4[4], o4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t f = lane + WAVE * u;
        float s = 0.f;
        if (f < dp)
          for (int ch = 0; ch < a.chunks; ++ch) s += a.acc2[(((int64_t)2 * a.chunks + ch) * Bp + j) * dp + f];
        g4[u] = s;
      }
      normalize_bwd(g4, sh, a.hinv[ej], o4);
      const double c = half == 0 ? (double)bI : 1. - (double)bI;
#pragma unroll
      for (int u = 0; u < 4; ++u) dx[u] += c * o4[u];
    }
  } else {
    const int64_t ip = a.pinv[e];
    const double kap = a.kap[e], kem = a.kem[e], q1 = a.q1[e], it = a.inv_tau;
    const double q2 = ip >= 0 ? (double)a.q2[(int64_t)p * Bp + ip] : 0.;
    const double qr = a.qr[k];
    float hk[4], mh[4], c1[4], c2[4], oth[4];
    load4(a.H + e * dp, dp, lane, hk);
    const float minv = mix_row(a, p, lane, mh);
    load4(a.CH + e * dp, dp, lane, c1);
    load4(ip >= 0 ? a.CH + ((int64_t)p * Bp + ip) * dp : nullptr, dp, lane, c2);
    load4(a.H + ((int64_t)(1 - p) * Bp + k) * dp, dp, lane, oth);  // the rectangular term's other row: ph_k, or a_k
    double Srect = 0.;
    if (p == 0) {
      float S = 0.f;
      for (int ch = 0; ch < a.chunks; ++ch) S += a.rs[((int64_t)2 * a.chunks + ch) * Bp + k];
      Srect = S;
    }
    double g4[4], o4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t f = lane + WAVE * u;
      float s1 = 0.f, s2 = 0.f, sr = 0.f;
      if (f < dp)
        for (int ch = 0; ch < a.chunks; ++ch) {
          s1 += a.acc1[(((int64_t)p * a.chunks + ch) * Bp + k) * dp + f];
          s2 += a.acc2[(((int64_t)p * a.chunks + ch) * Bp + k) * dp + f];
          if (p == 0) sr += a.acc1[(((int64_t)2 * a.chunks + ch) * Bp + k) * dp + f];
        }
      double g = it * (kap * s1 + s2 + kem * mh[u] - q1 * c1[u] - q2 * c2[u]);
      if (p == 0) g += qr * ((double)sr / Srect - oth[u]);
      else g -= qr * oth[u];
      g4[u] = g;
    }
    normalize_bwd(g4, hk, a.hinv[e], o4);
#pragma unroll
    for (int u = 0; u < 4; ++u) dx[u] = o4[u];
    // through c_k (weight beta) and c_ip (weight 1 - beta)
    const double beta = a.beta[p];
    mixed_row_grad(a, p, k, lane, o4);
#pragma unroll
    for (int u = 0; u < 4; ++u) dx[u] += beta * o4[u];
    // every position j with pi(j) = k mixes x_k into c_j
    for (int64_t o = 0; o < B; o += WAVE) {
      const bool hit = o + lane < B && a.perm[p][o + lane] == k;
      unsigned long long m = __ballot(hit);
      while (m) {
        const int64_t j = o + __builtin_ctzll(m);
        m &= m - 1;
        mixed_row_grad(a, p, j, lane, o4);
#pragma unroll
        for (int u = 0; u < 4; ++u) dx[u] += (1. - beta) * o4[u];
      }
    }
    // through m: d mh = (1 / T) sum_k kappa_k e_km h_k
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t f = lane + WAVE * u;
      float s = 0.f;
      if (f < dp)
        for (int sl = 0; sl < SLICES; ++sl) s += a.dmpart[((int64_t)p * SLICES + sl) * dp + f];
      g4[u] = it * (double)s;
    }
    normalize_bwd(g4, mh, minv, o4);
    const double nk = a.nu[k];
#pragma unroll
    for (int u = 0; u < 4; ++u) dx[u] += nk * o4[u];
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < dp) a.dX[e * dp + f] = (float)dx[u];
  }
}

// One wave per batch position b of one id list: if no earlier position holds the same id, every occurrence of the id is
// added in batch order and the sum ADDED to the panel row (idg_tnce.hip's query scatter).
__global__ __launch_bounds__(BLOCK) void mix_scatter_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dq, int64_t B,
                                                            int64_t d, int64_t dp, float* __restrict__ g_rows) {
  const int64_t b = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (b >= B) return;
  const int64_t id = ids[b];
  bool e = false, l = false;
  for (int64_t o = 0; o < B; o += WAVE) {
    const int64_t i = o + lane;
    const bool hit = i < B && ids[i] == id;
    e |= hit && i < b;
    l |= hit && i > b;
  }
  if (__ballot(e) != 0) return;
  const int64_t end = __ballot(l) != 0 ? B : 0;
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
    if (lane + WAVE * u < d) g_rows[id * d + lane + WAVE * u] += g[u];
}

template <int MODE>
void launch_tile(int ndt, dim3 grid, hipStream_t st, const float* H, int64_t Bp, int64_t B, int per, int n_y, float scale2,
                 const float* coef, float* out_acc, float* out_rs) {
  switch (ndt) {
#define IDG_MIX_CASE(NN)                                                                                                  \
  case NN:                                                                                                                \
    hipLaunchKernelGGL((mix_tile_kernel<NN, MODE>), grid, dim3(BLOCK), 0, st, H, Bp, B, per, n_y, scale2, coef, out_acc,   \
                       out_rs);                                                                                           \
    break;
    IDG_MIX_CASE(1) IDG_MIX_CASE(2) IDG_MIX_CASE(3) IDG_MIX_CASE(4)
    IDG_MIX_CASE(5) IDG_MIX_CASE(6) IDG_MIX_CASE(7) IDG_MIX_CASE(8)
#undef IDG_MIX_CASE
  }
}

}  // namespace

extern "C" {

size_t idg_mix_nce_workspace_bytes(int64_t B, int64_t d) {
  if (B <= 0 || B >= ((int64_t)1 << 22) || d <= 0 || d > 32 * MAX_NDT) return 0;
  return layout(B, d).total;
}

int idg_mix_nce_f32(const float* panel, int64_t n, int64_t d, int64_t num_users, const int64_t* users, const int64_t* pos,
                    const int64_t* neg, int64_t B, const int64_t* user_perm, const int64_t* item_perm, const float* nu,
                    float user_beta, float item_beta, float temperature, float ssl_weight, float* loss, const float* upstream,
                    float* g_panel, void* ws, void* stream) {
  IDG_REQUIRE(panel && users && pos && neg && user_perm && item_perm && nu && ws, "idg_mix_nce_f32: NULL argument");
  IDG_REQUIRE(B >= 1 && B < ((int64_t)1 << 22), "idg_mix_nce_f32: B = %lld (1 .. 2^22 - 1)", (long long)B);
  IDG_REQUIRE(d >= 1 && d <= 32 * MAX_NDT, "idg_mix_nce_f32: d = %lld (1 .. %d are built)", (long long)d, 32 * MAX_NDT);
  IDG_REQUIRE(num_users >= 1 && n > num_users, "idg_mix_nce_f32: bad panel (n = %lld rows, %lld of them users)", (long long)n,
              (long long)num_users);
  IDG_REQUIRE(temperature > 0.f && std::isfinite(temperature), "idg_mix_nce_f32: temperature must be positive");
  IDG_REQUIRE(user_beta >= 0.f && user_beta <= 1.f && item_beta >= 0.f && item_beta <= 1.f,
              "idg_mix_nce_f32: mixing weights outside [0, 1] (%g, %g)", (double)user_beta, (double)item_beta);
  IDG_REQUIRE(std::isfinite(ssl_weight), "idg_mix_nce_f32: ssl_weight is not finite");
  IDG_REQUIRE(loss || g_panel, "idg_mix_nce_f32: nothing to compute");
  IDG_REQUIRE(((uintptr_t)panel | (uintptr_t)g_panel | (uintptr_t)nu | (uintptr_t)loss) % 4 == 0 && (uintptr_t)ws % 256 == 0,
              "idg_mix_nce_f32: misaligned panel or workspace (panels 4 bytes, ws 256 bytes)");
  IDG_REQUIRE(!idg::overlap(g_panel, idg::extent(n, d, d), panel, idg::extent(n, d, d)),
              "idg_mix_nce_f32: g_panel overlaps panel");
  hipStream_t st = (hipStream_t)stream;
  const Geo g = geo_of(B, d);
  const Ws w = layout(B, d);
  char* base = reinterpret_cast<char*>(ws);
  auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  Args a;
  a.panel = panel;
  a.d = d, a.dp = g.dp, a.U = num_users, a.B = B, a.Bp = g.Bp;
  a.ids[0] = users, a.ids[1] = pos, a.ids[2] = neg;
  a.perm[0] = user_perm, a.perm[1] = item_perm;
  a.nu = nu;
  a.beta[0] = user_beta, a.beta[1] = item_beta;
  a.inv_tau = 1.f / temperature;
  a.scale2 = a.inv_tau * LOG2E;
  a.ssl_weight = ssl_weight;
  a.upstream = upstream;
  a.chunks = g.chunks;
  a.H = at(w.H), a.hinv = at(w.hinv), a.CH = at(w.CH), a.cinv = at(w.cinv);
  a.pinv = reinterpret_cast<int32_t*>(base + w.pinv);
  a.mpart = at(w.mpart), a.rs = at(w.rs), a.acc1 = at(w.acc1), a.kap = at(w.kap), a.q1 = at(w.q1), a.q2 = at(w.q2);
  a.kem = at(w.kem), a.qr = at(w.qr), a.lrow = at(w.lrow), a.acc2 = at(w.acc2), a.dmpart = at(w.dmpart), a.dX = at(w.dX);
  const bool grads = g_panel != nullptr;
  const int ndt = (int)(g.dp / 32);
  auto blocks = [](int64_t waves) { return dim3((unsigned)((waves + WPB - 1) / WPB)); };

  hipLaunchKernelGGL(mix_prep_kernel, blocks(NPROB * g.Bp + 2 * SLICES), dim3(BLOCK), 0, st, a);
  const dim3 grid((unsigned)g.nbt, (unsigned)g.chunks, NPROB);
  if (grads) launch_tile<MODE_SUMS_ACC>(ndt, grid, st, a.H, g.Bp, B, g.per, g.nbt, a.scale2, nullptr, a.acc1, a.rs);
  else launch_tile<MODE_SUMS>(ndt, grid, st, a.H, g.Bp, B, g.per, g.nbt, a.scale2, nullptr, nullptr, a.rs);
  hipLaunchKernelGGL(mix_rows_kernel, blocks(NPROB * B), dim3(BLOCK), 0, st, a, grads ? 1 : 0);
  if (loss) hipLaunchKernelGGL(mix_loss_kernel, dim3(2), dim3(1024), 0, st, a, loss);
  if (grads) {
    launch_tile<MODE_COEF>(ndt, grid, st, a.H, g.Bp, B, g.per, g.nbt, a.scale2, a.kap, a.acc2, nullptr);
    hipLaunchKernelGGL(mix_col_kernel, blocks(2 * SLICES), dim3(BLOCK), 0, st, a);
    hipLaunchKernelGGL(mix_finish_kernel, blocks(NPROB * B), dim3(BLOCK), 0, st, a);
    const int64_t P = g.Bp * g.dp;
    for (int p = 0; p < NPROB; ++p)
      hipLaunchKernelGGL(mix_scatter_kernel, blocks(B), dim3(BLOCK), 0, st, a.ids[p], a.dX + p * P, B, d, g.dp,
                         g_panel + (p == 0 ? 0 : num_users) * d);
  }
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
