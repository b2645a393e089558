// DirectAU (Wang et al., KDD'22): alignment + uniformity loss over a batch's (user, positive item) rows and the
// gradients of both, without an autograd graph and without the B x B distance matrix.
//
//   a_i = normalize(final[users[i]]),  b_i = normalize(final[num_users + pos[i]])       (F.normalize, eps 1e-12)
//   loss[0] = mean_i ||a_i - b_i||^2
//   loss[1] = gamma (unif(a) + unif(b)) / 2,  unif(x) = log(sum_{i<j} s_ij / (B (B - 1) / 2)),  s_ij = exp(-2 ||x_i - x_j||^2)
//   loss[2] = reg_lambda (||E0[users]||^2 / 2B + ||E0[num_users + pos]||^2 / 2B)
//
// The uniformity term is a pass over 64 x 64 tiles of the pair matrix per row set: the Gram tile <x_i, x_j>, the squared
// distance q_i + q_j - 2 <x_i, x_j> with each row's own squared norm q (clamped at 0), s_ij with the diagonal and the
// columns past B zeroed, and two per-row sums r_i = sum_j s_ij and sum_j s_ij x_j — the tile never leaves the
// workgroup.  With R = sum_i r_i = 2 sum_{i<j} s_ij:  d loss[1] / d x_i = (-4 gamma / R) (r_i x_i - sum_{j != i} s_ij x_j).
// The column tiles of a 64-row stripe are cut into a few slices (one workgroup each, enough of them to fill the chip);
// slices are added in slice order, the row sums by a fixed tree: no float atomics, the same bits every run.
//
// Gradients reach the panel rows through the sorted (row, slot) plan of idg_bpr_plan_f32 run with neg := pos (its
// third slot of every triple is ignored): the occurrences of one row are added in batch order by one wave.
#include <hip/hip_runtime.h>

#include <cmath>

#include "idg_common.h"
#include "idg_device.h"

namespace {

using idg::align256;
using idg::f32x16;
using idg::WAVE;
using idg::wave_sum;
constexpr int BLOCK = 256;
constexpr int TS = 64;        // pair tile: 64 stripe rows x 64 columns
constexpr int LLD = TS + 4;   // LDS row stride (floats) of the MFMA form
constexpr int GK = 16;        // feature chunk of the generic form's Gram tile
constexpr int MAX_NF = 4;     // MFMA form: d = 64 NF, NF <= 4 (d <= 256)
constexpr int TARGET_WG = 256;
constexpr float NORM_EPS = 1e-12f;

// slices of a stripe's column tiles: enough workgroups (2 sets x stripes x slices) to cover the chip, a function of B only
struct Slices {
  int nt, per, gs;
};

Slices slices_of(int64_t B) {
  Slices s;
  s.nt = (int)((B + TS - 1) / TS);
  int want = TARGET_WG / (2 * s.nt);
  if (want < 1) want = 1;
  if (want > s.nt) want = s.nt;
  s.per = (s.nt + want - 1) / want;
  s.gs = (s.nt + s.per - 1) / s.per;
  return s;
}

struct AuWs {
  size_t plan, X, q, nrm, al, rq, pr, pacc, gx, scal, total;
};

AuWs au_layout(int64_t B, int64_t d) {
  const Slices sl = slices_of(B);
  AuWs w;
  size_t o = 0;
  w.plan = o;
  o += align256(idg_bpr_workspace_bytes(B, d));
  w.X = o;
  o += align256((size_t)2 * B * d * 4);
  w.q = o;
  o += align256((size_t)2 * B * 4);
  w.nrm = o;
  o += align256((size_t)2 * B * 4);
  w.al = o;
  o += align256((size_t)B * 4);
  w.rq = o;
  o += align256((size_t)2 * B * 4);
  w.pr = o;
  o += align256((size_t)2 * sl.gs * B * 4);
  w.pacc = o;
  o += align256((size_t)2 * sl.gs * B * d * 4);
  w.gx = o;
  o += align256((size_t)2 * B * d * 4);
  w.scal = o;
  o += 256;
  w.total = o;
  return w;
}

// One wave per batch position i: both normalised rows (X[0][i] = a_i, X[1][i] = b_i), their squared norms q, the raw
// norms (for the backward of normalize), ||a_i - b_i||^2 and the squared norms of the two ego rows.
__global__ __launch_bounds__(BLOCK) void au_prep_kernel(const float* __restrict__ fin, const float* __restrict__ ego,
                                                        const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
                                                        int64_t B, int64_t d, int64_t num_users, float* __restrict__ X,
                                                        float* __restrict__ q, float* __restrict__ nrm, float* __restrict__ al,
                                                        float* __restrict__ rq) {
  const int64_t i = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (i >= B) return;
  const int64_t r0 = users[i], r1 = num_users + pos[i];
  const float* e0 = fin + r0 * d;
  const float* e1 = fin + r1 * d;
  float s0 = 0.f, s1 = 0.f, g0 = 0.f, g1 = 0.f;
  for (int64_t f = lane; f < d; f += WAVE) {
    const float x0 = e0[f], x1 = e1[f];
    s0 = fmaf(x0, x0, s0);
    s1 = fmaf(x1, x1, s1);
    const float y0 = ego[r0 * d + f], y1 = ego[r1 * d + f];
    g0 = fmaf(y0, y0, g0);
    g1 = fmaf(y1, y1, g1);
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  g0 = wave_sum(g0);
  g1 = wave_sum(g1);
  const float n0 = sqrtf(s0), n1 = sqrtf(s1);
  const float den0 = fmaxf(n0, NORM_EPS), den1 = fmaxf(n1, NORM_EPS);
  float q0 = 0.f, q1 = 0.f, a = 0.f;
  for (int64_t f = lane; f < d; f += WAVE) {
    const float x0 = e0[f] / den0, x1 = e1[f] / den1;
    X[i * d + f] = x0;
    X[(B + i) * d + f] = x1;
    q0 = fmaf(x0, x0, q0);
    q1 = fmaf(x1, x1, q1);
    const float t = x0 - x1;
    a = fmaf(t, t, a);
  }
  q0 = wave_sum(q0);
  q1 = wave_sum(q1);
  a = wave_sum(a);
  if (lane == 0) {
    q[i] = q0;
    q[B + i] = q1;
    nrm[i] = n0;
    nrm[B + i] = n1;
    al[i] = a;
    rq[i] = g0;
    rq[B + i] = g1;
  }
}

__device__ __forceinline__ float pair_s(const float* __restrict__ qs, int64_t B, int64_t gi, int64_t gj, float g) {
  if (gi >= B || gj >= B || gi == gj) return 0.f;
  const float d2 = fmaxf(qs[gi] + qs[gj] - 2.f * g, 0.f);
  return expf(-2.f * d2);
}

// ---- the pair pass on the fp32 matrix cores (d = 64 NF).  v_mfma_f32_32x32x2_f32, exact fp32 products and accumulation,
// in the operand layout of ssl_logits_mfma_kernel: lane (i, h) feeds row i's K-values [kc + 32h, kc + 32h + 32); C/D map:
// column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
//   grid: (slices, stripes, 2 sets).  Per column tile: the 64 x 64 Gram tile (each wave a 32 x 32 quarter; operands from
//   64-deep LDS chunks of the stripe's and the tile's rows), s into LDS, the row sums, then S . X_tile (each wave 32 rows
//   x NF 32-wide feature tiles, the S operand from LDS, X's rows straight from memory: 128-byte runs per lane half).
template <int NF>
__global__ __launch_bounds__(BLOCK) void au_pair_mfma_kernel(const float* __restrict__ X, const float* __restrict__ q,
                                                             int64_t B, int per, int gs, float* __restrict__ pr,
                                                             float* __restrict__ pacc) {
  constexpr int64_t d = 64 * NF;
  __shared__ __attribute__((aligned(16))) float s_a[TS * LLD];
  __shared__ __attribute__((aligned(16))) float s_b[TS * LLD];
  __shared__ __attribute__((aligned(16))) float s_s[TS * LLD];
  const int set = blockIdx.z, slice = blockIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * TS;
  const int nt = (int)((B + TS - 1) / TS);
  const int t_lo = slice * per, t_hi = t_lo + per < nt ? t_lo + per : nt;
  const float* Xs = X + (int64_t)set * B * d;
  const float* qs = q + (int64_t)set * B;
  const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, i = lane & 31, h = lane >> 5;
  const int tr = 32 * (wave >> 1), tc = 32 * (wave & 1);
  f32x16 acc[NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nf][r] = 0.f;
  float rs = 0.f;  // threads < 64: the row sum of stripe row tid
  for (int t = t_lo; t < t_hi; ++t) {
    const int64_t j0 = (int64_t)t * TS;
    f32x16 g;
#pragma unroll
    for (int r = 0; r < 16; ++r) g[r] = 0.f;
    for (int64_t kc = 0; kc < d; kc += 64) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = tid + BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
        // (rows past the set: a valid row, its products never used)
        const int64_t ra = i0 + rr < B ? i0 + rr : B - 1, rb = j0 + rr < B ? j0 + rr : B - 1;
        *reinterpret_cast<float4*>(s_a + rr * LLD + c4) = *reinterpret_cast<const float4*>(Xs + ra * d + kc + c4);
        *reinterpret_cast<float4*>(s_b + rr * LLD + c4) = *reinterpret_cast<const float4*>(Xs + rb * d + kc + c4);
      }
      __syncthreads();
      const float* pa = s_a + (tr + i) * LLD + 32 * h;
      const float* pb = s_b + (tc + i) * LLD + 32 * h;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float4 x = *reinterpret_cast<const float4*>(pa + 4 * c);
        const float4 y = *reinterpret_cast<const float4*>(pb + 4 * c);
        g = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, g, 0, 0, 0);
        g = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, g, 0, 0, 0);
        g = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, g, 0, 0, 0);
        g = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, g, 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = tr + idg::mfma_c_row(r, h), col = tc + i;
      s_s[row * LLD + col] = pair_s(qs, B, i0 + row, j0 + col, g[r]);
    }
    __syncthreads();
    if (tid < TS)
      for (int c = 0; c < TS; ++c) rs += s_s[tid * LLD + c];
    const float* ps = s_s + (tr + i) * LLD + 32 * h;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const int64_t fc = 32 * ((wave & 1) + 2 * nf) + i;
#pragma unroll 8
      for (int c = 0; c < 32; ++c) {
        const int64_t jj = j0 + 32 * h + c;
        const float xv = jj < B ? Xs[jj * d + fc] : 0.f;
        acc[nf] = __builtin_amdgcn_mfma_f32_32x32x2f32(ps[c], xv, acc[nf], 0, 0, 0);
      }
    }
    __syncthreads();  // s_s is rewritten by the next tile
  }
  const int64_t base = (int64_t)set * gs + slice;
  if (tid < TS && i0 + tid < B) pr[base * B + i0 + tid] = rs;
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const int64_t fc = 32 * ((wave & 1) + 2 * nf) + i;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = i0 + tr + idg::mfma_c_row(r, h);
      if (row < B) pacc[(base * B + row) * d + fc] = acc[nf][r];
    }
  }
}

// ---- the same pass for any width (SIMT).  Gram tile: 4 x 4 per thread over 16-feature LDS chunks; S . X_tile: thread t
// owns stripe row t / 4 and features t % 4, t % 4 + 4, ... and adds its tile's sum into the slice's partial row (stored
// at the slice's first tile) — each element has one owner: no atomics.
__global__ __launch_bounds__(BLOCK) void au_pair_kernel(const float* __restrict__ X, const float* __restrict__ q, int64_t B,
                                                        int64_t d, int per, int gs, float* __restrict__ pr,
                                                        float* __restrict__ pacc) {
  __shared__ float s_a[TS][GK + 1];
  __shared__ float s_b[TS][GK + 1];
  __shared__ float s_s[TS][TS + 1];
  const int set = blockIdx.z, slice = blockIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * TS;
  const int nt = (int)((B + TS - 1) / TS);
  const int t_lo = slice * per, t_hi = t_lo + per < nt ? t_lo + per : nt;
  const float* Xs = X + (int64_t)set * B * d;
  const float* qs = q + (int64_t)set * B;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int64_t base = (int64_t)set * gs + slice;
  const int prow = tid >> 2, pf = tid & 3;
  float* out = pacc + (base * B + i0 + prow) * d;
  float rs = 0.f;
  for (int t = t_lo; t < t_hi; ++t) {
    const int64_t j0 = (int64_t)t * TS;
    float g[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) g[a][b] = 0.f;
    for (int64_t kc = 0; kc < d; kc += GK) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = tid + BLOCK * j, rr = e >> 4, c = e & 15;
        const int64_t f = kc + c;
        const int64_t ra = i0 + rr < B ? i0 + rr : B - 1, rb = j0 + rr < B ? j0 + rr : B - 1;
        s_a[rr][c] = f < d ? Xs[ra * d + f] : 0.f;
        s_b[rr][c] = f < d ? Xs[rb * d + f] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < GK; ++c)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) g[a][b] = fmaf(s_a[4 * ty + a][c], s_b[tx + 16 * b][c], g[a][b]);
      __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        s_s[4 * ty + a][tx + 16 * b] = pair_s(qs, B, i0 + 4 * ty + a, j0 + tx + 16 * b, g[a][b]);
    __syncthreads();
    if (tid < TS)
      for (int c = 0; c < TS; ++c) rs += s_s[tid][c];
    if (i0 + prow < B) {
      const int cmax = (int)(B - j0 < TS ? B - j0 : TS);
      for (int64_t f = pf; f < d; f += 4) {
        float sum = 0.f;
        for (int c = 0; c < cmax; ++c) sum = fmaf(s_s[prow][c], Xs[(j0 + c) * d + f], sum);
        out[f] = t == t_lo ? sum : out[f] + sum;
      }
    }
    __syncthreads();
  }
  if (tid < TS && i0 + tid < B) pr[base * B + i0 + tid] = rs;
}

// loss[0..2] and the gradient scales — one workgroup, a fixed tree of 1024 leaves.  scal[0..1]: the uniformity
// coefficients -4 gamma / R_set, scal[2]: the alignment's, scal[3]: the regulariser's upstream factor (upstream: device
// [3], d total / d loss[k]; NULL = ones).
__global__ __launch_bounds__(1024) void au_reduce_kernel(const float* __restrict__ al, const float* __restrict__ rq,
                                                         const float* __restrict__ pr, int64_t B, int gs, float gamma,
                                                         float reg_lambda, const float* __restrict__ upstream,
                                                         float* __restrict__ loss, float* __restrict__ scal) {
  __shared__ float s[5][1024];
  const int tid = threadIdx.x;
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t i = tid; i < B; i += 1024) {
    acc[0] += al[i];
    acc[1] += rq[i];
    acc[2] += rq[B + i];
    for (int set = 0; set < 2; ++set) {
      float r = 0.f;
      for (int sl = 0; sl < gs; ++sl) r += pr[((int64_t)set * gs + sl) * B + i];
      acc[3 + set] += r;
    }
  }
  for (int k = 0; k < 5; ++k) s[k][tid] = acc[k];
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o)
      for (int k = 0; k < 5; ++k) s[k][tid] += s[k][tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float fB = (float)B;
    const float up0 = upstream ? upstream[0] : 1.f, up1 = upstream ? upstream[1] : 1.f;
    scal[2] = up0;
    scal[3] = upstream ? upstream[2] : 1.f;
    loss[0] = s[0][0] / fB;
    if (B >= 2) {
      // mean over the B (B - 1) / 2 pairs of s = (R / 2) / (B (B - 1) / 2)
      const float pairs = fB * (fB - 1.f);
      loss[1] = gamma * (logf(s[3][0] / pairs) + logf(s[4][0] / pairs)) * 0.5f;
      scal[0] = (-4.f * gamma / s[3][0]) * up1;
      scal[1] = (-4.f * gamma / s[4][0]) * up1;
    } else {
      // torch.pdist of one row is empty: its mean (and the log) is NaN, and no gradient flows from it
      loss[1] = __builtin_nanf("");
      scal[0] = scal[1] = 0.f;
    }
    float reg = 0.f;
    for (int k = 1; k < 3; ++k) {
      const float nr = sqrtf(s[k][0]);  // embedding.norm(2)
      reg += 0.5f * (nr * nr) / fB;
    }
    loss[2] = reg_lambda * reg;
  }
}

// One wave per (set, i): d (loss[0] + loss[1]) / d x = coef (r_i x_i - sum_slices S X) + (2 / B) (x_i - y_i), back through
// normalize(): (g - <g, x> x) / ||e|| for ||e|| >= eps, g / eps below.  Into gx[set][i].
__global__ __launch_bounds__(BLOCK) void au_slot_grad_kernel(const float* __restrict__ X, const float* __restrict__ nrm,
                                                             const float* __restrict__ pr, const float* __restrict__ pacc,
                                                             const float* __restrict__ scal, int64_t B, int64_t d, int gs,
                                                             float* __restrict__ gx) {
  const int64_t idx = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (idx >= 2 * B) return;
  const int set = idx >= B ? 1 : 0;
  const int64_t i = idx - set * B;
  const float* x = X + idx * d;
  const float* y = X + ((1 - set) * B + i) * d;
  float r = 0.f;
  for (int sl = 0; sl < gs; ++sl) r += pr[((int64_t)set * gs + sl) * B + i];
  const float coef = scal[set], ca = (2.f / (float)B) * scal[2];
  float* out = gx + idx * d;
  float dot = 0.f;
  for (int64_t f = lane; f < d; f += WAVE) {
    float sx = 0.f;
    for (int sl = 0; sl < gs; ++sl) sx += pacc[(((int64_t)set * gs + sl) * B + i) * d + f];
    const float xf = x[f];
    const float g = coef * (r * xf - sx) + ca * (xf - y[f]);
    out[f] = g;
    dot = fmaf(g, xf, dot);
  }
  dot = wave_sum(dot);
  const float n = nrm[idx];
  const bool proj = n >= NORM_EPS;
  const float den = proj ? n : NORM_EPS;
  for (int64_t f = lane; f < d; f += WAVE) {
    const float g = out[f];
    out[f] = (proj ? g - dot * x[f] : g) / den;
  }
}

// One wave per distinct row of the sorted plan (slot 3i: users[i] <- gx[0][i]; 3i + 1: num_users + pos[i] <- gx[1][i];
// 3i + 2: the plan's copy of the positive, ignored), occurrences added in batch order; the regulariser's gradient
// (reg_lambda / B) x ego row once per occurrence.  accumulate = 0: the rows are STORED.
__global__ __launch_bounds__(BLOCK) void au_scatter_kernel(const int32_t* __restrict__ skeys, const int32_t* __restrict__ sslots,
                                                           const float* __restrict__ gx, const float* __restrict__ ego,
                                                           int64_t B, int64_t d, float reg_scale, const float* __restrict__ scal,
                                                           float* __restrict__ g_final,
                                                           float* __restrict__ g_ego, int accumulate) {
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int64_t n3 = 3 * B;
  if (j >= n3) return;
  const int32_t row = skeys[j];
  if (j > 0 && skeys[j - 1] == row) return;
  int64_t e = j + 1;
  while (e < n3 && skeys[e] == row) ++e;
  for (int64_t f = lane; f < d; f += WAVE) {
    float acc = 0.f;
    int cnt = 0;
    for (int64_t t = j; t < e; ++t) {
      const int32_t s = sslots[t];
      const int64_t i = s / 3;
      const int kind = s - 3 * (int32_t)i;
      if (kind == 2) continue;
      const float v = gx[((int64_t)kind * B + i) * d + f];
      acc = cnt == 0 ? v : acc + v;
      ++cnt;
    }
    const int64_t o = (int64_t)row * d + f;
    const float r1 = (reg_scale * scal[3]) * ego[o];
    float reg = r1;
    for (int c = 1; c < cnt; ++c) reg += r1;
    if (g_final && g_final == g_ego) {
      g_final[o] = accumulate ? g_final[o] + (acc + reg) : acc + reg;
    } else {
      if (g_final) g_final[o] = accumulate ? g_final[o] + acc : acc;
      if (g_ego) g_ego[o] = accumulate ? g_ego[o] + reg : reg;
    }
  }
}

}  // namespace

extern "C" {

size_t idg_align_uniform_workspace_bytes(int64_t B, int64_t d) {
  if (B <= 0 || d <= 0) return 0;
  return au_layout(B, d).total;
}

int idg_align_uniform_f32(const float* final_panel, const float* ego_panel, int64_t n, int64_t d, const int64_t* users,
                          const int64_t* pos, int64_t B, int64_t num_users, float gamma, float reg_lambda, float* loss,
                          const float* upstream, float* g_final, float* g_ego, int accumulate, const void* plan_ws, void* ws,
                          void* stream) {
  IDG_REQUIRE(final_panel && ego_panel && users && pos && loss && ws, "idg_align_uniform_f32: NULL argument");
  IDG_REQUIRE(B > 0 && d > 0 && num_users >= 0 && n >= num_users, "idg_align_uniform_f32: bad sizes");
  IDG_REQUIRE(n < ((int64_t)1 << 31) && 3 * B < ((int64_t)1 << 31), "idg_align_uniform_f32: sizes exceed int32 keys");
  hipStream_t st = (hipStream_t)stream;
  const AuWs w = au_layout(B, d);
  const Slices sl = slices_of(B);
  char* base = reinterpret_cast<char*>(ws);
  float* X = reinterpret_cast<float*>(base + w.X);
  float* q = reinterpret_cast<float*>(base + w.q);
  float* nrm = reinterpret_cast<float*>(base + w.nrm);
  float* al = reinterpret_cast<float*>(base + w.al);
  float* rq = reinterpret_cast<float*>(base + w.rq);
  float* pr = reinterpret_cast<float*>(base + w.pr);
  float* pacc = reinterpret_cast<float*>(base + w.pacc);
  float* gx = reinterpret_cast<float*>(base + w.gx);
  float* scal = reinterpret_cast<float*>(base + w.scal);
  const bool grads = g_final || g_ego;
  if (grads && !plan_ws) {  // the scatter plan of (users, pos, pos), in-call
    const int rc = idg_bpr_plan_f32(users, pos, pos, B, num_users, n, base + w.plan, stream);
    if (rc != IDG_OK) return rc;
  }
  const unsigned nb = (unsigned)((B + (BLOCK / WAVE) - 1) / (BLOCK / WAVE));
  hipLaunchKernelGGL(au_prep_kernel, dim3(nb), dim3(BLOCK), 0, st, final_panel, ego_panel, users, pos, B, d, num_users, X, q,
                     nrm, al, rq);
  const dim3 grid((unsigned)sl.gs, (unsigned)sl.nt, 2);
  const int nf = (int)(d / 64);
  if (d % 64 == 0 && nf <= MAX_NF) {
    switch (nf) {
      case 1: hipLaunchKernelGGL(au_pair_mfma_kernel<1>, grid, dim3(BLOCK), 0, st, X, q, B, sl.per, sl.gs, pr, pacc); break;
      case 2: hipLaunchKernelGGL(au_pair_mfma_kernel<2>, grid, dim3(BLOCK), 0, st, X, q, B, sl.per, sl.gs, pr, pacc); break;
      case 3: hipLaunchKernelGGL(au_pair_mfma_kernel<3>, grid, dim3(BLOCK), 0, st, X, q, B, sl.per, sl.gs, pr, pacc); break;
      default: hipLaunchKernelGGL(au_pair_mfma_kernel<4>, grid, dim3(BLOCK), 0, st, X, q, B, sl.per, sl.gs, pr, pacc); break;
    }
  } else {
    hipLaunchKernelGGL(au_pair_kernel, grid, dim3(BLOCK), 0, st, X, q, B, d, sl.per, sl.gs, pr, pacc);
  }
  hipLaunchKernelGGL(au_reduce_kernel, dim3(1), dim3(1024), 0, st, al, rq, pr, B, sl.gs, gamma, reg_lambda, upstream, loss,
                     scal);
  if (grads) {
    const unsigned nb2 = (unsigned)((2 * B + (BLOCK / WAVE) - 1) / (BLOCK / WAVE));
    hipLaunchKernelGGL(au_slot_grad_kernel, dim3(nb2), dim3(BLOCK), 0, st, X, nrm, pr, pacc, scal, B, d, sl.gs, gx);
    const int32_t *skeys = nullptr, *sslots = nullptr;
    idg::bpr_plan_lists(plan_ws ? plan_ws : base + w.plan, B, &skeys, &sslots);
    const unsigned nb3 = (unsigned)((3 * B + (BLOCK / WAVE) - 1) / (BLOCK / WAVE));
    hipLaunchKernelGGL(au_scatter_kernel, dim3(nb3), dim3(BLOCK), 0, st, skeys, sslots, gx, ego_panel, B, d,
                       reg_lambda / (float)B, scal, g_final, g_ego, accumulate ? 1 : 0);
  }
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
