// SCCF (Wu et al., KDD'24; models/SCCF.py:54-81 of the reference): the in-batch second-order contrastive loss over a
// batch's (user, positive item) rows and its gradient, without an autograd graph, a [Nu, Ni] matrix or torch.unique.
//
//   a_i = normalize(final[users[i]]),  b_i = normalize(final[num_users + pos[i]])          (F.normalize, eps 1e-12)
//   f(s) = exp(s / T) + exp(s^2 / T),  f'(s) = (exp(s / T) + 2 s exp(s^2 / T)) / T
//   loss[0] = -(1 / B) sum_i log f(a_i.b_i)
//   loss[1] = log(mean over [Nu, Ni] of f(ah_k.bh_l) cu_k ci_l)        (distinct users / positives, their multiplicities)
//           = log(sum_{i<B} sum_{j<B} f(a_i.b_j) / (Nu Ni))            (cu_k ci_l counts the pair's occurrences in B x B)
// so the second term is ONE rectangular Gram problem over the batch rows as they come, plus the two distinct-id counts:
// the run heads of the sorted (row, slot) plan of idg_bpr_plan_f32(users, pos, pos) (user rows < num_users <= item rows;
// the plan's third slot repeats the positive and adds no row).  With Z = sum sum f the weight of every pair's gradient is
// the same scalar 1 / Z, so the score tiles are formed once: the pass that sums f also accumulates sum_j f'(s_ij) b_j per
// user slot and sum_i f'(s_ij) a_i per item slot, unnormalised; 1 / Z is applied in the per-slot stage.
// Scores are cosines: exp((s - 1) / T) and exp((s^2 - 1) / T) are <= 1 and 1 / T goes back into the log (idg_mixnce.hip's
// convention); the factor cancels in f' / Z.
//
//   prep     one wave per (padded) batch position: both normalised rows into zero-padded [Bp, 32 NDT] operand copies
//            (idg_tile128.h), the raw norms, log f(a_i.b_i) and f' / f at a_i.b_i.
//   pair     grid (row tile, column tile): the 128 x 128 score tile on the matrix cores, rows and columns >= B masked; the
//            tile's sum of f (thread order, then a fixed tree, in double); f' into the LDS tile; then tile . B-rows (into slice
//            `column tile` of the user slots) and tile^T . A-rows (into slice `row tile` of the item slots), each element
//            of the slices written by exactly one workgroup.
//   reduce   one workgroup: Z (tile order, a fixed tree, double), the counts from the plan, both losses, up[1] / Z, up[0] / B.
//   slices   idg::slices_reduce: the partial gradient rows added in slice order.
//   slot     one wave per (side, i): the slot's gradient, back through normalize(), formed and kept in double.
//   scatter  one wave per distinct row of the plan: occurrences added in batch order in double and rounded once, then
//            ADDED into or STORED to g_final;
//            store mode also writes the row of g_ego as zeros (SCCF has no term on the ego rows).
// No float atomics, every sum in a fixed order: the same bits every run, and the same loss bits with or without gradients.
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
constexpr int WPB = BLOCK / WAVE;
constexpr float NORM_EPS = 1e-12f;
constexpr float LOG2E = 1.4426950408889634f;

struct Geo {
  int64_t dp, Bp;
  int nbt;
};

Geo geo_of(int64_t B, int64_t d) {
  Geo g;
  g.dp = round_up(d, 32);
  g.Bp = round_up(B, T);
  g.nbt = (int)(g.Bp / T);
  return g;
}

// Offsets (bytes) into the workspace.  H: [2][Bp][dp] (users' rows, positives' rows); part: [nbt][2][Bp][dp].
struct Ws {
  size_t plan, H, nrm, lup, cup, zt, part, gsum, gx, scal, total;
};

Ws layout(int64_t B, int64_t d) {
  const Geo g = geo_of(B, d);
  Ws w;
  size_t o = 0;
  const size_t P = (size_t)g.Bp * (size_t)g.dp * 4;
  w.plan = o, o += align256(idg_bpr_workspace_bytes(B, d));
  w.H = o, o += align256(2 * P);
  w.nrm = o, o += align256((size_t)2 * g.Bp * 4);
  w.lup = o, o += align256((size_t)g.Bp * 4);
  w.cup = o, o += align256((size_t)g.Bp * 4);
  w.zt = o, o += align256((size_t)g.nbt * g.nbt * 8);
  w.part = o, o += align256((size_t)g.nbt * 2 * P);
  w.gsum = o, o += align256(2 * P);
  w.gx = o, o += align256((size_t)2 * B * d * 8);
  w.scal = o, o += 256;
  w.total = o;
  return w;
}

// The four features a lane holds of a row of at most 256 floats (0 past `lim`).
__device__ __forceinline__ void load4(const float* __restrict__ row, int64_t lim, int lane, float (&v)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    v[u] = f < lim ? row[f] : 0.f;
  }
}

__device__ __forceinline__ float dot4(const float (&x)[4], const float (&y)[4]) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) s = fmaf(x[u], y[u], s);
  return wave_sum(s);
}

// ---- prep.  One wave per padded batch position.
__global__ __launch_bounds__(BLOCK) void sccf_prep_kernel(const float* __restrict__ fin, const int64_t* __restrict__ users,
                                                          const int64_t* __restrict__ pos, int64_t B, int64_t Bp, int64_t d,
                                                          int64_t dp, int64_t num_users, float inv_tau, float* __restrict__ H,
                                                          float* __restrict__ nrm, float* __restrict__ lup,
                                                          float* __restrict__ cup) {
  const int64_t i = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (i >= Bp) return;
  float* ha = H + i * dp;
  float* hb = H + (Bp + i) * dp;
  if (i >= B) {
    for (int64_t f = lane; f < dp; f += WAVE) ha[f] = 0.f, hb[f] = 0.f;
    if (lane == 0) nrm[i] = 0.f, nrm[Bp + i] = 0.f, lup[i] = 0.f, cup[i] = 0.f;
    return;
  }
  float x[4], y[4];
  load4(fin + users[i] * d, d, lane, x);
  load4(fin + (num_users + pos[i]) * d, d, lane, y);
  const float n0 = sqrtf(dot4(x, x)), n1 = sqrtf(dot4(y, y));
  const float den0 = fmaxf(n0, NORM_EPS), den1 = fmaxf(n1, NORM_EPS);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    x[u] = f < d ? x[u] / den0 : 0.f;
    y[u] = f < d ? y[u] / den1 : 0.f;
    if (f < dp) ha[f] = x[u], hb[f] = y[u];
  }
  const float s = dot4(x, y);
  if (lane == 0) {
    // log f(s) = m / T + log(e1 + e2) with m = max(s, s^2): finite for every T > 0
    const float s2 = s * s, m = fmaxf(s, s2);
    const float e1 = expf((s - m) * inv_tau), e2 = expf((s2 - m) * inv_tau);
    nrm[i] = n0;
    nrm[Bp + i] = n1;
    lup[i] = m * inv_tau + logf(e1 + e2);
    cup[i] = (e1 + 2.f * s * e2) / (e1 + e2) * inv_tau;
  }
}

// ---- the pair pass.  Workgroup (I, J): rows [128 I, 128 I + 128) of the users' operand against rows [128 J, ...) of the
// positives'.  Wave w computes the 64 x 64 quarter (w >> 1, w & 1) of the score tile, then rows [32 w, 32 w + 32) x all
// features of both products: the A operand (the tile, or its transpose) from LDS, the B operand (the rows) from memory.
template <int NDT, bool GRADS>
__global__ __launch_bounds__(BLOCK, NDT <= 4 ? 2 : 1) void sccf_pair_kernel(const float* __restrict__ H, int64_t Bp, int64_t B,
                                                                            float scale2, float inv_tau, double* __restrict__ zt,
                                                                            float* __restrict__ part) {
  constexpr int64_t dp = 32 * NDT;
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  __shared__ double s_z[BLOCK];
  float* s_x = lds;
  float* s_y = lds + T * LK;
  float* s_g = lds;
  const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, i = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t x0 = (int64_t)blockIdx.x * T, y0 = (int64_t)blockIdx.y * T;
  const float* X = H + x0 * dp;
  const float* Y = H + (Bp + y0) * dp;

  f32x16 s[2][2];
  score_tile_128<NDT>(X, Y, s_x, s_y, s);
  double z = 0.;  // Z is a common factor of every gradient row: summed in double (a one-user batch amplifies its error tenfold)
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int col = 64 * wc + 32 * n + i;
    const bool col_ok = y0 + col < B;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 64 * wr + 32 * m + mfma_c_row(r, h);
        const bool ok = col_ok && x0 + row < B;
        const float sc = s[m][n][r];
        const float e1 = __builtin_amdgcn_exp2f((sc - 1.f) * scale2);
        const float e2 = __builtin_amdgcn_exp2f((sc * sc - 1.f) * scale2);
        z += ok ? (double)e1 + (double)e2 : 0.;
        if (GRADS) s_g[row * LG + col] = ok ? fmaf(2.f * sc, e2, e1) * inv_tau : 0.f;
      }
  }
  const double zsum = idg::block_tree_sum<BLOCK>(z, s_z);  // (its barriers also publish the tile)
  if (tid == 0) zt[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = zsum;
  if (!GRADS) return;

  // Both products run one 32-column feature tile at a time, its 128-term sum as FOUR fp32 chains of 32 terms (columns
  // [16 q, 16 q + 16) of each lane half) added pairwise at the end: a quarter of the chain, half its rounding — the sums are a
  // common factor of every slot of a repeated id, where nothing averages it.
  // users' slots: sum_j f'(s_ij) b_j, slice = column tile
  {
    const float* ga = s_g + (32 * wave + i) * LG + 64 * h;
    const float* yb = Y + (int64_t)(64 * h) * dp + i;
    float* out = part + (((int64_t)blockIdx.y * 2 + 0) * Bp + x0) * dp;
#pragma unroll 1
    for (int ct = 0; ct < NDT; ++ct) {
      f32x16 a0, a1, a2, a3;
#pragma unroll
      for (int r = 0; r < 16; ++r) a0[r] = a1[r] = a2[r] = a3[r] = 0.f;
#pragma unroll 4
      for (int k = 0; k < 16; ++k) {
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[k], yb[k * dp + 32 * ct], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[16 + k], yb[(16 + k) * dp + 32 * ct], a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[32 + k], yb[(32 + k) * dp + 32 * ct], a2, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[48 + k], yb[(48 + k) * dp + 32 * ct], a3, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        out[(int64_t)(32 * wave + mfma_c_row(r, h)) * dp + 32 * ct + i] = (a0[r] + a1[r]) + (a2[r] + a3[r]);
    }
  }
  // positives' slots: sum_i f'(s_ij) a_i, slice = row tile
  {
    const float* gt = s_g + (64 * h) * LG + 32 * wave + i;
    const float* xb = X + (int64_t)(64 * h) * dp + i;
    float* out = part + (((int64_t)blockIdx.x * 2 + 1) * Bp + y0) * dp;
#pragma unroll 1
    for (int ct = 0; ct < NDT; ++ct) {
      f32x16 a0, a1, a2, a3;
#pragma unroll
      for (int r = 0; r < 16; ++r) a0[r] = a1[r] = a2[r] = a3[r] = 0.f;
#pragma unroll 4
      for (int k = 0; k < 16; ++k) {
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(gt[k * LG], xb[k * dp + 32 * ct], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(gt[(16 + k) * LG], xb[(16 + k) * dp + 32 * ct], a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(gt[(32 + k) * LG], xb[(32 + k) * dp + 32 * ct], a2, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(gt[(48 + k) * LG], xb[(48 + k) * dp + 32 * ct], a3, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        out[(int64_t)(32 * wave + mfma_c_row(r, h)) * dp + 32 * ct + i] = (a0[r] + a1[r]) + (a2[r] + a3[r]);
    }
  }
}

// ---- reduce.  One workgroup, fixed trees of 1024 leaves.  scal[0] = up[1] / Z, scal[1] = up[0] / B.
__global__ __launch_bounds__(1024) void sccf_reduce_kernel(const double* __restrict__ zt, int64_t ntiles, const float* __restrict__ lup,
                                                           int64_t B, const int32_t* __restrict__ skeys, int64_t num_users,
                                                           float inv_tau, const float* __restrict__ upstream,
                                                           float* __restrict__ loss, double* __restrict__ scal) {
  __shared__ double s[1024];
  const int tid = threadIdx.x;
  double acc = 0.;
  for (int64_t t = tid; t < ntiles; t += 1024) acc += zt[t];
  const double Z = idg::block_tree_sum<1024>(acc, s);
  __syncthreads();
  acc = 0.;
  for (int64_t b = tid; b < B; b += 1024) acc += (double)lup[b];
  const double up = idg::block_tree_sum<1024>(acc, s);
  __syncthreads();
  // run heads of the sorted rows: distinct users (< num_users) and distinct positives
  double cu = 0., ci = 0.;
  for (int64_t j = tid; j < 3 * B; j += 1024) {
    const int32_t row = skeys[j];
    if (j == 0 || skeys[j - 1] != row) {
      if (row < num_users) cu += 1.;
      else ci += 1.;
    }
  }
  const double Nu = idg::block_tree_sum<1024>(cu, s);
  __syncthreads();
  const double Ni = idg::block_tree_sum<1024>(ci, s);
  if (tid == 0) {
    loss[0] = (float)(-up / (double)B);
    loss[1] = (float)(log(Z / (Nu * Ni)) + (double)inv_tau);
    scal[0] = (double)(upstream ? upstream[1] : 1.f) / Z;  // (kept in double: a common factor of every gradient row)
    scal[1] = (double)(upstream ? upstream[0] : 1.f) / (double)B;
  }
}

// ---- slot.  One wave per (side, i): g = (up[1] / Z) sum f' other-rows - (up[0] / B) (f' / f)(a_i.b_i) other_i, back through
// normalize(): (g - <g, h> h) / ||x|| for ||x|| >= eps, g / eps below.  Into gx[side][i] (row stride d), in double: the
// occurrences of one row may nearly cancel (one user met B times: the two terms' shares of its gradient do), so the slots are
// formed and added in double and rounded once, by the scatter.
__global__ __launch_bounds__(BLOCK) void sccf_slot_kernel(const float* __restrict__ H, const float* __restrict__ nrm,
                                                          const float* __restrict__ cup, const float* __restrict__ gsum,
                                                          const double* __restrict__ scal, int64_t B, int64_t Bp, int64_t d,
                                                          int64_t dp, double* __restrict__ gx) {
  const int64_t idx = (int64_t)blockIdx.x * WPB + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (idx >= 2 * B) return;
  const int side = idx >= B ? 1 : 0;
  const int64_t i = idx - side * B, e = side * Bp + i;
  float hx[4], ho[4], gs[4];
  load4(H + e * dp, dp, lane, hx);
  load4(H + ((1 - side) * Bp + i) * dp, dp, lane, ho);
  load4(gsum + e * dp, dp, lane, gs);
  const double cz = scal[0], ca = scal[1] * (double)cup[i];
  double g[4];
  double dot = 0.;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    g[u] = cz * (double)gs[u] - ca * (double)ho[u];
    dot += g[u] * (double)hx[u];
  }
  dot = wave_sum(dot);
  const float n = nrm[e];
  const bool proj = n >= NORM_EPS;
  const double den = proj ? (double)n : (double)NORM_EPS;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < d) gx[idx * d + f] = (g[u] - (proj ? dot * (double)hx[u] : 0.)) / den;
  }
}

// ---- scatter.  One wave per distinct row of the sorted plan (slot 3i: users[i] <- gx[0][i]; 3i + 1: num_users + pos[i] <-
// gx[1][i]; 3i + 2: the plan's copy of the positive, ignored), occurrences added in batch order in double, rounded once.
__global__ __launch_bounds__(BLOCK) void sccf_scatter_kernel(const int32_t* __restrict__ skeys, const int32_t* __restrict__ sslots,
                                                             const double* __restrict__ gx, int64_t B, int64_t d,
                                                             float* __restrict__ g_final, float* __restrict__ g_ego,
                                                             int accumulate) {
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
    if (!accumulate && g_ego) g_ego[o] = 0.f;
  }
}

template <bool GRADS>
void launch_pair(int ndt, dim3 grid, hipStream_t st, const float* H, int64_t Bp, int64_t B, float scale2, float inv_tau, double* zt,
                 float* part) {
  switch (ndt) {
#define IDG_SCCF_CASE(NN)                                                                                                     \
  case NN:                                                                                                                    \
    hipLaunchKernelGGL((sccf_pair_kernel<NN, GRADS>), grid, dim3(BLOCK), 0, st, H, Bp, B, scale2, inv_tau, zt, part);          \
    break;
    IDG_SCCF_CASE(1) IDG_SCCF_CASE(2) IDG_SCCF_CASE(3) IDG_SCCF_CASE(4)
    IDG_SCCF_CASE(5) IDG_SCCF_CASE(6) IDG_SCCF_CASE(7) IDG_SCCF_CASE(8)
#undef IDG_SCCF_CASE
  }
}

}  // namespace

extern "C" {

size_t idg_sccf_workspace_bytes(int64_t B, int64_t d) {
  if (B <= 0 || B >= ((int64_t)1 << 22) || d <= 0 || d > 32 * MAX_NDT) return 0;
  return layout(B, d).total;
}

int idg_sccf_loss_f32(const float* final_panel, int64_t n, int64_t d, const int64_t* users, const int64_t* pos, int64_t B,
                      int64_t num_users, float temperature, float* loss, const float* upstream, float* g_final, float* g_ego,
                      int accumulate, const void* plan_ws, void* ws, void* stream) {
  IDG_REQUIRE(final_panel && users && pos && loss && ws, "idg_sccf_loss_f32: NULL argument");
  IDG_REQUIRE(B >= 1 && B < ((int64_t)1 << 22), "idg_sccf_loss_f32: B = %lld (1 .. 2^22 - 1)", (long long)B);
  IDG_REQUIRE(d >= 1 && d <= 32 * MAX_NDT, "idg_sccf_loss_f32: d = %lld (1 .. %d are built)", (long long)d, 32 * MAX_NDT);
  IDG_REQUIRE(num_users >= 1 && n > num_users && n < ((int64_t)1 << 31),
              "idg_sccf_loss_f32: bad panel (n = %lld rows, %lld of them users)", (long long)n, (long long)num_users);
  IDG_REQUIRE(temperature > 0.f && std::isfinite(temperature), "idg_sccf_loss_f32: temperature must be positive");
  IDG_REQUIRE(!g_ego || (g_final && g_ego != g_final), "idg_sccf_loss_f32: g_ego needs a g_final distinct from it");
  IDG_REQUIRE(!idg::overlap(g_final, idg::extent(n, d, d), final_panel, idg::extent(n, d, d)) &&
                  !idg::overlap(g_ego, idg::extent(n, d, d), final_panel, idg::extent(n, d, d)) &&
                  !idg::overlap(g_ego, idg::extent(n, d, d), g_final, idg::extent(n, d, d)),
              "idg_sccf_loss_f32: gradient panels overlap the input or each other");
  IDG_REQUIRE((uintptr_t)ws % 256 == 0, "idg_sccf_loss_f32: ws must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Geo g = geo_of(B, d);
  const Ws w = layout(B, d);
  char* base = reinterpret_cast<char*>(ws);
  auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  float *H = at(w.H), *nrm = at(w.nrm), *lup = at(w.lup), *cup = at(w.cup), *part = at(w.part);
  double* zt = reinterpret_cast<double*>(base + w.zt);
  float* gsum = at(w.gsum);
  double* scal = reinterpret_cast<double*>(base + w.scal);
  double* gx = reinterpret_cast<double*>(base + w.gx);
  const bool grads = g_final != nullptr;
  if (!plan_ws) {  // the plan of (users, pos, pos) in-call, also for the loss alone: the counts come from it
    const int rc = idg_bpr_plan_f32(users, pos, pos, B, num_users, n, base + w.plan, stream);
    if (rc != IDG_OK) return rc;
  }
  const int32_t *skeys = nullptr, *sslots = nullptr;
  idg::bpr_plan_lists(plan_ws ? plan_ws : base + w.plan, B, &skeys, &sslots);
  const float inv_tau = 1.f / temperature;
  auto blocks = [](int64_t waves) { return dim3((unsigned)((waves + WPB - 1) / WPB)); };
  hipLaunchKernelGGL(sccf_prep_kernel, blocks(g.Bp), dim3(BLOCK), 0, st, final_panel, users, pos, B, g.Bp, d, g.dp, num_users,
                     inv_tau, H, nrm, lup, cup);
  const dim3 grid((unsigned)g.nbt, (unsigned)g.nbt);
  const int ndt = (int)(g.dp / 32);
  if (grads) launch_pair<true>(ndt, grid, st, H, g.Bp, B, inv_tau * LOG2E, inv_tau, zt, part);
  else launch_pair<false>(ndt, grid, st, H, g.Bp, B, inv_tau * LOG2E, inv_tau, zt, nullptr);
  hipLaunchKernelGGL(sccf_reduce_kernel, dim3(1), dim3(1024), 0, st, zt, (int64_t)g.nbt * g.nbt, lup, B, skeys, num_users,
                     inv_tau, upstream, loss, scal);
  if (grads) {
    const int rc = idg::slices_reduce(part, g.nbt, 2 * g.Bp * g.dp, gsum, false, stream);
    if (rc != IDG_OK) return rc;
    hipLaunchKernelGGL(sccf_slot_kernel, blocks(2 * B), dim3(BLOCK), 0, st, H, nrm, cup, gsum, scal, B, g.Bp, d, g.dp, gx);
    hipLaunchKernelGGL(sccf_scatter_kernel, blocks(3 * B), dim3(BLOCK), 0, st, skeys, sslots, gx, B, d, g_final, g_ego,
                       accumulate ? 1 : 0);
  }
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
