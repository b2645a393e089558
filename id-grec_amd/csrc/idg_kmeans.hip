// Lloyd's k-means on the device: the E-step of NCL (Lin et al. WWW'22; models/NCL.py:66-81 of the reference, which copies
// both embedding tables to the host every epoch and runs faiss.Kmeans there).
//
//   assign   a_i = argmin_j ||x_i - c_j||^2, evaluated as ||c_j||^2 - 2 <x_i, c_j> (||x_i||^2 does not move the arg-min),
//            ties to the lowest j; dist2_i = max(0, ||x_i||^2 + that minimum).
//   update   c_j = the mean of the rows with a_i = j; a cluster without rows keeps its centroid bit for bit.
//
// Layout.  X and C are copied into the workspace with rows padded to a multiple of 128 and columns to a multiple of 32
// (zeros), so every d <= 256 runs the same matrix-core tiles and no tile load needs a bounds check; a padding centroid
// has ||c||^2 = +inf and is never the minimum.  Every product is v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums.
//   prep     one wave per row: the padded copy and the squared norm (one fixed order: equal rows give equal bits).
//   tile     grid (row tile, centroid chunk): a workgroup owns 128 rows of X and walks the 128-centroid tiles of its chunk
//            (idg_tnce.hip's tiling).  Per tile: S = X C^T from 32-column LDS chunks, ||c||^2 - 2 S into a 128 x 128 LDS
//            tile (row stride 129), then thread t scans 64 columns of row t / 2 in ascending order with a strict <.  The
//            running (min, arg-min) pair stays in registers across the tiles; the [N, K] matrix is never stored.  One
//            pair per (chunk, row) is written.
//   combine  one thread per row: the chunks' pairs in chunk order (equal values: the lower index), assign and dist2.
//   update   histogram of the assignment (integer atomics: the counts do not depend on arrival order), an exclusive scan,
//            a stable placement (one wave per cluster walks the assignment in row order and places its rows by ballot
//            rank: a counting sort whose output does not depend on arrival order), then one wave per cluster adds its
//            rows in ascending row order in double and stores the mean.
//   inertia  1024 contiguous segments of dist2 added in row order in double, then a fixed tree over the segments.
// No float atomics, every sum in a fixed order: the same bits every run.
#include <hip/hip_runtime.h>

#include <cmath>

#include "idg_common.h"
#include "idg_tile128.h"

namespace {

using namespace idg::tile128;  // T = 128 rows of an X tile / centroids of a C tile, LG the row stride of the distance tile
using idg::align256;
using idg::f32x16;
using idg::mfma_c_row;
using idg::round_up;
using idg::WAVE;
using idg::wave_sum;

constexpr int MAX_NDT = 8;    // d <= 256
constexpr int MAX_CHUNKS = 64;
constexpr int TARGET_WGS = 512;  // two 66 KB workgroups per CU
constexpr int RED = 1024;     // threads of the one-workgroup scan / reduction kernels

struct Geo {
  int64_t dp, Np, Kp;
  int nrt, nkt, chunks, per;
};

Geo geo_of(int64_t N, int64_t K, int64_t d) {
  Geo g;
  g.dp = round_up(d, 32);
  g.Np = round_up(N, T);
  g.Kp = round_up(K, T);
  g.nrt = (int)(g.Np / T);
  g.nkt = (int)(g.Kp / T);
  // too few row tiles to fill the device: the centroid tiles are split over workgroups
  int want = (TARGET_WGS + g.nrt - 1) / g.nrt;
  want = want > MAX_CHUNKS ? MAX_CHUNKS : want;
  want = want > g.nkt ? g.nkt : want;
  g.per = (g.nkt + want - 1) / want;
  g.chunks = (g.nkt + g.per - 1) / g.per;
  return g;
}

struct Ws {
  size_t Xp, xn, Cp, cn, pmin, parg, d2, offs, hist, order, total;
};

Ws layout(int64_t N, int64_t K, int64_t d) {
  const Geo g = geo_of(N, K, d);
  Ws w;
  size_t o = 0;
  w.Xp = o, o += align256((size_t)g.Np * g.dp * 4);
  w.xn = o, o += align256((size_t)g.Np * 4);
  w.Cp = o, o += align256((size_t)g.Kp * g.dp * 4);
  w.cn = o, o += align256((size_t)g.Kp * 4);
  w.pmin = o, o += align256((size_t)g.chunks * g.Np * 4);
  w.parg = o, o += align256((size_t)g.chunks * g.Np * 4);
  w.d2 = o, o += align256((size_t)N * 4);
  w.offs = o, o += align256((size_t)(K + 1) * 4);
  w.hist = o, o += align256((size_t)K * 4);
  w.order = o, o += align256((size_t)N * 4);
  w.total = o;
  return w;
}

// One wave per row of a padded operand: dst [rows_p, dp] <- src [rows, d] (row stride ld), zeros past rows / d;
// norm2[r] = ||row||^2, `pad_norm` for a padding row.
__global__ __launch_bounds__(BLOCK) void km_prep_kernel(const float* __restrict__ src, int64_t ld, int64_t rows, int64_t d,
                                                        int64_t rows_p, int64_t dp, float pad_norm, float* __restrict__ dst,
                                                        float* __restrict__ norm2) {
  const int64_t r = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (r >= rows_p) return;
  const float* s = r < rows ? src + r * ld : nullptr;
  float ss = 0.f;
  for (int64_t f = lane; f < dp; f += WAVE) {
    const float v = (s && f < d) ? s[f] : 0.f;
    ss = fmaf(v, v, ss);
    dst[r * dp + f] = v;
  }
  ss = wave_sum(ss);
  if (lane == 0) norm2[r] = s ? ss : pad_norm;
}

// The tile pass: see the head of the file.  Wave w computes the 64 x 64 quarter (w >> 1, w & 1) of the score tile as 2 x 2
// MFMA blocks.  C/D map of a block: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
template <int NDT>
__global__ __launch_bounds__(BLOCK, 2) void km_tile_kernel(const float* __restrict__ Xp, const float* __restrict__ Cp,
                                                           const float* __restrict__ cn, int per, int nkt, int64_t Np,
                                                           float* __restrict__ pmin, int32_t* __restrict__ parg) {
  constexpr int64_t dp = 32 * NDT;
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  float* s_x = lds;            // [128][LK]   (score phase)
  float* s_y = lds + T * LK;   // [128][LK]
  float* s_g = lds;            // [128][LG]   (after the score phase)
  const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, i = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t x0 = (int64_t)blockIdx.x * T;
  const float* X = Xp + x0 * dp;
  const int lo = blockIdx.y * per, hi = lo + per < nkt ? lo + per : nkt;
  const int row = tid >> 1, hh = tid & 1;
  // the running pair of this thread: row `row`, columns [64 hh, 64 hh + 64) of every tile.  The first centroid of the chunk
  // is a real one (every tile holds at least one), so the index stays inside [0, K) whatever the data.
  float best = INFINITY;
  int32_t barg = lo * T;

  for (int p = lo; p < hi; ++p) {
    const int64_t y0 = (int64_t)p * T;
    const float* Y = Cp + y0 * dp;
    f32x16 s[2][2];
    score_tile_128<NDT>(X, Y, s_x, s_y, s);  // ---- S = X C^T
    // ---- ||c||^2 - 2 <x, c> into the tile (2 s is exact: one rounding)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = 64 * wc + 32 * n + i;
      const float c2 = cn[y0 + col];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rw = 64 * wr + 32 * m + mfma_c_row(r, h);
          s_g[rw * LG + col] = c2 - 2.f * s[m][n][r];
        }
    }
    __syncthreads();
    // ---- the row minima: ascending columns, strict <, so the lowest index of equal values stays
    {
      const float* g = s_g + row * LG + 64 * hh;
      const int32_t c0 = (int32_t)y0 + 64 * hh;
#pragma unroll 8
      for (int k = 0; k < 64; ++k) {
        const float v = g[k];
        if (v < best) {
          best = v;
          barg = c0 + k;
        }
      }
    }
    __syncthreads();  // the tile is overwritten by the next tile's operands
  }
  // the pair of threads of a row meets: the smaller value, the lower index of equal ones
  const float ob = __shfl_xor(best, 1, WAVE);
  const int32_t oa = __shfl_xor(barg, 1, WAVE);
  if (ob < best || (ob == best && oa < barg)) {
    best = ob;
    barg = oa;
  }
  if (hh == 0) {
    pmin[(int64_t)blockIdx.y * Np + x0 + row] = best;
    parg[(int64_t)blockIdx.y * Np + x0 + row] = barg;
  }
}

__global__ __launch_bounds__(BLOCK) void km_combine_kernel(const float* __restrict__ pmin, const int32_t* __restrict__ parg,
                                                           const float* __restrict__ xn, int64_t N, int64_t Np, int chunks,
                                                           int32_t* __restrict__ assign, float* __restrict__ dist2) {
  const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= N) return;
  float best = pmin[r];
  int32_t barg = parg[r];
  for (int ch = 1; ch < chunks; ++ch) {
    const float v = pmin[(int64_t)ch * Np + r];
    const int32_t a = parg[(int64_t)ch * Np + r];
    if (v < best || (v == best && a < barg)) {
      best = v;
      barg = a;
    }
  }
  assign[r] = barg;
  if (dist2) dist2[r] = fmaxf(0.f, xn[r] + best);
}

__global__ __launch_bounds__(BLOCK) void km_zero_kernel(int32_t* __restrict__ p, int64_t n) {
  const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r < n) p[r] = 0;
}

// Integer atomics: the counts are the same whatever the arrival order.  An index outside [0, K) is not counted.
__global__ __launch_bounds__(BLOCK) void km_hist_kernel(const int32_t* __restrict__ assign, int64_t N, int64_t K,
                                                        int32_t* __restrict__ hist) {
  const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= N) return;
  const int32_t a = assign[r];
  if (a >= 0 && a < K) atomicAdd(&hist[a], 1);
}

// offs[j] = sum_{j' < j} hist[j'], offs[K] = the total; one workgroup, thread t owns a contiguous run of clusters.
__global__ __launch_bounds__(RED) void km_scan_kernel(const int32_t* __restrict__ hist, int64_t K, int32_t* __restrict__ offs,
                                                      int32_t* __restrict__ counts) {
  __shared__ int32_t s[RED];
  const int tid = threadIdx.x;
  const int64_t per = (K + RED - 1) / RED, lo = tid * per < K ? tid * per : K, hi = lo + per < K ? lo + per : K;
  int32_t sum = 0;
  for (int64_t j = lo; j < hi; ++j) sum += hist[j];
  s[tid] = sum;
  __syncthreads();
  for (int o = 1; o < RED; o <<= 1) {
    const int32_t v = tid >= o ? s[tid - o] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  int32_t run = s[tid] - sum;
  for (int64_t j = lo; j < hi; ++j) {
    const int32_t c = hist[j];
    offs[j] = run;
    if (counts) counts[j] = c;
    run += c;
  }
  if (tid == RED - 1) offs[K] = s[RED - 1];
}

// One wave per cluster: its rows, in ascending row order, into order[offs[j] .. offs[j + 1]).
__global__ __launch_bounds__(BLOCK) void km_place_kernel(const int32_t* __restrict__ assign, int64_t N, int64_t K,
                                                         const int32_t* __restrict__ offs, int32_t* __restrict__ order) {
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (j >= K) return;
  int32_t at = offs[j];
  const int32_t end = offs[j + 1];
  for (int64_t o = 0; o < N && at < end; o += WAVE) {
    const int64_t r = o + lane;
    const bool hit = r < N && assign[r] == (int32_t)j;
    const unsigned long long m = __ballot(hit);
    if (hit) order[at + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)r;
    at += __popcll(m);
  }
}

// One wave per cluster: the mean of its rows, added in ascending row order (double), four rows in flight.  A cluster
// without rows is left as it is.
__global__ __launch_bounds__(BLOCK) void km_mean_kernel(const float* __restrict__ X, int64_t ldx, int64_t d, int64_t K,
                                                        const int32_t* __restrict__ offs, const int32_t* __restrict__ order,
                                                        float* __restrict__ C) {
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  if (j >= K) return;
  const int32_t lo = offs[j], hi = offs[j + 1];
  if (hi <= lo) return;
  double acc[4] = {0., 0., 0., 0.};
  int32_t t = lo;
  for (; t + 4 <= hi; t += 4) {
    const float* r0 = X + (int64_t)order[t] * ldx;
    const float* r1 = X + (int64_t)order[t + 1] * ldx;
    const float* r2 = X + (int64_t)order[t + 2] * ldx;
    const float* r3 = X + (int64_t)order[t + 3] * ldx;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t f = lane + WAVE * u;
      if (f < d) {
        const float v0 = r0[f], v1 = r1[f], v2 = r2[f], v3 = r3[f];
        acc[u] += (double)v0;
        acc[u] += (double)v1;
        acc[u] += (double)v2;
        acc[u] += (double)v3;
      }
    }
  }
  for (; t < hi; ++t) {
    const float* r0 = X + (int64_t)order[t] * ldx;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t f = lane + WAVE * u;
      if (f < d) acc[u] += (double)r0[f];
    }
  }
  const double cnt = (double)(hi - lo);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t f = lane + WAVE * u;
    if (f < d) C[j * d + f] = (float)(acc[u] / cnt);
  }
}

// out[0] = sum_i v[i]: thread t adds the contiguous run [t per, t per + per) in row order (double), then a fixed tree.
__global__ __launch_bounds__(RED) void km_sum_kernel(const float* __restrict__ v, int64_t N, float* __restrict__ out) {
  __shared__ double s[RED];
  const int tid = threadIdx.x;
  const int64_t per = (N + RED - 1) / RED, lo = tid * per < N ? tid * per : N, hi = lo + per < N ? lo + per : N;
  double acc = 0.;
  for (int64_t r = lo; r < hi; ++r) acc += (double)v[r];
  const double sum = idg::block_tree_sum<RED>(acc, s);
  if (tid == 0) out[0] = (float)sum;
}

void launch_tile(int ndt, dim3 grid, hipStream_t st, const float* Xp, const float* Cp, const float* cn, int per, int nkt,
                 int64_t Np, float* pmin, int32_t* parg) {
  switch (ndt) {
#define IDG_KM_CASE(NN)                                                                                                  \
  case NN:                                                                                                               \
    hipLaunchKernelGGL((km_tile_kernel<NN>), grid, dim3(BLOCK), 0, st, Xp, Cp, cn, per, nkt, Np, pmin, parg);            \
    break;
    IDG_KM_CASE(1) IDG_KM_CASE(2) IDG_KM_CASE(3) IDG_KM_CASE(4)
    IDG_KM_CASE(5) IDG_KM_CASE(6) IDG_KM_CASE(7) IDG_KM_CASE(8)
#undef IDG_KM_CASE
  }
}

struct Bufs {
  Geo g;
  float *Xp, *xn, *Cp, *cn, *pmin, *d2;
  int32_t *parg, *offs, *hist, *order;
};

Bufs bufs_of(void* ws, int64_t N, int64_t K, int64_t d) {
  const Ws w = layout(N, K, d);
  char* base = reinterpret_cast<char*>(ws);
  Bufs b;
  b.g = geo_of(N, K, d);
  b.Xp = reinterpret_cast<float*>(base + w.Xp);
  b.xn = reinterpret_cast<float*>(base + w.xn);
  b.Cp = reinterpret_cast<float*>(base + w.Cp);
  b.cn = reinterpret_cast<float*>(base + w.cn);
  b.pmin = reinterpret_cast<float*>(base + w.pmin);
  b.parg = reinterpret_cast<int32_t*>(base + w.parg);
  b.d2 = reinterpret_cast<float*>(base + w.d2);
  b.offs = reinterpret_cast<int32_t*>(base + w.offs);
  b.hist = reinterpret_cast<int32_t*>(base + w.hist);
  b.order = reinterpret_cast<int32_t*>(base + w.order);
  return b;
}

constexpr int WPB = BLOCK / WAVE;
inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

void prep_x(const Bufs& b, const float* X, int64_t ldx, int64_t N, int64_t d, hipStream_t st) {
  hipLaunchKernelGGL(km_prep_kernel, dim3(blocks_of(b.g.Np, WPB)), dim3(BLOCK), 0, st, X, ldx, N, d, b.g.Np, b.g.dp, 0.f, b.Xp,
                     b.xn);
}

// the padded copy of X is in the workspace already
void assign_prepared(const Bufs& b, int64_t N, int64_t d, const float* C, int64_t K, int32_t* assign, float* dist2,
                     hipStream_t st) {
  hipLaunchKernelGGL(km_prep_kernel, dim3(blocks_of(b.g.Kp, WPB)), dim3(BLOCK), 0, st, C, d, K, d, b.g.Kp, b.g.dp, INFINITY,
                     b.Cp, b.cn);
  launch_tile((int)(b.g.dp / 32), dim3((unsigned)b.g.nrt, (unsigned)b.g.chunks), st, b.Xp, b.Cp, b.cn, b.g.per, b.g.nkt, b.g.Np,
              b.pmin, b.parg);
  hipLaunchKernelGGL(km_combine_kernel, dim3(blocks_of(N, BLOCK)), dim3(BLOCK), 0, st, b.pmin, b.parg, b.xn, N, b.g.Np,
                     b.g.chunks, assign, dist2);
}

void update(const Bufs& b, const float* X, int64_t ldx, int64_t N, int64_t d, const int32_t* assign, int64_t K, float* C,
            int32_t* counts, hipStream_t st) {
  hipLaunchKernelGGL(km_zero_kernel, dim3(blocks_of(K, BLOCK)), dim3(BLOCK), 0, st, b.hist, K);
  hipLaunchKernelGGL(km_hist_kernel, dim3(blocks_of(N, BLOCK)), dim3(BLOCK), 0, st, assign, N, K, b.hist);
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(RED), 0, st, b.hist, K, b.offs, counts);
  hipLaunchKernelGGL(km_place_kernel, dim3(blocks_of(K, WPB)), dim3(BLOCK), 0, st, assign, N, K, b.offs, b.order);
  hipLaunchKernelGGL(km_mean_kernel, dim3(blocks_of(K, WPB)), dim3(BLOCK), 0, st, X, ldx, d, K, b.offs, b.order, C);
}

bool built(int64_t N, int64_t K, int64_t d) {
  const int64_t lim = ((int64_t)1 << 31) - T;
  return N >= 1 && K >= 1 && d >= 1 && d <= 32 * MAX_NDT && N < lim && K < lim;
}

}  // namespace

extern "C" {

size_t idg_kmeans_workspace_bytes(int64_t N, int64_t K, int64_t d) {
  if (!built(N, K, d)) return 0;
  return layout(N, K, d).total;
}

#define IDG_KM_SIZES(who)                                                                                                  \
  IDG_REQUIRE(N >= 1 && K >= 1, who ": bad sizes (N = %lld, K = %lld)", (long long)N, (long long)K);                       \
  IDG_REQUIRE(d >= 1 && d <= 32 * MAX_NDT, who ": d = %lld (1 .. %d are built)", (long long)d, 32 * MAX_NDT);              \
  IDG_REQUIRE(ldx >= d, who ": ldx = %lld is below d = %lld", (long long)ldx, (long long)d);                               \
  IDG_REQUIRE(built(N, K, d), who ": sizes exceed int32 positions");                                                      \
  IDG_REQUIRE((uintptr_t)X % 4 == 0 && (uintptr_t)C % 4 == 0 && (uintptr_t)assign % 4 == 0 && (uintptr_t)ws % 256 == 0,    \
              who ": misaligned argument (panels 4 bytes, ws 256 bytes)")

int idg_kmeans_assign_f32(const float* X, int64_t ldx, int64_t N, int64_t d, const float* C, int64_t K, int32_t* assign,
                          float* dist2, void* ws, void* stream) {
  IDG_REQUIRE(X && C && assign && ws, "idg_kmeans_assign_f32: NULL argument");
  IDG_KM_SIZES("idg_kmeans_assign_f32");
  hipStream_t st = (hipStream_t)stream;
  const Bufs b = bufs_of(ws, N, K, d);
  prep_x(b, X, ldx, N, d, st);
  assign_prepared(b, N, d, C, K, assign, dist2, st);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int idg_kmeans_update_f32(const float* X, int64_t ldx, int64_t N, int64_t d, const int32_t* assign, int64_t K, float* C,
                          int32_t* counts, void* ws, void* stream) {
  IDG_REQUIRE(X && C && assign && ws, "idg_kmeans_update_f32: NULL argument");
  IDG_KM_SIZES("idg_kmeans_update_f32");
  update(bufs_of(ws, N, K, d), X, ldx, N, d, assign, K, C, counts, (hipStream_t)stream);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int idg_kmeans_f32(const float* X, int64_t ldx, int64_t N, int64_t d, int64_t K, int niter, float* C, int32_t* assign,
                   float* inertia, void* ws, void* stream) {
  IDG_REQUIRE(X && C && assign && ws, "idg_kmeans_f32: NULL argument");
  IDG_KM_SIZES("idg_kmeans_f32");
  IDG_REQUIRE(niter >= 0, "idg_kmeans_f32: niter = %d", niter);
  hipStream_t st = (hipStream_t)stream;
  const Bufs b = bufs_of(ws, N, K, d);
  prep_x(b, X, ldx, N, d, st);
  for (int t = 0; t <= niter; ++t) {
    assign_prepared(b, N, d, C, K, assign, inertia ? b.d2 : nullptr, st);
    if (inertia) hipLaunchKernelGGL(km_sum_kernel, dim3(1), dim3(RED), 0, st, b.d2, N, inertia + t);
    if (t < niter) update(b, X, ldx, N, d, assign, K, C, nullptr, st);
  }
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
