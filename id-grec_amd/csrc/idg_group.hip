// IMP-GCN's two operations (reference: models/IMPGCN.py:50-88), d = 64, fp32.
//
// 1. idg_group_assign_f32 — the group membership of every node in ONE launch:
//      temp   = keep1 * leaky_relu((ego + side) . W_fc^T + b_fc)          keep1: idg_dropout.h's mask over (row, feature < 64)
//      scores = keep2 * (temp . W_grp^T + b_grp)                          keep2: the same function over (row, g < G)
//      member[r] = bitmask of { g : scores[r, g] == max_g scores[r, :] }  for r < num_users, (1 << G) - 1 for the item rows
//    W_fc [64, 64] and W_grp [G, 64] in nn.Linear's [out, in] layout.  A workgroup owns 64 rows: ego + side is staged once,
//    coalesced, into an LDS tile (idg_layer64.h); the 64 x 64 product runs on the matrix cores (v_mfma_f32_32x32x2_f32)
//    as FOUR independent chains added pairwise (that header's tile_times_w<4>); the activation goes back into the tile,
//    and the d -> G product, both masks and the compare run from the tile with 16 lanes per row: temp never goes to
//    memory.  The compare is by VALUE (-0.0 == 0.0 ties).
//
// 2. idg_grouped_spmm_f32 — ONE walk of a plain CSR for all G sub-graph products A_g = D_g A D_g, D_g = diag([g in m(r)]):
//      t_g[r] = sum_k values[k] * [g in m(col_k)] * (X_g[col_k] + V[col_k])      for g in m(r)
//      Y_g[r] = t_g[r]  (rows with g not in m(r): NOT written)        S[r] = (S_in ? S_in[r] : 0) + sum_{g in m(r)} t_g[r]
//    A wave walks eight consecutive rows, one after the other: a row's entries are loaded 64 at a time, coalesced, one per
//    lane (column, value, the column's membership byte) and handed round by lane shuffles; the four 16-lane groups of the
//    wave each take every fourth entry, a lane holding four features, with one float4 accumulator per group.  An entry costs
//    ONE gather per group that its two endpoints share — the first and (a tied user) the second such group's rows are
//    requested for four entries ahead of their use, a third and beyond in a loop; the group only enters the ADDRESS, the
//    accumulators are picked by compile-time index (G is a template parameter).  While a row gathers, the next two rows'
//    entry blocks are in flight: columns and values two rows ahead, membership bytes one row ahead.
//    THE PUBLISHED ORDER of a row's sum, which no launch geometry changes: the row's entries are cut into chunks of
//    IDG_GROUP_CHUNK = 512; inside a chunk lane group q adds the entries k = q (mod 4) in ascending k, then the four partial
//    sums are added as (q0 + q1) + (q2 + q3); the chunks' sums are added in chunk order.  Rows longer than one chunk may be
//    listed by the caller (long_rows / long_chunk0): their chunks then run on one wave EACH (partial sums to a workspace,
//    added in chunk order by a third kernel) — the same order, hence the same bits, as the one-wave walk of an unlisted row.
//    No atomics anywhere: two calls give equal bits.
//
// 3. idg_group_grad_f32 — the ego gradient of the fused step from the Horner chain's sum:
//      out[r] = a * S[r] + (r flagged ? b * gF[r] + GE[r] : 0)
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), scratch 0 in every instantiation:
//   group_assign64_kernel        : 113 VGPRs, 19,456 bytes of LDS, occupancy 4 waves / SIMD
//   grouped_rows_kernel<3, .>    : 137 VGPRs (grouped X) / 112 (shared X), occupancy 3 / 4; <8, grouped>: 177, occupancy 2
//   grouped_chunks_kernel<3, .>  : 122 / 77 VGPRs, occupancy 4 / 6
//   grouped_long_rows_kernel<3>  : 24 VGPRs;  group_grad_kernel: 14 VGPRs
// (__launch_bounds__(256, 4) on grouped_rows_kernel<3, grouped> spills 44 bytes per lane: not used.)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idg_common.h"
#include "idg_device.h"
#include "idg_dropout.h"
#include "idg_layer64.h"

namespace {

using idg::f32x16;
using idg::layer64::LDT;
using idg::layer64::RB;  // rows per workgroup tile of the assignment

constexpr int BLOCK = 256;
constexpr int D = 64;
constexpr int GMAX = 8;
constexpr int NCH = 4;   // MFMA chains of the 64 x 64 product
constexpr int CHUNK = IDG_GROUP_CHUNK;
constexpr int XLIVE = 0x100, VLIVE = 0x200;  // next to the 8 membership bits of an entry

__global__ __launch_bounds__(BLOCK, 4) void group_assign64_kernel(const float* __restrict__ ego, const float* __restrict__ side,
                                                               const float* __restrict__ Wfc, const float* __restrict__ bfc,
                                                               const float* __restrict__ Wgrp, const float* __restrict__ bgrp,
                                                               int64_t n, int G, int64_t num_users, float slope, float p,
                                                               uint64_t seed, uint64_t stream1, uint64_t stream2,
                                                               uint8_t* __restrict__ member, float* __restrict__ scores_out) {
  __shared__ __attribute__((aligned(16))) float s_t[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_wg[GMAX * D];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 31, h = lane >> 5;
  const int rt = w >> 1, ct = w & 1;  // this wave's 32 x 32 tile of the 64 x 64 block
  const int col = 32 * ct + i;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  // B operand of temp = x . W_fc^T: B[k][col] = W_fc[col][k], K-values 32 h ... of output column `col`: 8 float4 per lane
  f32x16 wr[2];
  idg::layer64::load_w_row(Wfc, D, col, h, wr[0], wr[1]);
  for (int e = tid; e < G * D; e += BLOCK) s_wg[e] = Wgrp[e];
  // (idg::layer64::stage_panel's loop with the sum of two panels as the value staged)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = tid + BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
    const int64_t row = r0 + rr < n ? r0 + rr : n - 1;  // rows past the end read the last row (and are not written)
    const float4 a = *reinterpret_cast<const float4*>(ego + row * D + c4);
    const float4 b = *reinterpret_cast<const float4*>(side + row * D + c4);
    *reinterpret_cast<float4*>(s_t + rr * LDT + c4) = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
  __syncthreads();
  const f32x16 acc = idg::layer64::tile_times_w<NCH>(s_t, rt, i, h, wr[0], wr[1]);
  __syncthreads();  // every operand has left the tile: it becomes the tile of leaky_relu(. + b_fc)
  {
    const float bb = bfc[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float t = acc[r] + bb;
      s_t[(32 * rt + idg::mfma_c_row(r, h)) * LDT + col] = t > 0.f ? t : t * slope;
    }
  }
  __syncthreads();
  // 16 lanes per row: the first mask, the d -> G product (4 features per lane, then the butterfly of 16 lanes), the second
  // mask and the compare
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = tid + BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
    const int64_t row = r0 + rr;
    float4 v = *reinterpret_cast<const float4*>(s_t + rr * LDT + c4);
    float kp[4];
    idg::keep_scale4(p, seed, stream1, row, c4, kp);
    v.x *= kp[0], v.y *= kp[1], v.z *= kp[2], v.w *= kp[3];
    float sc[GMAX];
    float top = 0.f;
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
      sc[g] = 0.f;
      if (g < G) {
        const float4 wv = *reinterpret_cast<const float4*>(s_wg + g * D + c4);
        float t = v.x * wv.x;
        t += v.y * wv.y, t += v.z * wv.z, t += v.w * wv.w;
        t = idg::lanes_sum<16>(t);
        sc[g] = (t + bgrp[g]) * idg::keep_scale(p, seed, stream2, row, g);
        top = g == 0 ? sc[0] : fmaxf(top, sc[g]);
      }
    }
    if ((e & 15) == 0 && row < n) {
      unsigned m = 0;
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) {
          m |= sc[g] == top ? 1u << g : 0u;
          if (scores_out) scores_out[row * G + g] = sc[g];
        }
      member[row] = (uint8_t)(row < num_users ? m : (1u << G) - 1u);
    }
  }
}

struct GroupedArgs {
  const int64_t* indptr;
  const int32_t* indices;
  const float* values;
  const uint8_t* member;
  const float* X;
  int64_t xgs;  // floats between the groups of X (0: one shared panel)
  const uint32_t* x_rows;
  const float* V;
  const uint32_t* v_rows;
  float* Y;
  int64_t ygs;
  const float* S_in;
  float* S;
  int64_t n;
};

__device__ __forceinline__ void fma4(float4& a, float s, const float4& t) {
  a.x += s * t.x, a.y += s * t.y, a.z += s * t.z, a.w += s * t.w;
}

// One entry per lane of a block of 64 consecutive entries: its column, value and — in m — the column's membership byte with
// the XLIVE / VLIVE flags (0: nothing to read through this entry).  Loaded in two stages, so that a wave can have the NEXT
// rows' stages in flight while it gathers for the current row.
struct Block {
  int col;
  float val;
  int m;
};

__device__ __forceinline__ Block block_cv(const GroupedArgs& a, int64_t kb, int64_t k1, int lane) {
  Block b = {0, 0.f, 0};
  if (kb + lane < k1) {
    b.col = a.indices[kb + lane];
    b.val = a.values[kb + lane];
  }
  return b;
}

__device__ __forceinline__ void block_m(const GroupedArgs& a, Block& b, int64_t kb, int64_t k1, int lane) {
  b.m = 0;
  if (kb + lane < k1) {
    int m = a.member[b.col];
    const unsigned bit = 1u << (b.col & 31);
    int flags = 0;
    if (!a.x_rows || (a.x_rows[b.col >> 5] & bit)) flags |= XLIVE;
    if (a.V && (!a.v_rows || (a.v_rows[b.col >> 5] & bit))) flags |= VLIVE;
    b.m = flags ? (m | flags) : 0;
  }
}

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const int lo = __shfl((int)v, src, 64), hi = __shfl((int)(v >> 32), src, 64);
  return ((int64_t)hi << 32) | (int64_t)(unsigned)lo;
}

// The sums of entries k0 .. k1 - 1 (at most CHUNK of them) of a row whose membership is mr, for every group, on every lane:
// acc[g] for the lane's four features.  `first`: the block at k0, complete (the caller had it in flight).  The order is the
// file header's.
template <int G, bool GROUPED>
__device__ __forceinline__ void chunk_sum(const GroupedArgs& a, int64_t k0, int64_t k1, unsigned mr, int lane, float4 (&acc)[G],
                                          Block first) {
  const int q = lane >> 4, c4 = (lane & 15) * 4;
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t kb = k0; kb < k1; kb += 64) {
    Block b = first;
    if (kb != k0) {
      b = block_cv(a, kb, k1, lane);
      block_m(a, b, kb, k1, lane);
    }
    const int col_l = b.col;
    const float val_l = b.val;
    const int m_l = (b.m & (int)mr) ? (b.m & (int)(mr | XLIVE | VLIVE)) : 0;
    const int nb = (int)(k1 - kb < 64 ? k1 - kb : 64);
#pragma unroll 1
    for (int j0 = 0; j0 < 16 && 4 * j0 < nb; j0 += 4) {
      int col[4], m[4];
      float val[4];
      float4 x[4], x2[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = 4 * (j0 + u) + q;
        col[u] = __shfl(col_l, e, 64), m[u] = __shfl(m_l, e, 64), val[u] = __shfl(val_l, e, 64);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        x[u] = x2[u] = v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        const unsigned live = m[u] & 0xff;
        if (live) {
          const int64_t off = (int64_t)col[u] * D + c4;
          if (m[u] & VLIVE) v[u] = *reinterpret_cast<const float4*>(a.V + off);
          if (GROUPED) {
            x[u] = *reinterpret_cast<const float4*>(a.X + (int64_t)(__ffs(live) - 1) * a.xgs + off);
            const unsigned rest = live & (live - 1);  // a tied user: its second group rides along
            if (rest) x2[u] = *reinterpret_cast<const float4*>(a.X + (int64_t)(__ffs(rest) - 1) * a.xgs + off);
          } else if (m[u] & XLIVE) {
            x[u] = *reinterpret_cast<const float4*>(a.X + off);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        unsigned live = m[u] & 0xff;
        if (!live) continue;
        const float4 t = make_float4(x[u].x + v[u].x, x[u].y + v[u].y, x[u].z + v[u].z, x[u].w + v[u].w);
        if (!GROUPED) {
#pragma unroll
          for (int g = 0; g < G; ++g)
            if ((live >> g) & 1u) fma4(acc[g], val[u], t);
        } else {
          const int g0 = __ffs(live) - 1;
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (g == g0) fma4(acc[g], val[u], t);
          live &= live - 1;
          if (live) {
            const int g1 = __ffs(live) - 1;
            const float4 t2 = make_float4(x2[u].x + v[u].x, x2[u].y + v[u].y, x2[u].z + v[u].z, x2[u].w + v[u].w);
#pragma unroll
            for (int g = 0; g < G; ++g)
              if (g == g1) fma4(acc[g], val[u], t2);
            for (live &= live - 1; live; live &= live - 1) {  // a third group and beyond
              const int gk = __ffs(live) - 1;
              const float4 xg = *reinterpret_cast<const float4*>(a.X + (int64_t)gk * a.xgs + (int64_t)col[u] * D + c4);
              const float4 tg = make_float4(xg.x + v[u].x, xg.y + v[u].y, xg.z + v[u].z, xg.w + v[u].w);
#pragma unroll
              for (int g = 0; g < G; ++g)
                if (g == gk) fma4(acc[g], val[u], tg);
            }
          }
        }
      }
    }
  }
  // (q0 + q1) + (q2 + q3), on every lane
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int o = 16; o <= 32; o *= 2) {
      acc[g].x += __shfl_xor(acc[g].x, o, 64), acc[g].y += __shfl_xor(acc[g].y, o, 64);
      acc[g].z += __shfl_xor(acc[g].z, o, 64), acc[g].w += __shfl_xor(acc[g].w, o, 64);
    }
  }
}

// Row r's outputs from its t_g (lane group 0 writes: 16 lanes x float4 = the row)
template <int G>
__device__ __forceinline__ void row_out(const GroupedArgs& a, int64_t r, unsigned mr, int lane, const float4 (&t)[G]) {
  if (lane >= 16) return;
  const int64_t off = r * D + lane * 4;
  float4 s = a.S_in ? *reinterpret_cast<const float4*>(a.S_in + off) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int g = 0; g < G; ++g)
    if ((mr >> g) & 1u) {
      if (a.Y) *reinterpret_cast<float4*>(a.Y + (int64_t)g * a.ygs + off) = t[g];
      s.x += t[g].x, s.y += t[g].y, s.z += t[g].z, s.w += t[g].w;
    }
  if (a.S) *reinterpret_cast<float4*>(a.S + off) = s;
}

// One wave per RPW consecutive rows, one after the other, with the next two rows' first blocks in flight: row i + 2's
// columns and values and row i + 1's membership bytes are requested before row i's gathers, so a short row (yelp2018: 35
// entries on average) costs its gathers' latency and not four dependent ones.  skip_long: rows longer than a chunk belong
// to the two kernels below.
constexpr int RPW = 8;

template <int G, bool GROUPED>
__global__ __launch_bounds__(BLOCK) void grouped_rows_kernel(GroupedArgs a, int skip_long) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = ((int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6)) * RPW;
  if (r0 >= a.n) return;
  const int nr = (int)(a.n - r0 < RPW ? a.n - r0 : RPW);
  const int64_t kp = lane <= nr ? a.indptr[r0 + lane] : 0;      // lane j: where row r0 + j begins (j = nr: where the last ends)
  const unsigned mrl = lane < nr ? a.member[r0 + lane] : 0u;
  // (row j >= nr: the empty range at the end)
#define IDG_ROW_RANGE(j, k0, k1)                                  \
  const int64_t k0 = shfl64(kp, (j) < nr ? (j) : nr), k1 = shfl64(kp, (j) + 1 < nr ? (j) + 1 : nr)
  IDG_ROW_RANGE(0, a0, a1);
  IDG_ROW_RANGE(1, b0, b1);
  Block cur = block_cv(a, a0, a1, lane);
  Block nxt = block_cv(a, b0, b1, lane);
  block_m(a, cur, a0, a1, lane);
#pragma unroll 1
  for (int i = 0; i < nr; ++i) {
    IDG_ROW_RANGE(i, k0, k1);
    IDG_ROW_RANGE(i + 1, n0, n1);
    IDG_ROW_RANGE(i + 2, f0, f1);
    Block far = block_cv(a, f0, f1, lane);
    block_m(a, nxt, n0, n1, lane);
    const unsigned mr = __shfl(mrl, i, 64);
    if (!(skip_long && k1 - k0 > CHUNK)) {
      float4 t[G], acc[G];
#pragma unroll
      for (int g = 0; g < G; ++g) t[g] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int64_t c0 = k0; c0 < k1; c0 += CHUNK) {
        const int64_t c1 = c0 + CHUNK < k1 ? c0 + CHUNK : k1;
        Block first = cur;
        if (c0 != k0) {
          first = block_cv(a, c0, c1, lane);
          block_m(a, first, c0, c1, lane);
        }
        chunk_sum<G, GROUPED>(a, c0, c1, mr, lane, acc, first);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (c0 == k0)
            t[g] = acc[g];
          else
            t[g].x += acc[g].x, t[g].y += acc[g].y, t[g].z += acc[g].z, t[g].w += acc[g].w;
        }
      }
      row_out<G>(a, r0 + i, mr, lane, t);
    }
    cur = nxt;
    nxt = far;
  }
#undef IDG_ROW_RANGE
}

// One wave per chunk of a listed long row: part[chunk][g][64] for the groups of the row
template <int G, bool GROUPED>
__global__ __launch_bounds__(BLOCK) void grouped_chunks_kernel(GroupedArgs a, const int32_t* __restrict__ long_rows,
                                                             const int32_t* __restrict__ long_chunk0, int n_long, int n_chunks,
                                                             float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (c >= n_chunks) return;
  int lo = 0, hi = n_long - 1;  // the last long row whose first chunk is <= c
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (long_chunk0[mid] <= c) lo = mid; else hi = mid - 1;
  }
  const int64_t r = long_rows[lo];
  if (r < 0 || r >= a.n) return;
  const int64_t row0 = a.indptr[r], row1 = a.indptr[r + 1];
  const int64_t k0 = row0 + (int64_t)(c - long_chunk0[lo]) * CHUNK;
  if (k0 >= row1) return;
  const unsigned mr = a.member[r];
  float4 acc[G];
  const int64_t k1 = k0 + CHUNK < row1 ? k0 + CHUNK : row1;
  Block first = block_cv(a, k0, k1, lane);
  block_m(a, first, k0, k1, lane);
  chunk_sum<G, GROUPED>(a, k0, k1, mr, lane, acc, first);
  if (lane < 16) {
#pragma unroll
    for (int g = 0; g < G; ++g)
      if ((mr >> g) & 1u) *reinterpret_cast<float4*>(part + ((int64_t)c * G + g) * D + lane * 4) = acc[g];
  }
}

// One 16-lane group per listed long row: its chunks' sums in chunk order, then the row's outputs
template <int G>
__global__ __launch_bounds__(BLOCK) void grouped_long_rows_kernel(GroupedArgs a, const int32_t* __restrict__ long_rows,
                                                                const int32_t* __restrict__ long_chunk0, int n_long, int n_chunks,
                                                                const float* __restrict__ part) {
  const int lane = threadIdx.x & 15;
  const int li = blockIdx.x * (BLOCK / 16) + (threadIdx.x >> 4);
  if (li >= n_long) return;
  const int64_t r = long_rows[li];
  if (r < 0 || r >= a.n) return;
  const int64_t len = a.indptr[r + 1] - a.indptr[r];
  if (len <= CHUNK) return;  // (not a long row: grouped_rows_kernel has written it)
  const int c0 = long_chunk0[li];
  int nc = (int)((len + CHUNK - 1) / CHUNK);
  if (c0 < 0 || c0 + nc > n_chunks) return;
  const unsigned mr = a.member[r];
  float4 t[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    t[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((mr >> g) & 1u) {
      for (int c = 0; c < nc; ++c) {
        const float4 u = *reinterpret_cast<const float4*>(part + ((int64_t)(c0 + c) * G + g) * D + lane * 4);
        if (c == 0)
          t[g] = u;
        else
          t[g].x += u.x, t[g].y += u.y, t[g].z += u.z, t[g].w += u.w;
      }
    }
  }
  row_out<G>(a, r, mr, lane, t);
}

__global__ __launch_bounds__(BLOCK) void group_grad_kernel(const float* __restrict__ S, float a, const float* __restrict__ gF, float b,
                                                         const float* __restrict__ GE, const uint32_t* __restrict__ rows, int64_t n,
                                                         float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;  // one float4
  if (e >= n * (D / 4)) return;
  const int64_t r = e >> 4;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (S) {
    const float4 s = *reinterpret_cast<const float4*>(S + 4 * e);
    o = make_float4(a * s.x, a * s.y, a * s.z, a * s.w);
  }
  if (idg::bit_at(rows, r)) {
    const float4 g = *reinterpret_cast<const float4*>(gF + 4 * e);
    const float4 x = *reinterpret_cast<const float4*>(GE + 4 * e);
    o.x += b * g.x + x.x, o.y += b * g.y + x.y, o.z += b * g.z + x.z, o.w += b * g.w + x.w;
  }
  *reinterpret_cast<float4*>(out + 4 * e) = o;
}

using idg::overlap;
using idg::Span;

template <int G>
void launch_grouped(const GroupedArgs& a, const int32_t* long_rows, const int32_t* long_chunk0, int n_long, int n_chunks, float* ws,
                    hipStream_t st) {
  const bool grouped = a.xgs != 0;
  const int64_t row_waves = (a.n + RPW - 1) / RPW;
  const unsigned row_wgs = (unsigned)((row_waves + BLOCK / 64 - 1) / (BLOCK / 64));
  const int skip = n_long > 0;
  if (grouped)
    hipLaunchKernelGGL((grouped_rows_kernel<G, true>), dim3(row_wgs), dim3(BLOCK), 0, st, a, skip);
  else
    hipLaunchKernelGGL((grouped_rows_kernel<G, false>), dim3(row_wgs), dim3(BLOCK), 0, st, a, skip);
  if (!skip) return;
  const unsigned chunk_wgs = (unsigned)((n_chunks + BLOCK / 64 - 1) / (BLOCK / 64));
  if (grouped)
    hipLaunchKernelGGL((grouped_chunks_kernel<G, true>), dim3(chunk_wgs), dim3(BLOCK), 0, st, a, long_rows, long_chunk0, n_long, n_chunks, ws);
  else
    hipLaunchKernelGGL((grouped_chunks_kernel<G, false>), dim3(chunk_wgs), dim3(BLOCK), 0, st, a, long_rows, long_chunk0, n_long, n_chunks, ws);
  hipLaunchKernelGGL((grouped_long_rows_kernel<G>), dim3((unsigned)((n_long + BLOCK / 16 - 1) / (BLOCK / 16))), dim3(BLOCK), 0, st, a,
                     long_rows, long_chunk0, n_long, n_chunks, ws);
}

}  // namespace

extern "C" {

int idg_group_assign_f32(const float* ego, const float* side, const float* W_fc, const float* b_fc, const float* W_grp,
                         const float* b_grp, int64_t n, int64_t d, int G, int64_t num_users, float negative_slope, float p,
                         uint64_t seed, uint64_t stream_fc, uint64_t stream_grp, uint8_t* member, float* scores_out, void* stream) {
  IDG_REQUIRE(ego && side && W_fc && b_fc && W_grp && b_grp && member, "idg_group_assign_f32: NULL argument");
  IDG_REQUIRE(d == D, "idg_group_assign_f32: d = 64 only (got %lld)", (long long)d);
  IDG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "idg_group_assign_f32: bad sizes (n = %lld)", (long long)n);
  IDG_REQUIRE(G >= 1 && G <= GMAX, "idg_group_assign_f32: G = %d outside 1 .. 8 (a membership is one byte)", G);
  IDG_REQUIRE(num_users >= 0 && num_users <= n, "idg_group_assign_f32: num_users = %lld outside 0 .. n", (long long)num_users);
  IDG_REQUIRE(p >= 0.f && p < 1.f, "idg_group_assign_f32: drop probability p = %g outside [0, 1)", (double)p);
  IDG_REQUIRE(((uintptr_t)ego | (uintptr_t)side | (uintptr_t)W_fc) % 16 == 0 &&
                  ((uintptr_t)b_fc | (uintptr_t)W_grp | (uintptr_t)b_grp | (uintptr_t)scores_out) % 4 == 0,
              "idg_group_assign_f32: misaligned argument (panels and W_fc 16 bytes; biases, W_grp and scores_out 4 bytes)");
  const size_t panel = (size_t)n * D * sizeof(float);
  const Span outs[2] = {{member, (size_t)n}, {scores_out, (size_t)n * (size_t)G * sizeof(float)}};
  const Span ins[6] = {{ego, panel}, {side, panel}, {W_fc, sizeof(float) * D * D}, {b_fc, sizeof(float) * D},
                       {W_grp, sizeof(float) * D * (size_t)G}, {b_grp, sizeof(float) * (size_t)G}};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 2, ins, 6), "idg_group_assign_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 2), "idg_group_assign_f32: member and scores_out overlap");
  hipLaunchKernelGGL(group_assign64_kernel, dim3((unsigned)((n + RB - 1) / RB)), dim3(BLOCK), 0, (hipStream_t)stream, ego, side, W_fc,
                     b_fc, W_grp, b_grp, n, G, num_users, negative_slope, p, seed, stream_fc, stream_grp, member, scores_out);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int64_t idg_grouped_spmm_chunk(void) { return CHUNK; }

size_t idg_grouped_spmm_workspace_bytes(int64_t n_chunks, int G) {
  if (n_chunks <= 0 || G < 1 || G > GMAX) return 0;
  return (size_t)n_chunks * (size_t)G * D * sizeof(float);
}

int idg_grouped_spmm_f32(int64_t n, int64_t nnz, const int64_t* indptr, const int32_t* indices, const float* values, int64_t d, int G,
                         const uint8_t* member, const float* X, int64_t x_group_stride, const uint32_t* x_rows, const float* V,
                         const uint32_t* v_rows, float* Y, int64_t y_group_stride, const float* S_in, float* S,
                         const int32_t* long_rows, const int32_t* long_chunk0, int64_t n_long, int64_t n_chunks, void* ws,
                         void* stream) {
  IDG_REQUIRE(indptr && member && X && (Y || S) && (nnz == 0 || (indices && values)),
              "idg_grouped_spmm_f32: NULL argument (at least one of Y and S must be given)");
  IDG_REQUIRE(d == D, "idg_grouped_spmm_f32: d = 64 only (got %lld); other widths: row-masked panels through idg_spmm_f32", (long long)d);
  IDG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) && nnz >= 0, "idg_grouped_spmm_f32: bad sizes (n = %lld, nnz = %lld)", (long long)n,
              (long long)nnz);
  IDG_REQUIRE(G >= 1 && G <= GMAX, "idg_grouped_spmm_f32: G = %d outside 1 .. 8 (a membership is one byte)", G);
  IDG_REQUIRE(x_group_stride == 0 || x_group_stride >= n * D, "idg_grouped_spmm_f32: x_group_stride = %lld (0: one shared panel; else >= n * 64)",
              (long long)x_group_stride);
  IDG_REQUIRE(x_group_stride % 4 == 0 && y_group_stride % 4 == 0, "idg_grouped_spmm_f32: group strides must be multiples of 4 floats");
  IDG_REQUIRE(!Y || y_group_stride >= n * D, "idg_grouped_spmm_f32: y_group_stride = %lld below n * 64", (long long)y_group_stride);
  IDG_REQUIRE(!x_rows || x_group_stride == 0, "idg_grouped_spmm_f32: x_rows names the live rows of a SHARED X only");
  IDG_REQUIRE(!v_rows || V, "idg_grouped_spmm_f32: v_rows without V");
  IDG_REQUIRE(S || !S_in, "idg_grouped_spmm_f32: S_in without S");
  IDG_REQUIRE(((uintptr_t)X | (uintptr_t)V | (uintptr_t)Y | (uintptr_t)S_in | (uintptr_t)S | (uintptr_t)ws) % 16 == 0 &&
                  ((uintptr_t)indptr % 8 == 0) &&
                  ((uintptr_t)indices | (uintptr_t)values | (uintptr_t)x_rows | (uintptr_t)v_rows | (uintptr_t)long_rows | (uintptr_t)long_chunk0) % 4 == 0,
              "idg_grouped_spmm_f32: misaligned argument (panels and ws 16 bytes, indptr 8, the other arrays 4)");
  IDG_REQUIRE(n_long >= 0 && n_chunks >= 0 && n_long < ((int64_t)1 << 31) && n_chunks < ((int64_t)1 << 31) &&
                  (n_long == 0 ? n_chunks == 0 : (long_rows && long_chunk0 && ws && n_chunks >= 2 * n_long)),
              "idg_grouped_spmm_f32: bad long-row schedule (n_long = %lld, n_chunks = %lld; each listed row has >= 2 chunks)",
              (long long)n_long, (long long)n_chunks);
  const size_t panel = (size_t)n * D * sizeof(float), bits = (size_t)((n + 31) / 32) * sizeof(uint32_t);
  const size_t xb = x_group_stride ? ((size_t)(G - 1) * (size_t)x_group_stride + (size_t)n * D) * sizeof(float) : panel;
  const size_t yb = Y ? ((size_t)(G - 1) * (size_t)y_group_stride + (size_t)n * D) * sizeof(float) : 0;
  const size_t wsb = idg_grouped_spmm_workspace_bytes(n_chunks, G);
  const Span outs[3] = {{Y, yb}, {S, panel}, {n_long ? ws : nullptr, wsb}};
  const Span ins[11] = {{indptr, (size_t)(n + 1) * 8}, {indices, (size_t)nnz * 4}, {values, (size_t)nnz * 4}, {member, (size_t)n},
                        {X, xb}, {x_rows, bits}, {V, panel}, {v_rows, bits}, {long_rows, (size_t)n_long * 4},
                        {long_chunk0, (size_t)(n_long + 1) * 4}, {S_in == S ? nullptr : S_in, panel}};  // S_in may BE S (row by row)
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 3, ins, 11), "idg_grouped_spmm_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 3), "idg_grouped_spmm_f32: two outputs overlap");
  const GroupedArgs a = {indptr, indices, values, member, X, x_group_stride, x_rows, V, v_rows, Y, y_group_stride, S_in, S, n};
  hipStream_t st = (hipStream_t)stream;
  const int nl = (int)n_long, nc = (int)n_chunks;
  float* part = reinterpret_cast<float*>(ws);
  switch (G) {
    case 1: launch_grouped<1>(a, long_rows, long_chunk0, nl, nc, part, st); break;
    case 2: launch_grouped<2>(a, long_rows, long_chunk0, nl, nc, part, st); break;
    case 3: launch_grouped<3>(a, long_rows, long_chunk0, nl, nc, part, st); break;
    case 4: launch_grouped<4>(a, long_rows, long_chunk0, nl, nc, part, st); break;
    case 5: launch_grouped<5>(a, long_rows, long_chunk0, nl, nc, part, st); break;
    case 6: launch_grouped<6>(a, long_rows, long_chunk0, nl, nc, part, st); break;
    case 7: launch_grouped<7>(a, long_rows, long_chunk0, nl, nc, part, st); break;
    default: launch_grouped<8>(a, long_rows, long_chunk0, nl, nc, part, st); break;
  }
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int idg_group_grad_f32(const float* S, float a, const float* gF, float b, const float* GE, const uint32_t* rows, int64_t n, int64_t d,
                       float* out, void* stream) {
  IDG_REQUIRE(gF && GE && rows && out, "idg_group_grad_f32: NULL argument");
  IDG_REQUIRE(d == D, "idg_group_grad_f32: d = 64 only (got %lld)", (long long)d);
  IDG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "idg_group_grad_f32: bad sizes (n = %lld)", (long long)n);
  IDG_REQUIRE(((uintptr_t)S | (uintptr_t)gF | (uintptr_t)GE | (uintptr_t)out) % 16 == 0 && (uintptr_t)rows % 4 == 0,
              "idg_group_grad_f32: misaligned argument (panels 16 bytes, rows 4)");
  const size_t panel = (size_t)n * D * sizeof(float);
  IDG_REQUIRE(!overlap(out, panel, gF, panel) && !overlap(out, panel, GE, panel) &&
                  !overlap(out, panel, rows, (size_t)((n + 31) / 32) * 4) && (S == out || !overlap(out, panel, S, panel)),
              "idg_group_grad_f32: out overlaps an input (S may BE out)");
  hipLaunchKernelGGL(group_grad_kernel, dim3((unsigned)((n * (D / 4) + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, S, a, gF, b,
                     GE, rows, n, out);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
