// BIGCF's intent layer (Zhang et al., SIGIR'24) on every row of a propagated panel X, d = 64, k = 128, fp32 throughout:
//   S = X . W [n, k],  P = softmax(S, dim 1) (row maximum subtracted),  T = P . W^T [n, d],  F = X + T o Z,  Z ~ N(0, 1)
// as ONE kernel per direction.  S and P never leave the chip; the backward saves nothing but X: P is recomputed from X and
// W, and Z is idg_normal.h's function of (seed, stream, global row, feature) (or read from a panel, for fixtures).
//   forward : X -> T, F (and, optionally, the Z that was used)
//   backward: gT = gT_in (at the rows of its own bitmap, when given) + gF o Z [never stored];  gP = gT . W;  gS = P o (gP - rowsum(P o gP));
//             gX = gF + gS . W^T;  gW = X^T . gS + gT^T . P
// The shape is idg_gccf.hip's: a workgroup owns a tile of 64 rows (rows row0 + 64 t ...: the first row need not be
// tile-aligned), the panel tile is read ONCE, coalesced (16 lanes x 16 bytes per row), into LDS at idg_layer64.h's row
// stride of 68 floats; S / P (and gP / gS) sit in LDS at a row stride of 132 floats (for the same reason: rows 16-byte
// aligned, b128 operand reads of 16 rows hit 64 distinct banks).  The MFMA row operands (v_mfma_f32_32x32x2_f32) come out
// of LDS.
//
// Where W lives: in the waves' REGISTERS, not in LDS.  W is 32 KB; each product needs it in one of two orders — W[k-step,
// column] for X . W and gT . W (32 registers per lane: one 32-column slice per wave), W[column, k-step] for P . W^T and
// gS . W^T (64 registers per lane: one 32-feature slice per wave) — and in both a lane's operands are fixed for the whole
// launch.  The workgroups are persistent, so the registers are loaded once per workgroup (from L2) and every MFMA's second
// operand costs no LDS read; W in LDS would take 32 KB more of it per workgroup (the backward already holds 102 KB) and add
// one LDS read per MFMA to kernels whose LDS pipe already feeds the first operand.
//
// gW [d, k] is a sum over rows and runs in a fixed order — row slices on the persistent workgroups, accumulators in
// registers across a workgroup's tiles, slices added in slice order by idg::slices_reduce (idg_common.h): two runs give
// the same bits, no float atomics.  A tile with no flagged row is skipped; rows whose bit is clear are neither read nor written.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   intent_fwd_kernel          : 242 VGPRs, 0 AGPRs, 84 SGPRs, 51,456 bytes of LDS, scratch 0, occupancy 2 waves / SIMD
//   intent_bwd_kernel          : 244 VGPRs, 0 AGPRs, 95 SGPRs, 102,912 bytes of LDS, scratch 0, occupancy 2 waves / SIMD
//   intent_noise_kernel        : 36 VGPRs, 0 AGPRs, 40 SGPRs, 0 bytes of LDS, scratch 0, occupancy 8 waves / SIMD
// (The forward at 3 waves / SIMD — 168 VGPRs — spills 356 bytes per lane: both W orders stay in registers across the tiles,
// so it is built for 2.)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idg_common.h"
#include "idg_device.h"
#include "idg_layer64.h"
#include "idg_normal.h"

namespace {

using idg::f32x16;
using idg::layer64::LDT;  // LDS row stride of a [64, d] tile, in floats
using idg::layer64::RB;

constexpr int D = 64;
constexpr int K = 128;
constexpr int LDP = 132;  // LDS row stride of a [64, k] tile, in floats
constexpr int FWD_BLOCK = 256;
constexpr int FWD_WGS = 512;  // resident workgroups of the forward kernel (2 x 256 threads per CU: its registers allow two waves per SIMD)
constexpr int BWD_BLOCK = 512;
constexpr int BWD_WGS = 256;  // resident workgroups of the backward kernel (1 x 512 threads per CU: 102 KB of LDS) = most slices of gW
constexpr int64_t WCOUNT = D * K;

// Z of features c4 .. c4 + 3 of one global row: the panel's, or the generator's
__device__ __forceinline__ void noise4(const float* __restrict__ noise, uint64_t seed, uint64_t stream, int64_t row, int c4, float z[4]) {
  if (noise) {
    const float4 v = *reinterpret_cast<const float4*>(noise + row * D + c4);
    z[0] = v.x, z[1] = v.y, z[2] = v.z, z[3] = v.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) z[c] = idg::normal_of(seed, stream, row, c4 + c);
  }
}

// S = X . W and gP = gT . W (K = 64) are idg::layer64::tile_times_w<2>: TWO chains of MFMAs take alternate groups of four
// K-steps and are added at the end.  The logits reach |S| ~ 100 in a trained model, where every rounding of a partial sum is
// a relative error of 4e-6 in exp(S - max) — chains half as long keep the kernels at the distance from float64 of a float32
// GEMM (and the two chains issue back to back).
constexpr int SCH = 2;

// The same over K = 128, for P . W^T and gS . W^T: A row of an LDS tile at pa, lane half h takes K-values 64 h ... 64 h + 63
__device__ __forceinline__ f32x16 mfma_k128(const float* __restrict__ pa, const float (&wr)[64]) {
  f32x16 acc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = 0.f, acc[1][r] = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float4 x = *reinterpret_cast<const float4*>(pa + 4 * q);
    const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[q & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[c], wr[4 * q + c], acc[q & 1], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] += acc[1][r];
  return acc[0];
}

// Persistent 256-thread workgroups: tile b, b + grid, ... of 64 rows.  Wave w forms columns 32 w ... of S for all 64 rows
// (two accumulators), the softmax runs four lanes to a row out of LDS, then wave w forms the 32 x 32 tile (w >> 1, w & 1) of
// T, which leaves — with F — coalesced through LDS.
__global__ __launch_bounds__(FWD_BLOCK, 2) void intent_fwd_kernel(const float* __restrict__ X, int64_t ldx, int64_t row0, int64_t nrows,
                                                                const float* __restrict__ W, const uint32_t* __restrict__ bits,
                                                                const float* __restrict__ noise, uint64_t seed, uint64_t stream,
                                                                float* __restrict__ T, int64_t ldt, float* __restrict__ F, int64_t ldf,
                                                                float* __restrict__ noise_out) {
  __shared__ __attribute__((aligned(16))) float s_x[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_p[RB * LDP];  // S, then P, then (stride LDT) the tile of T
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = w >> 1, ct = w & 1;
  f32x16 wa[2];  // W[32 h + s, 32 w + i]
  float wb[64];  // W[32 ct + i, 64 h + s]
  idg::layer64::load_w_col(W, K, 32 * w + i, h, wa[0], wa[1]);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float4 u = *reinterpret_cast<const float4*>(W + (32 * ct + i) * K + 64 * h + 4 * q);
    wb[4 * q + 0] = u.x, wb[4 * q + 1] = u.y, wb[4 * q + 2] = u.z, wb[4 * q + 3] = u.w;
  }
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * RB;  // first row of the tile, counted from row0
    // ---- which of this thread's four (row, 4 features) pieces are live; a tile with no flagged row is skipped
    bool live[4];
    int any = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rr = (tid + FWD_BLOCK * j) >> 4;
      live[j] = t0 + rr < nrows && (!bits || idg::bit_at(bits, row0 + t0 + rr));
      any |= live[j];
    }
    if (!__syncthreads_or(any)) continue;  // (also: the tile buffers of the previous tile are free)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + FWD_BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live[j]) v = *reinterpret_cast<const float4*>(X + (row0 + t0 + rr) * ldx + c4);
      *reinterpret_cast<float4*>(s_x + rr * LDT + c4) = v;
    }
    __syncthreads();
    // ---- S = X . W: columns 32 w + i, rows of both row tiles
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const f32x16 acc = idg::layer64::tile_times_w<SCH>(s_x, t, i, h, wa[0], wa[1]);
#pragma unroll
      for (int r = 0; r < 16; ++r) s_p[(32 * t + idg::mfma_c_row(r, h)) * LDP + 32 * w + i] = acc[r];
    }
    __syncthreads();
    // ---- P = softmax(S) in place: four lanes to a row, lane q the columns q, q + 4, ...
    {
      const int rr = tid >> 2, q = tid & 3;
      float* ps = s_p + rr * LDP + q;
      float v[32];
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < 32; ++j) v[j] = ps[4 * j], m = fmaxf(m, v[j]);
      m = fmaxf(m, __shfl_xor(m, 1, 64));
      m = fmaxf(m, __shfl_xor(m, 2, 64));
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) v[j] = expf(v[j] - m), sum += v[j];
      sum = idg::lanes_sum<4>(sum);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int j = 0; j < 32; ++j) ps[4 * j] = v[j] * inv;
    }
    __syncthreads();
    // ---- T = P . W^T: the wave's 32 x 32 tile
    const f32x16 acc = mfma_k128(s_p + (32 * rt + i) * LDP + 64 * h, wb);
    __syncthreads();  // every operand has left P: its space becomes the tile of T
#pragma unroll
    for (int r = 0; r < 16; ++r) s_p[(32 * rt + idg::mfma_c_row(r, h)) * LDT + 32 * ct + i] = acc[r];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + FWD_BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
      if (live[j]) {
        const int64_t row = row0 + t0 + rr;
        const float4 x = *reinterpret_cast<const float4*>(s_x + rr * LDT + c4);
        const float4 t = *reinterpret_cast<const float4*>(s_p + rr * LDT + c4);
        float z[4];
        noise4(noise, seed, stream, row, c4, z);
        *reinterpret_cast<float4*>(T + row * ldt + c4) = t;
        *reinterpret_cast<float4*>(F + row * ldf + c4) = make_float4(x.x + t.x * z[0], x.y + t.y * z[1], x.z + t.z * z[2], x.w + t.w * z[3]);
        if (noise_out) *reinterpret_cast<float4*>(noise_out + row * D + c4) = make_float4(z[0], z[1], z[2], z[3]);
      }
    }
    // (the next tile's first barrier, the __syncthreads_or, frees s_x and s_p)
  }
}

// Persistent 512-thread workgroups.  Wave w8 forms the 32 x 32 tile (w8 >> 2, w8 & 3) of S and of gP (one W operand for
// both); the softmax and gS run eight lanes to a row out of LDS; waves 0-3 then form gX (one 32 x 32 tile each) and all
// eight waves add the tile's share of gW (features 32 (w8 >> 2) ... x intent columns 32 (w8 & 3) ...) to an accumulator
// that lives in their registers across the tiles.
__global__ __launch_bounds__(BWD_BLOCK, 1) void intent_bwd_kernel(const float* __restrict__ gF, int64_t ldgf, const float* __restrict__ gTin,
                                                                int64_t ldgt, const uint32_t* __restrict__ gt_bits,
                                                                const uint32_t* __restrict__ bits,
                                                                const float* __restrict__ X, int64_t ldx, int64_t row0, int64_t nrows,
                                                                const float* __restrict__ W, const float* __restrict__ noise,
                                                                uint64_t seed, uint64_t stream, float* __restrict__ gX, int64_t ldgx,
                                                                float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_x[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_gt[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_p[RB * LDP];   // S, then P
  __shared__ __attribute__((aligned(16))) float s_gp[RB * LDP];  // gP, then gS
  __shared__ int s_live[RB];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = w8 >> 2, c4t = w8 & 3;  // S, gP: rows 32 rt ..., columns 32 c4t ...; gW: features 32 rt ... x columns 32 c4t ...
  const int xrt = (w8 >> 1) & 1, xct = w8 & 1;  // gX (waves 0-3): rows 32 xrt ..., features 32 xct ...
  f32x16 wa[2];
  float wb[64];
  idg::layer64::load_w_col(W, K, 32 * c4t + i, h, wa[0], wa[1]);
  if (w8 < 4) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 u = *reinterpret_cast<const float4*>(W + (32 * xct + i) * K + 64 * h + 4 * q);
      wb[4 * q + 0] = u.x, wb[4 * q + 1] = u.y, wb[4 * q + 2] = u.z, wb[4 * q + 3] = u.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 64; ++s) wb[s] = 0.f;
  }
  f32x16 gw;
#pragma unroll
  for (int r = 0; r < 16; ++r) gw[r] = 0.f;
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * RB;
    bool live[2];
    int any = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rr = (tid + BWD_BLOCK * j) >> 4;
      live[j] = t0 + rr < nrows && (!bits || idg::bit_at(bits, row0 + t0 + rr));
      any |= live[j];
    }
    if (!__syncthreads_or(any)) continue;  // (also: the tile buffers of the previous tile are free)
    // ---- stage X and gT = gT_in + gF o Z; rows that are not live are zero in both (they add nothing to gW)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = tid + BWD_BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f), g = x;
      if (live[j]) {
        const int64_t row = row0 + t0 + rr;
        x = *reinterpret_cast<const float4*>(X + row * ldx + c4);
        const float4 f = *reinterpret_cast<const float4*>(gF + row * ldgf + c4);
        float z[4];
        noise4(noise, seed, stream, row, c4, z);
        g = make_float4(f.x * z[0], f.y * z[1], f.z * z[2], f.w * z[3]);
        if (gTin && (!gt_bits || idg::bit_at(gt_bits, row))) {
          const float4 u = *reinterpret_cast<const float4*>(gTin + row * ldgt + c4);
          g.x = u.x + g.x, g.y = u.y + g.y, g.z = u.z + g.z, g.w = u.w + g.w;
        }
      }
      *reinterpret_cast<float4*>(s_x + rr * LDT + c4) = x;
      *reinterpret_cast<float4*>(s_gt + rr * LDT + c4) = g;
      if (c4 == 0) s_live[rr] = live[j];
    }
    __syncthreads();
    // ---- S = X . W and gP = gT . W: the wave's 32 x 32 tile of each
    {
      f32x16 acc = idg::layer64::tile_times_w<SCH>(s_x, rt, i, h, wa[0], wa[1]);
#pragma unroll
      for (int r = 0; r < 16; ++r) s_p[(32 * rt + idg::mfma_c_row(r, h)) * LDP + 32 * c4t + i] = acc[r];
      acc = idg::layer64::tile_times_w<SCH>(s_gt, rt, i, h, wa[0], wa[1]);
#pragma unroll
      for (int r = 0; r < 16; ++r) s_gp[(32 * rt + idg::mfma_c_row(r, h)) * LDP + 32 * c4t + i] = acc[r];
    }
    __syncthreads();
    // ---- P = softmax(S), gS = P o (gP - rowsum(P o gP)), both in place: eight lanes to a row, lane q the columns q, q + 8, ...
    {
      const int rr = tid >> 3, q = tid & 7;
      float* ps = s_p + rr * LDP + q;
      float* pg = s_gp + rr * LDP + q;
      float v[16], g[16];
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = ps[8 * j], g[j] = pg[8 * j], m = fmaxf(m, v[j]);
      m = fmaxf(m, __shfl_xor(m, 1, 64));
      m = fmaxf(m, __shfl_xor(m, 2, 64));
      m = fmaxf(m, __shfl_xor(m, 4, 64));
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = expf(v[j] - m), sum += v[j];
      sum = idg::lanes_sum<8>(sum);
      const float inv = 1.0f / sum;
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] *= inv, dot += v[j] * g[j];
      dot = idg::lanes_sum<8>(dot);
#pragma unroll
      for (int j = 0; j < 16; ++j) ps[8 * j] = v[j], pg[8 * j] = v[j] * (g[j] - dot);
    }
    __syncthreads();
    if (w8 < 4) {
      // ---- gX = gF + gS . W^T at the live rows (a register's 32 lanes of one row: one 128-byte line)
      const f32x16 acc = mfma_k128(s_gp + (32 * xrt + i) * LDP + 64 * h, wb);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = 32 * xrt + idg::mfma_c_row(r, h);
        if (s_live[rr]) {
          const int64_t row = row0 + t0 + rr;
          gX[row * ldgx + 32 * xct + i] = gF[row * ldgf + 32 * xct + i] + acc[r];
        }
      }
    }
    // ---- gW += X^T . gS + gT^T . P.  K runs over the tile's rows: step s takes rows 2 s + h
#pragma unroll 8
    for (int s = 0; s < 32; ++s) {
      const int rr = 2 * s + h;
      gw = __builtin_amdgcn_mfma_f32_32x32x2f32(s_x[rr * LDT + 32 * rt + i], s_gp[rr * LDP + 32 * c4t + i], gw, 0, 0, 0);
      gw = __builtin_amdgcn_mfma_f32_32x32x2f32(s_gt[rr * LDT + 32 * rt + i], s_p[rr * LDP + 32 * c4t + i], gw, 0, 0, 0);
    }
    // (the next tile's first barrier, the __syncthreads_or, frees the tiles)
  }
  // this workgroup's slice of gW [d, k]
  float* out = part + (int64_t)blockIdx.x * WCOUNT;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[(32 * rt + idg::mfma_c_row(r, h)) * K + 32 * c4t + i] = gw[r];
}

// Z[row, f] for rows row0 .. row0 + nrows - 1 of a contiguous [., d] panel (any d): four features per thread
__global__ __launch_bounds__(256) void intent_noise_kernel(int64_t row0, int64_t nrows, int64_t d, uint64_t seed, uint64_t stream,
                                                           float* __restrict__ out) {
  const int64_t q = (d + 3) / 4, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nrows * q) return;
  const int64_t row = row0 + e / q, f0 = 4 * (e % q);
  for (int64_t f = f0; f < f0 + 4 && f < d; ++f) out[row * d + f] = idg::normal_of(seed, stream, row, f);
}

using idg::Span;

// the bytes a call touches of a panel indexed by the global row: rows row0 .. row0 + nrows - 1, d floats of each
Span span(const float* base, int64_t row0, int64_t nrows, int64_t ld) {
  if (!base) return {nullptr, 0};
  return {base + row0 * ld, idg::extent(nrows, D, ld)};
}

Span bits_span(const uint32_t* bits, int64_t row0, int64_t nrows) {
  if (!bits) return {nullptr, 0};
  const int64_t w0 = row0 / 32, w1 = (row0 + nrows - 1) / 32;
  return {bits + w0, (size_t)(w1 - w0 + 1) * sizeof(uint32_t)};
}

bool bad_ld(int64_t ld) { return ld < D || ld % 4 != 0 || ld >= (1 << 20); }

}  // namespace

extern "C" {

int idg_intent_fwd_f32(const float* X, int64_t ldx, int64_t row0, int64_t nrows, const float* W, int64_t d, int64_t k,
                       const uint32_t* rows_bitmap, const float* noise, uint64_t seed, uint64_t stream_id, float* T, int64_t ldt, float* F,
                       int64_t ldf, float* noise_out, void* stream) {
  IDG_REQUIRE(X && W && T && F, "idg_intent_fwd_f32: NULL argument");
  IDG_REQUIRE(d == D && k == K, "idg_intent_fwd_f32: (d, k) = (64, 128) only (got (%lld, %lld)); other widths: dense products and a softmax",
              (long long)d, (long long)k);
  IDG_REQUIRE(nrows >= 1 && row0 >= 0 && row0 + nrows < ((int64_t)1 << 31), "idg_intent_fwd_f32: bad sizes (row0 = %lld, nrows = %lld)",
              (long long)row0, (long long)nrows);
  IDG_REQUIRE(!bad_ld(ldx) && !bad_ld(ldt) && !bad_ld(ldf),
              "idg_intent_fwd_f32: bad leading dimension (ldx = %lld, ldt = %lld, ldf = %lld: >= d, a multiple of 4, below 2^20)",
              (long long)ldx, (long long)ldt, (long long)ldf);
  IDG_REQUIRE(((uintptr_t)X | (uintptr_t)W | (uintptr_t)noise | (uintptr_t)T | (uintptr_t)F | (uintptr_t)noise_out) % 16 == 0 &&
                  (uintptr_t)rows_bitmap % 4 == 0,
              "idg_intent_fwd_f32: misaligned argument (panels and W 16 bytes, rows_bitmap 4 bytes)");
  const Span outs[3] = {span(T, row0, nrows, ldt), span(F, row0, nrows, ldf), span(noise_out, row0, nrows, D)};
  const Span ins[4] = {span(X, row0, nrows, ldx), {W, sizeof(float) * WCOUNT}, bits_span(rows_bitmap, row0, nrows), span(noise, row0, nrows, D)};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 3, ins, 4), "idg_intent_fwd_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 3), "idg_intent_fwd_f32: two outputs overlap");
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  const int64_t wgs = n_tiles < FWD_WGS ? n_tiles : FWD_WGS;
  hipLaunchKernelGGL(intent_fwd_kernel, dim3((unsigned)wgs), dim3(FWD_BLOCK), 0, (hipStream_t)stream, X, ldx, row0, nrows, W, rows_bitmap,
                     noise, seed, stream_id, T, ldt, F, ldf, noise_out);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int idg_intent_noise_f32(int64_t row0, int64_t nrows, int64_t d, uint64_t seed, uint64_t stream_id, float* noise_out, void* stream) {
  IDG_REQUIRE(noise_out, "idg_intent_noise_f32: NULL argument");
  IDG_REQUIRE(nrows >= 1 && row0 >= 0 && row0 + nrows < ((int64_t)1 << 31) && d >= 1 && d < (1 << 20),
              "idg_intent_noise_f32: bad sizes (row0 = %lld, nrows = %lld, d = %lld)", (long long)row0, (long long)nrows, (long long)d);
  const int64_t work = nrows * ((d + 3) / 4);
  hipLaunchKernelGGL(intent_noise_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, row0, nrows, d, seed,
                     stream_id, noise_out);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

size_t idg_intent_bwd_workspace_bytes(int64_t d, int64_t k) {
  if (d != D || k != K) return 0;
  return (size_t)BWD_WGS * (size_t)WCOUNT * sizeof(float);
}

int idg_intent_bwd_f32(const float* gF, int64_t ldgf, const float* gT_in, int64_t ldgt, const uint32_t* gt_rows,
                       const uint32_t* rows_bitmap, const float* X,
                       int64_t ldx, int64_t row0, int64_t nrows, const float* W, int64_t d, int64_t k, const float* noise, uint64_t seed,
                       uint64_t stream_id, float* gX, int64_t ldgx, float* gW, void* ws, void* stream) {
  IDG_REQUIRE(gF && X && W && gX && gW && ws, "idg_intent_bwd_f32: NULL argument");
  IDG_REQUIRE(d == D && k == K, "idg_intent_bwd_f32: (d, k) = (64, 128) only (got (%lld, %lld)); other widths: dense products and a softmax",
              (long long)d, (long long)k);
  IDG_REQUIRE(nrows >= 1 && row0 >= 0 && row0 + nrows < ((int64_t)1 << 31), "idg_intent_bwd_f32: bad sizes (row0 = %lld, nrows = %lld)",
              (long long)row0, (long long)nrows);
  IDG_REQUIRE(!bad_ld(ldgf) && !bad_ld(ldx) && !bad_ld(ldgx) && (!gT_in || !bad_ld(ldgt)),
              "idg_intent_bwd_f32: bad leading dimension (ldgf = %lld, ldgt = %lld, ldx = %lld, ldgx = %lld: >= d, a multiple of 4, below 2^20)",
              (long long)ldgf, (long long)ldgt, (long long)ldx, (long long)ldgx);
  IDG_REQUIRE(((uintptr_t)gF | (uintptr_t)gT_in | (uintptr_t)X | (uintptr_t)W | (uintptr_t)noise | (uintptr_t)gX) % 16 == 0 &&
                  ((uintptr_t)rows_bitmap | (uintptr_t)gt_rows | (uintptr_t)gW | (uintptr_t)ws) % 4 == 0,
              "idg_intent_bwd_f32: misaligned argument (panels and W 16 bytes, the bitmaps, gW and ws 4 bytes)");
  const size_t wsb = idg_intent_bwd_workspace_bytes(d, k);
  const Span outs[3] = {span(gX, row0, nrows, ldgx), {gW, sizeof(float) * WCOUNT}, {ws, wsb}};
  const Span ins[7] = {span(gF, row0, nrows, ldgf), span(gT_in, row0, nrows, ldgt), bits_span(rows_bitmap, row0, nrows),
                       span(X, row0, nrows, ldx),   {W, sizeof(float) * WCOUNT},    span(noise, row0, nrows, D),
                       bits_span(gT_in ? gt_rows : nullptr, row0, nrows)};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 3, ins, 7), "idg_intent_bwd_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 3), "idg_intent_bwd_f32: two outputs overlap");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  const int64_t wgs = n_tiles < BWD_WGS ? n_tiles : BWD_WGS;
  float* part = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(intent_bwd_kernel, dim3((unsigned)wgs), dim3(BWD_BLOCK), 0, st, gF, ldgf, gT_in, ldgt, gt_rows, rows_bitmap, X, ldx, row0, nrows,
                     W, noise, seed, stream_id, gX, ldgx, part);
  return idg::slices_reduce(part, wgs, WCOUNT, gW, false, stream);
}

}  // extern "C"
