// HCCF's hypergraph layer (Xia et al., SIGIR'22; models/HCCF.py:56-74) on the rows of one side of the panel, d = h = 64, fp32:
//   Hb = E0 . W [n_s, h],  H = M o Hb / keep (M: a Bernoulli(keep) mask),  L = H^T . X [h, d],  Y = H . L [n_s, d]
// H is a tall-skinny [n_s, 64] panel that the reference forms anew in every layer; here it NEVER reaches global memory:
// every kernel restages the tile of E0, forms Hb = E0 . W on the matrix core (W in the waves' registers) and regenerates the
// mask — idg_dropout.h's function of (seed, stream, global row, hyper column), or a uint8 panel for fixtures.
//   latent : L  = sum over rows of H[r, :]^T . X[r, :]            (the backward calls it with gY for gL = H^T . gY)
//   expand : Y  = H . L,  next = side + Y,  total += next          (the layer's two element-wise passes ride in the epilogue)
//   bwd    : gX += H . gL,  gHb (+)= M o (gY . L^T + X . gL^T) / keep
//   close  : gE0 += gHb . W^T,  gW = E0^T . gHb
// The shape is idg_intent.hip's: persistent 256-thread workgroups over tiles of 64 rows (rows row0 + 64 t ...: the first row
// need not be tile-aligned; 512 threads in the backward), panels staged ONCE, coalesced (16 lanes x 16 bytes per row), into LDS at idg_layer64.h's row
// stride of 68 floats; rows past the end are staged as zeros and never written.  Wave w owns the 32 x 32 tile (w >> 1, w & 1)
// of every 64 x 64 result.  Hb goes through layer64::tile_times_w<NCH> with ONE NCH in all four kernels, and the mask is
// applied by one expression (Hb * k, k = 1 / keep or 0): the backward's H has the forward's bits.
//
// The sums over rows (L, gL, gW) take the tile's rows as the K dimension of v_mfma_f32_32x32x2_f32: step s takes rows
// 2 s + h.  Their A operand is a COLUMN walk of an LDS tile — lane i reads float 32 t + i of row 2 s + h: 32 consecutive
// banks per 32-lane half of a ds_read_b32, no conflict.  They run in a fixed order: row slices on the persistent workgroups
// (tile b, b + grid, ...), accumulators in registers across a workgroup's tiles, slices added in slice order by
// idg::slices_reduce: two runs give the same bits, no float atomics.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   hyper_latent_kernel : 132 VGPRs, 0 AGPRs, 60 SGPRs, 52,224 bytes of LDS, scratch 0, occupancy 3 waves / SIMD
//   hyper_expand_kernel : 196 VGPRs, 0 AGPRs, 74 SGPRs, 34,816 bytes of LDS, scratch 0, occupancy 2 waves / SIMD
//   hyper_bwd_kernel    : 226 VGPRs, 0 AGPRs, 76 SGPRs, 69,632 bytes of LDS, scratch 0, occupancy 2 waves / SIMD
//   hyper_close_kernel  : 148 VGPRs, 0 AGPRs, 42 SGPRs, 34,816 bytes of LDS, scratch 0, occupancy 3 waves / SIMD
// (The backward as ONE group of four waves holding all four of its weight operands spills 204 bytes per lane at two waves per
// SIMD: it is built as two groups of four waves, see there.)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idg_common.h"
#include "idg_device.h"
#include "idg_dropout.h"
#include "idg_layer64.h"

namespace {

using idg::f32x16;
using idg::layer64::LDT;  // LDS row stride of a [64, 64] tile, in floats
using idg::layer64::RB;

constexpr int D = 64;   // embedding width
constexpr int HY = 64;  // hyperedges
constexpr int BLOCK = 256;
constexpr int WGS = 512;  // resident workgroups of the latent, expand and close kernels (2 x 256 threads per CU) = most slices of L / gW
constexpr int BWD_BLOCK = 512;
constexpr int BWD_WGS = 256;  // resident workgroups of the backward kernel (1 x 512 threads per CU)
constexpr int64_t LCOUNT = HY * D;
constexpr int NCH = 2;  // chains of every tile x weight product (see idg_layer64.h); Hb = E0 . W is formed alike everywhere

struct Mask {
  const uint8_t* mask;  // [., h] indexed by the global row, or NULL: the generator
  float p;              // 1 - keep (<= 0: every element is kept)
  uint64_t seed, stream;
};

// the factors of hyper columns c4 .. c4 + 3 of one global row: 1 / keep where the element is kept, 0 where it is dropped
__device__ __forceinline__ void keep4(const Mask& m, int64_t row, int c4, float k[4]) {
  if (m.mask) {
    const uint32_t b = *reinterpret_cast<const uint32_t*>(m.mask + row * HY + c4);
    const float scale = m.p <= 0.f ? 1.0f : 1.0f / (1.0f - m.p);  // keep_of_bits' expression
#pragma unroll
    for (int c = 0; c < 4; ++c) k[c] = ((b >> (8 * c)) & 0xFFu) ? scale : 0.0f;
  } else {
    idg::keep_scale4(m.p, m.seed, m.stream, row, c4, k);
  }
}

// rows row0 + t0 ... of a panel into a tile; rows past the end (t0 + rr >= nrows) are zeros
template <int THREADS = BLOCK>
__device__ __forceinline__ void stage(float* __restrict__ s_t, const float* __restrict__ P, int64_t ld, int64_t row0, int64_t t0, int64_t nrows,
                                      int tid) {
#pragma unroll
  for (int j = 0; j < RB * 16 / THREADS; ++j) {
    const int e = tid + THREADS * j, rr = e >> 4, c4 = (e & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 + rr < nrows) v = *reinterpret_cast<const float4*>(P + (row0 + t0 + rr) * ld + c4);
    *reinterpret_cast<float4*>(s_t + rr * LDT + c4) = v;
  }
}

// the wave's 32 x 32 tile of a 64 x 64 result into an LDS tile
__device__ __forceinline__ void put_tile(float* __restrict__ s_t, const f32x16& acc, int rt, int ct, int i, int h) {
#pragma unroll
  for (int r = 0; r < 16; ++r) s_t[(32 * rt + idg::mfma_c_row(r, h)) * LDT + 32 * ct + i] = acc[r];
}

// s_h (Hb = E0 . W, behind a barrier) becomes H = M o Hb / keep for the tile at t0, by THREADS threads.  Ends behind a barrier.
// mask_out (nullable) receives the tile's mask.
template <int THREADS = BLOCK>
__device__ __forceinline__ void mask_tile(float* __restrict__ s_h, int tid, const Mask& m, int64_t row0, int64_t t0, int64_t nrows,
                                          uint8_t* __restrict__ mask_out) {
  if (m.mask || m.p > 0.f || mask_out) {
#pragma unroll
    for (int j = 0; j < RB * 16 / THREADS; ++j) {
      const int e = tid + THREADS * j, rr = e >> 4, c4 = (e & 15) * 4;
      if (t0 + rr < nrows) {
        const int64_t row = row0 + t0 + rr;
        float k[4];
        keep4(m, row, c4, k);
        float4 v = *reinterpret_cast<const float4*>(s_h + rr * LDT + c4);
        v.x *= k[0], v.y *= k[1], v.z *= k[2], v.w *= k[3];
        *reinterpret_cast<float4*>(s_h + rr * LDT + c4) = v;
        if (mask_out)
          *reinterpret_cast<uint32_t*>(mask_out + row * HY + c4) =
              (k[0] != 0.f ? 1u : 0u) | (k[1] != 0.f ? 1u << 8 : 0u) | (k[2] != 0.f ? 1u << 16 : 0u) | (k[3] != 0.f ? 1u << 24 : 0u);
      }
    }
    __syncthreads();
  }
}

// s_h = M o (s_e . W) / keep for the tile at t0 (s_e staged and behind a barrier; wa: W's column form), four waves.
__device__ __forceinline__ void form_h(float* __restrict__ s_h, const float* __restrict__ s_e, const f32x16& wa0, const f32x16& wa1, int rt,
                                       int ct, int i, int h, int tid, const Mask& m, int64_t row0, int64_t t0, int64_t nrows,
                                       uint8_t* __restrict__ mask_out) {
  put_tile(s_h, idg::layer64::tile_times_w<NCH>(s_e, rt, i, h, wa0, wa1), rt, ct, i, h);
  __syncthreads();
  mask_tile(s_h, tid, m, row0, t0, nrows, mask_out);
}

// acc += A^T . B over the tile's 64 rows: A's columns 32 rt ..., B's columns 32 ct ...; step s takes rows 2 s + h
__device__ __forceinline__ void rows_product(f32x16& acc, const float* __restrict__ s_a, const float* __restrict__ s_b, int rt, int ct, int i,
                                             int h) {
#pragma unroll 8
  for (int s = 0; s < 32; ++s) {
    const int rr = 2 * s + h;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_a[rr * LDT + 32 * rt + i], s_b[rr * LDT + 32 * ct + i], acc, 0, 0, 0);
  }
}

// (rows 32 rt ... of tile A) . a + (rows 32 rt ... of tile B) . b, K = 64 each in layer64::tile_times_w's operand order: one
// chain of MFMAs per product, issued alternately and added at the end (nothing re-forms this sum: its order is its own)
__device__ __forceinline__ f32x16 two_products(const float* __restrict__ s_a, const f32x16& a0, const f32x16& a1, const float* __restrict__ s_b,
                                               const f32x16& b0, const f32x16& b1, int rt, int i, int h) {
  f32x16 acc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = 0.f, acc[1][r] = 0.f;
  const float* pa = s_a + (32 * rt + i) * LDT + 32 * h;
  const float* pb = s_b + (32 * rt + i) * LDT + 32 * h;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 x = *reinterpret_cast<const float4*>(pa + 4 * q);
    const float4 y = *reinterpret_cast<const float4*>(pb + 4 * q);
    const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[c], (q < 4 ? a0 : a1)[4 * (q & 3) + c], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ys[c], (q < 4 ? b0 : b1)[4 * (q & 3) + c], acc[1], 0, 0, 0);
    }
  }
  acc[0] += acc[1];
  return acc[0];
}

// this workgroup's slice of a [64, 64] sum over rows
__device__ __forceinline__ void put_slice(float* __restrict__ part, const f32x16& acc, int rt, int ct, int i, int h) {
  float* out = part + (int64_t)blockIdx.x * LCOUNT;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[(32 * rt + idg::mfma_c_row(r, h)) * D + 32 * ct + i] = acc[r];
}

__global__ __launch_bounds__(BLOCK, 2) void hyper_latent_kernel(const float* __restrict__ E0, int64_t lde, const float* __restrict__ W,
                                                                const float* __restrict__ X, int64_t ldx, int64_t row0, int64_t nrows, Mask m,
                                                                uint8_t* __restrict__ mask_out, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_e[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_h[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_x[RB * LDT];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = w >> 1, ct = w & 1;
  f32x16 wa[2];  // W[32 h + s, 32 ct + i]
  idg::layer64::load_w_col(W, HY, 32 * ct + i, h, wa[0], wa[1]);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * RB;
    __syncthreads();  // the tiles of the previous round are free
    stage(s_e, E0, lde, row0, t0, nrows, tid);
    stage(s_x, X, ldx, row0, t0, nrows, tid);
    __syncthreads();
    form_h(s_h, s_e, wa[0], wa[1], rt, ct, i, h, tid, m, row0, t0, nrows, mask_out);
    rows_product(acc, s_h, s_x, rt, ct, i, h);  // L[hyper 32 rt ..., feature 32 ct ...]
  }
  put_slice(part, acc, rt, ct, i, h);
}

__global__ __launch_bounds__(BLOCK, 2) void hyper_expand_kernel(const float* __restrict__ E0, int64_t lde, const float* __restrict__ W,
                                                                const float* __restrict__ L, int64_t row0, int64_t nrows, Mask m,
                                                                float* __restrict__ Y, int64_t ldy, const float* __restrict__ side, int64_t lds,
                                                                float* __restrict__ next, int64_t ldn, float* __restrict__ total,
                                                                int64_t ldtot) {
  __shared__ __attribute__((aligned(16))) float s_e[RB * LDT];  // E0, then the tile of Y
  __shared__ __attribute__((aligned(16))) float s_h[RB * LDT];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = w >> 1, ct = w & 1;
  f32x16 wa[2], la[2];  // W[32 h + s, 32 ct + i], L[32 h + s, 32 ct + i]
  idg::layer64::load_w_col(W, HY, 32 * ct + i, h, wa[0], wa[1]);
  idg::layer64::load_w_col(L, D, 32 * ct + i, h, la[0], la[1]);
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * RB;
    __syncthreads();
    stage(s_e, E0, lde, row0, t0, nrows, tid);
    __syncthreads();
    form_h(s_h, s_e, wa[0], wa[1], rt, ct, i, h, tid, m, row0, t0, nrows, nullptr);
    // (every operand has left s_e behind form_h's barrier: its space becomes the tile of Y)
    put_tile(s_e, idg::layer64::tile_times_w<NCH>(s_h, rt, i, h, la[0], la[1]), rt, ct, i, h);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RB * 16 / BLOCK; ++j) {
      const int e = tid + BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
      if (t0 + rr < nrows) {
        const int64_t row = row0 + t0 + rr;
        float4 y = *reinterpret_cast<const float4*>(s_e + rr * LDT + c4);
        *reinterpret_cast<float4*>(Y + row * ldy + c4) = y;
        if (side) {
          const float4 s = *reinterpret_cast<const float4*>(side + row * lds + c4);
          y = make_float4(s.x + y.x, s.y + y.y, s.z + y.z, s.w + y.w);
          *reinterpret_cast<float4*>(next + row * ldn + c4) = y;
        }
        if (total) {
          float4* pt = reinterpret_cast<float4*>(total + row * ldtot + c4);
          const float4 t = *pt;
          *pt = make_float4(t.x + y.x, t.y + y.y, t.z + y.z, t.w + y.w);
        }
      }
    }
  }
}

// 512 threads, one workgroup per CU: the four weight operands of this kernel (W and gL by columns, L and gL by rows) are 128
// registers per lane in one wave and spill at two waves per SIMD, so two groups of four waves hold two each and work side by
// side — 64 MFMAs per tile either way.  Waves 0-3 form H (wave w its tile (w >> 1, w & 1)) and then gX += H . gL; waves 4-7
// form gH = gY . L^T + X . gL^T meanwhile and park it in E0's tile once H is done with that.
__global__ __launch_bounds__(BWD_BLOCK, 1) void hyper_bwd_kernel(const float* __restrict__ E0, int64_t lde, const float* __restrict__ W,
                                                                 const float* __restrict__ X, int64_t ldx, const float* __restrict__ gY,
                                                                 int64_t ldgy, const float* __restrict__ L, const float* __restrict__ gL,
                                                                 int64_t row0, int64_t nrows, Mask m, float* __restrict__ gX, int64_t ldgx,
                                                                 float* __restrict__ gHb, int64_t ldgh, int accumulate) {
  __shared__ __attribute__((aligned(16))) float s_e[RB * LDT];  // E0, then the tile of gH
  __shared__ __attribute__((aligned(16))) float s_h[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_x[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_g[RB * LDT];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = w8 >> 2, rt = (w8 >> 1) & 1, ct = w8 & 1;
  f32x16 wa[2], wb[2];
  if (grp == 0) {
    idg::layer64::load_w_col(W, HY, 32 * ct + i, h, wa[0], wa[1]);   // W[32 h + s, hyper 32 ct + i]: E0 . W
    idg::layer64::load_w_col(gL, D, 32 * ct + i, h, wb[0], wb[1]);   // gL[hyper 32 h + s, feature 32 ct + i]: H . gL
  } else {
    idg::layer64::load_w_row(L, D, 32 * ct + i, h, wa[0], wa[1]);    // L[hyper 32 ct + i, feature 32 h + s]: gY . L^T
    idg::layer64::load_w_row(gL, D, 32 * ct + i, h, wb[0], wb[1]);   // gL[hyper 32 ct + i, feature 32 h + s]: X . gL^T
  }
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * RB;
    __syncthreads();
    stage<BWD_BLOCK>(s_e, E0, lde, row0, t0, nrows, tid);
    stage<BWD_BLOCK>(s_x, X, ldx, row0, t0, nrows, tid);
    stage<BWD_BLOCK>(s_g, gY, ldgy, row0, t0, nrows, tid);
    __syncthreads();
    f32x16 gh;
    if (grp == 0)
      put_tile(s_h, idg::layer64::tile_times_w<NCH>(s_e, rt, i, h, wa[0], wa[1]), rt, ct, i, h);  // as form_h does
    else
      gh = two_products(s_g, wa[0], wa[1], s_x, wb[0], wb[1], rt, i, h);
    __syncthreads();
    mask_tile<BWD_BLOCK>(s_h, tid, m, row0, t0, nrows, nullptr);
    if (grp == 0) {
      // gX += H . gL (a register's 32 lanes of one row: one 128-byte line)
      const f32x16 acc = idg::layer64::tile_times_w<NCH>(s_h, rt, i, h, wb[0], wb[1]);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = 32 * rt + idg::mfma_c_row(r, h);
        if (t0 + rr < nrows) gX[(row0 + t0 + rr) * ldgx + 32 * ct + i] += acc[r];
      }
    } else {
      put_tile(s_e, gh, rt, ct, i, h);  // (E0's tile was last read before the barrier above)
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RB * 16 / BWD_BLOCK; ++j) {
      const int e = tid + BWD_BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
      if (t0 + rr < nrows) {
        const int64_t row = row0 + t0 + rr;
        float k[4];
        keep4(m, row, c4, k);
        float4 v = *reinterpret_cast<const float4*>(s_e + rr * LDT + c4);
        v.x *= k[0], v.y *= k[1], v.z *= k[2], v.w *= k[3];
        float4* pg = reinterpret_cast<float4*>(gHb + row * ldgh + c4);
        if (accumulate) {
          const float4 o = *pg;
          v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
        }
        *pg = v;
      }
    }
  }
}

__global__ __launch_bounds__(BLOCK, 2) void hyper_close_kernel(const float* __restrict__ E0, int64_t lde, const float* __restrict__ W,
                                                               const float* __restrict__ gHb, int64_t ldgh, int64_t row0, int64_t nrows,
                                                               float* __restrict__ gE0, int64_t ldge, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_e[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_g[RB * LDT];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = w >> 1, ct = w & 1;
  f32x16 wr[2];  // W[feature 32 ct + i, hyper 32 h + s]: gHb . W^T
  idg::layer64::load_w_row(W, HY, 32 * ct + i, h, wr[0], wr[1]);
  f32x16 gw;
#pragma unroll
  for (int r = 0; r < 16; ++r) gw[r] = 0.f;
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * RB;
    __syncthreads();
    stage(s_e, E0, lde, row0, t0, nrows, tid);
    stage(s_g, gHb, ldgh, row0, t0, nrows, tid);
    __syncthreads();
    const f32x16 acc = idg::layer64::tile_times_w<NCH>(s_g, rt, i, h, wr[0], wr[1]);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = 32 * rt + idg::mfma_c_row(r, h);
      if (t0 + rr < nrows) gE0[(row0 + t0 + rr) * ldge + 32 * ct + i] += acc[r];
    }
    rows_product(gw, s_e, s_g, rt, ct, i, h);  // gW[feature 32 rt ..., hyper 32 ct ...]
  }
  put_slice(part, gw, rt, ct, i, h);
}

using idg::Span;

// the bytes a call touches of a panel indexed by the global row: rows row0 .. row0 + nrows - 1, 64 floats of each
Span span(const float* base, int64_t row0, int64_t nrows, int64_t ld) {
  if (!base) return {nullptr, 0};
  return {base + row0 * ld, idg::extent(nrows, D, ld)};
}

Span mask_span(const uint8_t* mask, int64_t row0, int64_t nrows) {
  if (!mask) return {nullptr, 0};
  return {mask + row0 * HY, (size_t)nrows * HY};
}

bool bad_ld(int64_t ld) { return ld < D || ld % 4 != 0 || ld >= (1 << 20); }
bool bad_rows(int64_t row0, int64_t nrows) { return nrows < 1 || row0 < 0 || row0 + nrows >= ((int64_t)1 << 31); }
bool bad_keep(float keep) { return !(keep > 0.f); }

unsigned grid_of(int64_t nrows, int wgs = WGS) {
  const int64_t n_tiles = (nrows + RB - 1) / RB;
  return (unsigned)(n_tiles < wgs ? n_tiles : wgs);
}

Mask mask_of(const uint8_t* mask, float keep, uint64_t seed, uint64_t stream_id) { return {mask, keep >= 1.f ? 0.f : 1.0f - keep, seed, stream_id}; }

Span MAT(const void* p) { return {p, sizeof(float) * LCOUNT}; }  // a [64, 64] matrix

}  // namespace

#define HYPER_WIDTHS(name)                                                                                                        \
  IDG_REQUIRE(d == D && h == HY, name ": (d, h) = (64, 64) only (got (%lld, %lld)); other widths: dense products and a mask", \
              (long long)d, (long long)h)
#define HYPER_ROWS(name) \
  IDG_REQUIRE(!bad_rows(row0, nrows), name ": bad sizes (row0 = %lld, nrows = %lld)", (long long)row0, (long long)nrows)

extern "C" {

size_t idg_hyper_latent_workspace_bytes(int64_t d, int64_t h) {
  if (d != D || h != HY) return 0;
  return (size_t)WGS * (size_t)LCOUNT * sizeof(float);
}

size_t idg_hyper_close_workspace_bytes(int64_t d, int64_t h) { return idg_hyper_latent_workspace_bytes(d, h); }

int idg_hyper_latent_f32(const float* E0, int64_t lde, const float* W, int64_t d, int64_t h, const float* X, int64_t ldx, int64_t row0,
                         int64_t nrows, float keep, const uint8_t* mask, uint64_t seed, uint64_t stream_id, float* L, uint8_t* mask_out,
                         void* ws, void* stream) {
  IDG_REQUIRE(E0 && W && X && L && ws, "idg_hyper_latent_f32: NULL argument");
  HYPER_WIDTHS("idg_hyper_latent_f32");
  HYPER_ROWS("idg_hyper_latent_f32");
  IDG_REQUIRE(!bad_keep(keep), "idg_hyper_latent_f32: keep = %g is not positive", (double)keep);
  IDG_REQUIRE(!bad_ld(lde) && !bad_ld(ldx), "idg_hyper_latent_f32: bad leading dimension (lde = %lld, ldx = %lld: >= d, a multiple of 4, below 2^20)",
              (long long)lde, (long long)ldx);
  IDG_REQUIRE(((uintptr_t)E0 | (uintptr_t)W | (uintptr_t)X | (uintptr_t)L | (uintptr_t)ws) % 16 == 0 &&
                  ((uintptr_t)mask | (uintptr_t)mask_out) % 4 == 0,
              "idg_hyper_latent_f32: misaligned argument (panels, W, L and ws 16 bytes, the masks 4 bytes)");
  const Span outs[3] = {MAT(L), {ws, idg_hyper_latent_workspace_bytes(d, h)}, mask_span(mask_out, row0, nrows)};
  const Span ins[4] = {span(E0, row0, nrows, lde), MAT(W), span(X, row0, nrows, ldx), mask_span(mask, row0, nrows)};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 3, ins, 4), "idg_hyper_latent_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 3), "idg_hyper_latent_f32: two outputs overlap");
  const unsigned wgs = grid_of(nrows);
  float* part = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(hyper_latent_kernel, dim3(wgs), dim3(BLOCK), 0, (hipStream_t)stream, E0, lde, W, X, ldx, row0, nrows,
                     mask_of(mask, keep, seed, stream_id), mask_out, part);
  return idg::slices_reduce(part, wgs, LCOUNT, L, false, stream);
}

int idg_hyper_expand_f32(const float* E0, int64_t lde, const float* W, int64_t d, int64_t h, const float* L, int64_t row0, int64_t nrows,
                         float keep, const uint8_t* mask, uint64_t seed, uint64_t stream_id, float* Y, int64_t ldy, const float* side,
                         int64_t lds, float* next, int64_t ldn, float* total, int64_t ldtot, void* stream) {
  IDG_REQUIRE(E0 && W && L && Y, "idg_hyper_expand_f32: NULL argument");
  IDG_REQUIRE(!side == !next, "idg_hyper_expand_f32: side and next come together (next = side + Y)");
  HYPER_WIDTHS("idg_hyper_expand_f32");
  HYPER_ROWS("idg_hyper_expand_f32");
  IDG_REQUIRE(!bad_keep(keep), "idg_hyper_expand_f32: keep = %g is not positive", (double)keep);
  IDG_REQUIRE(!bad_ld(lde) && !bad_ld(ldy) && (!side || (!bad_ld(lds) && !bad_ld(ldn))) && (!total || !bad_ld(ldtot)),
              "idg_hyper_expand_f32: bad leading dimension (lde = %lld, ldy = %lld, lds = %lld, ldn = %lld, ldtot = %lld: >= d, a multiple "
              "of 4, below 2^20)",
              (long long)lde, (long long)ldy, (long long)lds, (long long)ldn, (long long)ldtot);
  IDG_REQUIRE(((uintptr_t)E0 | (uintptr_t)W | (uintptr_t)L | (uintptr_t)Y | (uintptr_t)side | (uintptr_t)next | (uintptr_t)total) % 16 == 0 &&
                  (uintptr_t)mask % 4 == 0,
              "idg_hyper_expand_f32: misaligned argument (panels, W and L 16 bytes, the mask 4 bytes)");
  const Span outs[3] = {span(Y, row0, nrows, ldy), span(next, row0, nrows, ldn), span(total, row0, nrows, ldtot)};
  const Span ins[5] = {span(E0, row0, nrows, lde), MAT(W), MAT(L), span(side, row0, nrows, lds), mask_span(mask, row0, nrows)};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 3, ins, 5), "idg_hyper_expand_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 3), "idg_hyper_expand_f32: two outputs overlap");
  hipLaunchKernelGGL(hyper_expand_kernel, dim3(grid_of(nrows)), dim3(BLOCK), 0, (hipStream_t)stream, E0, lde, W, L, row0, nrows,
                     mask_of(mask, keep, seed, stream_id), Y, ldy, side, lds, next, ldn, total, ldtot);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int idg_hyper_bwd_f32(const float* E0, int64_t lde, const float* W, int64_t d, int64_t h, const float* X, int64_t ldx, const float* gY,
                      int64_t ldgy, const float* L, const float* gL, int64_t row0, int64_t nrows, float keep, const uint8_t* mask,
                      uint64_t seed, uint64_t stream_id, float* gX, int64_t ldgx, float* gHb, int64_t ldgh, int accumulate, void* stream) {
  IDG_REQUIRE(E0 && W && X && gY && L && gL && gX && gHb, "idg_hyper_bwd_f32: NULL argument");
  HYPER_WIDTHS("idg_hyper_bwd_f32");
  HYPER_ROWS("idg_hyper_bwd_f32");
  IDG_REQUIRE(!bad_keep(keep), "idg_hyper_bwd_f32: keep = %g is not positive", (double)keep);
  IDG_REQUIRE(!bad_ld(lde) && !bad_ld(ldx) && !bad_ld(ldgy) && !bad_ld(ldgx) && !bad_ld(ldgh),
              "idg_hyper_bwd_f32: bad leading dimension (lde = %lld, ldx = %lld, ldgy = %lld, ldgx = %lld, ldgh = %lld: >= d, a multiple of "
              "4, below 2^20)",
              (long long)lde, (long long)ldx, (long long)ldgy, (long long)ldgx, (long long)ldgh);
  IDG_REQUIRE(((uintptr_t)E0 | (uintptr_t)W | (uintptr_t)X | (uintptr_t)gY | (uintptr_t)L | (uintptr_t)gL | (uintptr_t)gX | (uintptr_t)gHb) % 16 == 0 &&
                  (uintptr_t)mask % 4 == 0,
              "idg_hyper_bwd_f32: misaligned argument (panels, W, L and gL 16 bytes, the mask 4 bytes)");
  const Span outs[2] = {span(gX, row0, nrows, ldgx), span(gHb, row0, nrows, ldgh)};
  const Span ins[7] = {span(E0, row0, nrows, lde), MAT(W), span(X, row0, nrows, ldx), span(gY, row0, nrows, ldgy), MAT(L), MAT(gL),
                       mask_span(mask, row0, nrows)};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 2, ins, 7), "idg_hyper_bwd_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 2), "idg_hyper_bwd_f32: two outputs overlap");
  hipLaunchKernelGGL(hyper_bwd_kernel, dim3(grid_of(nrows, BWD_WGS)), dim3(BWD_BLOCK), 0, (hipStream_t)stream, E0, lde, W, X, ldx, gY, ldgy, L, gL, row0,
                     nrows, mask_of(mask, keep, seed, stream_id), gX, ldgx, gHb, ldgh, accumulate);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int idg_hyper_close_f32(const float* E0, int64_t lde, const float* W, int64_t d, int64_t h, const float* gHb, int64_t ldgh, int64_t row0,
                        int64_t nrows, float* gE0, int64_t ldge, float* gW, void* ws, void* stream) {
  IDG_REQUIRE(E0 && W && gHb && gE0 && gW && ws, "idg_hyper_close_f32: NULL argument");
  HYPER_WIDTHS("idg_hyper_close_f32");
  HYPER_ROWS("idg_hyper_close_f32");
  IDG_REQUIRE(!bad_ld(lde) && !bad_ld(ldgh) && !bad_ld(ldge),
              "idg_hyper_close_f32: bad leading dimension (lde = %lld, ldgh = %lld, ldge = %lld: >= d, a multiple of 4, below 2^20)",
              (long long)lde, (long long)ldgh, (long long)ldge);
  IDG_REQUIRE(((uintptr_t)E0 | (uintptr_t)W | (uintptr_t)gHb | (uintptr_t)gE0 | (uintptr_t)gW | (uintptr_t)ws) % 16 == 0,
              "idg_hyper_close_f32: misaligned argument (16 bytes)");
  const Span outs[3] = {span(gE0, row0, nrows, ldge), MAT(gW), {ws, idg_hyper_close_workspace_bytes(d, h)}};
  const Span ins[3] = {span(E0, row0, nrows, lde), MAT(W), span(gHb, row0, nrows, ldgh)};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 3, ins, 3), "idg_hyper_close_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 3), "idg_hyper_close_f32: two outputs overlap");
  const unsigned wgs = grid_of(nrows);
  float* part = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(hyper_close_kernel, dim3(wgs), dim3(BLOCK), 0, (hipStream_t)stream, E0, lde, W, gHb, ldgh, row0, nrows, gE0, ldge, part);
  return idg::slices_reduce(part, wgs, LCOUNT, gW, false, stream);
}

}  // extern "C"
