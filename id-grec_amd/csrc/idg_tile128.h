// The 128 x 128 fp32 score tile S = X Y^T of a 256-thread workgroup on the matrix cores (idg_tnce.hip, idg_kmeans.hip):
// X and Y are 128 rows of 32 NDT floats each (row stride 32 NDT: padded operands, no bounds check on the loads), staged
// through LDS in 32-column chunks.  Wave w computes the 64 x 64 quarter (w >> 1, w & 1) as 2 x 2 MFMA blocks.  Every product
// is v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums, the features added in ascending order.
#pragma once
#include "idg_device.h"

namespace idg {
namespace tile128 {

constexpr int BLOCK = 256;
constexpr int T = 128;        // rows of an X / Y tile
constexpr int KC = 32;        // feature chunk of a score tile
constexpr int LK = KC + 4;    // its LDS row stride (floats): ds_read_b128 of 16 consecutive rows covers all 64 banks
constexpr int LG = T + 1;     // row stride of the 128 x 128 tile the caller writes from the scores: 32 rows of one column, or
                              // 32 columns of one row, on 32 banks
constexpr int LDS_FLOATS = T * LG;  // that tile; the score operands (2 x 128 x LK) alias it: two workgroups per CU

// s[m][n] = block (m, n) of this wave's quarter.  s_x, s_y: [128][LK] each.  Ends behind a barrier: the caller may
// overwrite s_x and s_y at once.
template <int NDT>
__device__ __forceinline__ void score_tile_128(const float* X, const float* Y, float* s_x, float* s_y, f32x16 (&s)[2][2]) {
  constexpr int64_t dp = 32 * NDT;
  const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, i = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[m][n][r] = 0.f;
  // The chunk loop: unrolled in full up to 5 chunks (d <= 160), rolled above.  Stated, because left to itself the
  // compiler decides differently for this loop inlined from here than for the same loop written in a kernel (registers,
  // and barriers per tile, follow)
  constexpr int CHUNKS_UNROLLED = NDT <= 5 ? NDT : 1;
#pragma unroll CHUNKS_UNROLLED
  for (int kc = 0; kc < NDT; ++kc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + BLOCK * j, rr = e >> 3, c4 = (e & 7) * 4;
      *reinterpret_cast<float4*>(s_x + rr * LK + c4) = *reinterpret_cast<const float4*>(X + rr * dp + kc * KC + c4);
      *reinterpret_cast<float4*>(s_y + rr * LK + c4) = *reinterpret_cast<const float4*>(Y + rr * dp + kc * KC + c4);
    }
    __syncthreads();
    const float* pa = s_x + (64 * wr + i) * LK + 16 * h;
    const float* pb = s_y + (64 * wc + i) * LK + 16 * h;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 a0 = *reinterpret_cast<const float4*>(pa + 4 * c);
      const float4 a1 = *reinterpret_cast<const float4*>(pa + 32 * LK + 4 * c);
      const float4 b0 = *reinterpret_cast<const float4*>(pb + 4 * c);
      const float4 b1 = *reinterpret_cast<const float4*>(pb + 32 * LK + 4 * c);
#define IDG_TILE128_STEP(F)                                                           \
  s[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.F, b0.F, s[0][0], 0, 0, 0);       \
  s[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.F, b1.F, s[0][1], 0, 0, 0);       \
  s[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.F, b0.F, s[1][0], 0, 0, 0);       \
  s[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.F, b1.F, s[1][1], 0, 0, 0);
      IDG_TILE128_STEP(x) IDG_TILE128_STEP(y) IDG_TILE128_STEP(z) IDG_TILE128_STEP(w)
#undef IDG_TILE128_STEP
    }
    __syncthreads();
  }
}

}  // namespace tile128
}  // namespace idg
