// The 64-row tile of the d = 64 layer kernels (idg_ngcf.hip, idg_gccf.hip, idg_gcmc.hip, idg_intent.hip, idg_group.hip): its
// LDS layout, the coalesced staging of a panel into it, the two register forms of a weight operand and the tile x weight
// product on v_mfma_f32_32x32x2_f32.  For .hip files only.  The operand order of the product is part of the bit pattern of
// every result behind it — and a backward kernel that recomputes a forward product must get the forward's bits — so it is
// written once, here.
#pragma once
#include <cstdint>

#include "idg_device.h"

namespace idg {
namespace layer64 {

constexpr int RB = 64;   // rows of a workgroup's tile
// LDS row stride of a [64, 64] tile, in floats.  Rows stay 16-byte aligned, and the MFMA row operand (lane i reads a float4
// of row 32 rt + i) is free of bank conflicts: row r starts at bank 68 r mod 64 = 4 r, so the b128 reads of 16 consecutive
// rows hit sixteen distinct groups of four banks, all 64 banks once.  (A stride of 64 puts all 16 rows on the same four.)
constexpr int LDT = 68;

// Rows r0 .. r0 + 63 of a contiguous [n, 64] panel into a tile, by THREADS threads: 16 lanes x 16 bytes per row, coalesced.
// Rows past the end read row n - 1 (the caller does not write them).
template <int THREADS>
__device__ __forceinline__ void stage_panel(float* __restrict__ s_t, const float* __restrict__ P, int64_t n, int64_t r0, int tid) {
#pragma unroll
  for (int j = 0; j < RB * 16 / THREADS; ++j) {
    const int e = tid + THREADS * j, rr = e >> 4, c4 = (e & 15) * 4;
    const int64_t row = r0 + rr < n ? r0 + rr : n - 1;
    *reinterpret_cast<float4*>(s_t + rr * LDT + c4) = *reinterpret_cast<const float4*>(P + row * 64 + c4);
  }
}

// A lane's 32 values of a weight operand, in (w0, w1): step s of the product below takes register s.
// Column form, the B operand of X . W: W[32 h + s, col] of a row-major W with leading dimension ld (32 strided loads).
__device__ __forceinline__ void load_w_col(const float* __restrict__ W, int ld, int col, int h, f32x16& w0, f32x16& w1) {
#pragma unroll
  for (int s = 0; s < 32; ++s) (s < 16 ? w0 : w1)[s & 15] = W[(32 * h + s) * ld + col];
}

// Row form, the B operand of G . W^T (or of X . V^T for a V in nn.Linear's [out, in] layout): W[row, 32 h + s], 8 float4.
__device__ __forceinline__ void load_w_row(const float* __restrict__ W, int ld, int row, int h, f32x16& w0, f32x16& w1) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 u = *reinterpret_cast<const float4*>(W + row * ld + 32 * h + 4 * q);
    f32x16& w = q < 4 ? w0 : w1;
    w[4 * (q & 3) + 0] = u.x, w[4 * (q & 3) + 1] = u.y, w[4 * (q & 3) + 2] = u.z, w[4 * (q & 3) + 3] = u.w;
  }
}

// (rows 32 rt ... of the tile) . (the 32 weight values per lane in w0, w1): K-values 32 h + s at step s, summed as NCH
// independent chains of MFMAs (chain q % NCH takes the float4 groups q) that are added pairwise at the end — a shorter
// dependent chain for the matrix core and a shorter sequential float32 sum: a chain of 32 steps carries the rounding of 32
// partial sums, NCH chains of 32 / NCH steps and log2(NCH) additions carry that many.  A product that two kernels must form
// alike (a forward's and its backward's recomputation) uses ONE value of NCH: same operands, same order, same bits.
template <int NCH>
__device__ __forceinline__ f32x16 tile_times_w(const float* __restrict__ s_t, int rt, int i, int h, const f32x16& w0, const f32x16& w1) {
  f32x16 acc[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
  const float* ps = s_t + (32 * rt + i) * LDT + 32 * h;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 x = *reinterpret_cast<const float4*>(ps + 4 * q);
    const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      acc[q % NCH] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[c], (q < 4 ? w0 : w1)[4 * (q & 3) + c], acc[q % NCH], 0, 0, 0);
  }
#pragma unroll
  for (int o = 1; o < NCH; o *= 2)
#pragma unroll
    for (int k = 0; k + o < NCH; k += 2 * o) acc[k] += acc[k + o];
  return acc[0];
}

}  // namespace layer64
}  // namespace idg
