// Device-side helpers shared by the kernel files: the wave width, the lane-group and one-workgroup sums, and the register
// types and maps of v_mfma_f32_32x32x2_f32.  Includes the HIP runtime header, so only .hip files include it (the host
// .cpp files keep idg_common.h).  Every sum here has ONE fixed order: that order is part of the bit pattern of every
// result that passes through it, and changing it changes those bits.
#pragma once
#include <hip/hip_runtime.h>

namespace idg {

constexpr int WAVE = 64;

// Bit r of a row bitmap (32 rows to a word, row r at bit r & 31 of word r >> 5).
__device__ __forceinline__ bool bit_at(const uint32_t* __restrict__ bits, int64_t r) { return (bits[r >> 5] >> (r & 31)) & 1u; }

// The accumulator (C/D operand) of one 32 x 32 MFMA block: 16 registers per lane.
using f32x16 = __attribute__((ext_vector_type(16))) float;

// C/D map of v_mfma_f32_32x32x2_f32: register r of lane (i, h) = (lane & 31, lane >> 5) holds row
// (r & 3) + 8 (r >> 2) + 4 h, column i of the block.
__device__ __forceinline__ int mfma_c_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Sum over each aligned group of LPR lanes (a power of two <= 64), the result on every lane of the group: an xor
// butterfly with the offsets LPR / 2, ..., 2, 1 in that order.  No LDS, no atomics.
template <int LPR, typename V>
__device__ __forceinline__ V lanes_sum(V v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LPR);
  return v;
}

__device__ __forceinline__ float wave_sum(float v) { return lanes_sum<WAVE>(v); }
__device__ __forceinline__ double wave_sum(double v) { return lanes_sum<WAVE>(v); }

// Sum of one value per thread over a workgroup of N threads (a power of two) by a fixed tree through s[N]: leaf t is
// thread t's value, level by level s[t] += s[t + o] for o = N / 2, ..., 1.  Every thread must call it; the sum is returned
// on every thread.  s may be reused after the call only behind a barrier of the caller's.
template <int N, typename V>
__device__ __forceinline__ V block_tree_sum(V acc, V* s) {
  const int tid = threadIdx.x;
  s[tid] = acc;
  __syncthreads();
  for (int o = N / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  return s[0];
}

}  // namespace idg
