// One LR-GCCF layer (Chen et al., AAAI'20: E_l = dropout(side . W + b), side = G . E_{l-1}) as ONE kernel per direction, d = 64.
//
// The layer is linear between the mask and the product: no bilinear term, no LeakyReLU, no row norm.  It is NOT an NGCF
// layer with parameters zeroed (idg_ngcf.hip would stage a second panel, issue twice the MFMAs and normalise rows that
// LR-GCCF concatenates as they are), and its backward needs no saved activation: the mask is a function of
// (seed, stream, row, feature) (idg_dropout.h), so gT is formed from the upstream gradients alone.
//   forward : side -> E = keep * (side . W + b), written with leading dimension lde (its slot of the final panel)
//   backward: (gE, gN, side) -> gT = keep * (gE + gN at the flagged rows)   [never stored]
//             g_side = gT . W^T,  gW = side^T . gT,  gb = column sums of gT
// The shape is idg_ngcf.hip's: a workgroup owns 64 rows, the panel tile is read ONCE, coalesced, into LDS (idg_layer64.h:
// the tile, its staging and the tile x weight product); the MFMA operands (v_mfma_f32_32x32x2_f32) come out of LDS, the
// weight operands out of registers.  Forward: one tile, 32 MFMAs per wave,
// the result leaves coalesced through the tile.  Backward: persistent 512-thread workgroups, two tiles (gT, side); waves
// 0-3 form g_side while waves 4-7 add the block's share of gW / gb to accumulators that live in their registers across
// the blocks.  The sums over rows run in a fixed order — slices of rows on the persistent workgroups, added in slice
// order by idg::slices_reduce (idg_common.h): two runs give the same bits, no float atomics.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   gccf_layer_fwd64_kernel  : 75 VGPRs, 0 AGPRs, 26 SGPRs, 17,408 bytes of LDS, scratch 0, occupancy 6 waves / SIMD
//   gccf_layer_bwd64_kernel  : 124 VGPRs, 0 AGPRs, 75 SGPRs, 34,816 bytes of LDS, scratch 0, occupancy 4 waves / SIMD
#include <hip/hip_runtime.h>

#include <cstdint>

#include "idg_common.h"
#include "idg_device.h"
#include "idg_dropout.h"
#include "idg_layer64.h"

namespace {

using idg::f32x16;
using idg::layer64::LDT;
using idg::layer64::RB;

constexpr int BLOCK = 256;
constexpr int D = 64;
constexpr int BWD_BLOCK = 512;
constexpr int BWD_WGS = 512;  // resident workgroups of the backward kernel (2 x 512 threads per CU) = most slices of its sums
constexpr int64_t WCOUNT = D * D + D;  // [gW | gb]

__global__ __launch_bounds__(BLOCK, 4) void gccf_layer_fwd64_kernel(const float* __restrict__ side, const float* __restrict__ W,
                                                                 const float* __restrict__ b, int64_t n, float p, uint64_t seed,
                                                                 uint64_t stream, float* __restrict__ E, int64_t lde) {
  __shared__ __attribute__((aligned(16))) float s_t[RB * LDT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 31, h = lane >> 5;
  const int rt = w >> 1, ct = w & 1;  // this wave's 32 x 32 tile of the 64 x 64 block
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  // the wave's 32 weights per lane (column 32 ct + i, K-values 32 h ...): issued first, in flight across the staging
  f32x16 wr[2];
  idg::layer64::load_w_col(W, D, 32 * ct + i, h, wr[0], wr[1]);
  idg::layer64::stage_panel<BLOCK>(s_t, side, n, r0, tid);
  __syncthreads();
  const f32x16 acc = idg::layer64::tile_times_w<1>(s_t, rt, i, h, wr[0], wr[1]);
  __syncthreads();  // every operand has left the tile: it becomes the tile of side . W + b
  {
    const int col = 32 * ct + i;
    const float bb = b[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) s_t[(32 * rt + idg::mfma_c_row(r, h)) * LDT + col] = acc[r] + bb;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = tid + BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
    if (r0 + rr < n) {
      float4 v = *reinterpret_cast<const float4*>(s_t + rr * LDT + c4);
      float kp[4];
      idg::keep_scale4(p, seed, stream, r0 + rr, c4, kp);
      v.x *= kp[0], v.y *= kp[1], v.z *= kp[2], v.w *= kp[3];
      *reinterpret_cast<float4*>(E + (r0 + rr) * lde + c4) = v;
    }
  }
}

// Persistent 512-thread workgroups: block b, b + grid, ... of 64 rows.  All eight waves stage the two tiles; then waves 0-3
// form g_side (one 32 x 32 tile of the 64 rows x 64 input features each) while waves 4-7 add the block's share of gW
// (features 32 mt ... x output columns 32 nt ...) and of gb to registers that live across the blocks.
__global__ __launch_bounds__(BWD_BLOCK, 4) void gccf_layer_bwd64_kernel(const float* __restrict__ gE, const float* __restrict__ gN,
                                                                     int64_t ldgn, const uint32_t* __restrict__ gn_rows,
                                                                     const float* __restrict__ side, const float* __restrict__ W,
                                                                     int64_t n, float p, uint64_t seed, uint64_t stream,
                                                                     float* __restrict__ gSide, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_g[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_side[RB * LDT];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: the role branches below are wave-uniform
  const bool input_role = w8 < 4;
  const int w = w8 & 3;
  const int rt = w >> 1, kt = w & 1;  // g_side: rows 32 rt ..., input features 32 kt ...
  const int mt = w >> 1, nt = w & 1;  // gW: features 32 mt ... x output columns 32 nt ...
  const int k1 = 32 * kt;
  // One set of 32 registers, two uses: input waves hold their W^T operand in it (the 32 weights of input feature k1 + i,
  // output columns 32 h ...), parameter waves their accumulator, R[0].
  f32x16 R[2];
  float cs = 0.f;
  if (input_role) {
    idg::layer64::load_w_row(W, D, k1 + i, h, R[0], R[1]);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) R[0][r] = 0.f, R[1][r] = 0.f;
  }
  const int64_t n_blocks = (n + RB - 1) / RB;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int64_t r0 = blk * RB;
    // ---- stage side and gT = keep * (gE + gN at the flagged rows); addresses as a block base + a 32-bit lane offset
    const float* side_b = side + r0 * D;
    const float* gE_b = gE ? gE + r0 * D : nullptr;
    const float* gN_b = gN ? gN + r0 * ldgn : nullptr;
    const int last = (int)(n - 1 - r0 < RB - 1 ? n - 1 - r0 : RB - 1);  // rows past the end read the last row (their gT is 0)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = tid + BWD_BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
      const bool live = rr <= last;
      const int rc = live ? rr : last;
      const int64_t row = r0 + rc;
      *reinterpret_cast<float4*>(s_side + rr * LDT + c4) = *reinterpret_cast<const float4*>(side_b + (rc * D + c4));
      const bool has_n = gN && (!gn_rows || idg::bit_at(gn_rows, row));
      float out[4] = {0.f, 0.f, 0.f, 0.f};
      if (live && (has_n || gE)) {  // (the 16 lanes of a row decide alike)
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (gE) {
          const float4 x = *reinterpret_cast<const float4*>(gE_b + (rc * D + c4));
          g[0] = x.x, g[1] = x.y, g[2] = x.z, g[3] = x.w;
        }
        if (has_n) {
          const float4 x = *reinterpret_cast<const float4*>(gN_b + (rc * (int)ldgn + c4));
          g[0] += x.x, g[1] += x.y, g[2] += x.z, g[3] += x.w;
        }
        float kp[4];
        idg::keep_scale4(p, seed, stream, row, c4, kp);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = g[c] * kp[c];
      }
      *reinterpret_cast<float4*>(s_g + rr * LDT + c4) = make_float4(out[0], out[1], out[2], out[3]);
    }
    __syncthreads();
    if (input_role) {
      // ---- g_side = gT . W^T
      const f32x16 acc = idg::layer64::tile_times_w<1>(s_g, rt, i, h, R[0], R[1]);
      float* gs_b = gSide + r0 * D;  // (a register's 32 lanes of one row: one 128-byte line)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = 32 * rt + idg::mfma_c_row(r, h);
        if (rr <= last) gs_b[rr * D + k1 + i] = acc[r];
      }
    } else {
      // ---- gW += side^T gT, gb += column sums of gT.  K runs over the tile's rows: step s takes rows 2 s + h (rows
      // past the end carry gT = 0)
#pragma unroll 8
      for (int s = 0; s < 32; ++s) {
        const int rr = 2 * s + h;
        const float sv = s_side[rr * LDT + 32 * mt + i], gv = s_g[rr * LDT + 32 * nt + i];
        R[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv, gv, R[0], 0, 0, 0);
        cs += gv;
      }
    }
    __syncthreads();  // the tiles are free for the next block
  }
  if (input_role) return;
  // this workgroup's slice of the sums, in the layout [gW | gb]
  float* out = part + (int64_t)blockIdx.x * WCOUNT;
#pragma unroll
  for (int r = 0; r < 16; ++r) out[(32 * mt + idg::mfma_c_row(r, h)) * D + 32 * nt + i] = R[0][r];
  cs += __shfl_xor(cs, 32, 64);
  if (mt == 0 && h == 0) out[D * D + 32 * nt + i] = cs;
}

}  // namespace

extern "C" {

int idg_gccf_layer_fwd_f32(const float* side, const float* W, const float* b, int64_t n, int64_t d, float p, uint64_t seed,
                           uint64_t stream_id, float* E, int64_t lde, void* stream) {
  IDG_REQUIRE(side && W && b && E, "idg_gccf_layer_fwd_f32: NULL argument");
  IDG_REQUIRE(d == D, "idg_gccf_layer_fwd_f32: d = 64 only (got %lld); other widths: a dense product and idg_ngcf_tail_ex_f32 with slope 1",
              (long long)d);
  IDG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "idg_gccf_layer_fwd_f32: bad sizes (n = %lld)", (long long)n);
  IDG_REQUIRE(lde >= d && lde % 4 == 0, "idg_gccf_layer_fwd_f32: bad leading dimension lde = %lld (>= d, a multiple of 4)",
              (long long)lde);
  IDG_REQUIRE(p >= 0.f && p < 1.f, "idg_gccf_layer_fwd_f32: drop probability p = %g outside [0, 1)", (double)p);
  IDG_REQUIRE(((uintptr_t)side | (uintptr_t)E) % 16 == 0 && ((uintptr_t)W | (uintptr_t)b) % 4 == 0,
              "idg_gccf_layer_fwd_f32: misaligned argument (panels 16 bytes, W and b 4 bytes)");
  const idg::Span out = {E, idg::extent(n, d, lde)}, ins[3] = {{side, idg::extent(n, d, d)}, {W, sizeof(float) * D * D}, {b, sizeof(float) * D}};
  IDG_REQUIRE(!idg::outputs_meet_inputs(&out, 1, ins, 3), "idg_gccf_layer_fwd_f32: E overlaps an input");
  hipLaunchKernelGGL(gccf_layer_fwd64_kernel, dim3((unsigned)((n + RB - 1) / RB)), dim3(BLOCK), 0, (hipStream_t)stream, side, W, b, n,
                     p, seed, stream_id, E, lde);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

size_t idg_gccf_layer_bwd_workspace_bytes(int64_t d) {
  if (d != D) return 0;
  return (size_t)BWD_WGS * (size_t)WCOUNT * sizeof(float);
}

int idg_gccf_layer_bwd_f32(const float* gE, const float* gN, int64_t ldgn, const uint32_t* gn_rows, const float* side, const float* W,
                           int64_t n, int64_t d, float p, uint64_t seed, uint64_t stream_id, float* g_side, float* w_grads, void* ws,
                           void* stream) {
  IDG_REQUIRE((gE || gN) && side && W && g_side && w_grads && ws,
              "idg_gccf_layer_bwd_f32: NULL argument (at least one of gE and gN must be given)");
  IDG_REQUIRE(d == D, "idg_gccf_layer_bwd_f32: d = 64 only (got %lld); other widths: idg_ngcf_tail_bwd_ex_f32 with slope 1, idg_linear_wgrad_f32 and a dense product", (long long)d);
  IDG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "idg_gccf_layer_bwd_f32: bad sizes (n = %lld)", (long long)n);
  IDG_REQUIRE(!gN || (ldgn >= d && ldgn % 4 == 0 && ldgn < (1 << 20)),
              "idg_gccf_layer_bwd_f32: bad leading dimension ldgn = %lld (>= d, a multiple of 4, below 2^20)", (long long)ldgn);
  IDG_REQUIRE(p >= 0.f && p < 1.f, "idg_gccf_layer_bwd_f32: drop probability p = %g outside [0, 1)", (double)p);
  IDG_REQUIRE(((uintptr_t)gE | (uintptr_t)gN | (uintptr_t)side | (uintptr_t)W | (uintptr_t)g_side) % 16 == 0 &&
                  ((uintptr_t)gn_rows | (uintptr_t)w_grads | (uintptr_t)ws) % 4 == 0,
              "idg_gccf_layer_bwd_f32: misaligned argument (panels and W 16 bytes, gn_rows, w_grads and ws 4 bytes)");
  const size_t panel = idg::extent(n, d, d), gnb = gN ? idg::extent(n, d, ldgn) : 0, wb = sizeof(float) * D * D;
  const size_t bits = (size_t)((n + 31) / 32) * sizeof(uint32_t), wg = sizeof(float) * WCOUNT;
  const size_t wsb = idg_gccf_layer_bwd_workspace_bytes(d);
  const idg::Span outs[3] = {{g_side, panel}, {w_grads, wg}, {ws, wsb}},
                  ins[5] = {{gE, panel}, {gN, gnb}, {gn_rows, bits}, {side, panel}, {W, wb}};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 3, ins, 5), "idg_gccf_layer_bwd_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 3), "idg_gccf_layer_bwd_f32: two outputs overlap");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_blocks = (n + RB - 1) / RB;
  // two resident workgroups on EVERY CU (a count in between leaves some CUs with one workgroup and some with two)
  const int64_t wgs = n_blocks < BWD_WGS ? n_blocks : BWD_WGS;
  float* part = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(gccf_layer_bwd64_kernel, dim3((unsigned)wgs), dim3(BWD_BLOCK), 0, st, gE, gN, ldgn, gn_rows, side, W, n, p, seed,
                     stream_id, g_side, part);
  return idg::slices_reduce(part, wgs, WCOUNT, w_grads, false, stream);
}

}  // extern "C"
