// One GCMC layer (reference: models/GCMC.py:73-90) as ONE kernel per direction, d = 64:
//   H = side . Wg + bg,  A = LeakyReLU(H),  M = A . Wm + bm,  T = keep * M (the next layer's input),  N = T / max(|T|, 1e-12)
// Two CHAINED 64 x 64 products with the nonlinearity between them and a row normalisation behind the mask: neither
// idg_gccf.hip's layer (one product, no activation) nor idg_ngcf.hip's (two parallel products summed before the activation).
// H and A never leave the chip: the forward keeps them in its LDS tile, the backward recomputes them from `side` with the
// forward's operand order — so the recomputed H has the forward's bits, and LeakyReLU' the forward's branch.
//   forward : side -> T [n, 64] contiguous, N with leading dimension ldn (its slot of the final panel)
//   backward: (T, gE, gN, side) -> N, den rebuilt from T;  gM = keep * (gE + J_normalize(T)^T gN at the flagged rows)
//             gA = gM . Wm^T,  gH = gA o LeakyReLU'(H),  g_side = gH . Wg^T
//             gWm = A^T . gM,  gbm = column sums of gM,  gWg = side^T . gH,  gbg = column sums of gH
//             (gM, H, A, gA, gH are never stored)
// The shape is idg_gccf.hip's: a workgroup owns 64 rows, a panel tile is read ONCE, coalesced, into LDS (idg_layer64.h: the
// tile, its staging and the tile x weight product); the MFMA operands (v_mfma_f32_32x32x2_f32) come out of LDS, the weight
// operands out of registers.  Forward: 256 threads, one tile used three
// times (side, A, M), 64 MFMAs per wave.  A product's 32 MFMA steps run as independent chains added pairwise at the end
// (tile_times_w: two chains for H, which the backward recomputes with the same instantiation, four for M, which only the
// forward forms): a single chain of 32 sequential float32 partial sums put T at n = 1, p = 0.9 at 8.4e-7 of its largest entry
// against 2.0e-7 for a float32 GEMV of the same expressions; the chains bring it to 3.0e-7, and the dependent MFMA chain is
// shorter.
//
// Backward: persistent 512-thread workgroups, four tiles (side, gM, A, gH), five 64 x 64 x 64 products per block of rows.
// How the eight waves split them — by which operands a wave must HOLD, not by MFMA count:
//   waves 0-3 ("input"):      H = side . Wg  and  g_side = gH . Wg^T     hold Wg as both operand forms (64 registers)
//   waves 4-7 ("parameter"):  gA = gM . Wm^T,  gWm += A^T . gM,  gWg += side^T . gH
//                             hold Wm^T (32 registers) and the two accumulators that live across the blocks (32 registers)
// Every wave then carries 64 registers of state next to one 16-register working accumulator and stays under the 128 registers
// of four waves per SIMD; giving gWm to the input waves (an even 80 / 80 MFMA split) would put 96 registers of state on them.
// The uneven count (64 vs 96 MFMAs) costs no matrix-core time: waves w and w + 4 share a SIMD, so each SIMD issues 40 MFMAs
// per block whatever the split.  Phases of a block (a barrier between them): stage side, gM | H -> A next to gA |
// gH = gA o LeakyReLU'(A) (the parameter waves hold gA in the accumulator layout of the tile of A they read) | g_side next to
// the two parameter products.  LeakyReLU' is read off A: A > 0 iff H > 0, and the slope applies where H <= 0.
// The sums over rows run in a fixed order — slices of rows on the persistent workgroups, added in slice order by
// idg::slices_reduce (idg_common.h): two runs give the same bits, no float atomics.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   gcmc_layer_fwd64_kernel  : 111 VGPRs, 0 AGPRs, 26 SGPRs, 17,408 bytes of LDS, scratch 0, occupancy 4 waves / SIMD
//   gcmc_layer_bwd64_kernel  : 128 VGPRs, 0 AGPRs, 90 SGPRs, 69,632 bytes of LDS, scratch 0, occupancy 4 waves / SIMD (two workgroups per CU: 139,264 of its 163,840 bytes of LDS)
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
using idg::layer64::tile_times_w;

constexpr int BLOCK = 256;
constexpr int D = 64;
constexpr int BWD_BLOCK = 512;
constexpr int BWD_WGS = 512;  // resident workgroups of the backward kernel (2 x 512 threads per CU) = most slices of its sums
constexpr int64_t WCOUNT = 2 * (D * D + D);  // [gWg | gbg | gWm | gbm]
constexpr int HCH = 2;  // MFMA chains of H = side . Wg (forward and the backward's recomputation: one value)
constexpr int MCH = 4;  // ... of M = A . Wm (forward only)

__device__ __forceinline__ float leaky(float t, float slope) { return t > 0.f ? t : t * slope; }

__global__ __launch_bounds__(BLOCK, 4) void gcmc_layer_fwd64_kernel(const float* __restrict__ side, const float* __restrict__ Wg,
                                                                 const float* __restrict__ bg, const float* __restrict__ Wm,
                                                                 const float* __restrict__ bm, int64_t n, float slope, float p,
                                                                 uint64_t seed, uint64_t stream, float* __restrict__ T,
                                                                 float* __restrict__ N, int64_t ldn) {
  __shared__ __attribute__((aligned(16))) float s_t[RB * LDT];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 31, h = lane >> 5;
  const int rt = w >> 1, ct = w & 1;  // this wave's 32 x 32 tile of the 64 x 64 block
  const int col = 32 * ct + i;
  const int64_t r0 = (int64_t)blockIdx.x * RB;
  // the wave's 32 weights per lane (column 32 ct + i, K-values 32 h ...): issued first, in flight across the staging
  f32x16 wr[2];
  idg::layer64::load_w_col(Wg, D, col, h, wr[0], wr[1]);
  idg::layer64::stage_panel<BLOCK>(s_t, side, n, r0, tid);
  __syncthreads();
  f32x16 acc = tile_times_w<HCH>(s_t, rt, i, h, wr[0], wr[1]);
  // the second product's weights: in flight across the barrier and the activation
  idg::layer64::load_w_col(Wm, D, col, h, wr[0], wr[1]);
  __syncthreads();  // every operand has left the tile: it becomes the tile of A = LeakyReLU(side . Wg + bg)
  {
    const float bb = bg[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) s_t[(32 * rt + idg::mfma_c_row(r, h)) * LDT + col] = leaky(acc[r] + bb, slope);
  }
  __syncthreads();
  acc = tile_times_w<MCH>(s_t, rt, i, h, wr[0], wr[1]);
  __syncthreads();  // ... and now the tile of M = A . Wm + bm
  {
    const float bb = bm[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) s_t[(32 * rt + idg::mfma_c_row(r, h)) * LDT + col] = acc[r] + bb;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = tid + BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
    float4 v = *reinterpret_cast<const float4*>(s_t + rr * LDT + c4);
    float kp[4];
    idg::keep_scale4(p, seed, stream, r0 + rr, c4, kp);
    v.x *= kp[0], v.y *= kp[1], v.z *= kp[2], v.w *= kp[3];
    float ss = 0.f;
    ss += v.x * v.x, ss += v.y * v.y, ss += v.z * v.z, ss += v.w * v.w;
    ss = idg::lanes_sum<16>(ss);  // (the 16 lanes of a row; every lane of the wave takes part)
    const float den = fmaxf(sqrtf(ss), 1e-12f);
    if (r0 + rr < n) {
      *reinterpret_cast<float4*>(T + (r0 + rr) * D + c4) = v;
      *reinterpret_cast<float4*>(N + (r0 + rr) * ldn + c4) = make_float4(v.x / den, v.y / den, v.z / den, v.w / den);
    }
  }
}

// Persistent 512-thread workgroups: block b, b + grid, ... of 64 rows; the roles and phases are the file header's.
__global__ __launch_bounds__(BWD_BLOCK, 4) void gcmc_layer_bwd64_kernel(
    const float* __restrict__ T, const float* __restrict__ gE, const float* __restrict__ gN, int64_t ldgn,
    const uint32_t* __restrict__ gn_rows, const float* __restrict__ side, const float* __restrict__ Wg, const float* __restrict__ bg,
    const float* __restrict__ Wm, int64_t n, float slope, float p, uint64_t seed, uint64_t stream, float* __restrict__ gSide,
    float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float s_side[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_gm[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_a[RB * LDT];
  __shared__ __attribute__((aligned(16))) float s_gh[RB * LDT];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: the role branches below are wave-uniform
  const bool input_role = w8 < 4;
  const int w = w8 & 3;
  const int rt = w >> 1, kt = w & 1;  // H, gA, gH, g_side: rows 32 rt ..., columns 32 kt ...
  const int mt = w >> 1, nt = w & 1;  // gWg, gWm: features 32 mt ... x output columns 32 nt ...
  const int k1 = 32 * kt;
  // One set of 64 registers, two uses (idg_ngcf.hip: the compiler keeps two variables that are live across the block loop
  // apart even when no wave uses both).  R[0..1]: the W^T operand (the 32 weights of input feature k1 + i, output columns
  // 32 h ...) of Wg on the input waves, of Wm on the parameter waves.  R[2..3]: on the input waves the forward's operand of
  // Wg (column k1 + i, K-values 32 h ...), on the parameter waves the accumulators of gWg and gWm.
  f32x16 R[4];
  float cs_g = 0.f, cs_m = 0.f, bb = 0.f;
  idg::layer64::load_w_row(input_role ? Wg : Wm, D, k1 + i, h, R[0], R[1]);
  if (input_role) {
    idg::layer64::load_w_col(Wg, D, k1 + i, h, R[2], R[3]);
    bb = bg[k1 + i];
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) R[2][r] = 0.f, R[3][r] = 0.f;
  }
  const int64_t n_blocks = (n + RB - 1) / RB;
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const int64_t r0 = blk * RB;
    // lane ids re-defined per block behind an empty asm (idg_ngcf.hip): left to itself the compiler hoists every
    // lane-dependent offset of the block loop out of it and then spills them around the loop
    int tid_l = tid, i_l = i, h_l = h;
    asm volatile("" : "+v"(tid_l), "+v"(i_l), "+v"(h_l));
    // ---- stage side and gM = keep * (gE + J_normalize(T)^T gN at the flagged rows), formed as idg_ngcf_tail_bwd_ex_f32
    // forms it; addresses as a block base + a 32-bit lane offset
    const float* side_b = side + r0 * D;
    const float* T_b = T + r0 * D;
    const float* gE_b = gE ? gE + r0 * D : nullptr;
    const float* gN_b = gN ? gN + r0 * ldgn : nullptr;
    const int last = (int)(n - 1 - r0 < RB - 1 ? n - 1 - r0 : RB - 1);  // rows past the end read the last row (their gM is 0)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int e = tid_l + BWD_BLOCK * j, rr = e >> 4, c4 = (e & 15) * 4;
      const bool live = rr <= last;
      const int rc = live ? rr : last;
      const int64_t row = r0 + rc;
      *reinterpret_cast<float4*>(s_side + rr * LDT + c4) = *reinterpret_cast<const float4*>(side_b + (rc * D + c4));
      const bool has_n = gN && (!gn_rows || idg::bit_at(gn_rows, row));
      float out[4] = {0.f, 0.f, 0.f, 0.f};
      if (live && (has_n || gE)) {  // (the 16 lanes of a row decide alike)
        float ge[4] = {0.f, 0.f, 0.f, 0.f};
        if (gE) {
          const float4 x = *reinterpret_cast<const float4*>(gE_b + (rc * D + c4));
          ge[0] = x.x, ge[1] = x.y, ge[2] = x.z, ge[3] = x.w;
        }
        if (has_n) {
          const float4 t4 = *reinterpret_cast<const float4*>(T_b + (rc * D + c4));
          const float4 x = *reinterpret_cast<const float4*>(gN_b + (rc * (int)ldgn + c4));
          const float tv[4] = {t4.x, t4.y, t4.z, t4.w}, gn[4] = {x.x, x.y, x.z, x.w};
          float ss = 0.f, dot = 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c) ss += tv[c] * tv[c], dot += gn[c] * tv[c];
          ss = idg::lanes_sum<16>(ss);
          dot = idg::lanes_sum<16>(dot);
          const float nrm = sqrtf(ss);
          const float den = fmaxf(nrm, 1e-12f);
#pragma unroll
          for (int c = 0; c < 4; ++c) ge[c] += nrm > 1e-12f ? (gn[c] - dot * tv[c] / (den * den)) / den : gn[c] / den;
        }
        float kp[4];
        idg::keep_scale4(p, seed, stream, row, c4, kp);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = ge[c] * kp[c];
      }
      *reinterpret_cast<float4*>(s_gm + rr * LDT + c4) = make_float4(out[0], out[1], out[2], out[3]);
    }
    __syncthreads();
    f32x16 acc;
    if (input_role) {
      // ---- H = side . Wg + bg with the forward's operands in the forward's order; A = LeakyReLU(H) into its tile
      acc = tile_times_w<HCH>(s_side, rt, i_l, h_l, R[2], R[3]);
#pragma unroll
      for (int r = 0; r < 16; ++r) s_a[(32 * rt + idg::mfma_c_row(r, h_l)) * LDT + k1 + i_l] = leaky(acc[r] + bb, slope);
    } else {
      // ---- gA = gM . Wm^T, kept in the accumulator
      acc = tile_times_w<1>(s_gm, rt, i_l, h_l, R[0], R[1]);
    }
    __syncthreads();
    if (!input_role) {
      // ---- gH = gA o LeakyReLU'(H): 1 where A > 0 (H > 0), the slope elsewhere (H <= 0, as torch's backward at exactly 0)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = (32 * rt + idg::mfma_c_row(r, h_l)) * LDT + k1 + i_l;
        s_gh[o] = s_a[o] > 0.f ? acc[r] : acc[r] * slope;
      }
    }
    __syncthreads();
    if (input_role) {
      // ---- g_side = gH . Wg^T
      acc = tile_times_w<1>(s_gh, rt, i_l, h_l, R[0], R[1]);
      float* gs_b = gSide + r0 * D;  // (a register's 32 lanes of one row: one 128-byte line)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = 32 * rt + idg::mfma_c_row(r, h_l);
        if (rr <= last) gs_b[rr * D + k1 + i_l] = acc[r];
      }
    } else {
      // ---- gWg += side^T gH, gbg += column sums of gH; gWm += A^T gM, gbm += column sums of gM.  K runs over the tile's
      // rows: step s takes rows 2 s + h (rows past the end carry gM = gH = 0)
#pragma unroll 8
      for (int s = 0; s < 32; ++s) {
        const int rr = 2 * s + h_l;
        const float sv = s_side[rr * LDT + 32 * mt + i_l], hv = s_gh[rr * LDT + 32 * nt + i_l];
        const float av = s_a[rr * LDT + 32 * mt + i_l], mv = s_gm[rr * LDT + 32 * nt + i_l];
        R[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(sv, hv, R[2], 0, 0, 0);
        R[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, mv, R[3], 0, 0, 0);
        cs_g += hv;
        cs_m += mv;
      }
    }
    __syncthreads();  // the tiles are free for the next block
  }
  if (input_role) return;
  // this workgroup's slice of the sums, in the layout [gWg | gbg | gWm | gbm]  (lane ids once more behind an empty asm: an
  // offset of this epilogue computed ahead of the block loop is a register carried, and spilled, across it)
  int tid_e = tid;
  asm volatile("" : "+v"(tid_e));
  const int i_e = tid_e & 31, h_e = (tid_e >> 5) & 1;
  constexpr int64_t half = D * D + D;
  float* out = part + (int64_t)blockIdx.x * WCOUNT;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = (32 * mt + idg::mfma_c_row(r, h_e)) * D + 32 * nt + i_e;
    out[o] = R[2][r];
    out[half + o] = R[3][r];
  }
  cs_g += __shfl_xor(cs_g, 32, 64);
  cs_m += __shfl_xor(cs_m, 32, 64);
  if (mt == 0 && h_e == 0) {
    out[D * D + 32 * nt + i_e] = cs_g;
    out[half + D * D + 32 * nt + i_e] = cs_m;
  }
}

}  // namespace

extern "C" {

int idg_gcmc_layer_fwd_f32(const float* side, const float* Wg, const float* bg, const float* Wm, const float* bm, int64_t n,
                           int64_t d, float negative_slope, float p, uint64_t seed, uint64_t stream_id, float* T, float* N,
                           int64_t ldn, void* stream) {
  IDG_REQUIRE(side && Wg && bg && Wm && bm && T && N, "idg_gcmc_layer_fwd_f32: NULL argument");
  IDG_REQUIRE(d == D, "idg_gcmc_layer_fwd_f32: d = 64 only (got %lld); other widths: two dense products and idg_ngcf_tail_ex_f32",
              (long long)d);
  IDG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "idg_gcmc_layer_fwd_f32: bad sizes (n = %lld)", (long long)n);
  IDG_REQUIRE(ldn >= d && ldn % 4 == 0, "idg_gcmc_layer_fwd_f32: bad leading dimension ldn = %lld (>= d, a multiple of 4)",
              (long long)ldn);
  IDG_REQUIRE(p >= 0.f && p < 1.f, "idg_gcmc_layer_fwd_f32: drop probability p = %g outside [0, 1)", (double)p);
  IDG_REQUIRE(((uintptr_t)side | (uintptr_t)T | (uintptr_t)N) % 16 == 0 &&
                  ((uintptr_t)Wg | (uintptr_t)bg | (uintptr_t)Wm | (uintptr_t)bm) % 4 == 0,
              "idg_gcmc_layer_fwd_f32: misaligned argument (panels 16 bytes, weights and biases 4 bytes)");
  const size_t panel = idg::extent(n, d, d), wb = sizeof(float) * D * D, bb = sizeof(float) * D;
  const idg::Span outs[2] = {{T, panel}, {N, idg::extent(n, d, ldn)}}, ins[5] = {{side, panel}, {Wg, wb}, {bg, bb}, {Wm, wb}, {bm, bb}};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 2, ins, 5), "idg_gcmc_layer_fwd_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 2), "idg_gcmc_layer_fwd_f32: T and N overlap");
  hipLaunchKernelGGL(gcmc_layer_fwd64_kernel, dim3((unsigned)((n + RB - 1) / RB)), dim3(BLOCK), 0, (hipStream_t)stream, side, Wg, bg,
                     Wm, bm, n, negative_slope, p, seed, stream_id, T, N, ldn);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

size_t idg_gcmc_layer_bwd_workspace_bytes(int64_t d) {
  if (d != D) return 0;
  return (size_t)BWD_WGS * (size_t)WCOUNT * sizeof(float);
}

int idg_gcmc_layer_bwd_f32(const float* T, const float* gE, const float* gN, int64_t ldgn, const uint32_t* gn_rows,
                           const float* side, const float* Wg, const float* bg, const float* Wm, int64_t n, int64_t d,
                           float negative_slope, float p, uint64_t seed, uint64_t stream_id, float* g_side, float* w_grads,
                           void* ws, void* stream) {
  IDG_REQUIRE(T && (gE || gN) && side && Wg && bg && Wm && g_side && w_grads && ws,
              "idg_gcmc_layer_bwd_f32: NULL argument (at least one of gE and gN must be given)");
  IDG_REQUIRE(d == D, "idg_gcmc_layer_bwd_f32: d = 64 only (got %lld); other widths: idg_ngcf_tail_bwd_ex_f32, idg_linear_wgrad_f32 and dense products",
              (long long)d);
  IDG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "idg_gcmc_layer_bwd_f32: bad sizes (n = %lld)", (long long)n);
  IDG_REQUIRE(!gN || (ldgn >= d && ldgn % 4 == 0 && ldgn < (1 << 20)),
              "idg_gcmc_layer_bwd_f32: bad leading dimension ldgn = %lld (>= d, a multiple of 4, below 2^20)", (long long)ldgn);
  IDG_REQUIRE(p >= 0.f && p < 1.f, "idg_gcmc_layer_bwd_f32: drop probability p = %g outside [0, 1)", (double)p);
  IDG_REQUIRE(((uintptr_t)T | (uintptr_t)gE | (uintptr_t)gN | (uintptr_t)side | (uintptr_t)Wg | (uintptr_t)Wm | (uintptr_t)g_side) % 16 == 0 &&
                  ((uintptr_t)gn_rows | (uintptr_t)bg | (uintptr_t)w_grads | (uintptr_t)ws) % 4 == 0,
              "idg_gcmc_layer_bwd_f32: misaligned argument (panels, Wg and Wm 16 bytes; gn_rows, bg, w_grads and ws 4 bytes)");
  const size_t panel = idg::extent(n, d, d), gnb = gN ? idg::extent(n, d, ldgn) : 0, wb = sizeof(float) * D * D;
  const size_t bits = (size_t)((n + 31) / 32) * sizeof(uint32_t), wg = sizeof(float) * WCOUNT;
  const size_t wsb = idg_gcmc_layer_bwd_workspace_bytes(d);
  const idg::Span outs[3] = {{g_side, panel}, {w_grads, wg}, {ws, wsb}};
  const idg::Span ins[8] = {{T, panel}, {gE, panel}, {gN, gnb}, {gn_rows, bits}, {side, panel}, {Wg, wb}, {bg, sizeof(float) * D}, {Wm, wb}};
  IDG_REQUIRE(!idg::outputs_meet_inputs(outs, 3, ins, 8), "idg_gcmc_layer_bwd_f32: an output overlaps an input");
  IDG_REQUIRE(!idg::outputs_meet(outs, 3), "idg_gcmc_layer_bwd_f32: two outputs overlap");
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_blocks = (n + RB - 1) / RB;
  // two resident workgroups on EVERY CU (a count in between leaves some CUs with one workgroup and some with two)
  const int64_t wgs = n_blocks < BWD_WGS ? n_blocks : BWD_WGS;
  float* part = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(gcmc_layer_bwd64_kernel, dim3((unsigned)wgs), dim3(BWD_BLOCK), 0, st, T, gE, gN, ldgn, gn_rows, side, Wg, bg, Wm, n,
                     negative_slope, p, seed, stream_id, g_side, part);
  return idg::slices_reduce(part, wgs, WCOUNT, w_grads, false, stream);
}

}  // extern "C"
