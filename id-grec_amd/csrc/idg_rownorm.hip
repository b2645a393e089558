// Row normalisation of a dense fp32 panel and its backward: the per-layer step of LightGCN++ (Lee et al., RecSys'24;
// models/LightGCN_pp.py:82-84 of the reference: norm = torch.norm(x, dim=1) + 1e-12; x = x / norm[:, None]).
//
//   idg_rows_normalize_f32      norms[r] = ||X[r]||_2,  Y[r] = X[r] / (norms[r] + eps)
//   idg_rows_normalize_bwd_f32  out[r] = a G[r] + add2[r] + J_r(T[r]),  J the Jacobian-transpose product of the row's
//                               normalisation, from the saved Y and norms
//
// One row is held by one group of LPR lanes of a wave64 (LPR a power of two, 4 .. 64), NV float4s (d % 4 == 0) or NV floats
// (any other d) per lane, lane l of the group holding units l, l + LPR, ..: a group's loads and stores are contiguous.  The
// row stays in registers between the reduction (an xor butterfly of __shfl_xor over the group: no LDS, no atomics, every
// lane ends with the same bits) and the store, so each input panel is read once and each output written once.  A lane reads
// every input element it owns before it writes the output element at that position, and no other lane touches that
// position: this is what makes the in-place forms (Y == X; out == T, G or add2) exact.
#include <hip/hip_runtime.h>

#include <cmath>

#include "idg_common.h"
#include "idg_device.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_WIDTH = 512;

template <int NV, bool VEC>
struct Regs {
  float v[NV * (VEC ? 4 : 1)];
};

// units of lane l: float4s (VEC) or floats at unit index j * LPR + l; dead lanes and the padding past d read as 0
template <int LPR, int NV, bool VEC>
__device__ __forceinline__ void load_row(const float* row, int d, int l, bool live, Regs<NV, VEC>& x) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int u = j * LPR + l;
    if (VEC) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live && u * 4 < d) t = *reinterpret_cast<const float4*>(row + u * 4);
      x.v[4 * j + 0] = t.x;
      x.v[4 * j + 1] = t.y;
      x.v[4 * j + 2] = t.z;
      x.v[4 * j + 3] = t.w;
    } else {
      x.v[j] = (live && u < d) ? row[u] : 0.f;
    }
  }
}

template <int LPR, int NV, bool VEC>
__device__ __forceinline__ void store_row(float* row, int d, int l, bool live, const Regs<NV, VEC>& x) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int u = j * LPR + l;
    if (VEC) {
      if (live && u * 4 < d)
        *reinterpret_cast<float4*>(row + u * 4) = make_float4(x.v[4 * j], x.v[4 * j + 1], x.v[4 * j + 2], x.v[4 * j + 3]);
    } else {
      if (live && u < d) row[u] = x.v[j];
    }
  }
}

template <int LPR, int NV, bool VEC>
__global__ __launch_bounds__(BLOCK) void rows_normalize_kernel(const float* X, int64_t n, int d, float eps, float* Y,
                                                               float* __restrict__ norms) {
  constexpr int E = NV * (VEC ? 4 : 1), RPB = BLOCK / LPR;
  const int l = threadIdx.x % LPR;
  const int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const bool live = r < n;
  const int64_t base = live ? r * d : 0;
  Regs<NV, VEC> x;
  load_row<LPR, NV, VEC>(X + base, d, l, live, x);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) ss += x.v[i] * x.v[i];
  ss = idg::lanes_sum<LPR>(ss);
  const float nrm = sqrtf(ss), den = nrm + eps;
#pragma unroll
  for (int i = 0; i < E; ++i) x.v[i] = x.v[i] / den;  // a zero row: 0 / eps == 0 exactly
  store_row<LPR, NV, VEC>(Y + base, d, l, live, x);
  if (live && l == 0) norms[r] = nrm;
}

// J(t) = (t - y <y, t> (n + e) / n) / (n + e) for n > 0; for n == 0 the saved y is 0 and the coefficient is set to 0, which
// leaves t / e: torch's norm has gradient 0 at the origin.
template <int LPR, int NV, bool VEC>
__global__ __launch_bounds__(BLOCK) void rows_normalize_bwd_kernel(const float* T, const float* __restrict__ Y,
                                                                   const float* __restrict__ norms, float eps, const float* G,
                                                                   float a, const float* add2, float* out, int64_t n, int d) {
  constexpr int E = NV * (VEC ? 4 : 1), RPB = BLOCK / LPR;
  const int l = threadIdx.x % LPR;
  const int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
  const bool live = r < n;
  const int64_t base = live ? r * d : 0;
  Regs<NV, VEC> t, y, g;
  load_row<LPR, NV, VEC>(T + base, d, l, live, t);
  load_row<LPR, NV, VEC>(Y + base, d, l, live, y);
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) dot += y.v[i] * t.v[i];
  dot = idg::lanes_sum<LPR>(dot);
  const float nrm = live ? norms[r] : 1.f;
  const float den = nrm + eps;
  const float coef = nrm > 0.f ? dot * (den / nrm) : 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) t.v[i] = (t.v[i] - y.v[i] * coef) / den;
  if (G != nullptr) {
    load_row<LPR, NV, VEC>(G + base, d, l, live, g);
#pragma unroll
    for (int i = 0; i < E; ++i) t.v[i] = t.v[i] + a * g.v[i];
  }
  if (add2 != nullptr) {
    load_row<LPR, NV, VEC>(add2 + base, d, l, live, g);
#pragma unroll
    for (int i = 0; i < E; ++i) t.v[i] = t.v[i] + g.v[i];
  }
  store_row<LPR, NV, VEC>(out + base, d, l, live, t);
}

struct FwdArgs {
  const float* X;
  int64_t n;
  int d;
  float eps;
  float* Y;
  float* norms;
};

struct BwdArgs {
  const float *T, *Y, *norms;
  float eps;
  const float* G;
  float a;
  const float* add2;
  float* out;
  int64_t n;
  int d;
};

template <int LPR, int NV, bool VEC>
void launch(const FwdArgs& p, hipStream_t st) {
  constexpr int RPB = BLOCK / LPR;
  hipLaunchKernelGGL((rows_normalize_kernel<LPR, NV, VEC>), dim3((unsigned)((p.n + RPB - 1) / RPB)), dim3(BLOCK), 0, st, p.X, p.n,
                     p.d, p.eps, p.Y, p.norms);
}

template <int LPR, int NV, bool VEC>
void launch(const BwdArgs& p, hipStream_t st) {
  constexpr int RPB = BLOCK / LPR;
  hipLaunchKernelGGL((rows_normalize_bwd_kernel<LPR, NV, VEC>), dim3((unsigned)((p.n + RPB - 1) / RPB)), dim3(BLOCK), 0, st, p.T,
                     p.Y, p.norms, p.eps, p.G, p.a, p.add2, p.out, p.n, p.d);
}

// the narrowest lane group that holds the row with one unit per lane; past 64 units, 2, 4 or 8 units per lane
template <bool VEC, class Args>
void dispatch_units(const Args& p, int units, hipStream_t st) {
  if (units <= 4) return launch<4, 1, VEC>(p, st);
  if (units <= 8) return launch<8, 1, VEC>(p, st);
  if (units <= 16) return launch<16, 1, VEC>(p, st);
  if (units <= 32) return launch<32, 1, VEC>(p, st);
  if (units <= 64) return launch<64, 1, VEC>(p, st);
  if (units <= 128) return launch<64, 2, VEC>(p, st);
  if constexpr (!VEC) {  // d <= 512: the float4 path ends at 128 units
    if (units <= 256) return launch<64, 4, false>(p, st);
    return launch<64, 8, false>(p, st);
  }
}

template <class Args>
void dispatch(const Args& p, hipStream_t st) {
  if (p.d % 4 == 0)
    dispatch_units<true>(p, p.d / 4, st);
  else
    dispatch_units<false>(p, p.d, st);
}

using idg::overlap;

// the same panel (allowed where stated) or disjoint from it; anything in between is refused
bool same_or_apart(const void* p, const void* q, size_t bytes) { return p == q || !overlap(p, bytes, q, bytes); }

}  // namespace

extern "C" {

#define IDG_RN_SIZES(who)                                                                                                \
  IDG_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), who ": bad sizes (n = %lld)", (long long)n);                             \
  IDG_REQUIRE(d >= 1 && d <= MAX_WIDTH, who ": d = %lld (1 .. %d are built)", (long long)d, MAX_WIDTH);                  \
  IDG_REQUIRE(eps > 0.f && eps < INFINITY, who ": eps = %g (a positive finite value)", (double)eps)

int idg_rows_normalize_f32(const float* X, int64_t n, int64_t d, float eps, float* Y, float* norms, void* stream) {
  IDG_REQUIRE(X && Y && norms, "idg_rows_normalize_f32: NULL argument");
  IDG_RN_SIZES("idg_rows_normalize_f32");
  IDG_REQUIRE((uintptr_t)X % 16 == 0 && (uintptr_t)Y % 16 == 0 && (uintptr_t)norms % 4 == 0,
              "idg_rows_normalize_f32: misaligned argument (panels 16 bytes, norms 4 bytes)");
  const size_t panel = (size_t)n * (size_t)d * sizeof(float), vec = (size_t)n * sizeof(float);
  IDG_REQUIRE(same_or_apart(Y, X, panel), "idg_rows_normalize_f32: Y overlaps X without being X (aliasing: Y == X only)");
  IDG_REQUIRE(!overlap(norms, vec, X, panel) && !overlap(norms, vec, Y, panel),
              "idg_rows_normalize_f32: norms overlaps a panel (aliasing: Y == X only)");
  dispatch(FwdArgs{X, n, (int)d, eps, Y, norms}, (hipStream_t)stream);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

int idg_rows_normalize_bwd_f32(const float* T, const float* Y, const float* norms, float eps, const float* G, float a,
                               const float* add2, float* out, int64_t n, int64_t d, void* stream) {
  IDG_REQUIRE(T && Y && norms && out, "idg_rows_normalize_bwd_f32: NULL argument");
  IDG_RN_SIZES("idg_rows_normalize_bwd_f32");
  IDG_REQUIRE((uintptr_t)T % 16 == 0 && (uintptr_t)Y % 16 == 0 && (uintptr_t)G % 16 == 0 && (uintptr_t)add2 % 16 == 0 &&
                  (uintptr_t)out % 16 == 0 && (uintptr_t)norms % 4 == 0,
              "idg_rows_normalize_bwd_f32: misaligned argument (panels 16 bytes, norms 4 bytes)");
  const size_t panel = (size_t)n * (size_t)d * sizeof(float), vec = (size_t)n * sizeof(float);
  IDG_REQUIRE(!overlap(out, panel, Y, panel) && !overlap(out, panel, norms, vec),
              "idg_rows_normalize_bwd_f32: out overlaps Y or norms (aliasing: out == T, G or add2 only)");
  IDG_REQUIRE(same_or_apart(out, T, panel) && (!G || same_or_apart(out, G, panel)) && (!add2 || same_or_apart(out, add2, panel)),
              "idg_rows_normalize_bwd_f32: out overlaps an input without being it (aliasing: out == T, G or add2 only)");
  dispatch(BwdArgs{T, Y, norms, eps, G, a, add2, out, n, (int)d}, (hipStream_t)stream);
  IDG_HIP(hipGetLastError());
  return IDG_OK;
}

}  // extern "C"
