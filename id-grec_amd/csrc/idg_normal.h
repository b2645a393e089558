// CVGA's reparameterisation noise (models/CVGA.py:63-67: eps = torch.randn_like(std)): a counter-based standard normal,
// a function of (seed, stream, row, feature) only, so the backward kernels regenerate eps instead of reading it.  The bits
// come from idg_dropout.h's mix, taken on the complemented stream id: a dropout mask and the normal draws of one stream id
// never share a mix.  One mix gives two uniforms (24 bits each) and, through Box-Muller, the normals of the feature pair
// (2j, 2j + 1).
#pragma once
#include <cstdint>

#include "idg_dropout.h"

namespace idg {

__device__ __forceinline__ float normal_of(uint64_t seed, uint64_t stream, int64_t row, int64_t f) {
  const uint64_t z = mix64(seed, ~stream, row, f >> 1);
  const float u1 = (float)((z >> 40) + 1) * (1.0f / 16777216.0f);  // (0, 1]
  const float u2 = (float)(z & 0xFFFFFFu) * (1.0f / 16777216.0f);  // [0, 1)
  const float r = sqrtf(-2.0f * logf(u1));
  const float a = 6.28318530717958647692f * u2;
  return (f & 1) ? r * sinf(a) : r * cosf(a);
}

}  // namespace idg
