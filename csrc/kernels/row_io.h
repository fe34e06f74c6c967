// Lane loads / stores of the per-channel row kernels (bn_scale.hip, se.hip): V consecutive
// channels of a row as fp32 values.  V = 8 bf16 or 4 fp32 per 16-byte access, V = 1 the scalar
// tail path (DT: 0 bf16, 1 fp32).  Element offsets are 64-bit.
#pragma once
#include "common.h"

namespace {

template <int V, int DT>
SN_DEV void ldx(const void* p, long long e, float* f) {
  if constexpr (V == 8) {
    unpack8(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(p) + e), f);
  } else if constexpr (V == 4) {
    const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + e);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  } else if constexpr (DT) {
    f[0] = reinterpret_cast<const float*>(p)[e];
  } else {
    f[0] = bf2f(reinterpret_cast<const bf16_t*>(p)[e]);
  }
}

template <int V, int DT>
SN_DEV void stx(void* p, long long e, const float* f) {
  if constexpr (V == 8) {
    *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(p) + e) = pack8(f);
  } else if constexpr (V == 4) {
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + e) = make_float4(f[0], f[1], f[2], f[3]);
  } else if constexpr (DT) {
    reinterpret_cast<float*>(p)[e] = f[0];
  } else {
    reinterpret_cast<bf16_t*>(p)[e] = f2bf(f[0]);
  }
}

}  // namespace
