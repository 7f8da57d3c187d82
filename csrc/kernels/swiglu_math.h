// SiLU value and derivative shared by the SwiGLU forward and backward
// (swiglu.hip), in the manner of gelu_math.h: one v_exp with a pre-scaled
// argument and one hardware reciprocal per element.
//
// σ(g) = 1 / (1 + 2^(−g·log2 e)). The exponential overflows to +inf from
// g ≈ −88.7 down, where the reciprocal gives exactly 0 (σ → 0, silu → −0),
// and underflows to 0 from g ≈ +88 up (σ = 1): no NaN for any finite g.
#pragma once

#include <hip/hip_runtime.h>

namespace dcp {
namespace kern {
namespace sw {

constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ float sigmoid(float g) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-kLog2e * g));
}

// silu(g) = g · σ(g)
__device__ __forceinline__ float silu(float g) { return g * sigmoid(g); }

// (silu(g), silu'(g)) from one σ: silu' = σ · (1 + g · (1 − σ))
__device__ __forceinline__ void silu_both(float g, float& v, float& d) {
  const float s = sigmoid(g);
  v = g * s;
  d = s * fmaf(g, 1.f - s, 1.f);
}

}  // namespace sw
}  // namespace kern
}  // namespace dcp
