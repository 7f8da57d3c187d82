// SwiGLU on the packed gate|up projection [M, 2F] bf16 (one packed GEMM of
// the two weights): y[M, F] = silu(gate) · up.
//
// Forward: 8 bf16 per 16-byte access, two vectors of each half per thread
// (all four loads issued first), fp32 math, one rounding to bf16: 6 bytes per
// output element. Backward: from dy and the saved packed input it writes the
// packed gradient (d_gate | d_up) in one pass — silu(gate) is recomputed,
// never stored: 10 bytes per element of y.
//
// Parity: replaces F.silu(gate) * up (a split copy, a SiLU and a multiply in
// the forward; five element-wise launches and a cat in the backward).
#include <hip/hip_runtime.h>

#include "bf16_vec.h"
#include "llama_kernels.h"
#include "swiglu_math.h"

namespace dcp {
namespace kern {
namespace {

constexpr int kT = 256;
constexpr int kU = 2;  // vectors per thread

__device__ __forceinline__ const uint4* v16(const uint16_t* p) { return reinterpret_cast<const uint4*>(p); }

// vector n of the [M, F/8] output grid -> element offset of its gate vector
// in the packed [M, 2F] input (the up vector sits F elements on)
__device__ __forceinline__ int64_t packed_off(int64_t n, int f8, int F) {
  const int64_t row = n / f8;
  return row * 2 * F + (n - row * f8) * 8;
}

__global__ void __launch_bounds__(kT) swiglu_fwd_kernel(const uint16_t* __restrict__ p, uint16_t* __restrict__ y,
                                                        int64_t n8, int F) {
  const int f8 = F >> 3;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kU * kT + threadIdx.x;
  uint4 g[kU], u[kU];
#pragma unroll
  for (int q = 0; q < kU; ++q)
    if (i0 + q * kT < n8) {
      const int64_t o = packed_off(i0 + q * kT, f8, F);
      g[q] = *v16(p + o);
      u[q] = *v16(p + o + F);
    }
#pragma unroll
  for (int q = 0; q < kU; ++q) {
    if (i0 + q * kT >= n8) break;
    const uint32_t gw[4] = {g[q].x, g[q].y, g[q].z, g[q].w}, uw[4] = {u[q].x, u[q].y, u[q].z, u[q].w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      o[k] = pack2(sw::silu(bf_lo(gw[k])) * bf_lo(uw[k]), sw::silu(bf_hi(gw[k])) * bf_hi(uw[k]));
    *reinterpret_cast<uint4*>(y + (i0 + q * kT) * 8) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

__global__ void __launch_bounds__(kT) swiglu_bwd_kernel(const uint16_t* __restrict__ dy,
                                                        const uint16_t* __restrict__ p, uint16_t* __restrict__ dp,
                                                        int64_t n8, int F) {
  const int f8 = F >> 3;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kU * kT + threadIdx.x;
  uint4 g[kU], u[kU], d[kU];
#pragma unroll
  for (int q = 0; q < kU; ++q)
    if (i0 + q * kT < n8) {
      const int64_t o = packed_off(i0 + q * kT, f8, F);
      g[q] = *v16(p + o);
      u[q] = *v16(p + o + F);
      d[q] = *v16(dy + (i0 + q * kT) * 8);
    }
#pragma unroll
  for (int q = 0; q < kU; ++q) {
    if (i0 + q * kT >= n8) break;
    const uint32_t gw[4] = {g[q].x, g[q].y, g[q].z, g[q].w}, uw[4] = {u[q].x, u[q].y, u[q].z, u[q].w};
    const uint32_t dw[4] = {d[q].x, d[q].y, d[q].z, d[q].w};
    uint32_t og[4], ou[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v0, d0, v1, d1;
      sw::silu_both(bf_lo(gw[k]), v0, d0);
      sw::silu_both(bf_hi(gw[k]), v1, d1);
      const float y0 = bf_lo(dw[k]), y1 = bf_hi(dw[k]);
      og[k] = pack2(y0 * bf_lo(uw[k]) * d0, y1 * bf_hi(uw[k]) * d1);
      ou[k] = pack2(y0 * v0, y1 * v1);
    }
    const int64_t o = packed_off(i0 + q * kT, f8, F);
    *reinterpret_cast<uint4*>(dp + o) = make_uint4(og[0], og[1], og[2], og[3]);
    *reinterpret_cast<uint4*>(dp + o + F) = make_uint4(ou[0], ou[1], ou[2], ou[3]);
  }
}

}  // namespace

void swiglu_fwd(const void* packed, void* y, int64_t M, int F, hipStream_t s) {
  const int64_t n8 = M * (F / 8);
  if (n8 == 0) return;
  const dim3 grid(static_cast<unsigned>((n8 + kU * kT - 1) / (kU * kT)));
  hipLaunchKernelGGL(swiglu_fwd_kernel, grid, dim3(kT), 0, s, static_cast<const uint16_t*>(packed),
                     static_cast<uint16_t*>(y), n8, F);
}

void swiglu_bwd(const void* dy, const void* packed, void* dpacked, int64_t M, int F, hipStream_t s) {
  const int64_t n8 = M * (F / 8);
  if (n8 == 0) return;
  const dim3 grid(static_cast<unsigned>((n8 + kU * kT - 1) / (kU * kT)));
  hipLaunchKernelGGL(swiglu_bwd_kernel, grid, dim3(kT), 0, s, static_cast<const uint16_t*>(dy),
                     static_cast<const uint16_t*>(packed), static_cast<uint16_t*>(dpacked), n8, F);
}

}  // namespace kern
}  // namespace dcp
