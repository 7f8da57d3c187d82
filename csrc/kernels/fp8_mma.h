// Device helpers shared by the fp8 kernels (gemm_fp8.hip, gemm_fp8_wgrad.hip):
// the fp8 cast, the 128 x 128 x 128 tile constants, the swizzled LDS image and
// its fragment read; the LDS DMA and the ring's ordering primitives come from
// lds_dma.h. gemm_fp8.hip's header has the image and DMA arguments.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fp8_kernels.h"
#include "lds_dma.h"

namespace dcp {
namespace kern {
namespace fp8dev {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int FMT>
struct Fp8Max;
template <>
struct Fp8Max<FP8_E4M3> {
  static constexpr float v = 448.f;
};
template <>
struct Fp8Max<FP8_E5M2> {
  static constexpr float v = 57344.f;
};

// four fp32 -> four fp8 bytes (RNE), the inputs already clamped to ±max
template <int FMT>
__device__ __forceinline__ uint32_t cvt4(float a, float b, float c, float d) {
  int w = 0;
  if constexpr (FMT == FP8_E4M3) {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
  }
  return static_cast<uint32_t>(w);
}

constexpr int kT = 256;
constexpr int kBM = 128, kBN = 128, kBK = 128;
constexpr int kTile = kBM * kBK;   // 16 KiB: one operand's k-step
constexpr int kStage = 2 * kTile;  // A | B
constexpr int kUnit = 0x7f7f7f7f;  // E8M0 1.0 in every byte: unit block scales

__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

// the LDS DMA (glds16s) and the ring's ordering primitives (wait_vm0, barrier):
// lds_dma.h, which has the reasons for their form
using namespace ldsdma;

// this lane's 32-byte K-run of MFMA k-step s: row r, chunks 4 s + 2 hh, + 1
__device__ __forceinline__ i32x8 frag(const char* img, int r, int s, int hh) {
  const int c = 4 * s + 2 * hh;
  const char* row = img + r * kBK;
  const uint4 lo = *reinterpret_cast<const uint4*>(row + 16 * (c ^ swz(r)));
  const uint4 hi = *reinterpret_cast<const uint4*>(row + 16 * ((c + 1) ^ swz(r)));
  i32x8 f;
  f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
  f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
  return f;
}

}  // namespace fp8dev
}  // namespace kern
}  // namespace dcp
