// Device-side vocabulary shared by the bf16 MFMA kernels: vector types, bf16
// pack / unpack on 32-bit words, streaming 16-B accesses, the XCD remap.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dcp {
namespace kern {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
// two fp32 → packed bf16 (RNE) in one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  const bf16x2 v = {static_cast<__bf16>(a), static_cast<__bf16>(b)};
  return __builtin_bit_cast(uint32_t, v);
}
// streaming 16-B accesses (batchnorm.hip: nothing caches these tensors between passes)
__device__ __forceinline__ uint4 ld16_nt(const uint16_t* p) {
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st16_nt(uint16_t* p, uint4 v) {
  const u32x4 w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(p));
}

// Hardware workgroup id → logical id, bijective on [0, P): the dispatcher deals
// consecutive ids round-robin to the 8 XCDs; the remap hands XCD x the x-th
// contiguous run of logical ids (the first P % 8 runs one longer), so
// neighbouring tiles share an L2.
__device__ __forceinline__ int xcd_remap(int wid, int P) {
  const int xcd = wid & 7, q8 = P >> 3, r8 = P & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (wid >> 3);
}

}  // namespace kern
}  // namespace dcp
