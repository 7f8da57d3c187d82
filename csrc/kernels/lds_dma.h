// The LDS DMA ring primitives shared by the flash-attention kernels
// (attn_mma.h) and the fp8 GEMMs (fp8_mma.h): global_load_lds in its saddr
// form, and the explicit wait + barrier that order a ring of tiles.
// (gemm.hip keeps its own glds16: the per-lane 64-bit pointer form.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dcp {
namespace kern {
namespace ldsdma {

// LDS DMA (16 / 4 B per lane) into the wave-uniform LDS address lds_dst (+
// lane x size). Inline asm on purpose: a compiler-visible global_load_lds is a
// pending LDS write to hipcc, which then put s_waitcnt vmcnt(0) before the
// first LDS read after it — in every loop iteration, so each tile waited for
// the NEXT tile's DMA to land in the middle of its own compute (PMC r5: 0.3 of
// wave cycles waiting, MFMA busy 0.14-0.22). Hidden, the ring is ordered by
// the explicit wait_vm0 + barrier at the top of each iteration only. M0 is
// compiler-reserved: set and restored in-statement. The source is a
// wave-uniform 64-bit base in SGPRs plus a 32-bit per-lane byte offset
// (saddr form): the per-lane part of a tile's source is
// loop-invariant, so each DMA costs no VALU address arithmetic (the 64-bit
// per-lane pointer form recomputed row × stride with two v_mad_u64_u32 and
// moves per DMA, ~20 VALU per key block)
__device__ __forceinline__ uint32_t lds_u32(const char* p) {
  return __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p)));
}
__device__ __forceinline__ void glds16s(const void* sbase, uint32_t voff, char* lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(lds_u32(lds_dst))
               : "memory");
}
__device__ __forceinline__ void glds4s(const void* sbase, uint32_t voff, char* lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(lds_u32(lds_dst))
               : "memory");
}
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

}  // namespace ldsdma
}  // namespace kern
}  // namespace dcp
