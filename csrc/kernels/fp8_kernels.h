// Launch API of the OCP fp8 kernels (gemm_fp8.hip): the row quantiser and the
// row-scaled fp8 MFMA GEMM behind the opt-in fp8 Linear.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dcp {
namespace kern {

// operand formats; the values are the MFMA's cbsz / blgp format selectors
enum Fp8Fmt { FP8_E4M3 = 0, FP8_E5M2 = 1 };

// ---- row quantiser: bf16 [R, K] (row stride ldx elements) -> fp8 [R, K]
// (contiguous) + fp32 scale [R]. Per row: s = amax / fmt_max (1 for an all-zero
// row), q = cvt_fp8(clamp(x / s, ±fmt_max)), round-to-nearest-even.
// K % 16 == 0, K <= 16384; x and q 16-byte aligned, ldx % 8 == 0.
bool fp8_quant_supported(int K);
void fp8_quant_rows(const void* x, int64_t ldx, void* q, float* scale, int64_t R, int K, int fmt, hipStream_t s);

// ---- C[M, N] (bf16, ldc) = (A8[M, K] · B8[N, K]ᵀ)[m, n] · sa[m] · sb[n]
// (+ bias[n], fp32), rounded to bf16 once. A8 in a_fmt, B8 always e4m3, both
// K-contiguous. Any M >= 1, N % 64 == 0, K % 64 == 0 (128-deep k-steps; a last
// half step where K % 128 == 64), K <= 2^24 (the DMA's
// 32-bit per-lane offset within a 128-row slab: 127·K + 127 < 2^31).
// C 16-byte aligned, ldc % 8 == 0. No atomics, no split-K: two runs give the
// same bits.
bool gemm_fp8_supported(int64_t M, int64_t N, int64_t K);
void gemm_fp8_bf16(const void* A8, const float* sa, const void* B8, const float* sb, void* C, int64_t M, int N, int K,
                   int64_t ldc, const float* bias, int a_fmt, hipStream_t s);

}  // namespace kern
}  // namespace dcp
