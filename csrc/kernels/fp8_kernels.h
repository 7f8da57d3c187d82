// Launch API of the OCP fp8 kernels: the row quantiser and the row-scaled fp8
// MFMA GEMM behind the opt-in fp8 Linear (gemm_fp8.hip), the transposing column
// quantiser and the split-K fp32 GEMM of its weight gradient (gemm_fp8_wgrad.hip).
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

// ---- transposing column quantiser: bf16 [M, C] (row stride ldx elements) ->
// fp8 [C, Mp] (contiguous, Mp = fp8_cols_padded(M) = M rounded up to 128, the
// bytes [M, Mp) of every row 0x00) + fp32 scale [C]. The row quantiser's recipe
// applied down each column, the scale of a non-zero column floored at the
// smallest normal fp32 (a subnormal scale keeps too few bits). part: fp32 scratch of fp8_quant_cols_slabs(M) · C
// elements (written before it is read; no zeroing). C % 64 == 0, 1 <= M < 2^31,
// x and q 16-byte aligned, ldx % 8 == 0. Two launches, no atomics.
int64_t fp8_cols_padded(int64_t M);
int fp8_quant_cols_slabs(int64_t M);
void fp8_quant_cols_t(const void* x, int64_t ldx, void* q, float* scale, float* part, int64_t M, int C, int fmt,
                      hipStream_t s);

// ---- out[N, K] (fp32, ldo) (=|+=) sa[n] · sb[k] · Σ_m A8[n, m] · B8[k, m]:
// the weight gradient from the two column-quantised, transposed operands. A8
// [N, Mp] in a_fmt, B8 [K, Mp] e4m3, Mp % 128 == 0 (at most 2^24: the DMA's
// 32-bit per-lane offset), N % 64 == 0, K % 64 == 0, out 16-byte aligned,
// ldo % 4 == 0. S in [1, Mp / 128] splits of the contraction
// (gemm_fp8_wgrad_splits: the host heuristic); S > 1 needs ws, fp32 [S, N, K]
// (no zeroing), summed in the order s = 0 … S − 1. No atomics: two runs give
// the same bits. gemm_fp8_wgrad_supported takes the token count M, not Mp.
bool gemm_fp8_wgrad_supported(int64_t N, int64_t K, int64_t M);
int gemm_fp8_wgrad_splits(int64_t N, int64_t K, int64_t Mp);
void gemm_fp8_wgrad_f32(const void* A8, const float* sa, const void* B8, const float* sb, float* out, int N, int K,
                        int64_t Mp, int64_t ldo, int a_fmt, bool accumulate, int S, float* ws, hipStream_t s);

}  // namespace kern
}  // namespace dcp
