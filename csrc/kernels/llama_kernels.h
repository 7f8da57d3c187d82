// Launch API of the Llama-style decoder block kernels: RMSNorm (rmsnorm.hip),
// rotary position embedding on the packed qkv projection (rope.hip) and the
// SwiGLU activation on the packed gate|up projection (swiglu.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ln_kernels.h"  // LnDType

namespace dcp {
namespace kern {

// ---- RMSNorm over [rows, D]: y = x · rsqrt(mean(x²) + eps) · w ------------
// Shapes: those of the LayerNorm kernels (D % 8 == 0, D <= 4096).
bool rms_supported(int D);
// rows of the backward's [rms_bwd_blocks][D] fp32 workspace
int rms_bwd_blocks(int64_t rows, int D);
// xdtype: x / dx; ydtype: y / dy (fp32 -> bf16 supported; bf16 x implies bf16 y)
void rms_forward(int xdtype, int ydtype, const void* x, const float* w, void* y, float* rstd, int64_t rows, int D,
                 float eps, hipStream_t s);
// dx = rstd · (dy·w) − x · rstd³ · mean(dy·w·x) (+ gres: the gradient of x's
// other consumer, the dual-output form); dw = Σ_rows dy · x · rstd through
// per-workgroup partial rows and a fixed-order second level (no float
// atomics); accum: dw += instead of =.
void rms_backward(int xdtype, int ydtype, const void* dy, const void* x, const float* w, const float* rstd, void* dx,
                  float* dw, float* part, int64_t rows, int D, bool accum, hipStream_t s,
                  const void* gres = nullptr);

// ---- rotary embedding on packed [rows = B·T, 3·heads·64] bf16 -------------
// Rotate-half pairs (i, i + 32) of every q and k head by the angle of table
// row (row % T); table: fp32 [T_max, 64] = cos[32] | sin[32] per position.
// out == in: in place (v is not touched); else v is copied through.
// inverse: rotate by −θ (the backward).
void rope_qkv(const void* in, void* out, const float* table, int64_t rows, int T, int heads, bool inverse,
              hipStream_t s);

// ---- SwiGLU on packed [M, 2F] bf16 (gate | up), F % 8 == 0 ----------------
// y[M, F] = silu(gate) · up
void swiglu_fwd(const void* packed, void* y, int64_t M, int F, hipStream_t s);
// dpacked[M, 2F] = (dy · up · silu'(gate) | dy · silu(gate))
void swiglu_bwd(const void* dy, const void* packed, void* dpacked, int64_t M, int F, hipStream_t s);

}  // namespace kern
}  // namespace dcp
