// Rotary position embedding on the packed qkv projection [B·T, 3·H·64] bf16
// that feeds flash_attn_qkv: the q and k thirds are rotated, head by head,
// in the rotate-half pairing (i, i + 32); v is left alone.
//
//   y_i      = x_i · cos θ − x_{i+32} · sin θ
//   y_{i+32} = x_{i+32} · cos θ + x_i · sin θ        θ = θ(t, i), t = row % T
//
// cos / sin come from an fp32 table [T_max, 2, 32] (cos row | sin row per
// position), the arithmetic is fp32 and the result is rounded to bf16 once.
// The backward is the same kernel with the sign of sin flipped (a rotation by
// −θ of the incoming gradient): nothing is saved by the forward.
//
// Work item = one 16-B vector of a head's first half together with its
// partner 32 elements on: 4 items per head, 8·H per row (q and k are
// adjacent: columns [0, 2·H·64)). Four consecutive lanes read two contiguous
// 64-B runs, so a wave covers 16 whole heads. In place (out == in) only those
// 2/3 of the bytes move each way; out of place the v third is copied through
// by 8·H more items per row.
#include <hip/hip_runtime.h>

#include "bf16_vec.h"
#include "llama_kernels.h"

namespace dcp {
namespace kern {
namespace {

constexpr int kT = 256;

__device__ __forceinline__ void ld8f(const float* p, float (&o)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// a·c − b·s by Kahan's difference of products: the rounding error of b·s is
// recovered with one FMA and added back, so the result is good to ~2 fp32
// ulps of ITSELF even when the two products cancel — a plain fma(a, c, −b·s)
// is only good to an ulp of the products, which after cancellation can exceed
// a bf16 ulp of the small result.
__device__ __forceinline__ float diff_of_products(float a, float c, float b, float s) {
  const float w = b * s;
  const float e = fmaf(-b, s, w);  // w − b·s, exact
  return fmaf(a, c, -w) + e;
}

// ipr = items per row: 8·H (in place) or 16·H (the second 8·H copy v).
// in / out may be the same buffer (no __restrict__): an item reads its 32
// bytes before it writes them and no other item touches them.
template <bool COPY_V>
__global__ void __launch_bounds__(kT) rope_qkv_kernel(const uint16_t* in, uint16_t* out,
                                                      const float* __restrict__ table, int64_t items, int T, int H,
                                                      float sgn) {
  const int64_t it = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (it >= items) return;
  const int ipr = (COPY_V ? 16 : 8) * H;
  const int64_t row = it / ipr;
  const int i = static_cast<int>(it - row * ipr);
  const int64_t base = row * (3 * 64 * static_cast<int64_t>(H));
  if (COPY_V && i >= 8 * H) {
    const int64_t o = base + 2 * 64 * static_cast<int64_t>(H) + (i - 8 * H) * 8;
    *reinterpret_cast<uint4*>(out + o) = *reinterpret_cast<const uint4*>(in + o);
    return;
  }
  const int head = i >> 2, j = i & 3;  // head over q then k; j: which 8 of the 32 pairs
  const int64_t o = base + head * 64 + j * 8;
  const uint4 a = *reinterpret_cast<const uint4*>(in + o);
  const uint4 b = *reinterpret_cast<const uint4*>(in + o + 32);
  const float* tr = table + static_cast<int64_t>(row % T) * 64 + j * 8;
  float c[8], s[8];
  ld8f(tr, c);
  ld8f(tr + 32, s);
  const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
  uint32_t ya[4], yb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float a0 = bf_lo(aw[k]), a1 = bf_hi(aw[k]), b0 = bf_lo(bw[k]), b1 = bf_hi(bw[k]);
    const float s0 = sgn * s[2 * k], s1 = sgn * s[2 * k + 1];
    ya[k] = pack2(diff_of_products(a0, c[2 * k], b0, s0), diff_of_products(a1, c[2 * k + 1], b1, s1));
    yb[k] = pack2(diff_of_products(b0, c[2 * k], a0, -s0), diff_of_products(b1, c[2 * k + 1], a1, -s1));
  }
  *reinterpret_cast<uint4*>(out + o) = make_uint4(ya[0], ya[1], ya[2], ya[3]);
  *reinterpret_cast<uint4*>(out + o + 32) = make_uint4(yb[0], yb[1], yb[2], yb[3]);
}

}  // namespace

void rope_qkv(const void* in, void* out, const float* table, int64_t rows, int T, int heads, bool inverse,
              hipStream_t s) {
  const bool copy_v = in != out;
  const int64_t items = rows * (copy_v ? 16 : 8) * heads;
  if (items == 0) return;
  const dim3 grid(static_cast<unsigned>((items + kT - 1) / kT));
  const auto* i = static_cast<const uint16_t*>(in);
  auto* o = static_cast<uint16_t*>(out);
  const float sgn = inverse ? -1.f : 1.f;
  if (copy_v) hipLaunchKernelGGL(rope_qkv_kernel<true>, grid, dim3(kT), 0, s, i, o, table, items, T, heads, sgn);
  else hipLaunchKernelGGL(rope_qkv_kernel<false>, grid, dim3(kT), 0, s, i, o, table, items, T, heads, sgn);
}

}  // namespace kern
}  // namespace dcp
