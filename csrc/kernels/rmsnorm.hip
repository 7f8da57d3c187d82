// RMSNorm forward/backward for [rows, D] (bf16 / fp32 activations, fp32
// weight): y = x · rsqrt(mean(x²) + eps) · w. The row kernels follow
// layernorm.hip: one wave64 per row (a half-wave at D = 768), the row held in
// registers as 16-B vectors (8 bf16 per lane), several rows' loads in flight
// per wave, each element read once from HBM in the forward. Backward: one
// read of (dy, x) per row for dx, plus one partial row of dw per workgroup
// (no float atomics) summed in a fixed order by a second small kernel, so two
// calls give the same bits.
//
// Parity: replaces the ATen pow / mean / rsqrt / mul chain of a Llama-style
// decoder's RMSNorm (five element-wise launches rounding through bf16).
#include <hip/hip_runtime.h>

#include "bf16_vec.h"
#include "llama_kernels.h"

namespace dcp {
namespace kern {
namespace {

constexpr int kWaves = 4;  // waves per workgroup
constexpr int kT = 64 * kWaves;
constexpr int kRows = 2;   // rows in flight per wave

template <int D>
struct V8;

template <>
struct V8<LN_BF16> {
  __device__ static void ld(const void* p, int64_t i, float (&o)[8]) {
    const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(p) + i);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[2 * k] = bf_lo(w[k]);
      o[2 * k + 1] = bf_hi(w[k]);
    }
  }
  __device__ static void st(void* p, int64_t i, const float (&o)[8]) {
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(p) + i) =
        make_uint4(pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7]));
  }
};

template <>
struct V8<LN_F32> {
  __device__ static void ld(const void* p, int64_t i, float (&o)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + i);
    const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + i + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
  __device__ static void st(void* p, int64_t i, const float (&o)[8]) {
    *reinterpret_cast<float4*>(static_cast<float*>(p) + i) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(static_cast<float*>(p) + i + 4) = make_float4(o[4], o[5], o[6], o[7]);
  }
};

// sum over the LPR lanes that share a row (64: the wave; 32: a half-wave)
template <int LPR>
__device__ __forceinline__ float rsum(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// VPL = 16-B vectors per lane (D <= VPL · 8 · LPR), R rows per wave with all
// their loads (and the weight's) issued before the first reduction. XD: dtype
// of x, YD: dtype of y — x fp32 / y bf16 is the autocast residual stream.
// LPR = lanes per row: 64, or 32 for D = 768 (3 vectors on every lane).
template <int XD, int YD, int VPL, int R, int LPR>
__global__ void __launch_bounds__(kT) rms_fwd_kernel(const void* __restrict__ x, const float* __restrict__ w,
                                                     void* __restrict__ y, float* __restrict__ rstd_out, int64_t rows,
                                                     int D, float eps) {
  const int lane = threadIdx.x & (LPR - 1);
  const int sub = LPR == 64 ? 0 : (threadIdx.x >> 5) & 1;
  const int64_t row0 = ((static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6)) * (64 / LPR) + sub) * R;
  if (row0 >= rows) return;
  const int nv = D >> 3;
  float wv[VPL][8];
  float v[R][VPL][8];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int vi = lane + j * LPR;
    if (vi < nv) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (row0 + r < rows) V8<XD>::ld(x, (row0 + r) * D + vi * 8, v[r][j]);
      V8<LN_F32>::ld(w, vi * 8, wv[j]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r;
    if (row >= rows) break;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
      if (lane + j * LPR < nv)
#pragma unroll
        for (int k = 0; k < 8; ++k) q = fmaf(v[r][j][k], v[r][j][k], q);
    const float rstd = rsqrtf(rsum<LPR>(q) / static_cast<float>(D) + eps);
    if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int vi = lane + j * LPR;
      if (vi < nv) {
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = v[r][j][k] * rstd * wv[j][k];
        V8<YD>::st(y, row * D + vi * 8, o);
      }
    }
  }
}

// dx = rstd · (g − xhat · mean(g · xhat)), g = dy · w, xhat = x · rstd
// part[blk][D] = Σ_(the workgroup's rows) dy · xhat
// Each wave takes R rows at a time with all their loads in flight together.
// R = 1 (lean): the weight re-read per row from L1 rather than held, gres
// loaded behind the reduction — 4 waves per SIMD (layernorm.hip's lean form).
template <int XD, int YD, int VPL, int R>
__global__ void __launch_bounds__(kT) __attribute__((amdgpu_waves_per_eu(R == 1 && VPL <= 2 ? 4 : 1)))
rms_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ x, const float* __restrict__ w,
               const float* __restrict__ rstd, void* __restrict__ dx, float* __restrict__ part, int64_t rows, int D,
               int rows_per_blk, const void* __restrict__ gres) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [kWaves][D]
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int nv = D >> 3;
  constexpr bool kLean = R == 1;
  float acc[VPL][8], wv[VPL][8];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
    if (!kLean && lane + j * 64 < nv) V8<LN_F32>::ld(w, (lane + j * 64) * 8, wv[j]);
  }
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_blk;
  const int64_t r1 = min(rows, r0 + rows_per_blk);
  for (int64_t rb = r0 + wid * R; rb < r1; rb += kWaves * R) {
    if (kLean) {
      const float* wp = w;
      asm volatile("" : "+s"(wp));  // keep the weight loads inside the loop
#pragma unroll
      for (int j = 0; j < VPL; ++j)
        if (lane + j * 64 < nv) V8<LN_F32>::ld(wp, (lane + j * 64) * 8, wv[j]);
    }
    // gres rows ride with the row's other loads while the registers allow
    constexpr bool kHoist = VPL <= 4 && !kLean;
    float dv[R][VPL][8], xh[R][VPL][8], gr[kHoist ? R : 1][kHoist ? VPL : 1][8], rs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = rb + r < r1 ? rb + r : r1 - 1;  // tail: recompute a valid row, store nothing
      rs[r] = rstd[row];
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const int vi = lane + j * 64;
        if (vi < nv) {
          V8<YD>::ld(dy, row * D + vi * 8, dv[r][j]);
          V8<XD>::ld(x, row * D + vi * 8, xh[r][j]);
          if (kHoist && gres) V8<XD>::ld(gres, row * D + vi * 8, gr[kHoist ? r : 0][kHoist ? j : 0]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool live = rb + r < r1;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        if (lane + j * 64 < nv) {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            xh[r][j][k] *= rs[r];
            if (live) acc[j][k] = fmaf(dv[r][j][k], xh[r][j][k], acc[j][k]);
            dv[r][j][k] *= wv[j][k];  // g
            s = fmaf(dv[r][j][k], xh[r][j][k], s);
          }
        }
      }
      const float m = rsum<64>(s) / static_cast<float>(D);
      if (!live) continue;
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const int vi = lane + j * 64;
        if (vi < nv) {
          float o[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) o[k] = rs[r] * (dv[r][j][k] - xh[r][j][k] * m);
          if (gres) {  // the residual stream's other gradient (dual-output form): dx += gres
            if (!kHoist) V8<XD>::ld(gres, (rb + r) * D + vi * 8, gr[0][0]);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] += gr[kHoist ? r : 0][kHoist ? j : 0][k];
          }
          V8<XD>::st(dx, (rb + r) * D + vi * 8, o);
        }
      }
    }
  }
  // the 4 waves' column partials through LDS, one partial row per workgroup
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int vi = lane + j * 64;
    if (vi < nv) {
#pragma unroll
      for (int k = 0; k < 8; ++k) smem[wid * D + vi * 8 + k] = acc[j][k];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += kT) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < kWaves; ++q) s += smem[q * D + c];
    part[static_cast<int64_t>(blockIdx.x) * D + c] = s;
  }
}

// The second level: workgroup = 64 of the D columns, its 16 waves stride over
// the nblk partial rows (8 loads in flight per lane), one LDS fold in wave
// order and the final (accumulating) store — ln_bwd_reduce_kernel's scheme.
__global__ void __launch_bounds__(1024) rms_bwd_reduce_kernel(const float* __restrict__ part, int nblk, int D,
                                                              float* __restrict__ dw, int accum) {
  __shared__ float red[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (c < D) {
    int b = w;
    for (; b + 7 * 16 < nblk; b += 8 * 16) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = part[static_cast<int64_t>(b + i * 16) * D + c];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; b < nblk; b += 16) s += part[static_cast<int64_t>(b) * D + c];
  }
  red[w][lane] = s;
  __syncthreads();
  if (w == 0 && c < D) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += red[i][lane];
    dw[c] = accum ? dw[c] + t : t;
  }
}

template <int XD, int YD>
void fwd_dispatch(int vpl, dim3 g, hipStream_t s, const void* x, const float* w, void* y, float* rstd, int64_t rows,
                  int D, float eps) {
#define DK_RMSF(V) \
  hipLaunchKernelGGL((rms_fwd_kernel<XD, YD, V, kRows, 64>), g, dim3(kT), 0, s, x, w, y, rstd, rows, D, eps)
  switch (vpl) {
    case 103:
      hipLaunchKernelGGL((rms_fwd_kernel<XD, YD, 3, kRows, 32>), dim3((g.x + 1) / 2), dim3(kT), 0, s, x, w, y, rstd,
                         rows, D, eps);
      break;
    case 1: DK_RMSF(1); break;
    case 2: DK_RMSF(2); break;
    case 4: DK_RMSF(4); break;
    default: DK_RMSF(8);
  }
#undef DK_RMSF
}

template <int XD, int YD>
void bwd_dispatch(int vpl, dim3 g, size_t sm, hipStream_t s, const void* dy, const void* x, const float* w,
                  const float* rstd, void* dx, float* part, int64_t rows, int D, int rpb, const void* gres) {
#define DK_RMSB(V, R) \
  hipLaunchKernelGGL((rms_bwd_kernel<XD, YD, V, R>), g, dim3(kT), sm, s, dy, x, w, rstd, dx, part, rows, D, rpb, gres)
  switch (vpl) {
    case -2: DK_RMSB(2, 1); break;
    case 1: DK_RMSB(1, kRows); break;
    case 2: DK_RMSB(2, kRows); break;
    case 4: DK_RMSB(4, kRows); break;
    default: DK_RMSB(8, kRows);
  }
#undef DK_RMSB
}

// 103: half-wave rows with 3 vectors per lane (nv = 96: D = 768), forward only
inline int vpl_for(int D) {
  const int nv = D / 8;
  if (nv == 96) return 103;
  const int v = (nv + 63) / 64;
  return v <= 1 ? 1 : v <= 2 ? 2 : v <= 4 ? 4 : 8;
}

// lean backward (R = 1, 4 waves per SIMD): bf16 x with rows of 2 vectors per
// lane — the split layernorm.hip measured (fp32 x keeps R = 2's bytes in flight)
bool bwd_lean(int D, int xdtype) {
  const int v = vpl_for(D);
  return xdtype == LN_BF16 && (v == 2 || v == 103);
}

// Backward workgroups: up to 1,024 (4 per CU for a memory-bound pass), each
// with >= 16 rows (lean: >= 8) and one [D] partial row
int bwd_grid(int64_t rows, int D, int xdtype) {
  constexpr int64_t cap = 1024;
  int64_t nb = bwd_lean(D, xdtype) ? (rows + 7) / 8 : (rows + 15) / 16;
  if (nb > cap) nb = cap;
  if (nb < 1) nb = 1;
  return static_cast<int>(nb);
}

}  // namespace

bool rms_supported(int D) { return ln_supported(D); }

int rms_bwd_blocks(int64_t rows, int D) { return bwd_grid(rows, D, LN_BF16); }  // >= the fp32-x grid

void rms_forward(int xdtype, int ydtype, const void* x, const float* w, void* y, float* rstd, int64_t rows, int D,
                 float eps, hipStream_t s) {
  const dim3 g(static_cast<unsigned>((rows + kWaves * kRows - 1) / (kWaves * kRows)));
  const int vpl = vpl_for(D);
  if (xdtype == LN_BF16) fwd_dispatch<LN_BF16, LN_BF16>(vpl, g, s, x, w, y, rstd, rows, D, eps);
  else if (ydtype == LN_BF16) fwd_dispatch<LN_F32, LN_BF16>(vpl, g, s, x, w, y, rstd, rows, D, eps);
  else fwd_dispatch<LN_F32, LN_F32>(vpl, g, s, x, w, y, rstd, rows, D, eps);
}

void rms_backward(int xdtype, int ydtype, const void* dy, const void* x, const float* w, const float* rstd, void* dx,
                  float* dw, float* part, int64_t rows, int D, bool accum, hipStream_t s, const void* gres) {
  const int nblk = bwd_grid(rows, D, xdtype);
  const int rpb = static_cast<int>((rows + nblk - 1) / nblk);
  const size_t sm = sizeof(float) * kWaves * D;
  int vpl = vpl_for(D);
  if (vpl == 103) vpl = 2;  // half-wave rows: forward only
  if (bwd_lean(D, xdtype)) vpl = -2;
  const dim3 g(nblk);
  if (xdtype == LN_BF16) bwd_dispatch<LN_BF16, LN_BF16>(vpl, g, sm, s, dy, x, w, rstd, dx, part, rows, D, rpb, gres);
  else if (ydtype == LN_BF16) bwd_dispatch<LN_F32, LN_BF16>(vpl, g, sm, s, dy, x, w, rstd, dx, part, rows, D, rpb, gres);
  else bwd_dispatch<LN_F32, LN_F32>(vpl, g, sm, s, dy, x, w, rstd, dx, part, rows, D, rpb, gres);
  hipLaunchKernelGGL(rms_bwd_reduce_kernel, dim3((D + 63) / 64), dim3(1024), 0, s, part, nblk, D, dw, accum ? 1 : 0);
}

}  // namespace kern
}  // namespace dcp
