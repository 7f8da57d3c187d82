// Backward of a bottleneck's conv3 (1x1, w → 4w channels) with BN3's backward
// apply fused in as a producer-side prologue (gfx950, w = 64 / 128).
//
// Unfused, an identity block streams the [M, 4w] tensors three times to hand
// conv3 its output gradient: bn_bwd_apply reads g and z3 and writes
// dz3 = k1·(g − k2 − (z3 − μ)·k3); the data-gradient GEMM reads dz3 back. Here
// a workgroup loads a 32-row × 4w tile of g and z3 into registers (one tile
// ahead of the tile being multiplied), forms dz3 in fp32 with
// bn_bwd_apply_kernel's expression and bf16 rounding, stores it once for the
// weight-gradient kernel and writes it into LDS in the swizzled image the MFMA
// fragment reads expect: the transform runs once per element, outside the
// MFMA loop, and the data gradient never re-reads dz3 from HBM.
//
// dy2[32, w] = dz3_tile · W3: wave v owns output channels 16v … 16v+15 of all
// 32 rows; its slice of W3ᵀ (16 rows × 4w k) stays in registers for the whole
// run (w/2 VGPRs), so LDS holds the dz3 tile only (16 / 32 KB). MFMA operands
// are swapped as in gemm_nt (W fragment as A): a lane's accumulator holds 4
// consecutive output channels of one row. Epilogue = gemm_nt's RED (EPI 2):
// dy2 stored as bf16, g2 = dy2·[x2·sc + sf > 0] from the bf16-rounded dy2,
// stats += (Σg2, Σg2·(x2 − μ2)) for the BN2 backward apply that follows.
//
// Persistent: P workgroups (XCD-remapped ids as in gemm_nt) stride over the
// row tiles. BN3's dγ / dβ come from acc alone (bn_dparams_kernel: the apply
// kernel's own expressions) because autograd needs them before this kernel's
// node runs.
#include <hip/hip_runtime.h>

#include <cstring>

#include "bf16_vec.h"
#include "kernels.h"

namespace dcp {
namespace kern {
namespace {

constexpr int kBM = 32;  // rows per tile: g + z3 of one tile = 32 KB (w = 64) / 64 KB (w = 128) in flight per workgroup

// gemm_tune "c3bwd64" / "c3bwd128" ("c3bwd" sets both): 0 = the unfused path,
// 1 = this kernel (dz3 stored for the weight gradient)
int g_mode64 = 1;
int g_mode128 = 1;
// gemm_tune "c3bwd_grid": > 0 caps the persistent grid (tests: several tiles per workgroup)
int g_grid = 0;

struct C3Args {
  const uint16_t* g;    // [M, 4w] masked gradient of BN3's output
  const uint16_t* z3;   // [M, 4w] BN3's input
  const uint16_t* wt;   // [w][4w] W3ᵀ bf16
  const uint16_t* x2;   // [M, w] BN2's input
  uint16_t* dz3;        // [M, 4w] out
  uint16_t* dy2;        // [M, w] out
  const float* gamma3;  // BN3
  const float* mean3;
  const float* invstd3;
  const float* acc3;    // (Σg, Σg·(z3 − μ3)) [2·4w]
  const float* gamma2;  // BN2 (nullable affine)
  const float* beta2;
  const float* mean2;
  const float* invstd2;
  float* stats;         // zeroed [2w]: += (Σg2, Σg2·(x2 − μ2))
  int64_t M;
  int tiles;
};

template <int W>
__global__ void __launch_bounds__(4 * W) conv3_bwd_kernel(const C3Args a) {
  constexpr int C = 4 * W;        // conv3 output channels = the data gradient's K
  constexpr int T = 4 * W;        // threads: one wave per 16 output channels
  constexpr int CPR = C / 8;      // 16-B chunks per row
  constexpr int RPP = T / CPR;    // rows per load pass (8)
  constexpr int NP = kBM / RPP;   // passes per tile (4)
  constexpr int KS = C / 32;      // MFMA k-steps
  constexpr int FM = kBM / 16;    // row fragments
  static_assert(RPP * NP == kBM && CPR >= 16, "tile shape");
  __shared__ __attribute__((aligned(16))) char sA[kBM * C * 2];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int cc = t % CPR, r0 = t / CPR;
  const int64_t M = a.M;

  // workgroup id → tile id through gemm_nt's bijective XCD remap
  const int P = gridDim.x, wg = xcd_remap(blockIdx.x, P);

  // BN3 backward coefficients of this thread's 8 channels (bn_bwd_apply_kernel's expressions)
  float k1[8], k2[8], k3[8], mu[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = cc * 8 + k;
    const float inv = a.invstd3[c];
    const float sb = a.acc3[c], sg = a.acc3[C + c];
    k1[k] = a.gamma3[c] * inv;
    k2[k] = sb / static_cast<float>(M);
    k3[k] = sg / static_cast<float>(M) * inv * inv;
    mu[k] = a.mean3[c];
  }
  // this wave's 16 rows of W3ᵀ as MFMA A fragments: row 16wv + (lane&15), k = 32ks + 8(lane>>4) … +7
  bf16x8 wf[KS];
  {
    const uint16_t* wp = a.wt + static_cast<int64_t>(16 * wv + (lane & 15)) * C + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[ks] = *reinterpret_cast<const bf16x8*>(wp + 32 * ks);
  }
  // RED: this lane's 4 epilogue channels 16wv + 4(lane>>4) + r
  const int nc = 16 * wv + 4 * (lane >> 4);
  float dmu[4], dsc[4], dsf[4], ssum[4], ssq[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = nc + r;
    const float m2 = a.mean2[c];
    const float sc = (a.gamma2 ? a.gamma2[c] : 1.f) * a.invstd2[c];
    dmu[r] = m2;
    dsc[r] = sc;
    dsf[r] = (a.beta2 ? a.beta2[c] : 0.f) - m2 * sc;
    ssum[r] = ssq[r] = 0.f;
  }

  uint4 gq[NP], zq[NP];
  uint2 xq[FM];
  // rows past M load row 0; they are zeroed / skipped where they are used
  auto load = [&](int tl) {
    const int64_t m0 = static_cast<int64_t>(tl) * kBM;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t m = m0 + r0 + RPP * i;
      const int64_t o = (m < M ? m : 0) * C + cc * 8;
      gq[i] = ld16_nt(a.g + o);
      zq[i] = ld16_nt(a.z3 + o);
    }
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int64_t m = m0 + 16 * j + (lane & 15);
      xq[j] = *reinterpret_cast<const uint2*>(a.x2 + (m < M ? m : 0) * W + nc);
    }
  };

  int tl = wg;
  if (tl < a.tiles) load(tl);
  for (; tl < a.tiles; tl += P) {
    const int64_t m0 = static_cast<int64_t>(tl) * kBM;
    // dz3 of this thread's NP chunks: global (once) and the swizzled LDS image
    // (physical chunk = chunk ^ (row & 15): a fragment read's 16 rows of one
    // chunk fall on 16 distinct 16-B slots of the 256-B bank row)
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = r0 + RPP * i;
      const int64_t m = m0 + row;
      const uint32_t g4[4] = {gq[i].x, gq[i].y, gq[i].z, gq[i].w};
      const uint32_t z4[4] = {zq[i].x, zq[i].y, zq[i].z, zq[i].w};
      float d[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float gk = (k & 1) ? bf_hi(g4[k >> 1]) : bf_lo(g4[k >> 1]);
        const float xk = (k & 1) ? bf_hi(z4[k >> 1]) : bf_lo(z4[k >> 1]);
        d[k] = k1[k] * (gk - k2[k] - (xk - mu[k]) * k3[k]);
      }
      uint4 v = make_uint4(pack2(d[0], d[1]), pack2(d[2], d[3]), pack2(d[4], d[5]), pack2(d[6], d[7]));
      if (m < M) st16_nt(a.dz3 + m * C + cc * 8, v);
      else v = make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(sA + row * (C * 2) + 16 * (cc ^ (row & 15))) = v;
    }
    uint2 xc[FM];
#pragma unroll
    for (int j = 0; j < FM; ++j) xc[j] = xq[j];
    __syncthreads();
    if (tl + P < a.tiles) load(tl + P);  // in flight across the MFMAs and the epilogue

    f32x4 acc[FM];
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        const int row = 16 * j + (lane & 15);
        const bf16x8 xf =
            *reinterpret_cast<const bf16x8*>(sA + row * (C * 2) + 16 * ((4 * ks + (lane >> 4)) ^ (row & 15)));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks], xf, acc[j], 0, 0, 0);
      }
    }
    // acc[j][r] = dy2[m0 + 16j + (lane&15)][nc + r]
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int64_t m = m0 + 16 * j + (lane & 15);
      if (m < M) {
        const uint2 v = make_uint2(pack2(acc[j][0], acc[j][1]), pack2(acc[j][2], acc[j][3]));
        *reinterpret_cast<uint2*>(a.dy2 + m * W + nc) = v;
        const uint32_t w2[2] = {v.x, v.y}, x2[2] = {xc[j].x, xc[j].y};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float xk = (r & 1) ? bf_hi(x2[r >> 1]) : bf_lo(x2[r >> 1]);
          float gk = (r & 1) ? bf_hi(w2[r >> 1]) : bf_lo(w2[r >> 1]);
          gk = fmaf(xk, dsc[r], dsf[r]) > 0.f ? gk : 0.f;
          ssum[r] += gk;
          ssq[r] = fmaf(gk, xk - dmu[r], ssq[r]);
        }
      }
    }
    __syncthreads();  // every wave is done with the tile image
  }
  // lanes with the same channels: lane ^ 1, 2, 4, 8; waves own disjoint channels
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      ssum[r] += __shfl_xor(ssum[r], o);
      ssq[r] += __shfl_xor(ssq[r], o);
    }
  if ((lane & 15) == 0 && wg < a.tiles) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      atomicAdd(a.stats + nc + r, ssum[r]);
      atomicAdd(a.stats + W + nc + r, ssq[r]);
    }
  }
}

// dγ = Σg(x−μ)·invstd, dβ = Σg from acc = (Σg, Σg·(x − μ)) [2C] — what
// bn_bwd_apply_kernel's first workgroup writes
__global__ void bn_dparams_kernel(const float* __restrict__ acc, const float* __restrict__ invstd,
                                  float* __restrict__ dgamma, float* __restrict__ dbeta, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    const float inv = invstd[c];
    const float sb = acc[c], sg = acc[C + c];
    dgamma[c] = sg * inv;
    dbeta[c] = sb;
  }
}

}  // namespace

bool conv3_bwd_tune(const char* key, int value) {
  const int m = value < 0 ? 0 : (value > 1 ? 1 : value);
  if (!strcmp(key, "c3bwd")) g_mode64 = g_mode128 = m;
  else if (!strcmp(key, "c3bwd64")) g_mode64 = m;
  else if (!strcmp(key, "c3bwd128")) g_mode128 = m;
  else if (!strcmp(key, "c3bwd_grid")) g_grid = value < 0 ? 0 : value;
  else return false;
  return true;
}

int conv3_bwd_tune_get(const char* key) {
  if (!strcmp(key, "c3bwd")) return g_mode64 < g_mode128 ? g_mode64 : g_mode128;
  if (!strcmp(key, "c3bwd64")) return g_mode64;
  if (!strcmp(key, "c3bwd128")) return g_mode128;
  if (!strcmp(key, "c3bwd_grid")) return g_grid;
  return -1;
}

int conv3_bwd_mode(int64_t M, int w) {
  if (M <= 0 || M >= (int64_t(1) << 31)) return 0;
  return w == 64 ? g_mode64 : (w == 128 ? g_mode128 : 0);
}

void conv3_bwd_bf16(const void* g, const void* z3, const void* wt, const void* x2, void* dz3, void* dy2, int64_t M,
                    int w, const float* gamma3, const float* mean3, const float* invstd3, const float* acc3,
                    const float* gamma2, const float* beta2, const float* mean2, const float* invstd2, float* stats,
                    hipStream_t s) {
  C3Args a;
  a.g = static_cast<const uint16_t*>(g);
  a.z3 = static_cast<const uint16_t*>(z3);
  a.wt = static_cast<const uint16_t*>(wt);
  a.x2 = static_cast<const uint16_t*>(x2);
  a.dz3 = static_cast<uint16_t*>(dz3);
  a.dy2 = static_cast<uint16_t*>(dy2);
  a.gamma3 = gamma3;
  a.mean3 = mean3;
  a.invstd3 = invstd3;
  a.acc3 = acc3;
  a.gamma2 = gamma2;
  a.beta2 = beta2;
  a.mean2 = mean2;
  a.invstd2 = invstd2;
  a.stats = stats;
  a.M = M;
  a.tiles = static_cast<int>((M + kBM - 1) / kBM);
  // resident workgroups: w = 64 → 256 threads, 176 VGPRs: 2 per CU;
  // w = 128 → 512 threads, 216 VGPRs: 1 per CU (64 KB of g + z3 in flight per CU either way)
  int P = 256 * (w == 64 ? 2 : 1);
  if (g_grid > 0 && g_grid < P) P = g_grid;
  if (P > a.tiles) P = a.tiles;
  if (w == 64) hipLaunchKernelGGL(conv3_bwd_kernel<64>, dim3(P), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(conv3_bwd_kernel<128>, dim3(P), dim3(512), 0, s, a);
}

void bn_dparams(const float* acc, const float* invstd, float* dgamma, float* dbeta, int C, hipStream_t s) {
  hipLaunchKernelGGL(bn_dparams_kernel, dim3((C + 255) / 256), dim3(256), 0, s, acc, invstd, dgamma, dbeta, C);
}

}  // namespace kern
}  // namespace dcp
