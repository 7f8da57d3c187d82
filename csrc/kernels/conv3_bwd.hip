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
//
// Downsample blocks (relu(bn3(z3) + bn_d(zd)), MODE below): the boundary hands
// the same g to two BNs. kDual (w = 64, stride-1 downsample conv of w → 4w
// channels) also loads zd, forms dzd with bn_bwd_apply2_kernel's expressions,
// stores it once and multiplies a second LDS image by Wdᵀ for the downsample
// conv's data gradient dx_d (no RED: no BN behind that conv's input here):
// g, z3, zd read once, dz3, dzd written once, neither re-read by a data-gradient
// GEMM.
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
// gemm_tune "c3bwd_ds64" / "c3bwd_ds128" ("c3bwd_ds" sets both): the downsample
// blocks' variants: kDual at w = 64 (on: −0.85 ms per step), kDzd at w = 128
// (off: inside the run-to-run spread alone; NOTES §39)
int g_ds64 = 1;
int g_ds128 = 0;
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
  // downsample variants only
  const uint16_t* zd;   // [M, 4w] the downsample BN's input
  const uint16_t* wdt;  // [w][4w] Wdᵀ bf16 (kDual)
  uint16_t* dzd;        // [M, 4w] out
  uint16_t* dxd;        // [M, w] out (kDual): the downsample conv's data gradient
  const float* gammad;  // downsample BN
  const float* meand;
  const float* invstdd;
  const float* accd;    // (Σg, Σg·(zd − μd)) [2·4w]
};

// kPlain: identity blocks. kDzd: also forms and stores dzd. kDual: kDzd + the
// downsample conv's data gradient from a second LDS image.
enum { kPlain = 0, kDzd = 1, kDual = 2 };

template <int W, int MODE>
__global__ void __launch_bounds__(4 * W, MODE == kDual ? 2 : 1) conv3_bwd_kernel(const C3Args a) {
  constexpr bool DS = MODE != kPlain, DUAL = MODE == kDual;
  constexpr int C = 4 * W;        // conv3 output channels = the data gradient's K
  constexpr int T = 4 * W;        // threads: one wave per 16 output channels
  constexpr int CPR = C / 8;      // 16-B chunks per row
  constexpr int RPP = T / CPR;    // rows per load pass (8)
  constexpr int NP = kBM / RPP;   // passes per tile (4)
  constexpr int KS = C / 32;      // MFMA k-steps
  constexpr int FM = kBM / 16;    // row fragments
  static_assert(RPP * NP == kBM && CPR >= 16, "tile shape");
  constexpr int IMG = kBM * C * 2;  // one swizzled tile image
  // kDual: the dzd image behind the dz3 image (32 KB at w = 64, two workgroups
  // per CU use 64 of 160 KB) instead of one buffer and a third barrier per tile
  __shared__ __attribute__((aligned(16))) char sA[IMG * (DUAL ? 2 : 1)];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int cc = t % CPR, r0 = t / CPR;
  const int64_t M = a.M;

  // workgroup id → tile id through gemm_nt's bijective XCD remap
  const int P = gridDim.x, wg = xcd_remap(blockIdx.x, P);

  // BN3 backward coefficients of this thread's 8 channels (bn_bwd_apply_kernel's expressions)
  float k1[8], k2[8], k3[8], mu[8];
  // downsample variants: both BNs' coefficients [k1 | k2 | k3 | μ][C] × 2 stay
  // in LDS (bn_bwd_apply2_kernel's expressions, the unfused path of these
  // blocks): 64 resident VGPRs would not fit beside both weight slices under
  // the 256 of two workgroups per CU (NOTES §39); a thread re-reads its 8
  // channels' 256 B per tile
  __shared__ __attribute__((aligned(16))) float sK[DS ? 8 * C : 4];
  if constexpr (DS) {
    const float inv_m = 1.f / static_cast<float>(M);
    for (int c = t; c < C; c += T) {
      const float i3 = a.invstd3[c], id = a.invstdd[c];
      sK[c] = a.gamma3[c] * i3;
      sK[C + c] = a.acc3[c] * inv_m;
      sK[2 * C + c] = a.acc3[C + c] * inv_m * i3 * i3;
      sK[3 * C + c] = a.mean3[c];
      sK[4 * C + c] = a.gammad[c] * id;
      sK[5 * C + c] = a.accd[c] * inv_m;
      sK[6 * C + c] = a.accd[C + c] * inv_m * id * id;
      sK[7 * C + c] = a.meand[c];
    }
    __syncthreads();
  } else {
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
  }
  // a thread's 8 channels of coefficient set q (0: BN3, 1: the downsample BN) from LDS
  auto coefs = [&](int q, float (&c1)[8], float (&c2)[8], float (&c3)[8], float (&cm)[8]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* kp = sK + 4 * q * C + cc * 8 + 4 * h;
      *reinterpret_cast<float4*>(c1 + 4 * h) = *reinterpret_cast<const float4*>(kp);
      *reinterpret_cast<float4*>(c2 + 4 * h) = *reinterpret_cast<const float4*>(kp + C);
      *reinterpret_cast<float4*>(c3 + 4 * h) = *reinterpret_cast<const float4*>(kp + 2 * C);
      *reinterpret_cast<float4*>(cm + 4 * h) = *reinterpret_cast<const float4*>(kp + 3 * C);
    }
  };
  // this wave's 16 rows of W3ᵀ as MFMA A fragments: row 16wv + (lane&15), k = 32ks + 8(lane>>4) … +7
  bf16x8 wf[KS];
  {
    const uint16_t* wp = a.wt + static_cast<int64_t>(16 * wv + (lane & 15)) * C + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[ks] = *reinterpret_cast<const bf16x8*>(wp + 32 * ks);
  }
  bf16x8 wdf[DUAL ? KS : 1];  // and of Wdᵀ
  if constexpr (DUAL) {
    const uint16_t* wp = a.wdt + static_cast<int64_t>(16 * wv + (lane & 15)) * C + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wdf[ks] = *reinterpret_cast<const bf16x8*>(wp + 32 * ks);
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

  uint4 gq[NP], zq[NP], dq[DS ? NP : 1];
  uint2 xq[FM];
  // rows past M load row 0; they are zeroed / skipped where they are used
  auto load = [&](int tl) {
    const int64_t m0 = static_cast<int64_t>(tl) * kBM;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t m = m0 + r0 + RPP * i;
      if constexpr (DS) {
        // rows past M load the tile's first row: an unsigned 32-bit lane offset
        // on a uniform tile base (three more 64-bit lane addresses per pass do not fit)
        const int rem = static_cast<int>(M - m0 < kBM ? M - m0 : kBM);
        const uint32_t lo = (r0 + RPP * i < rem ? r0 + RPP * i : 0) * C + cc * 8;
        gq[i] = ld16_nt(a.g + m0 * C + lo);
        zq[i] = ld16_nt(a.z3 + m0 * C + lo);
        dq[i] = ld16_nt(a.zd + m0 * C + lo);
        continue;
      }
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
      if constexpr (DS) coefs(0, k1, k2, k3, mu);
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
      if constexpr (DS) {
        const uint32_t y4[4] = {dq[i].x, dq[i].y, dq[i].z, dq[i].w};
        float e[8], j1[8], j2[8], j3[8], jm[8];
        coefs(1, j1, j2, j3, jm);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float gk = (k & 1) ? bf_hi(g4[k >> 1]) : bf_lo(g4[k >> 1]);
          const float xk = (k & 1) ? bf_hi(y4[k >> 1]) : bf_lo(y4[k >> 1]);
          e[k] = j1[k] * (gk - j2[k] - (xk - jm[k]) * j3[k]);
        }
        uint4 u = make_uint4(pack2(e[0], e[1]), pack2(e[2], e[3]), pack2(e[4], e[5]), pack2(e[6], e[7]));
        if (m < M) st16_nt(a.dzd + m * C + cc * 8, u);
        else u = make_uint4(0, 0, 0, 0);
        if constexpr (DUAL) *reinterpret_cast<uint4*>(sA + IMG + row * (C * 2) + 16 * (cc ^ (row & 15))) = u;
        // one pass at a time: interleaving the passes holds every unpacked operand at once
        __builtin_amdgcn_sched_barrier(0);
      }
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
    if constexpr (DUAL) {
      // the downsample conv's data gradient: the same loop on the dzd image against Wdᵀ
      f32x4 ad[FM];
#pragma unroll
      for (int j = 0; j < FM; ++j) ad[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          const int row = 16 * j + (lane & 15);
          const bf16x8 xf = *reinterpret_cast<const bf16x8*>(sA + IMG + row * (C * 2) +
                                                             16 * ((4 * ks + (lane >> 4)) ^ (row & 15)));
          ad[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wdf[ks], xf, ad[j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        const int64_t m = m0 + 16 * j + (lane & 15);
        if (m < M)
          *reinterpret_cast<uint2*>(a.dxd + m * W + nc) =
              make_uint2(pack2(ad[j][0], ad[j][1]), pack2(ad[j][2], ad[j][3]));
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
  else if (!strcmp(key, "c3bwd_ds")) g_ds64 = g_ds128 = m;
  else if (!strcmp(key, "c3bwd_ds64")) g_ds64 = m;
  else if (!strcmp(key, "c3bwd_ds128")) g_ds128 = m;
  else if (!strcmp(key, "c3bwd_grid")) g_grid = value < 0 ? 0 : value;
  else return false;
  return true;
}

int conv3_bwd_tune_get(const char* key) {
  if (!strcmp(key, "c3bwd")) return g_mode64 < g_mode128 ? g_mode64 : g_mode128;
  if (!strcmp(key, "c3bwd64")) return g_mode64;
  if (!strcmp(key, "c3bwd128")) return g_mode128;
  if (!strcmp(key, "c3bwd_ds")) return g_ds64 < g_ds128 ? g_ds64 : g_ds128;
  if (!strcmp(key, "c3bwd_ds64")) return g_ds64;
  if (!strcmp(key, "c3bwd_ds128")) return g_ds128;
  if (!strcmp(key, "c3bwd_grid")) return g_grid;
  return -1;
}

int conv3_bwd_mode(int64_t M, int w) {
  if (M <= 0 || M >= (int64_t(1) << 31)) return 0;
  return w == 64 ? g_mode64 : (w == 128 ? g_mode128 : 0);
}

int conv3_bwd_ds_mode(int64_t M, int w) {
  if (conv3_bwd_mode(M, w) <= 0) return 0;  // c3bwd=0 turns everything off
  return w == 64 ? (g_ds64 ? kDual : 0) : (g_ds128 ? kDzd : 0);
}

namespace {
int c3_grid(int per_cu, int tiles) {
  int P = 256 * per_cu;
  if (g_grid > 0 && g_grid < P) P = g_grid;
  return P > tiles ? tiles : P;
}
}  // namespace

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
  a.zd = a.wdt = nullptr;
  a.dzd = a.dxd = nullptr;
  a.gammad = a.meand = a.invstdd = a.accd = nullptr;
  const int P = c3_grid(w == 64 ? 2 : 1, a.tiles);
  if (w == 64) hipLaunchKernelGGL((conv3_bwd_kernel<64, kPlain>), dim3(P), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv3_bwd_kernel<128, kPlain>), dim3(P), dim3(512), 0, s, a);
}

void conv3_bwd_ds_bf16(const void* g, const void* z3, const void* zd, const void* wt, const void* wdt, const void* x2,
                       void* dz3, void* dzd, void* dy2, void* dxd, int64_t M, int w, const float* gamma3,
                       const float* mean3, const float* invstd3, const float* acc3, const float* gammad,
                       const float* meand, const float* invstdd, const float* accd, const float* gamma2,
                       const float* beta2, const float* mean2, const float* invstd2, float* stats, hipStream_t s) {
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
  a.zd = static_cast<const uint16_t*>(zd);
  a.wdt = static_cast<const uint16_t*>(wdt);
  a.dzd = static_cast<uint16_t*>(dzd);
  a.dxd = static_cast<uint16_t*>(dxd);
  a.gammad = gammad;
  a.meand = meand;
  a.invstdd = invstdd;
  a.accd = accd;
  // w = 64 → kDual, 234 VGPRs: 2 workgroups per CU; w = 128 → kDzd, 242 VGPRs: 1 per CU
  // (96 KB of g + z3 + zd in flight per CU either way)
  const int P = c3_grid(w == 64 ? 2 : 1, a.tiles);
  if (w == 64) hipLaunchKernelGGL((conv3_bwd_kernel<64, kDual>), dim3(P), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv3_bwd_kernel<128, kDzd>), dim3(P), dim3(512), 0, s, a);
}

void bn_dparams(const float* acc, const float* invstd, float* dgamma, float* dbeta, int C, hipStream_t s) {
  hipLaunchKernelGGL(bn_dparams_kernel, dim3((C + 255) / 256), dim3(256), 0, s, acc, invstd, dgamma, dbeta, C);
}

}  // namespace kern
}  // namespace dcp
