// Forward of a bottleneck block boundary with the NEXT block's conv1 (1x1,
// K = 4w → N channels) fed from the tile that forms y (gfx950; ⟨K, N⟩ =
// ⟨256, 64⟩, ⟨512, 128⟩, ⟨256, 128⟩).
//
// Unfused, the boundary streams the [M, K] tensors four times: bn_apply reads
// z3 and the residual and writes y = relu(bn3(z3) + r) (+ its mask bits); the
// conv1 GEMM reads y back. Here a workgroup loads a 32-row × K tile of z3 and
// the residual into registers (one tile ahead of the tile being multiplied),
// forms y in fp32 with bn_apply_kernel's expression and bf16 rounding, stores
// y and its mask bits once and writes y into LDS in the swizzled image the MFMA
// fragment reads expect: the transform runs once per element, outside the MFMA
// loop, and conv1 never re-reads y from HBM. RBN: the residual is the
// downsample branch's BN applied inline, r = x2·rsc + rsf (bn_apply_kernel's
// RBN).
//
// z1[32, N] = y_tile · W1ᵀ: wave v owns output channels 16v … 16v+15 of all 32
// rows; its 16 rows of W1 ([N][K]) stay in registers for the whole run (K/8
// VGPRs), so LDS holds the y tile only (16 / 32 KB). MFMA operands are swapped
// as in gemm_nt (W fragment as A): a lane's accumulator holds 4 consecutive
// output channels of one row. Epilogue = gemm_nt's STATS (EPI 1): z1 stored as
// bf16, stats += (Σz1, Σz1²) of the bf16-rounded z1 for the BN1 that follows.
//
// Persistent: P workgroups (XCD-remapped ids as in gemm_nt) stride over the
// row tiles. The folded BN coefficients come from bn_stats_coef's finalize
// launch (one per BN), which also publishes mean / invstd and updates the
// running statistics with bn_apply_kernel's own expressions.
#include <hip/hip_runtime.h>

#include <cstring>

#include "bf16_vec.h"
#include "kernels.h"

namespace dcp {
namespace kern {
namespace {

constexpr int kBM = 32;  // rows per tile: z3 + residual of one tile = 32 KB (K = 256) / 64 KB (K = 512) in flight per workgroup

// gemm_tune "c1fwd64" / "c1fwd128" / "c1fwd256x128" ("c1fwd" sets all three):
// 0 = the unfused path (bn_apply + gemm_nt), 1 = this kernel
int g_mode64 = 1;       // ⟨256, 64⟩
int g_mode128 = 1;      // ⟨512, 128⟩
int g_mode256x128 = 1;  // ⟨256, 128⟩
// gemm_tune "c1fwd_grid": > 0 caps the persistent grid (tests: several tiles per workgroup)
int g_grid = 0;

struct C1Args {
  const uint16_t* z3;   // [M, K] BN3's input
  const uint16_t* res;  // [M, K] the identity, or the downsample BN's input x2 (RBN)
  const uint16_t* w;    // [N][K] W1 bf16
  uint16_t* y;          // [M, K] out
  uint8_t* bits;        // [M·K/8] out: bit k of byte v = (y[8v + k] > 0)
  uint16_t* z1;         // [M, N] out
  const float* sc;      // BN3 folded scale / shift [K]
  const float* sf;
  const float* rsc;     // RBN: the downsample BN's folded scale / shift [K]
  const float* rsf;
  float* stats;         // zeroed [2N]: += (Σz1, Σz1²)
  int64_t M;
  int tiles;
};

template <int K, int N, bool RBN>
__global__ void __launch_bounds__(4 * N) conv1_fwd_kernel(const C1Args a) {
  constexpr int T = 4 * N;        // threads: one wave per 16 output channels
  constexpr int CPR = K / 8;      // 16-B chunks per row
  constexpr int RPP = T / CPR;    // rows per load pass (8 / 16)
  constexpr int NP = kBM / RPP;   // passes per tile (4 / 2)
  constexpr int KS = K / 32;      // MFMA k-steps
  constexpr int FM = kBM / 16;    // row fragments
  static_assert(RPP * NP == kBM && CPR % 16 == 0 && T % CPR == 0, "tile shape");
  __shared__ __attribute__((aligned(16))) char sA[kBM * K * 2];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int cc = t % CPR, r0 = t / CPR;
  const int64_t M = a.M;

  // workgroup id → tile id through gemm_nt's bijective XCD remap
  const int P = gridDim.x, wg = xcd_remap(blockIdx.x, P);

  // folded coefficients of this thread's 8 channels
  float sc[8], sf[8], rsc[RBN ? 8 : 1], rsf[RBN ? 8 : 1];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = cc * 8 + k;
    sc[k] = a.sc[c];
    sf[k] = a.sf[c];
    if (RBN) {
      rsc[k] = a.rsc[c];
      rsf[k] = a.rsf[c];
    }
  }
  // this wave's 16 rows of W1 as MFMA A fragments: row 16wv + (lane&15), k = 32ks + 8(lane>>4) … +7
  bf16x8 wf[KS];
  {
    const uint16_t* wp = a.w + static_cast<int64_t>(16 * wv + (lane & 15)) * K + 8 * (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[ks] = *reinterpret_cast<const bf16x8*>(wp + 32 * ks);
  }
  // STATS: this lane's 4 epilogue channels 16wv + 4(lane>>4) + r
  const int nc = 16 * wv + 4 * (lane >> 4);
  float ssum[4], ssq[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) ssum[r] = ssq[r] = 0.f;

  uint4 zq[NP], rq[NP];
  // rows past M load row 0; they are zeroed / skipped where they are used
  auto load = [&](int tl) {
    const int64_t m0 = static_cast<int64_t>(tl) * kBM;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t m = m0 + r0 + RPP * i;
      const int64_t o = (m < M ? m : 0) * K + cc * 8;
      zq[i] = ld16_nt(a.z3 + o);
      rq[i] = ld16_nt(a.res + o);
    }
  };

  int tl = wg;
  if (tl < a.tiles) load(tl);
  for (; tl < a.tiles; tl += P) {
    const int64_t m0 = static_cast<int64_t>(tl) * kBM;
    // y of this thread's NP chunks: global (once, with its mask byte) and the
    // swizzled LDS image (physical chunk = chunk ^ (row & 15): a fragment
    // read's 16 rows of one chunk fall on 16 distinct 16-B slots of the 256-B
    // bank row)
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = r0 + RPP * i;
      const int64_t m = m0 + row;
      const uint32_t z4[4] = {zq[i].x, zq[i].y, zq[i].z, zq[i].w};
      const uint32_t r4[4] = {rq[i].x, rq[i].y, rq[i].z, rq[i].w};
      float d[8];
      uint32_t bits = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float zk = (k & 1) ? bf_hi(z4[k >> 1]) : bf_lo(z4[k >> 1]);
        const float rk = (k & 1) ? bf_hi(r4[k >> 1]) : bf_lo(r4[k >> 1]);
        // bn_apply_kernel's expression (RES, ACT)
        float o = fmaf(zk, sc[k], sf[k]);
        o += RBN ? fmaf(rk, rsc[RBN ? k : 0], rsf[RBN ? k : 0]) : rk;
        bits |= (o > 0.f ? 1u : 0u) << k;
        d[k] = fmaxf(o, 0.f);
      }
      uint4 v = make_uint4(pack2(d[0], d[1]), pack2(d[2], d[3]), pack2(d[4], d[5]), pack2(d[6], d[7]));
      if (m < M) {
        st16_nt(a.y + m * K + cc * 8, v);
        a.bits[m * CPR + cc] = static_cast<uint8_t>(bits);
      } else {
        v = make_uint4(0, 0, 0, 0);
      }
      *reinterpret_cast<uint4*>(sA + row * (K * 2) + 16 * (cc ^ (row & 15))) = v;
    }
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
            *reinterpret_cast<const bf16x8*>(sA + row * (K * 2) + 16 * ((4 * ks + (lane >> 4)) ^ (row & 15)));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks], xf, acc[j], 0, 0, 0);
      }
    }
    // acc[j][r] = z1[m0 + 16j + (lane&15)][nc + r]
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int64_t m = m0 + 16 * j + (lane & 15);
      if (m < M) {
        const uint2 v = make_uint2(pack2(acc[j][0], acc[j][1]), pack2(acc[j][2], acc[j][3]));
        *reinterpret_cast<uint2*>(a.z1 + m * N + nc) = v;
        const uint32_t w2[2] = {v.x, v.y};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float zk = (r & 1) ? bf_hi(w2[r >> 1]) : bf_lo(w2[r >> 1]);
          ssum[r] += zk;
          ssq[r] = fmaf(zk, zk, ssq[r]);
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
      atomicAdd(a.stats + N + nc + r, ssq[r]);
    }
  }
}

int* mode_of(int K, int N) {
  if (K == 256 && N == 64) return &g_mode64;
  if (K == 512 && N == 128) return &g_mode128;
  if (K == 256 && N == 128) return &g_mode256x128;
  return nullptr;
}

template <int K, int N>
void launch(const C1Args& a, bool rbn, int per_cu, hipStream_t s) {
  int P = 256 * per_cu;
  if (g_grid > 0 && g_grid < P) P = g_grid;
  if (P > a.tiles) P = a.tiles;
  if (rbn) hipLaunchKernelGGL((conv1_fwd_kernel<K, N, true>), dim3(P), dim3(4 * N), 0, s, a);
  else hipLaunchKernelGGL((conv1_fwd_kernel<K, N, false>), dim3(P), dim3(4 * N), 0, s, a);
}

}  // namespace

bool conv1_fwd_tune(const char* key, int value) {
  const int m = value < 0 ? 0 : (value > 1 ? 1 : value);
  if (!strcmp(key, "c1fwd")) g_mode64 = g_mode128 = g_mode256x128 = m;
  else if (!strcmp(key, "c1fwd64")) g_mode64 = m;
  else if (!strcmp(key, "c1fwd128")) g_mode128 = m;
  else if (!strcmp(key, "c1fwd256x128")) g_mode256x128 = m;
  else if (!strcmp(key, "c1fwd_grid")) g_grid = value < 0 ? 0 : value;
  else return false;
  return true;
}

int conv1_fwd_tune_get(const char* key) {
  if (!strcmp(key, "c1fwd")) {
    const int m = g_mode64 < g_mode128 ? g_mode64 : g_mode128;
    return m < g_mode256x128 ? m : g_mode256x128;
  }
  if (!strcmp(key, "c1fwd64")) return g_mode64;
  if (!strcmp(key, "c1fwd128")) return g_mode128;
  if (!strcmp(key, "c1fwd256x128")) return g_mode256x128;
  if (!strcmp(key, "c1fwd_grid")) return g_grid;
  return -1;
}

int conv1_fwd_mode(int64_t M, int K, int N) {
  if (M <= 0 || M >= (int64_t(1) << 31)) return 0;
  const int* m = mode_of(K, N);
  return m ? *m : 0;
}

void conv1_fwd_bf16(const void* z3, const void* res, const void* w, void* y, uint8_t* bits, void* z1, int64_t M, int K,
                    int N, const float* scale, const float* shift, const float* rscale, const float* rshift,
                    float* stats, hipStream_t s) {
  C1Args a;
  a.z3 = static_cast<const uint16_t*>(z3);
  a.res = static_cast<const uint16_t*>(res);
  a.w = static_cast<const uint16_t*>(w);
  a.y = static_cast<uint16_t*>(y);
  a.bits = bits;
  a.z1 = static_cast<uint16_t*>(z1);
  a.sc = scale;
  a.sf = shift;
  a.rsc = rscale;
  a.rsf = rshift;
  a.stats = stats;
  a.M = M;
  a.tiles = static_cast<int>((M + kBM - 1) / kBM);
  const bool rbn = rscale != nullptr;
  // resident workgroups per CU by register count: ⟨256, 64⟩ 256 threads, 146 /
  // 155 VGPRs: 3; ⟨512, 128⟩ 512 threads, 186 / 195: 1; ⟨256, 128⟩ 512 threads,
  // 127 (identity): 2, 138 (RBN): 1
  if (K == 256 && N == 64) launch<256, 64>(a, rbn, 3, s);
  else if (K == 512 && N == 128) launch<512, 128>(a, rbn, 1, s);
  else launch<256, 128>(a, rbn, rbn ? 1 : 2, s);
}

}  // namespace kern
}  // namespace dcp
