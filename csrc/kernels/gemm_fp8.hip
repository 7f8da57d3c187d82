// OCP fp8 on gfx950: a row quantiser (bf16 -> e4m3 / e5m2 + one fp32 scale per
// row) and a row-scaled GEMM on v_mfma_scale_f32_32x32x64_f8f6f4, the pieces of
// the opt-in fp8 Linear (ops/fp8.py).
//
//   C[M, N] (bf16, ldc) = (A8[M, K] · B8[N, K]ᵀ)[m, n] · sa[m] · sb[n] (+ bias[n])
//
// Row scales factor out of the contraction, so the MFMA runs with unit block
// scales (E8M0 byte 0x7f) on the raw fp8 codes and the epilogue multiplies the
// fp32 accumulator by sa[m], then sb[n], adds the fp32 bias and rounds to bf16
// once. fp8 x fp8 products are exact in fp32; no split-K and no atomics, so
// two runs give the same bits.
//
// GEMM design
//
//  * Tile 128 x 128 x 128: 256 threads = 4 waves, wave (wr, wc) = (w / 2,
//    w % 2) owns rows [64 wr, +64) x columns [64 wc, +64) as 2 x 2 32x32
//    accumulators (64 registers). A k-step of 128 is two MFMA k-steps of 64:
//    8 MFMA per wave against 16 ds_read_b128. The operands are passed swapped
//    (the B8 fragment as the MFMA's first operand, format selector cbsz =
//    e4m3; the A8 fragment second, blgp = its format), so a lane holds 4
//    consecutive output COLUMNS of one row per accumulator quad.
//  * LDS image. A k-step of an operand tile is [128 rows][128 B]: fp8 rows are
//    half the bytes of bf16 rows, and the k-step is 128 deep (twice gemm_pp's
//    64) precisely so that a row is again 128 B = 8 chunks of 16 B. Chunk c of
//    row r lives at
//        r·128 + 16·(c ^ swz(r)),   swz(r) = (r >> 1) & 7.
//    The MFMA wants, in lane l, row l % 32 and the 32-byte K-run [64 s +
//    32 (l / 32), +32) of MFMA k-step s: chunks 4 s + 2 (l / 32) and the next,
//    two ds_read_b128. Unlike the bf16 16x16x32 fragments (one 16-B chunk per
//    lane, 4 lane groups on 4 chunks) all 32 lanes of a half-wave read the
//    SAME logical chunk of 32 consecutive rows. A ds_read_b128 is served 16
//    lanes at a time: rows R … R+15 (R a multiple of 16), one logical chunk c.
//    The 256-B bank image has 16 slots of 16 B; row r's chunk p sits in slot
//    8 (r & 1) + p. For the 8 even rows of the 16, swz takes the 8 values
//    (R >> 1) & 7 … + 7 (mod 8): c ^ swz is a bijection onto slots 0 … 7; the
//    8 odd rows likewise onto slots 8 … 15. 16 lanes, 16 distinct slots, all
//    64 banks once: no conflict, for either chunk of the run.
//  * DMA. Tiles arrive by global_load_lds_dwordx4 (inline asm) into a 2-deep
//    ring of (A | B) stages, 2 x 32 KiB = the 64 KiB static limit. A wave
//    instruction fills 1 KiB = 8 image rows lane-linearly, so the swizzle is
//    applied to the per-lane SOURCE: lane l of instruction u reads row 8 u +
//    l / 8, logical chunk (l % 8) ^ swz(row). 16 instructions per operand
//    tile, 4 + 4 per wave per k-step; the 8 per-lane offsets are computed
//    once, relative to the tile's first row (a wave-uniform 64-bit base in
//    SGPRs): at most 127·K + 127 < 2^31 for K <= 2^24 (checked on the host).
//    Rows past M (or N) are read at the clamped last row and never stored.
//    K % 128 == 64 (a Linear's data gradient contracts over its outputs, a
//    multiple of 64): the last k-step is one MFMA k-step; its DMA re-reads
//    bytes 0 … 63 of the step into the image's unused upper chunks instead
//    of reading past the row.
//    One iteration: vmcnt(0) + barrier (tile kt has landed everywhere, and
//    every wave has finished reading the other slot), issue tile kt + 1, then
//    the 16 reads and 8 MFMA of tile kt run over that DMA.
//  * Epilogue. After a last barrier each wave stages its 64 x 64 bf16 block
//    in its own 8 KiB of the ring (128-B rows, chunk ^ (row & 7)) and stores
//    whole 128-B row segments, 16 B per lane.
//
// Quantiser: layernorm.hip's row layout. A lane owns 16-element units (two
// 16-B loads, one 16-B fp8 store); a row is spread over 8 lanes (K <= 256:
// 8 rows in flight per wave) or a wave (up to 16 units per lane: K <= 16384),
// kept in registers as raw bf16 between the amax and the cast, read once.
// amax reduces by DPP / v_permlane16_swap / v_permlane32_swap.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>

#include "bf16_vec.h"
#include "fp8_kernels.h"
#include "fp8_mma.h"

namespace dcp {
namespace kern {
namespace {

using namespace fp8dev;  // cast, tile constants, LDS image, DMA (fp8_mma.h)

// ------------------------------------------------------------ quantiser ----
template <int CTRL>
__device__ __forceinline__ float dpp(float x) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xF, 0xF, false));
}
// max over each aligned group of LPR lanes (8 or 64), result in every lane:
// quad_perm xor 1, xor 2, row_half_mirror (8 lanes), then row_mirror (the two
// 8-groups of a row of 16), v_permlane16_swap and v_permlane32_swap
template <int LPR>
__device__ __forceinline__ float group_max(float x) {
  x = fmaxf(x, dpp<0xB1>(x));
  x = fmaxf(x, dpp<0x4E>(x));
  x = fmaxf(x, dpp<0x141>(x));
  if constexpr (LPR == 64) {
    x = fmaxf(x, dpp<0x140>(x));
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
  }
  return x;
}

constexpr int kQT = 256;  // quantiser threads (4 waves)

// UPL = 16-element units per lane, LPR = lanes per row (K <= 16 · UPL · LPR)
template <int FMT, int UPL, int LPR>
__global__ void __launch_bounds__(kQT) fp8_quant_rows_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                             uint8_t* __restrict__ q, float* __restrict__ scale,
                                                             int64_t R, int K) {
  constexpr int RPW = 64 / LPR;  // rows per wave
  constexpr float kMax = Fp8Max<FMT>::v;
  const int lane = threadIdx.x & (LPR - 1);
  const int64_t wrow = (static_cast<int64_t>(blockIdx.x) * (kQT / 64) + (threadIdx.x >> 6)) * RPW;
  if (wrow >= R) return;  // wave-uniform
  const int64_t row = wrow + (threadIdx.x & 63) / LPR;
  const bool live = row < R;
  const int64_t rr = live ? row : R - 1;  // tail: a valid row again, nothing stored (the DPP steps want every lane)
  const int nu = K >> 4;
  uint4 v[UPL][2];
#pragma unroll
  for (int j = 0; j < UPL; ++j) {
    const int u = lane + j * LPR;
    if (u < nu) {
      const uint16_t* p = x + rr * ldx + u * 16;
      v[j][0] = *reinterpret_cast<const uint4*>(p);
      v[j][1] = *reinterpret_cast<const uint4*>(p + 8);
    } else {
      v[j][0] = v[j][1] = make_uint4(0, 0, 0, 0);
    }
  }
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < UPL; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t w[4] = {v[j][h].x, v[j][h].y, v[j][h].z, v[j][h].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) amax = fmaxf(amax, fmaxf(fabsf(bf_lo(w[k])), fabsf(bf_hi(w[k]))));
    }
  amax = group_max<LPR>(amax);
  const float s = amax > 0.f ? amax / kMax : 1.f;
  if (!live) return;
  if (lane == 0) scale[row] = s;
#pragma unroll
  for (int j = 0; j < UPL; ++j) {
    const int u = lane + j * LPR;
    if (u < nu) {
      uint32_t o[4];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t w[4] = {v[j][h].x, v[j][h].y, v[j][h].z, v[j][h].w};
        float f[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          f[2 * k] = fminf(fmaxf(bf_lo(w[k]) / s, -kMax), kMax);
          f[2 * k + 1] = fminf(fmaxf(bf_hi(w[k]) / s, -kMax), kMax);
        }
        o[2 * h] = cvt4<FMT>(f[0], f[1], f[2], f[3]);
        o[2 * h + 1] = cvt4<FMT>(f[4], f[5], f[6], f[7]);
      }
      *reinterpret_cast<uint4*>(q + row * K + u * 16) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

template <int FMT, int UPL, int LPR>
void quant_launch(const void* x, int64_t ldx, void* q, float* scale, int64_t R, int K, hipStream_t s) {
  const int64_t rows_per_blk = (kQT / 64) * (64 / LPR);
  const unsigned grid = static_cast<unsigned>((R + rows_per_blk - 1) / rows_per_blk);
  fp8_quant_rows_kernel<FMT, UPL, LPR><<<grid, kQT, 0, s>>>(static_cast<const uint16_t*>(x), ldx,
                                                            static_cast<uint8_t*>(q), scale, R, K);
}

template <int FMT>
void quant_dispatch(const void* x, int64_t ldx, void* q, float* scale, int64_t R, int K, hipStream_t s) {
  const int nu = K >> 4;
  if (nu <= 16) return quant_launch<FMT, 2, 8>(x, ldx, q, scale, R, K, s);
  if (nu <= 64) return quant_launch<FMT, 1, 64>(x, ldx, q, scale, R, K, s);
  if (nu <= 128) return quant_launch<FMT, 2, 64>(x, ldx, q, scale, R, K, s);
  if (nu <= 256) return quant_launch<FMT, 4, 64>(x, ldx, q, scale, R, K, s);
  if (nu <= 512) return quant_launch<FMT, 8, 64>(x, ldx, q, scale, R, K, s);
  return quant_launch<FMT, 16, 64>(x, ldx, q, scale, R, K, s);
}

// ----------------------------------------------------------------- GEMM ----
template <int AFMT, bool BIAS>
__global__ void __launch_bounds__(kT, 2)
    gemm_fp8_kernel(const uint8_t* __restrict__ A, const float* __restrict__ sa, const uint8_t* __restrict__ B,
                    const float* __restrict__ sb, uint16_t* __restrict__ C, int64_t M, int N, int K, int64_t ldc,
                    const float* __restrict__ bias, int tiles_n) {
  __shared__ __attribute__((aligned(16))) char lds[2 * kStage];  // 64 KiB
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int l31 = lane & 31, hh = lane >> 5;

  // neighbouring tiles (the N-tiles of an M-tile) share an XCD's L2
  const int v = xcd_remap(static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x));
  const int64_t m0 = static_cast<int64_t>(v / tiles_n) * kBM;
  const int n0 = (v % tiles_n) * kBN;
  const int KT = (K + kBK - 1) / kBK;
  const bool tail = (K & (kBK - 1)) != 0;  // K % 128 == 64: the last k-step is one MFMA k-step

  // per-lane source byte offsets (k = 0) within the tile's 128-row slab.
  // cmask 7: a full k-step; 3: the 64-byte tail, where physical chunks that
  // would hold logical chunks 4 … 7 re-read 0 … 3 (in bounds, never used)
  auto src_off = [&](int j, int cmask, bool isb) -> uint32_t {
    const int i = (4 * w + j) * 8 + (lane >> 3);    // image row
    const int lc = ((lane & 7) ^ swz(i)) & cmask;   // logical chunk behind physical chunk lane % 8
    const int64_t r = isb ? (n0 + i < N ? i : N - 1 - n0) : (m0 + i < M ? i : M - 1 - m0);
    return static_cast<uint32_t>(r * K + lc * 16);
  };
  uint32_t offa[4], offb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    offa[j] = src_off(j, 7, false);
    offb[j] = src_off(j, 7, true);
  }
  const uint8_t* abase = A + m0 * K;
  const uint8_t* bbase = B + static_cast<int64_t>(n0) * K;
  auto issue = [&](int kt) {
    char* slot = lds + (kt & 1) * kStage + 4 * w * 1024;
    const uint8_t* ak = abase + static_cast<int64_t>(kt) * kBK;
    const uint8_t* bk = bbase + static_cast<int64_t>(kt) * kBK;
    const bool half = tail && kt == KT - 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      glds16s(ak, half ? src_off(j, 3, false) : offa[j], slot + j * 1024);
      glds16s(bk, half ? src_off(j, 3, true) : offb[j], slot + kTile + j * 1024);
    }
  };

  f32x16 acc[2][2];  // [mi][ni]
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  issue(0);
  for (int kt = 0; kt < KT; ++kt) {
    wait_vm0();
    barrier();
    if (kt + 1 < KT) issue(kt + 1);
    const char* ia = lds + (kt & 1) * kStage;
    const char* ib = ia + kTile;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s == 1 && tail && kt == KT - 1) break;
      i32x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = frag(ia, wr * 64 + i * 32 + l31, s, hh);
        fb[i] = frag(ib, wc * 64 + i * 32 + l31, s, hh);
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fb[ni], fa[mi], acc[mi][ni], FP8_E4M3, AFMT, 0,
                                                                        kUnit, 0, kUnit);
    }
  }
  barrier();  // every wave is done with the ring: it becomes the staging area

  // acc[mi][ni][4 g + e] is row 32 mi + l31, column 32 ni + 8 g + 4 hh + e of
  // the wave's block
  char* cst = lds + w * 8192;
  float sam[2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int64_t m = m0 + wr * 64 + mi * 32 + l31;
    sam[mi] = sa[m < M ? m : M - 1];
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = ni * 32 + 8 * g + 4 * hh;
      const int n = n0 + wc * 64 + col;
      const float4 sbn = *reinterpret_cast<const float4*>(sb + (n < N ? n : 0));
      float4 bn = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (BIAS) bn = *reinterpret_cast<const float4*>(bias + (n < N ? n : 0));
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int row = mi * 32 + l31;
        const float c0 = acc[mi][ni][4 * g + 0] * sam[mi] * sbn.x + bn.x;
        const float c1 = acc[mi][ni][4 * g + 1] * sam[mi] * sbn.y + bn.y;
        const float c2 = acc[mi][ni][4 * g + 2] * sam[mi] * sbn.z + bn.z;
        const float c3 = acc[mi][ni][4 * g + 3] * sam[mi] * sbn.w + bn.w;
        *reinterpret_cast<uint2*>(cst + row * 128 + 16 * ((col >> 3) ^ (row & 7)) + (col & 7) * 2) =
            make_uint2(pack2(c0, c1), pack2(c2, c3));
      }
    }
  const int cb = n0 + wc * 64 + (lane & 7) * 8;  // this lane's 8 output columns
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int row = it * 8 + (lane >> 3);
    const uint4 val = *reinterpret_cast<const uint4*>(cst + row * 128 + 16 * ((lane & 7) ^ (row & 7)));
    const int64_t m = m0 + wr * 64 + row;
    if (m < M && cb < N) *reinterpret_cast<uint4*>(C + m * ldc + cb) = val;
  }
}

template <int AFMT, bool BIAS>
void gemm_launch(const void* A8, const float* sa, const void* B8, const float* sb, void* C, int64_t M, int N, int K,
                 int64_t ldc, const float* bias, hipStream_t s) {
  const int tiles_n = (N + kBN - 1) / kBN;
  const int64_t tiles = ((M + kBM - 1) / kBM) * tiles_n;
  gemm_fp8_kernel<AFMT, BIAS><<<static_cast<unsigned>(tiles), kT, 0, s>>>(
      static_cast<const uint8_t*>(A8), sa, static_cast<const uint8_t*>(B8), sb, static_cast<uint16_t*>(C), M, N, K,
      ldc, bias, tiles_n);
}

}  // namespace

bool fp8_quant_supported(int K) { return K > 0 && K % 16 == 0 && K <= 16384; }

void fp8_quant_rows(const void* x, int64_t ldx, void* q, float* scale, int64_t R, int K, int fmt, hipStream_t s) {
  if (!fp8_quant_supported(K) || ldx < K || ldx % 8 != 0 || (fmt != FP8_E4M3 && fmt != FP8_E5M2) ||
      R >= (int64_t(1) << 31))
    throw std::invalid_argument("fp8_quant_rows: unsupported shape or format");
  if (R <= 0) return;
  if (fmt == FP8_E4M3)
    quant_dispatch<FP8_E4M3>(x, ldx, q, scale, R, K, s);
  else
    quant_dispatch<FP8_E5M2>(x, ldx, q, scale, R, K, s);
}

bool gemm_fp8_supported(int64_t M, int64_t N, int64_t K) {
  // K <= 2^24: the DMA's per-lane offset within a 128-row slab, 127·K + 127, stays below 2^31
  return M >= 1 && N >= 64 && N % 64 == 0 && K >= 64 && K % 64 == 0 && K <= (int64_t(1) << 24) &&
         N < (int64_t(1) << 31) && ((M + kBM - 1) / kBM) * ((N + kBN - 1) / kBN) < (int64_t(1) << 31);
}

void gemm_fp8_bf16(const void* A8, const float* sa, const void* B8, const float* sb, void* C, int64_t M, int N, int K,
                   int64_t ldc, const float* bias, int a_fmt, hipStream_t s) {
  if (!gemm_fp8_supported(M, N, K) || ldc < N || ldc % 8 != 0 || (a_fmt != FP8_E4M3 && a_fmt != FP8_E5M2))
    throw std::invalid_argument("gemm_fp8_bf16: unsupported shape or format");
  if (a_fmt == FP8_E4M3) {
    if (bias)
      gemm_launch<FP8_E4M3, true>(A8, sa, B8, sb, C, M, N, K, ldc, bias, s);
    else
      gemm_launch<FP8_E4M3, false>(A8, sa, B8, sb, C, M, N, K, ldc, bias, s);
  } else {
    if (bias)
      gemm_launch<FP8_E5M2, true>(A8, sa, B8, sb, C, M, N, K, ldc, bias, s);
    else
      gemm_launch<FP8_E5M2, false>(A8, sa, B8, sb, C, M, N, K, ldc, bias, s);
  }
}

}  // namespace kern
}  // namespace dcp
