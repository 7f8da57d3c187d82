// fp8 weight gradient of a Linear on gfx950: a transposing COLUMN quantiser and
// a split-K variant of the row-scaled fp8 MFMA GEMM (gemm_fp8.hip) with an fp32
// result.
//
//   dW[n, k] = Σ_m gy[m, n]·x[m, k] = sgy[n]·sx[k]·Σ_m qgy[m, n]·qx[m, k]
//
// The contraction runs over the tokens m, so the scales must not depend on m:
// one scale per COLUMN of x and of gy factors out where row scales do not. The
// NT GEMM wants the contraction contiguous, so the quantiser writes its output
// transposed: q [C, Mp], Mp = M rounded up to the GEMM's k-step of 128, the
// bytes [M, Mp) of every row 0x00 (zero in e4m3 and in e5m2): the GEMM has no
// contraction tail and M may be any value >= 1.
//
// Column quantiser: two launches, x read twice, no atomics, no memset
//
//  1. fp8_col_amax_kernel. Grid (C / 64, S), S = min(32, ceil(M / 128)) row
//     slabs. 256 threads = 32 row lanes x 8 column lanes; a lane loads 16 B =
//     8 columns of one row (the 8 column lanes read 128 contiguous bytes) and
//     keeps |max| of its 8 columns over every 32nd row of the slab; the 32 row
//     lanes meet in LDS and the block writes part[s][c0 … c0 + 63]. Every
//     entry of part is written (an empty slab writes 0), so the scratch is
//     at::empty. max is exact: no order dependence.
//  2. fp8_quant_cols_t_kernel. Grid (Mp / 128, C / 64): a 128-row x 64-column
//     tile per block. Prologue: thread c < 64 takes the max of part[0 … S)[c0 +
//     c] (at most 32 L2 reads) and forms s = amax / fmt_max (1 where amax is
//     0; never below the smallest normal fp32): every block of a column strip computes the same s, the block of the
//     first row tile stores it. Lane (cl, rg) = (t % 8, t / 8) loads rows
//     4 rg … + 3 x columns 8 cl … + 7 (four 16-B loads; rows >= M count as 0),
//     scales, clamps, and turns each column's 4 row values into ONE dword with
//     a cvt_pk pair: 4 consecutive m bytes of output row c. The 8 dwords go
//     into an LDS byte image [64 columns][144 B] (128 m-bytes + 16 pad), which
//     is read back as 16-B runs along m and stored as whole 128-B segments of
//     the output rows (8 lanes per row). (The compiler pairs the dword writes
//     of columns j, j + 1 into ds_write2_b32; each half is the write below.)
//
//     LDS image: byte (col, m) at  col·144 + 16·((m >> 4) ^ f(col)) + (m & 15),
//     f(col) = (col >> 3) & 6.
//     * dword writes (ds_write_b32, 64 lanes over 64 banks). In wave w, cl
//       takes 0 … 7 and rg takes 8 w … 8 w + 7; write j of a lane is column
//       8 cl + j, dword rg of its row: chunk k = rg >> 2 = 2 w + b (b = bit 2
//       of rg), dword rg & 3 of the chunk. f only touches bits 1 and 2, so
//       k ^ f = ((2 w) ^ (cl & 6)) | b. The bank is the dword address mod 64:
//           36·(8 cl + j) + 4·(k ^ f) + (rg & 3)
//         ≡ 32·(cl & 1) + 4·(k ^ f) + (rg & 3) + 36 j         (288 ≡ 32).
//       Bit 5 is cl & 1, bits 4 … 2 are ((2 w) ^ (cl & 6)) | b — a bijection of
//       (cl >> 1, b) — and bits 1 … 0 are rg & 3: the 64 lanes hit 64 distinct
//       banks, shifted by the wave-uniform 36 j. The pad is what gives bit 5:
//       at a pitch of 128 B every column of one write shares col & 1 and the
//       64 lanes would fall on 32 banks.
//     * 16-B reads (ds_read_b128, 16 lanes at a time over 16 slots of 16 B).
//       The 16 lanes read chunks k = 0 … 7 of TWO columns, b and b + 8 (bit 3
//       of b clear, so f(b) = f(b + 8)). Slot = (9 col + (k ^ f)) mod 16: the
//       8 chunks of column b fill 9 b + {0 … 7}, those of b + 8 fill 9 b + 72
//       + {0 … 7} ≡ 9 b + 8 + {0 … 7}: 16 distinct slots. (Two NEIGHBOURING
//       columns would collide once: 9 b + 9 + 7 ≡ 9 b.)
//     Bank-conflict counters: not measured.
//
// GEMM: out[N, K] (=|+=) sa[n]·sb[k]·Σ_m A8[n, m]·B8[k, m]
//
//  gemm_fp8_kernel's tile, fragments, swizzled image and DMA ring (fp8_mma.h),
//  with the contraction Mp a multiple of 128 (no half step). dW is small and
//  the contraction long, so the grid is tiles x S: workgroup (tile, s) runs
//  the contiguous k-steps [s·q + min(s, r), + q + (s < r)), q = KT / S, r =
//  KT % S. S == 1: the epilogue multiplies by sa[n], then sb[k], and stores or
//  adds into out. S > 1: raw fp32 accumulators go to slab s of an [S, N, K]
//  workspace (never zeroed: every element of every slab is written), and
//  fp8_wgrad_reduce_kernel sums the slabs in the order s = 0 … S − 1, scales,
//  and stores or adds. out is read-modify-written by exactly one thread; no
//  atomics anywhere: two runs give the same bits.
//  Output: a lane holds 4 consecutive columns of a row per accumulator quad and
//  stores them as one 16-B float4 straight from registers (a half-wave covers
//  32 rows x 32 B); the ring is not reused, so there is no closing barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>

#include "bf16_vec.h"
#include "fp8_kernels.h"
#include "fp8_mma.h"

namespace dcp {
namespace kern {
namespace {

using namespace fp8dev;

// ----------------------------------------------------- column quantiser ----
constexpr int kQC = 64;       // columns per block
constexpr int kQR = 128;      // rows per quantise tile = the GEMM's k-step
constexpr int kPitch = 144;   // image bytes per column: 128 m-bytes + 16 pad
constexpr int kMaxSlabs = 32; // row slabs of the amax pass
// the smallest normal fp32: a column of bf16 subnormals alone (amax < fmt_max · 2^-126) would get a subnormal
// scale, whose few bits put s · fmt_max visibly below amax
constexpr float kMinScale = 1.17549435e-38f;

__global__ void __launch_bounds__(256) fp8_col_amax_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                           float* __restrict__ part, int64_t M, int C, int64_t SR) {
  __shared__ __attribute__((aligned(16))) float red[32][kQC];
  const int t = threadIdx.x, cl = t & 7, rl = t >> 3;
  const int c0 = blockIdx.x * kQC;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * SR;
  const int64_t r1 = r0 + SR < M ? r0 + SR : M;
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const uint16_t* p = x + c0 + 8 * cl;
#pragma unroll 4
  for (int64_t r = r0 + rl; r < r1; r += 32) {
    const uint4 v = *reinterpret_cast<const uint4*>(p + r * ldx);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[2 * k] = fmaxf(a[2 * k], fabsf(bf_lo(w[k])));
      a[2 * k + 1] = fmaxf(a[2 * k + 1], fabsf(bf_hi(w[k])));
    }
  }
  *reinterpret_cast<float4*>(&red[rl][8 * cl]) = make_float4(a[0], a[1], a[2], a[3]);
  *reinterpret_cast<float4*>(&red[rl][8 * cl + 4]) = make_float4(a[4], a[5], a[6], a[7]);
  __syncthreads();
  if (t < kQC) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) m = fmaxf(m, red[i][t]);
    part[static_cast<int64_t>(blockIdx.y) * C + c0 + t] = m;
  }
}

__device__ __forceinline__ int colswz(int col) { return (col >> 3) & 6; }

template <int FMT>
__global__ void __launch_bounds__(256)
    fp8_quant_cols_t_kernel(const uint16_t* __restrict__ x, int64_t ldx, const float* __restrict__ part, int S,
                            uint8_t* __restrict__ q, float* __restrict__ scale, int64_t M, int64_t Mp, int C) {
  constexpr float kMax = Fp8Max<FMT>::v;
  __shared__ __attribute__((aligned(16))) char img[kQC * kPitch];
  __shared__ __attribute__((aligned(16))) float sc[kQC];
  const int t = threadIdx.x;
  const int c0 = blockIdx.y * kQC;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * kQR;
  if (t < kQC) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a = fmaxf(a, part[static_cast<int64_t>(s) * C + c0 + t]);
    const float sv = a > 0.f ? fmaxf(a / kMax, kMinScale) : 1.f;
    sc[t] = sv;
    if (blockIdx.x == 0) scale[c0 + t] = sv;
  }
  const int cl = t & 7, rg = t >> 3;
  uint4 v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + 4 * rg + i;
    v[i] = m < M ? *reinterpret_cast<const uint4*>(x + m * ldx + c0 + 8 * cl) : make_uint4(0, 0, 0, 0);
  }
  __syncthreads();
  const float4 s0 = *reinterpret_cast<const float4*>(&sc[8 * cl]);
  const float4 s1 = *reinterpret_cast<const float4*>(&sc[8 * cl + 4]);
  const float sj[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  const uint32_t w[4][4] = {{v[0].x, v[0].y, v[0].z, v[0].w},
                            {v[1].x, v[1].y, v[1].z, v[1].w},
                            {v[2].x, v[2].y, v[2].z, v[2].w},
                            {v[3].x, v[3].y, v[3].z, v[3].w}};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float e = (j & 1) ? bf_hi(w[i][j >> 1]) : bf_lo(w[i][j >> 1]);
      f[i] = fminf(fmaxf(e / sj[j], -kMax), kMax);
    }
    const int col = 8 * cl + j;
    *reinterpret_cast<uint32_t*>(img + col * kPitch + 16 * ((rg >> 2) ^ colswz(col)) + 4 * (rg & 3)) =
        cvt4<FMT>(f[0], f[1], f[2], f[3]);
  }
  __syncthreads();
  const int lane = t & 63, wv = t >> 6, k = lane & 7;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int g = (lane >> 4) + 4 * wv + 16 * it;  // 0 … 31: the column pair (b, b + 8)
    const int col = (g & 7) + 16 * (g >> 3) + 8 * ((lane >> 3) & 1);
    const uint4 val = *reinterpret_cast<const uint4*>(img + col * kPitch + 16 * (k ^ colswz(col)));
    *reinterpret_cast<uint4*>(q + static_cast<int64_t>(c0 + col) * Mp + m0 + 16 * k) = val;
  }
}

// ----------------------------------------------------------------- GEMM ----
constexpr int kCUs = 256;

// MODE 0: out = acc·sa[n]·sb[k]; 1: out += the same; 2: raw accumulators into
// slab blockIdx-split of out ([S, N, K], ldo == K)
template <int AFMT, int MODE>
__global__ void __launch_bounds__(kT, 2)
    gemm_fp8_wgrad_kernel(const uint8_t* __restrict__ A, const float* __restrict__ sa, const uint8_t* __restrict__ B,
                          const float* __restrict__ sb, float* __restrict__ out, int N, int K, int64_t Mp, int64_t ldo,
                          int tiles, int tiles_k, int S) {
  __shared__ __attribute__((aligned(16))) char lds[2 * kStage];  // 64 KiB
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int l31 = lane & 31, hh = lane >> 5;

  // the tiles of one split are neighbours (they share operand rows in an XCD's L2)
  const int v = xcd_remap(static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x));
  const int sp = v / tiles, tile = v % tiles;
  const int n0 = (tile / tiles_k) * kBM;
  const int k0 = (tile % tiles_k) * kBN;
  const int KT = static_cast<int>(Mp / kBK);
  const int qs = KT / S, rs = KT % S;
  const int kt0 = sp * qs + (sp < rs ? sp : rs);
  const int nk = qs + (sp < rs ? 1 : 0);  // >= 1: S <= KT

  // per-lane source byte offsets within the tile's 128-row slab (gemm_fp8.hip)
  auto src_off = [&](int j, bool isb) -> uint32_t {
    const int i = (4 * w + j) * 8 + (lane >> 3);  // image row
    const int lc = (lane & 7) ^ swz(i);           // logical chunk behind physical chunk lane % 8
    const int64_t r = isb ? (k0 + i < K ? i : K - 1 - k0) : (n0 + i < N ? i : N - 1 - n0);
    return static_cast<uint32_t>(r * Mp + lc * 16);
  };
  uint32_t offa[4], offb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    offa[j] = src_off(j, false);
    offb[j] = src_off(j, true);
  }
  const uint8_t* abase = A + static_cast<int64_t>(n0) * Mp + static_cast<int64_t>(kt0) * kBK;
  const uint8_t* bbase = B + static_cast<int64_t>(k0) * Mp + static_cast<int64_t>(kt0) * kBK;
  auto issue = [&](int i) {
    char* slot = lds + (i & 1) * kStage + 4 * w * 1024;
    const uint8_t* ak = abase + static_cast<int64_t>(i) * kBK;
    const uint8_t* bk = bbase + static_cast<int64_t>(i) * kBK;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      glds16s(ak, offa[j], slot + j * 1024);
      glds16s(bk, offb[j], slot + kTile + j * 1024);
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
  for (int i = 0; i < nk; ++i) {
    wait_vm0();
    barrier();
    if (i + 1 < nk) issue(i + 1);
    const char* ia = lds + (i & 1) * kStage;
    const char* ib = ia + kTile;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      i32x8 fa[2], fb[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        fa[u] = frag(ia, wr * 64 + u * 32 + l31, s, hh);
        fb[u] = frag(ib, wc * 64 + u * 32 + l31, s, hh);
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fb[ni], fa[mi], acc[mi][ni], FP8_E4M3, AFMT, 0,
                                                                        kUnit, 0, kUnit);
    }
  }

  // acc[mi][ni][4 g + e] is row 32 mi + l31, column 32 ni + 8 g + 4 hh + e of
  // the wave's block
  float* dst = out;
  if constexpr (MODE == 2) dst += static_cast<int64_t>(sp) * N * ldo;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int n = n0 + wr * 64 + mi * 32 + l31;
    float san = 1.f;
    if constexpr (MODE != 2) san = sa[n < N ? n : N - 1];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k = k0 + wc * 64 + ni * 32 + 8 * g + 4 * hh;
        if (n >= N || k >= K) continue;
        float4 c = make_float4(acc[mi][ni][4 * g + 0], acc[mi][ni][4 * g + 1], acc[mi][ni][4 * g + 2],
                               acc[mi][ni][4 * g + 3]);
        float4* o = reinterpret_cast<float4*>(dst + static_cast<int64_t>(n) * ldo + k);
        if constexpr (MODE != 2) {
          const float4 sbk = *reinterpret_cast<const float4*>(sb + k);
          c = make_float4(c.x * san * sbk.x, c.y * san * sbk.y, c.z * san * sbk.z, c.w * san * sbk.w);
        }
        if constexpr (MODE == 1) {
          const float4 old = *o;
          c = make_float4(old.x + c.x, old.y + c.y, old.z + c.z, old.w + c.w);
        }
        *o = c;
      }
  }
}

// out[n, k] (=|+=) sa[n]·sb[k]·Σ_s ws[s][n][k], s ascending; a float4 per thread
template <bool ACC>
__global__ void __launch_bounds__(256)
    fp8_wgrad_reduce_kernel(const float* __restrict__ ws, int S, const float* __restrict__ sa,
                            const float* __restrict__ sb, float* __restrict__ out, int N, int K, int64_t ldo) {
  const int k4 = K >> 2;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= static_cast<int64_t>(N) * k4) return;
  const int n = static_cast<int>(idx / k4), k = static_cast<int>(idx % k4) * 4;
  const int64_t slab = static_cast<int64_t>(N) * K;
  const float* p = ws + static_cast<int64_t>(n) * K + k;
  float4 c = *reinterpret_cast<const float4*>(p);
  for (int s = 1; s < S; ++s) {
    const float4 d = *reinterpret_cast<const float4*>(p + s * slab);
    c = make_float4(c.x + d.x, c.y + d.y, c.z + d.z, c.w + d.w);
  }
  const float san = sa[n];
  const float4 sbk = *reinterpret_cast<const float4*>(sb + k);
  c = make_float4(c.x * san * sbk.x, c.y * san * sbk.y, c.z * san * sbk.z, c.w * san * sbk.w);
  float4* o = reinterpret_cast<float4*>(out + static_cast<int64_t>(n) * ldo + k);
  if constexpr (ACC) {
    const float4 old = *o;
    c = make_float4(old.x + c.x, old.y + c.y, old.z + c.z, old.w + c.w);
  }
  *o = c;
}

template <int AFMT>
void wgrad_launch(const void* A8, const float* sa, const void* B8, const float* sb, float* out, int N, int K,
                  int64_t Mp, int64_t ldo, bool accumulate, int S, float* ws, hipStream_t s) {
  const int tiles_k = (K + kBN - 1) / kBN;
  const int tiles = ((N + kBM - 1) / kBM) * tiles_k;
  const unsigned grid = static_cast<unsigned>(tiles) * static_cast<unsigned>(S);
  const uint8_t* a = static_cast<const uint8_t*>(A8);
  const uint8_t* b = static_cast<const uint8_t*>(B8);
  if (S == 1) {
    if (accumulate)
      gemm_fp8_wgrad_kernel<AFMT, 1><<<grid, kT, 0, s>>>(a, sa, b, sb, out, N, K, Mp, ldo, tiles, tiles_k, 1);
    else
      gemm_fp8_wgrad_kernel<AFMT, 0><<<grid, kT, 0, s>>>(a, sa, b, sb, out, N, K, Mp, ldo, tiles, tiles_k, 1);
    return;
  }
  gemm_fp8_wgrad_kernel<AFMT, 2><<<grid, kT, 0, s>>>(a, sa, b, sb, ws, N, K, Mp, K, tiles, tiles_k, S);
  const unsigned rgrid = static_cast<unsigned>((static_cast<int64_t>(N) * (K >> 2) + 255) / 256);
  if (accumulate)
    fp8_wgrad_reduce_kernel<true><<<rgrid, 256, 0, s>>>(ws, S, sa, sb, out, N, K, ldo);
  else
    fp8_wgrad_reduce_kernel<false><<<rgrid, 256, 0, s>>>(ws, S, sa, sb, out, N, K, ldo);
}

}  // namespace

int64_t fp8_cols_padded(int64_t M) { return (M + kQR - 1) / kQR * kQR; }

int fp8_quant_cols_slabs(int64_t M) {
  return static_cast<int>(std::min<int64_t>(kMaxSlabs, (M + kQR - 1) / kQR));
}

void fp8_quant_cols_t(const void* x, int64_t ldx, void* q, float* scale, float* part, int64_t M, int C, int fmt,
                      hipStream_t s) {
  if (M < 1 || M >= (int64_t(1) << 31) || C < kQC || C % kQC != 0 || C / kQC > 65535 || ldx < C || ldx % 8 != 0 ||
      (fmt != FP8_E4M3 && fmt != FP8_E5M2))
    throw std::invalid_argument("fp8_quant_cols_t: unsupported shape or format");
  const int S = fp8_quant_cols_slabs(M);
  const int64_t SR = (M + S - 1) / S;
  const int64_t Mp = fp8_cols_padded(M);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  fp8_col_amax_kernel<<<dim3(C / kQC, S), 256, 0, s>>>(xp, ldx, part, M, C, SR);
  const dim3 grid(static_cast<unsigned>(Mp / kQR), C / kQC);
  if (fmt == FP8_E4M3)
    fp8_quant_cols_t_kernel<FP8_E4M3><<<grid, 256, 0, s>>>(xp, ldx, part, S, static_cast<uint8_t*>(q), scale, M, Mp, C);
  else
    fp8_quant_cols_t_kernel<FP8_E5M2><<<grid, 256, 0, s>>>(xp, ldx, part, S, static_cast<uint8_t*>(q), scale, M, Mp, C);
}

bool gemm_fp8_wgrad_supported(int64_t N, int64_t K, int64_t M) {
  // Mp <= 2^24: the DMA's per-lane offset within a 128-row slab, 127·Mp + 127, stays below 2^31
  const int64_t lim = int64_t(1) << 20;
  return M >= 1 && fp8_cols_padded(M) <= (int64_t(1) << 24) && N >= 64 && N % 64 == 0 && N <= lim && K >= 64 &&
         K % 64 == 0 && K <= lim;
}

int gemm_fp8_wgrad_splits(int64_t N, int64_t K, int64_t Mp) {
  const int64_t tiles = ((N + kBM - 1) / kBM) * ((K + kBN - 1) / kBN);
  const int64_t KT = Mp / kBK;
  // The time model of gemm_pp_splitk, not timed for this kernel: rounds of one
  // workgroup per CU x k-steps per split (~0.5 us per 128^3 fp8 k-step), plus
  // the slabs' fp32 write and read back at ~4 TB/s and one more launch. It
  // lands at one to two resident rounds (2 workgroups per CU) where dW is
  // small and at S = 1 from 256 tiles up.
  if (tiles >= kCUs) return 1;
  const double kt_us = 0.5, bw = 4.0e6;  // bytes per us
  auto cost = [&](int64_t S) {
    const int64_t rounds = (tiles * S + kCUs - 1) / kCUs;
    const double slabs = S > 1 ? (S * 8.0 * N * K) / bw + 4.0 : 0.0;
    return static_cast<double>(rounds) * ((KT + S - 1) / S) * kt_us + slabs;
  };
  int best = 1;
  double bc = cost(1);
  for (int64_t S = 2; S <= 32 && S <= KT && tiles * S <= 2 * kCUs; ++S) {
    const double c = cost(S);
    if (c < bc) {
      bc = c;
      best = static_cast<int>(S);
    }
  }
  return best;
}

void gemm_fp8_wgrad_f32(const void* A8, const float* sa, const void* B8, const float* sb, float* out, int N, int K,
                        int64_t Mp, int64_t ldo, int a_fmt, bool accumulate, int S, float* ws, hipStream_t s) {
  const int64_t tiles = (static_cast<int64_t>(N + kBM - 1) / kBM) * ((K + kBN - 1) / kBN);
  if (!gemm_fp8_wgrad_supported(N, K, Mp) || Mp % kBK != 0 || ldo < K || ldo % 4 != 0 ||
      (a_fmt != FP8_E4M3 && a_fmt != FP8_E5M2) || S < 1 || S > Mp / kBK || tiles * S >= (int64_t(1) << 31) ||
      (S > 1 && ws == nullptr))
    throw std::invalid_argument("gemm_fp8_wgrad_f32: unsupported shape, format or split");
  if (a_fmt == FP8_E4M3)
    wgrad_launch<FP8_E4M3>(A8, sa, B8, sb, out, N, K, Mp, ldo, accumulate, S, ws, s);
  else
    wgrad_launch<FP8_E5M2>(A8, sa, B8, sb, out, N, K, Mp, ldo, accumulate, S, ws, s);
}

}  // namespace kern
}  // namespace dcp
