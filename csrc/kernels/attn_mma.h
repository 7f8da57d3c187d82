// Device building blocks shared by the two flash-attention kernel families:
// attention.hip (head dim 64) and attention_d128.hip (head dim 128). Both are
// built on v_mfma_f32_32x32x16_bf16 with bf16 I/O and an fp32 online softmax.
//
// The shared design (CDNA4, wave64):
//  * "swapped" products: the forward computes Sᵀ = K·Qᵀ so each lane owns one
//    query (its 32 key scores sit in the lane's accumulator registers, the
//    other 32 in lane^32): row max / row sum are in-lane plus ONE cross-lane
//    step (max_xor32 / sum_xor32).
//  * the Sᵀ accumulator is directly the B operand of Oᵀ += Vᵀ·P (accumulator-
//    as-operand, CDNA4 guide §3; acc_frag): no LDS round trip for P; the
//    matching Vᵀ operand is read with ds_read_b64_tr_b16 (hardware transpose,
//    tr_op) from the row-major V tile.
//  * every LDS tile is [64 rows][D bf16] with one XOR swizzle per head dim
//    (swz) that is conflict-free for both the 16-B row reads and the
//    transposed reads.
//  * K/V (or Q/dO) tiles arrive by asynchronous LDS DMA (lds_dma.h) into a
//    2-deep ring, one barrier per tile; the per-lane source offsets of a tile
//    are computed once per tensor (TileOff).
//  * backward = two kernels (FA2 split, no float atomics: two runs give the
//    same bits): dK/dV with the key on the lane (S and dP accumulators feed
//    dVᵀ += dOᵀ·P and dKᵀ += Qᵀ·dS directly), and dQ with the query on the
//    lane (dQᵀ += Kᵀ·dSᵀ), which also produces δ = rowsum(dO ∘ O).
//  * causal: heaviest tiles first, serpentine per round of CUs (attn_item).
// Everything that depends on the head dim is a template on D ∈ {64, 128}; the
// kernels themselves stay with their files.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "attn_kernels.h"
#include "bf16_vec.h"
#include "lds_dma.h"

namespace dcp {
namespace kern {
namespace attndev {

using namespace ldsdma;  // lds_u32, glds16s, glds4s, wait_vm0, barrier

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}
// registers 8s … 8s+7 of an accumulator → bf16 operand fragment of k-step s
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& a, int s) {
  const uint4 u = make_uint4(pack2(a[8 * s + 0], a[8 * s + 1]), pack2(a[8 * s + 2], a[8 * s + 3]),
                             pack2(a[8 * s + 4], a[8 * s + 5]), pack2(a[8 * s + 6], a[8 * s + 7]));
  return __builtin_bit_cast(bf16x8, u);
}

// ---- LDS tile image [64][D] bf16: 16-B chunk c (0 … D/8 - 1) of row r lives
// at r·2D + 16·(c ^ swz<D>(r)).
//
// D = 64: 128-B rows, swz(r) = (((r >> 1) & 1) << 2) | ((r >> 2) & 3). Row
// reads (16 consecutive rows, one chunk) and transposed reads (rows R..R+3 and
// R+4.., chunks 0-3 or 4-7 per 32-lane half, i.e. 4 rows × 32 B per 16-lane
// group) both hit distinct bank slots: the row's parity supplies one bit of
// the bank slot, the swizzle the other three.
//
// D = 128: 256-B rows, so EVERY row starts at bank 0 (64 banks × 4 B) and the
// head-dim-64 image no longer separates rows.
// swz(r) = ((r & 3) << 2) | ((r >> 2) & 3):
//  - row reads (ds_read_b128, served 16 lanes at a time: rows R … R+15, R a
//    multiple of 16, one logical chunk c): swz is a bijection of r & 15 onto
//    0 … 15, so the 16 lanes hit the 16 distinct 16-B slots of the 256-B bank
//    image;
//  - transposed reads (ds_read_b64_tr_b16, served 32 lanes at a time: rows
//    R … R+3, R a multiple of 4, chunks C … C+3, C a multiple of 4, 8 B per
//    lane): slot = (C ^ ((R >> 2) & 3)) ^ (j ^ (q << 2)) for chunk C + j of
//    row R + q — j fills slot bits 0-1 and q slot bits 2-3, 16 distinct slots,
//    each read as its two 8-B halves by two lanes: all 64 banks once.
// The plain r & 15 XOR would serve the row reads but put the four rows of a
// transposed read on the same four slots (a 4-way conflict); swapping the two
// bit pairs serves both.
template <int D>
__device__ __forceinline__ int swz(int r) {
  static_assert(D == 64 || D == 128, "tile images exist for head dim 64 and 128");
  if constexpr (D == 64) return (((r >> 1) & 1) << 2) | ((r >> 2) & 3);
  else return ((r & 3) << 2) | ((r >> 2) & 3);
}
template <int D>
__device__ __forceinline__ int img(int r, int c) {
  return r * (2 * D) + 16 * (c ^ swz<D>(r));
}

template <int D>
__device__ __forceinline__ bf16x8 row_rd(const char* base, int r, int c) {
  return *reinterpret_cast<const bf16x8*>(base + img<D>(r, c));
}

// Operand A[x][row] = tile[row][x] for "A · X" with X an accumulator tile used
// as the B operand: element j of lane l ↔ tile row rbase + 8(j>>2) + 4(l>>5) +
// (j&3), column dcol0 + (l&31) — two ds_read_b64_tr_b16.
template <int D>
__device__ __forceinline__ bf16x8 tr_op(const char* base, int rbase, int dcol0, int lane) {
  const int g = lane >> 4, hh = lane >> 5, q = (lane >> 2) & 3, p = lane & 3;
  const int c0 = dcol0 + 16 * (g & 1);
  const int r0 = rbase + 4 * hh + q;
  const int ch = (c0 >> 3) + (p >> 1);
  const char* a0 = base + img<D>(r0, ch) + 8 * (p & 1);
  const char* a1 = base + img<D>(r0 + 8, ch) + 8 * (p & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a1));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// DMA rows [r0, r0+64) of a strided [T][D] head slice into a tile image: a
// tile is 128·D bytes = D/8 wave-instructions of 1 KiB (512/D rows each), D/32
// per wave. TileOff: this lane's byte offsets within the 64-row slab (row of
// 16-B unit u, swizzled chunk), computed once per tensor (D/32 registers); the
// slab base src + r0 · st is wave-uniform. The caller keeps r0 + 64 <= T, so
// rows r0 … r0+63 and columns 0 … D-1 of the head slice are all that is read.
// Largest offset: (63·st + (D/8 - 1)·8 + 7)·2 B with st < 2^24 elements
// (attn_view's check) is below 2^31, inside the 32-bit offset of the saddr
// form.
template <int D>
struct TileOff {
  uint32_t o[D / 32];
};
template <int D>
__device__ __forceinline__ TileOff<D> tile_off(int64_t st, int wave, int lane) {
  constexpr int N = D / 32;                 // wave-instructions per wave
  constexpr int kLogCh = D == 64 ? 3 : 4;   // D/8 chunks per row
  TileOff<D> t;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int u = (wave * N + j) * 64 + lane;  // 16-B unit of the image
    const int r = u >> kLogCh, lc = (u & (D / 8 - 1)) ^ swz<D>(r);
    t.o[j] = static_cast<uint32_t>((r * st + lc * 8) * 2);
  }
  return t;
}
template <int D>
__device__ __forceinline__ void stage_tile(const uint16_t* src, int64_t st, int r0, const TileOff<D>& to, char* dst,
                                           int wave) {
  constexpr int N = D / 32;
  const uint16_t* base = src + static_cast<int64_t>(r0) * st;
#pragma unroll
  for (int j = 0; j < N; ++j) glds16s(base, to.o[j], dst + (wave * N + j) * 1024);
}

// combine x with the lane 32 apart (lane ^ 32): gfx950's v_permlane32_swap
// (a VALU lane exchange) instead of __shfl_xor's ds_bpermute round trip
// through LDS on the softmax's critical path. With both operands x, the two
// results hold x and its partner in some order in every lane; max / + are
// symmetric, so every lane gets the same combined value
__device__ __forceinline__ float max_xor32(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float sum_xor32(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// (batch-head, tile) of this workgroup. Causal: tiles carry unequal work
// (query tile t of the forward / dQ sees t + 1 key tiles; key tile t of dK/dV
// is seen by nt - t query tiles). Workgroups are dispatched breadth-first, so
// CU c receives launch positions c, c + 256, c + 512, …; with the work items
// sorted heaviest first, odd rounds of 256 take them in reverse (serpentine)
// so every CU's set sums to about the mean instead of heavy + heavy + medium.
// heavy_last: the heaviest tile is the last one (forward, dQ) or tile 0
// (dK/dV). A bijection of the grid.
__device__ __forceinline__ void attn_item(bool causal, bool heavy_last, int& bh, int& tile) {
  const int nbh = static_cast<int>(gridDim.x), nt = static_cast<int>(gridDim.y);
  if (!causal) {
    bh = static_cast<int>(blockIdx.x);
    tile = static_cast<int>(blockIdx.y);
    return;
  }
  const int L = static_cast<int>(blockIdx.y) * nbh + static_cast<int>(blockIdx.x);
  const int G = nbh * nt;
  constexpr int C = 256;
  const int r = L / C, pos = L % C;
  int I = L;
  if (r & 1) {
    const int end = min(G, (r + 1) * C);  // a partial last round reverses within itself
    I = end - 1 - pos;
  }
  bh = I % nbh;
  const int rank = I / nbh;  // 0 = heaviest
  tile = heavy_last ? nt - 1 - rank : rank;
}

struct Ptrs {
  const uint16_t* p;
  int64_t st;
};
template <int D>
__device__ __forceinline__ Ptrs head(const AttnTensor& t, int b, int hd) {
  return Ptrs{static_cast<const uint16_t*>(t.ptr) + b * t.sb + hd * D, t.st};
}

// this lane's row of a head slice as D/16 operand fragments (columns 16ks +
// 8hh … +7); a row past T is read at row 0 (in bounds) and selected to zero.
// Load (row clamped), then select: `ok ? *p : zero` becomes a pointer select
// to a scratch copy of the zero (flat loads + scratch stores)
template <int D>
__device__ __forceinline__ void load_row(const Ptrs& X, int row, bool ok, int hh, bf16x8 (&f)[D / 16]) {
  const uint16_t* p = X.p + static_cast<int64_t>(ok ? row : 0) * X.st + 8 * hh;
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks) {
    const uint4 z = make_uint4(0, 0, 0, 0);
    const uint4 u = *reinterpret_cast<const uint4*>(p + 16 * ks);
    f[ks] = __builtin_bit_cast(bf16x8, ok ? u : z);
  }
}

// acc[dh][4g + e] · sc → columns 32dh + 8g + 4hh + e of this lane's row
template <int D>
__device__ __forceinline__ void store_row(uint16_t* row, const f32x16 (&acc)[D / 32], float sc, int hh) {
#pragma unroll
  for (int dh = 0; dh < D / 32; ++dh)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = 32 * dh + 8 * g + 4 * hh;
      *reinterpret_cast<uint2*>(row + d0) = make_uint2(pack2(acc[dh][4 * g] * sc, acc[dh][4 * g + 1] * sc),
                                                       pack2(acc[dh][4 * g + 2] * sc, acc[dh][4 * g + 3] * sc));
    }
}

}  // namespace attndev
}  // namespace kern
}  // namespace dcp
