// Flash attention for head dim 128 on gfx950: forward, dQ and dK/dV kernels on
// v_mfma_f32_32x32x16_bf16, bf16 I/O, fp32 online softmax, causal or not. No
// dropout and no key-padding mask (those stay with the head-dim-64 kernels of
// attention.hip).
//
// The design shared with head dim 64 is in attn_mma.h, with its reasons: the
// "swapped" product with one query (forward, dQ) or one key (dK/dV) per lane,
// the accumulator as the B operand of the second product, the 2-deep DMA ring
// of 64-row tiles, the FlashAttention-2 split of the backward with δ produced
// by the dQ kernel, and the causal serpentine work order. The [64][128] tile
// image, its swizzle and the bank argument for it are there too (swz<128>).
//
// What is particular to 128:
//
//  * DMA plan. A tile is 16 KiB = 16 wave-instructions of 1 KiB (4 rows each),
//    4 per wave (TileOff<128>: 4 registers per tensor).
//  * LDS budget. Forward and dQ: ring of 2 × (K | V) = 64 KiB, the static
//    limit exactly. dK/dV: ring of 2 × (Q | dO | lse | δ) = 65 KiB, dynamic
//    LDS (hipFuncAttributeMaxDynamicSharedMemorySize).
//  * Registers. Forward: 8 Q fragments (32) + 4 Oᵀ accumulators (64) + both
//    32-key halves of Sᵀ (32). dQ: Q and dO fragments (64) + 4 dQᵀ
//    accumulators (64) + Sᵀ, dPᵀ of one 32-key half (32). dK/dV: K and V
//    fragments (64) + dKᵀ and dVᵀ over all 128 columns (8 accumulators, 128) +
//    S, dP of one 32-query sub-tile (32): one pass over the Q/dO stream with
//    the whole head dim, one sub-tile in flight, rather than two passes over
//    64 columns each — two passes would recompute S and dP (16 of a sub-tile's
//    32 MFMAs) and stream Q/dO twice, 1.5× the matrix work and 2× the DMA, to
//    buy occupancy that the 65-KiB stage already limits to two workgroups per
//    CU. NOTES §44 has the resource table the compiler reports.
//
// Sliding window (WIN, with CAUSAL only; NOTES §49). Query i attends key j iff
// i − W < j ≤ i, W = Attn128Params::window at run time (0 < W < T: the launch
// functions route everything else to the kernels without window code). The
// band has a second edge, so each kernel gets what the causal edge already
// has, mirrored:
//
//  * a bound of the streamed range: forward and dQ start at the first 64-key
//    block that some query of the 128-query tile can see (it_lo) — the blocks
//    below are never staged; dK/dV ends its query stream after the last tile
//    that can see some key of the 128-key tile;
//  * a wave-uniform skip of staged blocks (32-row sub-tiles in dK/dV) that lie
//    wholly outside the band of this wave's 32 rows;
//  * an elementwise mask on the blocks the edge crosses, and only there.
//
// Tile geometry, LDS image, DMA ring and launch bounds are those of the causal
// kernels. The forward's running max needs one more step (there).
#include <hip/hip_runtime.h>

#include <cmath>

#include "attn_mma.h"

namespace dcp {
namespace kern {
namespace {

using namespace attndev;  // fragments, tile image, DMA plan, work order (attn_mma.h)

constexpr int kT = 256;
constexpr int kD = 128;
constexpr int kKS = kD / 16;          // k-steps of a product over the head dim
constexpr int kDH = kD / 32;          // 32-column accumulators over the head dim
constexpr int kKB = 64;               // rows per LDS tile
constexpr int kTile = kKB * kD * 2;   // 16 KiB
constexpr int kStageKV = 2 * kTile;   // K | V (forward, dQ)
constexpr int kStageQG = 2 * kTile + 2 * kKB * 4;  // Q | dO | lse | δ (dK/dV)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kScale = 0.08838834764831845f;  // 1/sqrt(128), rounded once to fp32

// ------------------------------------------------------------ forward ----
// grid (B*H, ceil(T/128)); wave w of a workgroup owns queries tile·128 + 32w …
// +31, one per lane pair (l, l + 32: the two halves of each 16-wide k-step).
template <bool CAUSAL, bool WIN = false>
__global__ void __launch_bounds__(kT) attn128_fwd_kernel(Attn128Params P, AttnTensor q, AttnTensor k, AttnTensor v,
                                                         AttnOut o, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) char lds[2 * kStageKV];  // [ring][K | V]: 64 KiB
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hh = lane >> 5;
  int bh, tile;
  attn_item(CAUSAL, true, bh, tile);
  const int b = bh / P.H, hd = bh % P.H;
  const int T = P.T;
  const int q0 = tile * 128 + wave * 32;  // this wave's first query
  const int qi = q0 + (lane & 31);        // this lane's query
  const bool qok = qi < T;
  const Ptrs Q = head<kD>(q, b, hd), K = head<kD>(k, b, hd), V = head<kD>(v, b, hd);

  bf16x8 qf[kKS];
  load_row<kD>(Q, qi, qok, hh, qf);
  const float c = kScale * kLog2e;

  float m = -INFINITY, l = 0.f;
  f32x16 oacc[kDH];
#pragma unroll
  for (int dh = 0; dh < kDH; ++dh) oacc[dh] = zero16();
  int nkb = T / kKB;
  if (CAUSAL) nkb = min(nkb, 2 * tile + 2);
  // window: the first block that some query of the tile sees, i.e. the one
  // with key 128·tile − W + 1 of the tile's first query (it_lo ≤ 2·tile < nkb).
  // The ring slot stays it & 1 in issue and consumer alike, whatever it_lo.
  const int W = WIN ? P.window : 0;
  const int it_lo = WIN ? max(0, 128 * tile - W + 1) / kKB : 0;

  const TileOff<kD> ko = tile_off<kD>(K.st, wave, lane), vo = tile_off<kD>(V.st, wave, lane);
  auto issue = [&](int it) {
    if (it >= nkb) return;
    char* base = lds + (it & 1) * kStageKV;
    stage_tile(K.p, K.st, it * kKB, ko, base, wave);
    stage_tile(V.p, V.st, it * kKB, vo, base + kTile, wave);
  };
  issue(it_lo);
  for (int it = it_lo; it < nkb; ++it) {
    wait_vm0();
    barrier();
    issue(it + 1);
    const char* sK = lds + (it & 1) * kStageKV;
    const char* sV = sK + kTile;
    const int kb = it * kKB;
    // a wave of a partial last tile whose queries all lie past T, and (causal)
    // a key block wholly after this wave's last query: DMA and barrier only
    if (q0 >= T) continue;
    if (CAUSAL && kb > q0 + 31) continue;
    // (window) or wholly below the first query's lowest key, hence below every query's
    if (WIN && kb + kKB - 1 < q0 - W + 1) continue;
    f32x16 s[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      s[kh] = zero16();
#pragma unroll
      for (int ks = 0; ks < kKS; ++ks) s[kh] = mfma(row_rd<kD>(sK, 32 * kh + (lane & 31), 2 * ks + hh), qf[ks], s[kh]);
    }
    // s[kh][r]: key kb + 32kh + (r&3) + 8(r>>2) + 4hh, query qi. Raw scores:
    // the max is taken before scaling (c > 0), the scale rides in the
    // exponent's fma. The causal mask only on blocks that reach past the
    // wave's first query (wave-uniform).
    if (CAUSAL && kb + kKB - 1 > q0) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb + 32 * kh + (r & 3) + 8 * (r >> 2) + 4 * hh;
          s[kh][r] = key > qi ? -INFINITY : s[kh][r];
        }
    }
    // the window's lower edge, only on blocks that reach below the lowest key
    // of the wave's last query (with W < 64 a block can take both masks)
    if (WIN && kb <= q0 + 31 - W) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kb + 32 * kh + (r & 3) + 8 * (r >> 2) + 4 * hh;
          s[kh][r] = key <= qi - W ? -INFINITY : s[kh][r];
        }
    }
    float mx = m;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int r = 0; r < 16; r += 2) mx = fmaxf(mx, fmaxf(s[kh][r], s[kh][r + 1]));
    mx = max_xor32(mx);
    // Without a window mx is finite: every wave's first block holds key 0 <= its
    // queries. With one, a wave's first block is visible to its first query but
    // can be wholly hidden from a later one (T 128, W 64, q0 96: block [0, 63]
    // holds key 63 for queries 96…126 and nothing for 127), and that row has
    // mx = m = -inf. Its exponents are then taken against 0, as in
    // attention.hip's key-mask forward: alpha and every p are exp2(-inf) = 0,
    // never (-inf) - (-inf); l stays 0 and O untouched until the row's first
    // visible key. A row's own key is always visible, so the final l > 0.
    float mxs = mx;
    if (WIN) mxs = mx == -INFINITY ? 0.f : mx;
    const float alpha = __builtin_amdgcn_exp2f((m - mxs) * c);
    const float nmc = -mxs * c;
    float rs = 0.f;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[kh][r] = __builtin_amdgcn_exp2f(fmaf(s[kh][r], c, nmc));
        rs += s[kh][r];
      }
    l = l * alpha + sum_xor32(rs);
    m = mx;
    if (!__all(alpha == 1.f)) {  // the running max moved in some lane: rescale O
#pragma unroll
      for (int dh = 0; dh < kDH; ++dh)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dh][r] *= alpha;
    }
    // Oᵀ += Vᵀ·P: the Sᵀ accumulator, packed to bf16, is the B operand
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        const bf16x8 pf = acc_frag(s[kh], sg);
#pragma unroll
        for (int dh = 0; dh < kDH; ++dh) oacc[dh] = mfma(tr_op<kD>(sV, 32 * kh + 16 * sg, 32 * dh, lane), pf, oacc[dh]);
      }
  }
  if (qok) {
    uint16_t* O = static_cast<uint16_t*>(o.ptr) + b * o.sb + hd * kD + static_cast<int64_t>(qi) * o.st;
    store_row<kD>(O, oacc, 1.f / l, hh);
    if (hh == 0) lse[static_cast<int64_t>(bh) * T + qi] = m * c + log2f(l);
  }
}

// --------------------------------------------------------- bwd: dQ -------
// query on the lane (as the forward): Sᵀ = K·Qᵀ, dPᵀ = V·dOᵀ,
// dSᵀ = Pᵀ∘(dPᵀ − δ), dQᵀ += Kᵀ·dSᵀ. δ = rowsum(dO ∘ O) is computed here from
// the query rows' dO (already loaded) and O, and stored for the dK/dV kernel,
// which runs after this one.
template <bool CAUSAL, bool WIN = false>
__global__ void __launch_bounds__(kT) attn128_bwd_dq_kernel(Attn128Params P, AttnTensor q, AttnTensor k,
                                                            AttnTensor v, AttnTensor dout, AttnTensor o,
                                                            const float* __restrict__ lse,
                                                            float* __restrict__ delta, AttnOut dq) {
  __shared__ __attribute__((aligned(16))) char lds[2 * kStageKV];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hh = lane >> 5;
  int bh, tile;
  attn_item(CAUSAL, true, bh, tile);
  const int b = bh / P.H, hd = bh % P.H;
  const int T = P.T;
  const int q0 = tile * 128 + wave * 32;
  const int qi = q0 + (lane & 31);
  const bool qok = qi < T;
  const Ptrs Q = head<kD>(q, b, hd), K = head<kD>(k, b, hd), V = head<kD>(v, b, hd), G = head<kD>(dout, b, hd),
             O = head<kD>(o, b, hd);
  bf16x8 qf[kKS], gf[kKS];
  load_row<kD>(Q, qi, qok, hh, qf);
  load_row<kD>(G, qi, qok, hh, gf);
  float dpart = 0.f;  // this lane's half of the row's 128 products (lanes l, l + 32: one row)
  {
    const uint16_t* po = O.p + static_cast<int64_t>(qok ? qi : 0) * O.st + 8 * hh;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      const uint4 uo = *reinterpret_cast<const uint4*>(po + 16 * ks);
      const uint4 g = __builtin_bit_cast(uint4, gf[ks]);
      const uint32_t aw[4] = {uo.x, uo.y, uo.z, uo.w}, gw[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dpart = fmaf(bf_lo(aw[e]), bf_lo(gw[e]), dpart);
        dpart = fmaf(bf_hi(aw[e]), bf_hi(gw[e]), dpart);
      }
    }
  }
  const float dlt = sum_xor32(dpart);  // 0 for rows past T (gf zeroed)
  const float lse2 = qok ? lse[static_cast<int64_t>(bh) * T + qi] : 0.f;
  if (qok && hh == 0) delta[static_cast<int64_t>(bh) * T + qi] = dlt;
  const float c = kScale * kLog2e;

  f32x16 dacc[kDH];
#pragma unroll
  for (int dh = 0; dh < kDH; ++dh) dacc[dh] = zero16();
  int nkb = T / kKB;
  if (CAUSAL) nkb = min(nkb, 2 * tile + 2);
  // window: the forward's block range, skip and lower-edge mask. No guard of
  // the exponent here: p is taken against the stored lse, which is finite.
  const int W = WIN ? P.window : 0;
  const int it_lo = WIN ? max(0, 128 * tile - W + 1) / kKB : 0;
  const TileOff<kD> ko = tile_off<kD>(K.st, wave, lane), vo = tile_off<kD>(V.st, wave, lane);
  auto issue = [&](int it) {
    if (it >= nkb) return;
    char* base = lds + (it & 1) * kStageKV;
    stage_tile(K.p, K.st, it * kKB, ko, base, wave);
    stage_tile(V.p, V.st, it * kKB, vo, base + kTile, wave);
  };
  issue(it_lo);
  for (int it = it_lo; it < nkb; ++it) {
    wait_vm0();
    barrier();
    issue(it + 1);
    const char* sK = lds + (it & 1) * kStageKV;
    const char* sV = sK + kTile;
    const int kb = it * kKB;
    if (q0 >= T) continue;
    if (CAUSAL && kb > q0 + 31) continue;
    if (WIN && kb + kKB - 1 < q0 - W + 1) continue;  // wholly below every query's lowest key
    // one 32-key half at a time (32 live accumulator registers, not 64)
#pragma unroll 1
    for (int kh = 0; kh < 2; ++kh) {
      // (window) a half wholly outside the band of the wave's queries adds nothing
      if (WIN && (kb + 32 * kh + 31 < q0 - W + 1 || kb + 32 * kh > q0 + 31)) continue;
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < kKS; ++ks) {
        s = mfma(row_rd<kD>(sK, 32 * kh + (lane & 31), 2 * ks + hh), qf[ks], s);
        dp = mfma(row_rd<kD>(sV, 32 * kh + (lane & 31), 2 * ks + hh), gf[ks], dp);
      }
      // causal mask only where this 32-key half reaches past the wave's first query
      const bool diag = CAUSAL && kb + 32 * kh + 31 > q0;
      // and the window's where it reaches below the last query's lowest key
      const bool low = WIN && kb + 32 * kh <= q0 + 31 - W;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb + 32 * kh + (r & 3) + 8 * (r >> 2) + 4 * hh;
        float p = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lse2));
        if (CAUSAL && diag) p = key > qi ? 0.f : p;
        if (WIN && low) p = key <= qi - W ? 0.f : p;
        s[r] = p * (dp[r] - dlt);  // dSᵀ (without the softmax scale)
      }
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        const bf16x8 df = acc_frag(s, sg);
#pragma unroll
        for (int dh = 0; dh < kDH; ++dh) dacc[dh] = mfma(tr_op<kD>(sK, 32 * kh + 16 * sg, 32 * dh, lane), df, dacc[dh]);
      }
    }
  }
  if (qok) {
    uint16_t* D = static_cast<uint16_t*>(dq.ptr) + b * dq.sb + hd * kD + static_cast<int64_t>(qi) * dq.st;
    store_row<kD>(D, dacc, kScale, hh);
  }
}

// ------------------------------------------------------ bwd: dK, dV ------
// key on the lane: S = Q·Kᵀ, dP = dO·Vᵀ (queries in the accumulator rows),
// dVᵀ += dOᵀ·P, dKᵀ += Qᵀ·dS. Q / dO tiles (+ lse, δ) stream through LDS; each
// wave keeps its 32 keys' dKᵀ, dVᵀ over all 128 columns in registers (file
// header: one pass, one 32-query sub-tile in flight).
template <bool CAUSAL, bool WIN = false>
__global__ void __launch_bounds__(kT) attn128_bwd_dkv_kernel(Attn128Params P, AttnTensor q, AttnTensor k,
                                                             AttnTensor v, AttnTensor dout,
                                                             const float* __restrict__ lse,
                                                             const float* __restrict__ delta, AttnOut dk,
                                                             AttnOut dv) {
  extern __shared__ __attribute__((aligned(16))) char lds[];  // [ring][Q | dO | lse | δ]: 2 · kStageQG
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hh = lane >> 5;
  int bh, tile;
  attn_item(CAUSAL, false, bh, tile);
  const int b = bh / P.H, hd = bh % P.H;
  const int T = P.T;
  const int kb0 = tile * 128;
  const int k0 = kb0 + wave * 32;    // this wave's first key
  const int key = k0 + (lane & 31);  // this lane's key
  const bool kok = key < T;
  const Ptrs Q = head<kD>(q, b, hd), K = head<kD>(k, b, hd), V = head<kD>(v, b, hd), G = head<kD>(dout, b, hd);
  bf16x8 kf[kKS], vf[kKS];
  load_row<kD>(K, key, kok, hh, kf);
  load_row<kD>(V, key, kok, hh, vf);
  const float c = kScale * kLog2e;
  const float* L = lse + static_cast<int64_t>(bh) * T;
  const float* DL = delta + static_cast<int64_t>(bh) * T;

  f32x16 dka[kDH], dva[kDH];
#pragma unroll
  for (int dh = 0; dh < kDH; ++dh) {
    dka[dh] = zero16();
    dva[dh] = zero16();
  }
  const int qt0 = CAUSAL ? kb0 / kKB : 0;  // first query tile that can see these keys (kb0 < T: qt0 < nqt)
  int nqt = T / kKB;
  // window: the last query that sees key j is j + W − 1, so the stream ends
  // with the tile that holds it for the tile's last key (issue and the loop
  // below both test against nqt; the new end is at least qt0 + 2)
  const int W = WIN ? P.window : 0;
  if (WIN) nqt = min(nqt, (kb0 + 127 + W - 1) / kKB + 1);
  const TileOff<kD> qo = tile_off<kD>(Q.st, wave, lane), go = tile_off<kD>(G.st, wave, lane);
  auto issue = [&](int it) {
    if (qt0 + it >= nqt) return;
    const int qb = (qt0 + it) * kKB;  // qb + 64 <= T
    char* base = lds + (it & 1) * kStageQG;
    stage_tile(Q.p, Q.st, qb, qo, base, wave);
    stage_tile(G.p, G.st, qb, go, base + kTile, wave);
    if (wave == 0) {
      glds4s(L + qb, lane * 4u, base + 2 * kTile);
      glds4s(DL + qb, lane * 4u, base + 2 * kTile + kKB * 4);
    }
  };
  issue(0);
  for (int it = 0; qt0 + it < nqt; ++it) {
    wait_vm0();
    barrier();
    issue(it + 1);
    const char* sQ = lds + (it & 1) * kStageQG;
    const char* sG = sQ + kTile;
    const float* sL = reinterpret_cast<const float*>(sQ + 2 * kTile);
    const float* sD = sL + kKB;
    const int qb = (qt0 + it) * kKB;
    if (k0 >= T) continue;                    // a wave of a partial last tile: all keys past T
    if (CAUSAL && qb + 63 < k0) continue;     // every query of the tile precedes every key
#pragma unroll 1
    for (int qs = 0; qs < 2; ++qs) {
      if (CAUSAL && qb + 32 * qs + 31 < k0) continue;  // every query precedes every key
      if (WIN && qb + 32 * qs > k0 + 31 + W - 1) continue;  // every query lies past every key's window
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < kKS; ++ks) {
        s = mfma(row_rd<kD>(sQ, 32 * qs + (lane & 31), 2 * ks + hh), kf[ks], s);
        dp = mfma(row_rd<kD>(sG, 32 * qs + (lane & 31), 2 * ks + hh), vf[ks], dp);
      }
      // the mask only where some query of the slice precedes the wave's last key
      const bool diag = CAUSAL && qb + 32 * qs < k0 + 31;
      // the window's edge only where the slice's last query lies past the first key's window
      const bool up = WIN && qb + 32 * qs + 31 >= k0 + W;
      // rows: query qb + 32qs + (r&3) + 8(r>>2) + 4hh; column: this lane's key.
      // P goes into s, dS into dp, in place.
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int rl = 32 * qs + 8 * g + 4 * hh;  // 4 consecutive rows rl … rl+3
        const float4 l4 = *reinterpret_cast<const float4*>(sL + rl);
        const float4 d4 = *reinterpret_cast<const float4*>(sD + rl);
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          float p = __builtin_amdgcn_exp2f(fmaf(s[r], c, -lv[e]));
          if (CAUSAL && diag) p = key > qb + rl + e ? 0.f : p;
          if (WIN && up) p = qb + rl + e >= key + W ? 0.f : p;
          s[r] = p;
          dp[r] = p * (dp[r] - dv4[e]);  // dS (without the softmax scale)
        }
      }
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        const bf16x8 pf = acc_frag(s, sg), df = acc_frag(dp, sg);
#pragma unroll
        for (int dh = 0; dh < kDH; ++dh) {
          dva[dh] = mfma(tr_op<kD>(sG, 32 * qs + 16 * sg, 32 * dh, lane), pf, dva[dh]);
          dka[dh] = mfma(tr_op<kD>(sQ, 32 * qs + 16 * sg, 32 * dh, lane), df, dka[dh]);
        }
      }
    }
  }
  if (kok) {
    uint16_t* DK = static_cast<uint16_t*>(dk.ptr) + b * dk.sb + hd * kD + static_cast<int64_t>(key) * dk.st;
    uint16_t* DV = static_cast<uint16_t*>(dv.ptr) + b * dv.sb + hd * kD + static_cast<int64_t>(key) * dv.st;
    store_row<kD>(DK, dka, kScale, hh);
    store_row<kD>(DV, dva, 1.f, hh);
  }
}

// the windowed instantiations only where the window hides something
bool windowed(const Attn128Params& p) { return p.causal && p.window > 0 && p.window < p.T; }

}  // namespace

bool attn128_supported(int T) { return T > 0 && T % kKB == 0 && T <= 8192; }

void attn128_fwd(const Attn128Params& p, AttnTensor q, AttnTensor k, AttnTensor v, AttnOut o, float* lse,
                 hipStream_t s) {
  const dim3 grid(p.B * p.H, (p.T + 127) / 128);
  if (windowed(p)) hipLaunchKernelGGL((attn128_fwd_kernel<true, true>), grid, dim3(kT), 0, s, p, q, k, v, o, lse);
  else if (p.causal) hipLaunchKernelGGL(attn128_fwd_kernel<true>, grid, dim3(kT), 0, s, p, q, k, v, o, lse);
  else hipLaunchKernelGGL(attn128_fwd_kernel<false>, grid, dim3(kT), 0, s, p, q, k, v, o, lse);
}

namespace {
template <bool CAUSAL, bool WIN = false>
hipError_t bwd_launch(const Attn128Params& p, AttnTensor q, AttnTensor k, AttnTensor v, AttnTensor o, AttnTensor dout,
                      const float* lse, float* delta, AttnOut dq, AttnOut dk, AttnOut dv, hipStream_t s) {
  constexpr int kLds = 2 * kStageQG;  // 65 KiB: above the 64-KiB default
  // (one static per instantiation: the windowed dK/dV kernel gets its own attribute call)
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(attn128_bwd_dkv_kernel<CAUSAL, WIN>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  if (attr != hipSuccess) return attr;
  const dim3 grid(p.B * p.H, (p.T + 127) / 128);
  // dQ first: it computes δ on the way and stores it for dK/dV
  hipLaunchKernelGGL((attn128_bwd_dq_kernel<CAUSAL, WIN>), grid, dim3(kT), 0, s, p, q, k, v, dout, o, lse, delta, dq);
  hipLaunchKernelGGL((attn128_bwd_dkv_kernel<CAUSAL, WIN>), grid, dim3(kT), kLds, s, p, q, k, v, dout, lse, delta, dk,
                     dv);
  return hipSuccess;
}
}  // namespace

hipError_t attn128_bwd(const Attn128Params& p, AttnTensor q, AttnTensor k, AttnTensor v, AttnTensor o,
                       AttnTensor dout, const float* lse, float* delta, AttnOut dq, AttnOut dk, AttnOut dv,
                       hipStream_t s) {
  if (windowed(p)) return bwd_launch<true, true>(p, q, k, v, o, dout, lse, delta, dq, dk, dv, s);
  return p.causal ? bwd_launch<true>(p, q, k, v, o, dout, lse, delta, dq, dk, dv, s)
                  : bwd_launch<false>(p, q, k, v, o, dout, lse, delta, dq, dk, dv, s);
}

}  // namespace kern
}  // namespace dcp
