// Launch API of the flash-attention kernels (attention.hip): head dim 64,
// bf16 I/O, fp32 softmax statistics, optional causal mask, optional key-padding
// mask (bit-packed, attn_pack_key_mask) and in-kernel dropout on the attention
// probabilities.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dcp {
namespace kern {

// A [B, T, H*64] bf16 activation with unit element stride: element (b, t, h, d)
// at ptr[b*sb + t*st + h*64 + d]. q/k/v may be slices of one packed [B, T, 3C].
struct AttnTensor {
  const void* ptr;
  int64_t sb, st;
};
struct AttnOut {
  void* ptr;
  int64_t sb, st;
};

// What every kernel reads; the backward kernels take exactly this by value, so
// a field only the forward reads (AttnParams) leaves their kernel arguments,
// and with them their instruction streams, as they are.
struct AttnCoreParams {
  int B, H, T;
  float scale;       // softmax scale (1/sqrt(64))
  bool causal;
  float p_drop;      // dropout probability on P (0 = off)
  // key-padding mask, packed by attn_pack_key_mask: [B][1 + T/64] uint64. Per
  // batch: word 0 = the number of leading 64-key blocks to visit (1 + the
  // index of the last block with a visible key, 0 if none), word 1 + j = key
  // block j (bit i set: key 64j + i takes part). Null: no mask (the
  // kernels without any mask code are launched). (In front of seed and mask,
  // which stay adjacent to each other and to the tensor arguments: the
  // unmasked kernels then keep their instruction streams, kernel-argument
  // offsets aside)
  const uint64_t* kmask;
  uint64_t seed;
  // dropout keep bits, [B*H][T/64][2][T] uint32 (attn_mask_words): written by
  // the forward (unless null: no backward will run), read by the backward;
  // unused when p_drop == 0
  uint32_t* mask;
};

// The forward's parameters (attn_bwd reads the AttnCoreParams part only).
struct AttnParams : AttnCoreParams {
  // device-resident seed offset (one uint64), read by the dropout forward
  // only: its hash runs on seed + *seed_off * 0x9E3779B97F4A7C15 (mod 2^64).
  // Null: no offset. A captured step passes the dropout counter here, so
  // every replay draws new keep decisions although `seed` is frozen into the
  // graph. (Behind mask: the fields above keep their kernel-argument offsets)
  const uint64_t* seed_off;
};

// uint64 words of the packed key mask
inline int64_t attn_kmask_words(int B, int T) { return static_cast<int64_t>(B) * (1 + T / 64); }

// uint32 words of the dropout keep-bit store (T² / 32 per batch-head)
inline int64_t attn_mask_words(int B, int H, int T) {
  return static_cast<int64_t>(B) * H * (T / 64) * 2 * T;
}

bool attn_supported(int T, int D);

// mask [B, T] bytes (non-zero = the key takes part) -> packed [B][1 + T/64]
// (AttnParams::kmask); T a multiple of 64
void attn_pack_key_mask(const uint8_t* mask, uint64_t* packed, int B, int T, hipStream_t s);

// o [B, T, H*64] (strided), lse [B*H, T] fp32 (log2 domain, internal to the backward)
void attn_fwd(const AttnParams& p, AttnTensor q, AttnTensor k, AttnTensor v, AttnOut o, float* lse,
              hipStream_t s);

// delta [B*H, T] fp32 workspace; dq/dk/dv strided outputs
void attn_bwd(const AttnParams& p, AttnTensor q, AttnTensor k, AttnTensor v, AttnTensor o, AttnTensor dout,
              const float* lse, float* delta, AttnOut dq, AttnOut dk, AttnOut dv, hipStream_t s);

}  // namespace kern
}  // namespace dcp
