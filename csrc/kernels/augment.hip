// On-device image augmentation: crop + bilinear resize + horizontal flip +
// per-channel normalise of stored uint8 RGB images, one launch per batch.
//
//   store [M, H, W, 3] uint8, index [N], box [N, 4] = (y0, x0, h, w), flip [N]
//   -> out [N, S, S, 3] bf16 / fp32 (a channels_last [N, 3, S, S] tensor)
//
// Semantics: F.interpolate(crop, (S, S), mode="bilinear", align_corners=False,
// antialias=False), then the flip, then v · a_c + b_c, one rounding to the
// output dtype.
//
// Coordinates are integers. The source coordinate of output column ox in a
// crop of width w is x0 + n / 2S with n = (2·ox' + 1)·w − S (ox' = S−1−ox when
// flipped): floor and remainder of n / 2S are taken in int32 (n > −2S, so the
// floor of a negative n is −1), which makes the neighbour pair exact; the
// weight r / 2S is one correctly rounded fp32 division. Both neighbours are
// clamped into the crop. Rows likewise.
//
// fp32 roundings per element (the k of tests/augment_ref.py): the two weight
// divisions, one fmaf per source row (top, bottom), bottom − top, the fmaf
// between the rows, v · a, + b: 8. A weight of 0 passes the sample through
// exactly, so an identity box gives fl(fl(v · a) + b) bit for bit; the affine
// is never contracted into an fma.
//
// Work: an output row is 3·S contiguous elements; a lane owns a run of 8 of
// them (up to 4 pixels) and keeps the run's column taps (byte offsets of the
// neighbour pair, weight) in registers over kRows rows. A workgroup covers
// 256 / lanes-per-row rows at a time; the row pair and weight are taken once
// per row. Stores are 16 B where the address allows (a full run at a 16-B
// boundary), scalar otherwise: at S = 7 an image is 294 B and a row 42 B, so
// most runs there take the scalar path. Loads are single bytes through the
// caches: a source pixel is read by at most a handful of neighbouring lanes.
#include <hip/hip_runtime.h>

#include "augment_kernels.h"
#include "bf16_vec.h"

namespace dcp {
namespace kern {
namespace {

constexpr int kT = 256;
constexpr int kRows = 8;  // output rows per lane

struct Tap {
  int lo, hi;  // neighbour pair, relative to the crop's origin, inside the crop
  float w;     // weight of hi
};

// output index o in [0, S), crop length len >= 1
__device__ __forceinline__ Tap tap(int o, int len, int S) {
  const int two = 2 * S;
  const int n = (2 * o + 1) * len - S;  // in (−2S, 2S·len)
  const int q = n < 0 ? -1 : static_cast<int>(static_cast<unsigned>(n) / static_cast<unsigned>(two));
  const int r = n - q * two;  // in [0, 2S)
  Tap t;
  t.lo = max(q, 0);            // q <= len − 1 because n / 2S < len − 1/2
  t.hi = min(q + 1, len - 1);
  t.w = static_cast<float>(r) / static_cast<float>(two);
  return t;
}

__device__ __forceinline__ float sel3(float v0, float v1, float v2, int c) { return c == 0 ? v0 : c == 1 ? v1 : v2; }

template <bool BF16>
__global__ void __launch_bounds__(kT) crop_resize_norm_kernel(const uint8_t* __restrict__ store,
                                                              const int64_t* __restrict__ index,
                                                              const int32_t* __restrict__ box,
                                                              const uint8_t* __restrict__ flip, void* __restrict__ out,
                                                              int64_t M, int H, int W, int S, int rl, int tiles,
                                                              int chunks, AugAffine aff) {
#pragma clang fp contract(off)
  const int runs = (3 * S + 7) >> 3;  // runs of 8 per output row
  const int rpb = kT / rl;            // rows the workgroup covers at a time
  unsigned bid = blockIdx.x;
  const int chunk = bid % chunks;
  bid /= chunks;
  const int tile = bid % tiles;
  const int64_t n = bid / tiles;
  const int rs = threadIdx.x / rl;
  const int run = chunk * rl + (threadIdx.x - rs * rl);
  if (rs >= rpb || run >= runs) return;

  // the image and its box, clamped: every read below stays inside store
  const int64_t idx = min(max(index[n], int64_t(0)), M - 1);
  const int y0 = min(max(box[4 * n + 0], 0), H - 1), x0 = min(max(box[4 * n + 1], 0), W - 1);
  const int h = min(max(box[4 * n + 2], 1), H - y0), w = min(max(box[4 * n + 3], 1), W - x0);
  const bool fl = flip[n] != 0;
  const int64_t pitch = static_cast<int64_t>(W) * 3;
  const uint8_t* img = store + idx * H * pitch + y0 * pitch + x0 * 3;

  // column taps of the run's (up to) 4 pixels, then per element
  const int e0 = run * 8;
  const int p0 = e0 / 3, m = e0 - 3 * p0;
  // (named taps, selected with ?: below: an indexed array of them would live in scratch)
  const auto col = [&](int p) {
    const int ox = min(p0 + p, S - 1);  // pixels past the row's end belong to elements that are not stored
    return tap(fl ? S - 1 - ox : ox, w, S);
  };
  const Tap t0 = col(0), t1 = col(1), t2 = col(2), t3 = col(3);
  int off_lo[8], off_hi[8];
  float wx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int t = m + j;
    const int p = (t >= 3) + (t >= 6) + (t >= 9), c = t - 3 * p;
    off_lo[j] = (p == 0 ? t0.lo : p == 1 ? t1.lo : p == 2 ? t2.lo : t3.lo) * 3 + c;
    off_hi[j] = (p == 0 ? t0.hi : p == 1 ? t1.hi : p == 2 ? t2.hi : t3.hi) * 3 + c;
    wx[j] = p == 0 ? t0.w : p == 1 ? t1.w : p == 2 ? t2.w : t3.w;
  }
  float ca[3], cb[3];  // the affine of elements j ≡ 0, 1, 2 (mod 3)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = m + k >= 3 ? m + k - 3 : m + k;
    ca[k] = sel3(aff.a[0], aff.a[1], aff.a[2], c);
    cb[k] = sel3(aff.b[0], aff.b[1], aff.b[2], c);
  }
  const int nv = min(8, 3 * S - e0);  // elements of the run inside the row

  const int row0 = tile * rpb * kRows + rs;
  for (int it = 0; it < kRows; ++it) {
    const int oy = row0 + it * rpb;
    if (oy >= S) break;
    const Tap ty = tap(oy, h, S);
    const uint8_t* r0 = img + ty.lo * pitch;
    const uint8_t* r1 = img + ty.hi * pitch;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int a0 = r0[off_lo[j]], b0 = r0[off_hi[j]], a1 = r1[off_lo[j]], b1 = r1[off_hi[j]];
      const float top = fmaf(wx[j], static_cast<float>(b0 - a0), static_cast<float>(a0));
      const float bot = fmaf(wx[j], static_cast<float>(b1 - a1), static_cast<float>(a1));
      const float val = fmaf(ty.w, bot - top, top);
      v[j] = val * ca[j % 3] + cb[j % 3];
    }
    const int64_t eo = (n * S + oy) * (3 * static_cast<int64_t>(S)) + e0;
    if constexpr (BF16) {
      uint16_t* o = static_cast<uint16_t*>(out) + eo;
      if (nv == 8 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        *reinterpret_cast<uint4*>(o) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]),
                                                  pack2(v[6], v[7]));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < nv) o[j] = static_cast<uint16_t>(pack2(v[j], 0.f) & 0xffffu);
      }
    } else {
      float* o = static_cast<float*>(out) + eo;
      if (nv == 8 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (j < nv) o[j] = v[j];
      }
    }
  }
}

// launch geometry for output side S
struct Plan {
  int rl, tiles, chunks;  // lanes per output row, row tiles, run chunks per row
};

Plan plan(int S) {
  const int runs = (3 * S + 7) / 8;
  Plan p;
  p.rl = runs < kT ? runs : kT;
  const int rows = (kT / p.rl) * kRows;  // rows per workgroup
  p.tiles = (S + rows - 1) / rows;
  p.chunks = (runs + p.rl - 1) / p.rl;
  return p;
}

}  // namespace

int64_t crop_resize_norm_blocks(int64_t N, int S) {
  const Plan p = plan(S);
  return N * p.tiles * p.chunks;
}

void crop_resize_norm(const uint8_t* store, const int64_t* index, const int32_t* box, const uint8_t* flip, void* out,
                      bool out_bf16, int64_t M, int H, int W, int64_t N, int S, AugAffine aff, hipStream_t s) {
  if (N == 0) return;
  const Plan p = plan(S);
  const dim3 grid(static_cast<unsigned>(crop_resize_norm_blocks(N, S)));
  if (out_bf16)
    hipLaunchKernelGGL(crop_resize_norm_kernel<true>, grid, dim3(kT), 0, s, store, index, box, flip, out, M, H, W, S,
                       p.rl, p.tiles, p.chunks, aff);
  else
    hipLaunchKernelGGL(crop_resize_norm_kernel<false>, grid, dim3(kT), 0, s, store, index, box, flip, out, M, H, W, S,
                       p.rl, p.tiles, p.chunks, aff);
}

}  // namespace kern
}  // namespace dcp
