// Launch API of the on-device image augmentation kernel (augment.hip): random
// / centre crop, bilinear resize, horizontal flip and per-channel normalise
// of stored uint8 images into the stem's channels_last input, in one pass.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dcp {
namespace kern {

// v · a[c] + b[c] on the resampled 0..255 value: a = 1/(255·std), b = −mean/std
struct AugAffine {
  float a[3];
  float b[3];
};

constexpr int kAugMaxSize = 4096;     // output side S
constexpr int kAugMaxSource = 16384;  // source H, W: (2S+1)·W stays inside int32

// store [M, H, W, 3] uint8; index [N] int64 (rows of store); box [N, 4] int32
// (y0, x0, h, w); flip [N] uint8; out [N, S, S, 3] (the NHWC memory of a
// channels_last [N, 3, S, S] tensor), bf16 when out_bf16 else fp32.
// Boxes are clamped into the image and indices into [0, M): no input value
// makes the kernel read outside store.
void crop_resize_norm(const uint8_t* store, const int64_t* index, const int32_t* box, const uint8_t* flip, void* out,
                      bool out_bf16, int64_t M, int H, int W, int64_t N, int S, AugAffine aff, hipStream_t s);
// workgroups of one launch (the wrapper bounds it: the grid is one-dimensional)
int64_t crop_resize_norm_blocks(int64_t N, int S);

}  // namespace kern
}  // namespace dcp
