// Torch wrapper + binding of the on-device image augmentation kernel
// (kernels/augment.hip): crop, bilinear resize, flip and normalise of stored
// uint8 images into the stem's channels_last input. One kernel launch on the
// current stream: no host sync, no memset / memcpy, so it can be graph-captured.
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "kernels/augment_kernels.h"

namespace dcp {
namespace augment {

// store [M, H, W, 3] uint8; index [N] int64; box [N, 4] int32 (y0, x0, h, w);
// flip [N] uint8 -> [N, 3, size, size] channels_last, bf16 or fp32.
at::Tensor crop_resize_norm(const at::Tensor& store, const at::Tensor& index, const at::Tensor& box,
                            const at::Tensor& flip, int64_t size, const std::vector<double>& mean,
                            const std::vector<double>& std_, at::ScalarType out_dtype) {
  DK_CHECK(store.is_cuda() && store.scalar_type() == at::kByte && store.dim() == 4 && store.is_contiguous() &&
               store.size(3) == 3,
           "crop_resize_norm: store must be a contiguous uint8 [M, H, W, 3] device tensor");
  const int64_t M = store.size(0), H = store.size(1), W = store.size(2);
  DK_CHECK(M >= 1 && H >= 1 && W >= 1 && H <= kern::kAugMaxSource && W <= kern::kAugMaxSource,
           "crop_resize_norm: store needs M >= 1 and 1 <= H, W <= ", kern::kAugMaxSource, ", got [", M, ", ", H, ", ",
           W, ", 3]");
  DK_CHECK(size >= 1 && size <= kern::kAugMaxSize, "crop_resize_norm: size must be in [1, ", kern::kAugMaxSize,
           "], got ", size);
  DK_CHECK(index.device() == store.device() && index.scalar_type() == at::kLong && index.dim() == 1 &&
               index.is_contiguous(),
           "crop_resize_norm: index must be a contiguous int64 [N] tensor on the store's device");
  const int64_t N = index.size(0);
  DK_CHECK(box.device() == store.device() && box.scalar_type() == at::kInt && box.dim() == 2 && box.size(0) == N &&
               box.size(1) == 4 && box.is_contiguous(),
           "crop_resize_norm: box must be a contiguous int32 [N, 4] tensor on the store's device, N = ", N);
  DK_CHECK(flip.device() == store.device() && flip.scalar_type() == at::kByte && flip.dim() == 1 &&
               flip.size(0) == N && flip.is_contiguous(),
           "crop_resize_norm: flip must be a contiguous uint8 [N] tensor on the store's device, N = ", N);
  DK_CHECK(mean.size() == 3 && std_.size() == 3, "crop_resize_norm: mean and std must have 3 entries");
  DK_CHECK(out_dtype == at::kBFloat16 || out_dtype == at::kFloat, "crop_resize_norm: out_dtype must be bf16 or fp32");
  DK_CHECK(kern::crop_resize_norm_blocks(N, static_cast<int>(size)) < (int64_t(1) << 23),
           "crop_resize_norm: batch too large for one launch");
  kern::AugAffine aff;
  for (int c = 0; c < 3; ++c) {
    DK_CHECK(std_[c] > 0, "crop_resize_norm: std must be positive");
    aff.a[c] = static_cast<float>(1.0 / (255.0 * std_[c]));
    aff.b[c] = static_cast<float>(-mean[c] / std_[c]);
  }
  c10::hip::HIPGuard guard(store.device().index());
  at::Tensor out = at::empty({N, 3, size, size}, store.options().dtype(out_dtype), at::MemoryFormat::ChannelsLast);
  kern::crop_resize_norm(store.data_ptr<uint8_t>(), index.data_ptr<int64_t>(), box.data_ptr<int32_t>(),
                         flip.data_ptr<uint8_t>(), out.data_ptr(), out_dtype == at::kBFloat16, M, static_cast<int>(H),
                         static_cast<int>(W), N, static_cast<int>(size), aff,
                         c10::hip::getCurrentHIPStream(store.device().index()).stream());
  return out;
}

void bind(pybind11::module& m) {
  namespace py = pybind11;
  m.def("crop_resize_norm", &crop_resize_norm,
        "crop (box) + bilinear resize + flip + (v/255 - mean)/std of uint8 [M,H,W,3] rows -> channels_last "
        "[N,3,size,size]",
        py::arg("store"), py::arg("index"), py::arg("box"), py::arg("flip"), py::arg("size"), py::arg("mean"),
        py::arg("std"), py::arg("out_dtype"));
}

}  // namespace augment
}  // namespace dcp
