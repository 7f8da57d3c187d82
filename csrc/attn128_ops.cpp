// Torch wrappers + bindings of the head-dim-128 flash attention kernels
// (kernels/attention_d128.hip): bf16 [B, T, H*128] views with unit last stride
// (slices of one packed [B, T, 3C] projection are read and written in place),
// causal or not, optionally with a sliding window on the causal mask, no
// dropout, no key-padding mask. Kernel launches on the current stream only: no host sync, no memset / memcpy (graph-capturable).
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <initializer_list>

#include "common.h"
#include "kernels/attn_kernels.h"

namespace dcp {
namespace attn128 {

namespace {

hipStream_t stream_of(const at::Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// the checks of the head-dim-64 op's views: bf16, unit last stride, 16-B
// aligned rows, and a row stride below 2^24 elements — the DMA's per-lane
// byte offset within a 64-row slab is at most (63·st + 127)·2 + 16 < 2^31
kern::AttnTensor view(const at::Tensor& t, const at::Tensor& q, const char* what) {
  DK_CHECK(t.is_cuda() && t.device() == q.device() && t.scalar_type() == at::kBFloat16 && t.dim() == 3 &&
               t.stride(2) == 1,
           what, ": bf16 [B, T, H*128] tensor with unit last stride on q's device required");
  DK_CHECK(t.sizes() == q.sizes(), what, ": shape mismatch");
  DK_CHECK(t.stride(1) % 8 == 0 && t.stride(0) % 8 == 0 && t.stride(1) >= t.size(2) && t.stride(0) >= 0 &&
               reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
           what, ": rows must be 16-byte aligned and must not overlap");
  DK_CHECK(t.stride(1) < (int64_t(1) << 24), what, ": row stride too large (32-bit DMA offsets within a 64-row slab)");
  return kern::AttnTensor{t.data_ptr(), t.stride(0), t.stride(1)};
}
kern::AttnOut out_view(const at::Tensor& t, const at::Tensor& q, const char* what) {
  const kern::AttnTensor v = view(t, q, what);
  return kern::AttnOut{t.data_ptr(), v.sb, v.st};
}

kern::Attn128Params params(const at::Tensor& q, int64_t heads, bool causal, int64_t window) {
  DK_CHECK(q.dim() == 3, "attention (head dim 128): [B, T, H*128] tensors required");
  const int64_t B = q.size(0), T = q.size(1), C = q.size(2);
  DK_CHECK(heads > 0 && C == heads * 128, "attention (head dim 128): last dim must be heads * 128");
  DK_CHECK(kern::attn128_supported(static_cast<int>(T)) && T <= 8192,
           "attention (head dim 128): sequence length must be a multiple of 64, at most 8192");
  DK_CHECK(B > 0 && B * heads < (int64_t(1) << 31) / 64, "attention (head dim 128): batch * heads out of range");
  DK_CHECK(window >= 0, "attention (head dim 128): window must be >= 1, or 0 for none");
  DK_CHECK(window == 0 || causal, "attention (head dim 128): a window requires causal");
  // any window >= T is plain causal attention: T stands for all of them
  return kern::Attn128Params{static_cast<int>(B), static_cast<int>(heads), static_cast<int>(T), causal,
                             static_cast<int>(std::min(window, T))};
}

}  // namespace

bool attn128_ok(int64_t T, int64_t C, int64_t heads) {
  return heads > 0 && C == heads * 128 && T > 0 && T <= 8192 && kern::attn128_supported(static_cast<int>(T));
}

// o [B, T, H*128] (contiguous), lse [B*H, T] fp32 (log2 domain, for the backward)
std::vector<at::Tensor> flash_attn128_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                          int64_t heads, bool causal, int64_t window) {
  const kern::Attn128Params p = params(q, heads, causal, window);
  const kern::AttnTensor vq = view(q, q, "flash_attn128_fwd: q"), vk = view(k, q, "flash_attn128_fwd: k"),
                         vv = view(v, q, "flash_attn128_fwd: v");
  c10::hip::HIPGuard guard(q.device().index());
  at::Tensor o = at::empty(q.sizes(), q.options().memory_format(at::MemoryFormat::Contiguous));
  at::Tensor lse = at::empty({q.size(0) * heads, q.size(1)}, q.options().dtype(at::kFloat));
  kern::attn128_fwd(p, vq, vk, vv, out_view(o, q, "flash_attn128_fwd: o"), lse.data_ptr<float>(), stream_of(q));
  return {o, lse};
}

// writes dq, dk, dv (strided views allowed, e.g. slices of one packed buffer)
void flash_attn128_bwd(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                       const at::Tensor& o, const at::Tensor& lse, int64_t heads, bool causal, at::Tensor& dq,
                       at::Tensor& dk, at::Tensor& dv, int64_t window) {
  const kern::Attn128Params p = params(q, heads, causal, window);
  DK_CHECK(lse.is_cuda() && lse.device() == q.device() && lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
               lse.numel() == q.size(0) * heads * q.size(1),
           "flash_attn128_bwd: lse must be the forward's fp32 [B*H, T] tensor");
  const kern::AttnTensor vq = view(q, q, "flash_attn128_bwd: q"), vk = view(k, q, "flash_attn128_bwd: k"),
                         vv = view(v, q, "flash_attn128_bwd: v"), vo = view(o, q, "flash_attn128_bwd: o"),
                         vg = view(dout, q, "flash_attn128_bwd: dout");
  const kern::AttnOut odq = out_view(dq, q, "flash_attn128_bwd: dq"), odk = out_view(dk, q, "flash_attn128_bwd: dk"),
                      odv = out_view(dv, q, "flash_attn128_bwd: dv");
  c10::hip::HIPGuard guard(q.device().index());
  at::Tensor delta = at::empty_like(lse);
  const hipError_t e = kern::attn128_bwd(p, vq, vk, vv, vo, vg, lse.data_ptr<float>(), delta.data_ptr<float>(), odq,
                                         odk, odv, stream_of(q));
  DK_CHECK(e == hipSuccess, "flash_attn128_bwd: ", hipGetErrorString(e));
}

void bind(pybind11::module& m) {
  namespace py = pybind11;
  m.def("attn128_ok", &attn128_ok);
  m.def("flash_attn128_fwd", &flash_attn128_fwd, "MFMA flash attention forward (head dim 128) -> (o, lse)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("heads"), py::arg("causal"), py::arg("window") = 0);
  m.def("flash_attn128_bwd", &flash_attn128_bwd, "MFMA flash attention backward (head dim 128) into dq/dk/dv",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("lse"), py::arg("heads"),
        py::arg("causal"), py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("window") = 0);
}

}  // namespace attn128
}  // namespace dcp
