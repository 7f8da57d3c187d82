// Torch wrappers + bindings of the Llama-style decoder block kernels:
// RMSNorm (kernels/rmsnorm.hip), rotary embedding on the packed qkv
// projection (kernels/rope.hip), SwiGLU on the packed gate|up projection
// (kernels/swiglu.hip). Every op is kernel launches on the current stream
// only: no host sync, no memset / memcpy, so each can be graph-captured.
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "kernels/llama_kernels.h"

namespace dcp {
namespace llama {

namespace {

hipStream_t stream_of(const at::Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

int act_dtype(const at::Tensor& x, const char* what) {
  if (x.scalar_type() == at::kBFloat16) return kern::LN_BF16;
  if (x.scalar_type() == at::kFloat) return kern::LN_F32;
  throw Error(str_cat(what, ": unsupported dtype ", c10::toString(x.scalar_type())));
}

bool aligned16(const at::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

void check_weight(const at::Tensor& w, int64_t D, const at::Tensor& x, const char* what) {
  DK_CHECK(w.is_cuda() && w.device() == x.device() && w.scalar_type() == at::kFloat && w.is_contiguous() &&
               w.numel() == D && aligned16(w),
           what, ": weight must be a contiguous fp32 [D] tensor on x's device");
}

}  // namespace

bool rms_norm_supported(int64_t D) { return D > 0 && D <= 4096 && kern::rms_supported(static_cast<int>(D)); }

// x: [..., D] contiguous. Returns (y, rstd) with rstd [rows] fp32.
// out_dtype: y's dtype (default x's; fp32 x -> bf16 y for autocast).
std::vector<at::Tensor> rms_norm_fwd(const at::Tensor& x, const at::Tensor& weight, double eps,
                                     c10::optional<at::ScalarType> out_dtype) {
  DK_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 1 && aligned16(x),
           "rms_norm_fwd: contiguous 16-B aligned device tensor required");
  const int64_t D = x.size(-1);
  DK_CHECK(rms_norm_supported(D), "rms_norm_fwd: D must be a multiple of 8 and <= 4096");
  check_weight(weight, D, x, "rms_norm_fwd");
  c10::hip::HIPGuard guard(x.device().index());
  const int64_t rows = x.numel() / D;
  at::Tensor y = at::empty_like(x, x.options().dtype(out_dtype.has_value() ? *out_dtype : x.scalar_type()));
  DK_CHECK(!(x.scalar_type() == at::kBFloat16 && y.scalar_type() == at::kFloat),
           "rms_norm_fwd: bf16 input with fp32 output is not supported");
  at::Tensor rstd = at::empty({rows}, x.options().dtype(at::kFloat));
  if (rows)
    kern::rms_forward(act_dtype(x, "rms_norm_fwd"), act_dtype(y, "rms_norm_fwd"), x.data_ptr(),
                      weight.data_ptr<float>(), y.data_ptr(), rstd.data_ptr<float>(), rows, static_cast<int>(D),
                      static_cast<float>(eps), stream_of(x));
  return {y, rstd};
}

// Returns (dx, dweight). With accumulate_into (weight.grad: fp32, contiguous
// [D]) the weight gradient is added into it by the reduction kernel and
// returned undefined. grad_residual: the gradient of x from its other consumer
// (the dual-output form), added into dx inside the kernel.
std::vector<at::Tensor> rms_norm_bwd(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& weight,
                                     const at::Tensor& rstd, const c10::optional<at::Tensor>& accumulate_into,
                                     const c10::optional<at::Tensor>& grad_residual) {
  DK_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 1 && aligned16(x),
           "rms_norm_bwd: contiguous 16-B aligned device tensor required");
  const int64_t D = x.size(-1);
  DK_CHECK(rms_norm_supported(D), "rms_norm_bwd: D must be a multiple of 8 and <= 4096");
  check_weight(weight, D, x, "rms_norm_bwd");
  c10::hip::HIPGuard guard(x.device().index());
  const int64_t rows = x.numel() / D;
  at::Tensor g = dy.contiguous();
  // dy arrives in y's dtype (bf16 when the forward wrote bf16 from fp32 x)
  if (!(x.scalar_type() == at::kFloat && g.scalar_type() == at::kBFloat16) && g.scalar_type() != x.scalar_type())
    g = g.to(x.scalar_type());
  DK_CHECK(g.numel() == x.numel() && g.device() == x.device() && aligned16(g), "rms_norm_bwd: dy must match x");
  DK_CHECK(rstd.is_cuda() && rstd.scalar_type() == at::kFloat && rstd.is_contiguous() && rstd.numel() == rows,
           "rms_norm_bwd: rstd must be a contiguous fp32 [rows] tensor");
  auto fopt = x.options().dtype(at::kFloat);
  at::Tensor dx = at::empty_like(x);
  const bool accum = accumulate_into.has_value() && accumulate_into->defined();
  at::Tensor dw;
  if (accum) {
    dw = *accumulate_into;
    DK_CHECK(dw.is_cuda() && dw.device() == x.device() && dw.scalar_type() == at::kFloat && dw.is_contiguous() &&
                 dw.numel() == D,
             "rms_norm_bwd: accumulate_into must be an fp32 contiguous [D] tensor on x's device");
  } else {
    dw = at::empty({D}, fopt);
  }
  at::Tensor gr;
  if (grad_residual.has_value() && grad_residual->defined()) {
    gr = grad_residual->scalar_type() == x.scalar_type() ? grad_residual->contiguous()
                                                         : grad_residual->to(x.scalar_type()).contiguous();
    DK_CHECK(gr.numel() == x.numel() && gr.device() == x.device() && aligned16(gr),
             "rms_norm_bwd: grad_residual must match x");
  }
  if (rows == 0) {
    if (!accum) dw.zero_();
    return {dx, accum ? at::Tensor() : dw};
  }
  at::Tensor part = at::empty({static_cast<int64_t>(kern::rms_bwd_blocks(rows, static_cast<int>(D))) * D}, fopt);
  kern::rms_backward(act_dtype(x, "rms_norm_bwd"), act_dtype(g, "rms_norm_bwd"), g.data_ptr(), x.data_ptr(),
                     weight.data_ptr<float>(), rstd.data_ptr<float>(), dx.data_ptr(), dw.data_ptr<float>(),
                     part.data_ptr<float>(), rows, static_cast<int>(D), accum, stream_of(x),
                     gr.defined() ? gr.data_ptr() : nullptr);
  return {dx, accum ? at::Tensor() : dw};
}

// qkv: contiguous bf16 [B, T, 3·heads·64]; table: fp32 [T_max, 2, 32] (cos |
// sin per position), T <= T_max. inplace: rotate qkv itself and return it;
// else a new tensor (v copied through). inverse: rotate by −θ (the backward).
at::Tensor rope_qkv(const at::Tensor& qkv, int64_t heads, const at::Tensor& table, bool inverse, bool inplace) {
  DK_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.dim() == 3 && qkv.is_contiguous() &&
               aligned16(qkv),
           "rope_qkv: contiguous 16-B aligned bf16 [B, T, 3*heads*64] device tensor required");
  DK_CHECK(heads > 0 && heads <= 4096 && qkv.size(2) == 3 * heads * 64, "rope_qkv: last dim must be 3*heads*64, got ",
           qkv.size(2), " for ", heads, " heads");
  const int64_t T = qkv.size(1);
  DK_CHECK(table.is_cuda() && table.device() == qkv.device() && table.scalar_type() == at::kFloat &&
               table.is_contiguous() && table.dim() == 3 && table.size(1) == 2 && table.size(2) == 32 &&
               aligned16(table),
           "rope_qkv: table must be a contiguous fp32 [T_max, 2, 32] tensor on qkv's device");
  DK_CHECK(T <= table.size(0), "rope_qkv: sequence length ", T, " exceeds the table's ", table.size(0), " rows");
  DK_CHECK(T < (int64_t(1) << 31), "rope_qkv: sequence too long");
  c10::hip::HIPGuard guard(qkv.device().index());
  at::Tensor out = inplace ? qkv : at::empty_like(qkv);
  if (qkv.numel())
    kern::rope_qkv(qkv.data_ptr(), out.data_ptr(), table.data_ptr<float>(), qkv.size(0) * T, static_cast<int>(T),
                   static_cast<int>(heads), inverse, stream_of(qkv));
  return out;
}

namespace {
void check_swiglu_operand(const at::Tensor& t, const char* what) {
  DK_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() && t.dim() >= 1 && aligned16(t), what,
           ": contiguous 16-B aligned bf16 device tensor required");
}
}  // namespace

bool swiglu_supported(int64_t F) { return F > 0 && F % 8 == 0 && F < (int64_t(1) << 30); }

// packed [..., 2F] (gate | up) -> y [..., F] = silu(gate) · up
at::Tensor swiglu_fwd(const at::Tensor& packed) {
  check_swiglu_operand(packed, "swiglu_fwd");
  DK_CHECK(packed.size(-1) % 2 == 0 && swiglu_supported(packed.size(-1) / 2),
           "swiglu_fwd: last dim must be 2F with F a multiple of 8");
  const int64_t F = packed.size(-1) / 2;
  const int64_t M = packed.numel() / (2 * F);
  c10::hip::HIPGuard guard(packed.device().index());
  auto shape = packed.sizes().vec();
  shape.back() = F;
  at::Tensor y = at::empty(shape, packed.options());
  if (M) kern::swiglu_fwd(packed.data_ptr(), y.data_ptr(), M, static_cast<int>(F), stream_of(packed));
  return y;
}

// (dy [..., F], packed [..., 2F]) -> dpacked [..., 2F] = (d_gate | d_up)
at::Tensor swiglu_bwd(const at::Tensor& dy, const at::Tensor& packed) {
  check_swiglu_operand(packed, "swiglu_bwd");
  check_swiglu_operand(dy, "swiglu_bwd");
  DK_CHECK(packed.size(-1) % 2 == 0 && swiglu_supported(packed.size(-1) / 2),
           "swiglu_bwd: last dim must be 2F with F a multiple of 8");
  const int64_t F = packed.size(-1) / 2;
  const int64_t M = packed.numel() / (2 * F);
  DK_CHECK(dy.size(-1) == F && dy.numel() == M * F && dy.device() == packed.device(),
           "swiglu_bwd: dy must be the [..., F] gradient of the packed input's output");
  c10::hip::HIPGuard guard(packed.device().index());
  at::Tensor dp = at::empty_like(packed);
  if (M) kern::swiglu_bwd(dy.data_ptr(), packed.data_ptr(), dp.data_ptr(), M, static_cast<int>(F), stream_of(packed));
  return dp;
}

void bind(pybind11::module& m) {
  namespace py = pybind11;
  m.def("rms_norm_supported", &rms_norm_supported);
  m.def("rms_norm_fwd", &rms_norm_fwd, "RMSNorm forward -> (y, rstd)", py::arg("x"), py::arg("weight"),
        py::arg("eps"), py::arg("out_dtype") = py::none());
  m.def("rms_norm_bwd", &rms_norm_bwd, "RMSNorm backward -> (dx, dweight)", py::arg("dy"), py::arg("x"),
        py::arg("weight"), py::arg("rstd"), py::arg("accumulate_into") = py::none(),
        py::arg("grad_residual") = py::none());
  m.def("rope_qkv", &rope_qkv, "rotary embedding on the q / k thirds of a packed bf16 [B, T, 3*heads*64] projection",
        py::arg("qkv"), py::arg("heads"), py::arg("table"), py::arg("inverse") = false, py::arg("inplace") = false);
  m.def("swiglu_supported", &swiglu_supported);
  m.def("swiglu_fwd", &swiglu_fwd, "silu(gate) * up on a packed bf16 [..., 2F] projection", py::arg("packed"));
  m.def("swiglu_bwd", &swiglu_bwd, "packed (d_gate | d_up) from dy and the packed input", py::arg("dy"),
        py::arg("packed"));
}

}  // namespace llama
}  // namespace dcp
