// Torch wrappers + bindings of the fp8 kernels (kernels/gemm_fp8.hip): the
// row quantiser and the row-scaled fp8 GEMM. Kernel launches on the current
// stream only: no host sync, no memset / memcpy (graph-capturable).
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "kernels/fp8_kernels.h"

namespace dcp {
namespace fp8 {

namespace {

hipStream_t stream_of(const at::Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

bool aligned16(const at::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

at::ScalarType fp8_dtype(int64_t fmt) {
  DK_CHECK(fmt == kern::FP8_E4M3 || fmt == kern::FP8_E5M2, "fp8: format must be 0 (e4m3) or 1 (e5m2)");
  return fmt == kern::FP8_E4M3 ? at::kFloat8_e4m3fn : at::kFloat8_e5m2;
}

// fp8 [rows, K] operand (float8 of the given format, or raw uint8) + fp32 scale [rows]
void check_operand(const at::Tensor& t, const at::Tensor& sc, int64_t fmt, const at::Tensor& ref, const char* what) {
  DK_CHECK(t.is_cuda() && t.device() == ref.device() && t.dim() == 2 && t.is_contiguous() && aligned16(t),
           what, ": contiguous 16-byte aligned [rows, K] tensor on one device required");
  DK_CHECK(t.scalar_type() == fp8_dtype(fmt) || t.scalar_type() == at::kByte, what, ": dtype does not match format");
  DK_CHECK(sc.is_cuda() && sc.device() == ref.device() && sc.scalar_type() == at::kFloat && sc.dim() == 1 &&
               sc.is_contiguous() && sc.size(0) == t.size(0) && aligned16(sc),
           what, ": scale must be a contiguous fp32 [rows] tensor");
}

}  // namespace

bool gemm_fp8_ok(int64_t M, int64_t N, int64_t K) { return kern::gemm_fp8_supported(M, N, K); }

// x [R, K] bf16 (unit last stride, any row stride) -> (q [R, K] float8, scale [R] fp32)
std::vector<at::Tensor> fp8_quant_rows(const at::Tensor& x, int64_t fmt) {
  const at::ScalarType qt = fp8_dtype(fmt);
  DK_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2, "fp8_quant_rows: bf16 [R, K] GPU tensor");
  const int64_t R = x.size(0), K = x.size(1);
  DK_CHECK(K <= 16384 && kern::fp8_quant_supported(static_cast<int>(K)),
           "fp8_quant_rows: K must be a multiple of 16, at most 16384");
  DK_CHECK(x.stride(1) == 1 && (R <= 1 || (x.stride(0) >= K && x.stride(0) % 8 == 0)) && aligned16(x),
           "fp8_quant_rows: unit last stride, 16-byte aligned non-overlapping rows required");
  DK_CHECK(R < (int64_t(1) << 31), "fp8_quant_rows: too many rows");
  c10::hip::HIPGuard guard(x.device().index());
  at::Tensor q = at::empty({R, K}, x.options().dtype(qt));
  at::Tensor sc = at::empty({R}, x.options().dtype(at::kFloat));
  const int64_t ldx = R <= 1 ? K : x.stride(0);
  kern::fp8_quant_rows(x.data_ptr(), ldx, q.data_ptr(), sc.data_ptr<float>(), R, static_cast<int>(K),
                       static_cast<int>(fmt), stream_of(x));
  return {q, sc};
}

// (a8 [M, K] · b8 [N, K]ᵀ) · sa[m] · sb[n] (+ bias[n]) -> bf16 [M, N]
at::Tensor gemm_fp8(const at::Tensor& a8, const at::Tensor& sa, const at::Tensor& b8, const at::Tensor& sb,
                    const c10::optional<at::Tensor>& bias, int64_t a_fmt) {
  check_operand(a8, sa, a_fmt, a8, "gemm_fp8: a");
  check_operand(b8, sb, kern::FP8_E4M3, a8, "gemm_fp8: b");
  const int64_t M = a8.size(0), K = a8.size(1), N = b8.size(0);
  DK_CHECK(b8.size(1) == K, "gemm_fp8: a [M, K] and b [N, K] disagree on K");
  // K <= 2^24 (in gemm_fp8_supported) bounds the DMA's 32-bit per-lane offset
  // within a 128-row slab: 127·K + 127 < 2^31
  DK_CHECK(kern::gemm_fp8_supported(M, N, K), "gemm_fp8: needs M >= 1, N % 64 == 0, K % 64 == 0, K <= 2^24; got ", M,
           " x ", N, " x ", K);
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    DK_CHECK(bias->is_cuda() && bias->device() == a8.device() && bias->scalar_type() == at::kFloat &&
                 bias->dim() == 1 && bias->size(0) == N && bias->is_contiguous() && aligned16(*bias),
             "gemm_fp8: bias must be a contiguous fp32 [N] tensor on a's device");
    bp = bias->data_ptr<float>();
  }
  c10::hip::HIPGuard guard(a8.device().index());
  at::Tensor c = at::empty({M, N}, a8.options().dtype(at::kBFloat16));
  kern::gemm_fp8_bf16(a8.data_ptr(), sa.data_ptr<float>(), b8.data_ptr(), sb.data_ptr<float>(), c.data_ptr(), M,
                      static_cast<int>(N), static_cast<int>(K), N, bp, static_cast<int>(a_fmt), stream_of(a8));
  return c;
}

void bind(pybind11::module& m) {
  namespace py = pybind11;
  m.def("gemm_fp8_ok", &gemm_fp8_ok);
  m.def("fp8_quant_rows", &fp8_quant_rows, "row-wise fp8 quantisation of bf16 [R, K] -> (q, scale)", py::arg("x"),
        py::arg("fmt"));
  m.def("gemm_fp8", &gemm_fp8, "row-scaled fp8 MFMA GEMM -> bf16 [M, N]", py::arg("a8"), py::arg("sa"),
        py::arg("b8"), py::arg("sb"), py::arg("bias"), py::arg("a_fmt"));
}

}  // namespace fp8
}  // namespace dcp
