// Torch wrappers + bindings of the fp8 kernels: the row quantiser and the
// row-scaled fp8 GEMM (kernels/gemm_fp8.hip), the transposing column quantiser
// and the split-K fp32 weight-gradient GEMM (kernels/gemm_fp8_wgrad.hip).
// Kernel launches on the current stream only: no host sync, no memset / memcpy
// (graph-capturable).
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

bool gemm_fp8_wgrad_ok(int64_t N, int64_t K, int64_t M) { return kern::gemm_fp8_wgrad_supported(N, K, M); }

// x [M, C] bf16 (unit last stride, any row stride) -> (q [C, Mp] float8, scale [C] fp32):
// one scale per column, the output transposed and zero-padded to Mp = ceil(M / 128) · 128
std::vector<at::Tensor> fp8_quant_cols_t(const at::Tensor& x, int64_t fmt) {
  const at::ScalarType qt = fp8_dtype(fmt);
  DK_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2, "fp8_quant_cols_t: bf16 [M, C] GPU tensor");
  const int64_t M = x.size(0), C = x.size(1);
  DK_CHECK(M >= 1 && M < (int64_t(1) << 31) && C >= 64 && C % 64 == 0 && C / 64 <= 65535,
           "fp8_quant_cols_t: needs 1 <= M < 2^31 rows and a multiple of 64 columns; got ", M, " x ", C);
  DK_CHECK(x.stride(1) == 1 && (M <= 1 || (x.stride(0) >= C && x.stride(0) % 8 == 0)) && aligned16(x),
           "fp8_quant_cols_t: unit last stride, 16-byte aligned non-overlapping rows required");
  c10::hip::HIPGuard guard(x.device().index());
  const int64_t Mp = kern::fp8_cols_padded(M);
  at::Tensor q = at::empty({C, Mp}, x.options().dtype(qt));
  at::Tensor sc = at::empty({C}, x.options().dtype(at::kFloat));
  at::Tensor part = at::empty({kern::fp8_quant_cols_slabs(M), C}, x.options().dtype(at::kFloat));
  const int64_t ldx = M <= 1 ? C : x.stride(0);
  kern::fp8_quant_cols_t(x.data_ptr(), ldx, q.data_ptr(), sc.data_ptr<float>(), part.data_ptr<float>(), M,
                         static_cast<int>(C), static_cast<int>(fmt), stream_of(x));
  return {q, sc};
}

// sa[n] · sb[k] · (a8 [N, Mp] · b8 [K, Mp]ᵀ) -> fp32 [N, K], stored, or added into accumulate_into
at::Tensor gemm_fp8_wgrad(const at::Tensor& a8, const at::Tensor& sa, const at::Tensor& b8, const at::Tensor& sb,
                          int64_t a_fmt, const c10::optional<at::Tensor>& accumulate_into, int64_t splits) {
  check_operand(a8, sa, a_fmt, a8, "gemm_fp8_wgrad: a");
  check_operand(b8, sb, kern::FP8_E4M3, a8, "gemm_fp8_wgrad: b");
  const int64_t N = a8.size(0), Mp = a8.size(1), K = b8.size(0);
  DK_CHECK(b8.size(1) == Mp, "gemm_fp8_wgrad: a [N, Mp] and b [K, Mp] disagree on Mp");
  DK_CHECK(Mp >= 128 && Mp % 128 == 0 && kern::gemm_fp8_wgrad_supported(N, K, Mp),
           "gemm_fp8_wgrad: needs N % 64 == 0, K % 64 == 0 (at most 2^20), Mp % 128 == 0, Mp <= 2^24; got ", N, " x ",
           K, " x ", Mp);
  DK_CHECK(splits >= 0 && splits <= Mp / 128, "gemm_fp8_wgrad: splits must be 0 (auto) or at most Mp / 128 = ",
           Mp / 128, "; got ", splits);
  const bool acc = accumulate_into.has_value() && accumulate_into->defined();
  if (acc) {
    const at::Tensor& t = *accumulate_into;
    DK_CHECK(t.is_cuda() && t.device() == a8.device() && t.scalar_type() == at::kFloat && t.dim() == 2 &&
                 t.size(0) == N && t.size(1) == K && t.is_contiguous() && aligned16(t),
             "gemm_fp8_wgrad: accumulate_into must be a contiguous fp32 [N, K] tensor on a's device");
  }
  c10::hip::HIPGuard guard(a8.device().index());
  at::Tensor out = acc ? *accumulate_into : at::empty({N, K}, a8.options().dtype(at::kFloat));
  const int S = splits > 0 ? static_cast<int>(splits) : kern::gemm_fp8_wgrad_splits(N, K, Mp);
  at::Tensor ws;
  if (S > 1) ws = at::empty({S, N, K}, a8.options().dtype(at::kFloat));
  kern::gemm_fp8_wgrad_f32(a8.data_ptr(), sa.data_ptr<float>(), b8.data_ptr(), sb.data_ptr<float>(),
                           out.data_ptr<float>(), static_cast<int>(N), static_cast<int>(K), Mp, K,
                           static_cast<int>(a_fmt), acc, S, S > 1 ? ws.data_ptr<float>() : nullptr, stream_of(a8));
  return out;
}

void bind(pybind11::module& m) {
  namespace py = pybind11;
  m.def("gemm_fp8_wgrad_ok", &gemm_fp8_wgrad_ok, "shapes gemm_fp8_wgrad takes: dW [N, K] over M tokens", py::arg("N"),
        py::arg("K"), py::arg("M"));
  m.def("gemm_fp8_wgrad_splits", [](int64_t N, int64_t K, int64_t Mp) { return kern::gemm_fp8_wgrad_splits(N, K, Mp); },
        "split count gemm_fp8_wgrad picks at splits = 0 (1 = none)");
  m.def("fp8_quant_cols_t", &fp8_quant_cols_t,
        "column-wise fp8 quantisation of bf16 [M, C], transposed -> (q [C, Mp], scale [C])", py::arg("x"),
        py::arg("fmt"));
  m.def("gemm_fp8_wgrad", &gemm_fp8_wgrad, "column-scaled split-K fp8 MFMA GEMM -> fp32 [N, K]", py::arg("a8"),
        py::arg("sa"), py::arg("b8"), py::arg("sb"), py::arg("a_fmt"), py::arg("accumulate_into") = py::none(),
        py::arg("splits") = 0);
  m.def("gemm_fp8_ok", &gemm_fp8_ok);
  m.def("fp8_quant_rows", &fp8_quant_rows, "row-wise fp8 quantisation of bf16 [R, K] -> (q, scale)", py::arg("x"),
        py::arg("fmt"));
  m.def("gemm_fp8", &gemm_fp8, "row-scaled fp8 MFMA GEMM -> bf16 [M, N]", py::arg("a8"), py::arg("sa"),
        py::arg("b8"), py::arg("sb"), py::arg("bias"), py::arg("a_fmt"));
}

}  // namespace fp8
}  // namespace dcp
