// Host-side launch API of the hand-written gfx950 kernels. Every launcher takes
// raw device pointers and the HIP stream; the torch-facing wrappers live in
// csrc/ops.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dcp {
namespace kern {

enum DType : int { F32 = 0, BF16 = 1, F16 = 2 };

// Elements per multi-tensor chunk (one workgroup iteration). Tensor chunk
// counts are prefix-summed on the host; each workgroup binary-searches its
// tensor, so one launch covers an arbitrary tensor list.
constexpr int64_t kChunk = 8192;

// Device-side tensor table, int64 words:
//   [0, n]            chunk prefix (n+1 entries)
//   [n+1, 2n+1)       numel per tensor
//   [2n+1 + d*n ...)  pointer list d (d = 0..depth-1)
struct TableView {
  const int64_t* base;
  int n;
};

// dst_i[k] = cast(scale * src_i[k]); list 0 = src, list 1 = dst.
void mt_copy(TableView t, int64_t nchunks, DType src, DType dst, float scale, hipStream_t s);

// Fused SGD (torch.optim.SGD semantics). lists: 0 param, 1 grad, 2 momentum buffer (optional).
// The complements (one_minus_dampening here, one_minus_beta1 / one_minus_beta2 /
// one_minus_rho below) are computed in double by the caller and rounded once,
// as LambParams::omb1 / omb2: the kernels never form 1.f - x.
void mt_sgd(TableView t, int64_t nchunks, DType p, float lr, float momentum, float dampening,
            float one_minus_dampening, float wd, bool nesterov, bool maximize, bool first_step, bool has_buf,
            float grad_scale, hipStream_t s);

// Fused Adam / AdamW. lists: 0 param, 1 grad, 2 exp_avg, 3 exp_avg_sq, 4 max_exp_avg_sq (amsgrad),
// then (shadow) a bf16 copy of the updated parameter.
void mt_adam(TableView t, int64_t nchunks, DType p, float lr, float beta1, float beta2, float one_minus_beta1,
             float one_minus_beta2, float eps, float wd, float bias_c1, float bias_c2_sqrt, bool amsgrad,
             bool decoupled_wd, bool maximize, float grad_scale, bool shadow, int step_list, hipStream_t s);

// Fused Adadelta. lists: 0 param, 1 grad, 2 square_avg, 3 acc_delta.
void mt_adadelta(TableView t, int64_t nchunks, DType p, float lr, float rho, float one_minus_rho, float eps, float wd,
                 bool maximize, float grad_scale, hipStream_t s);

// Sum of squares per tensor list -> out[0] (fp32, accumulated with atomics
// per workgroup) and non-finite flag out[1]. list 0 = tensors.
// out[1] tests the ELEMENTS, not the sum: it is set to 1 when any element is
// inf or NaN and stays 0 on finite input even where the squares overflow
// (x = 1e30 gives out[0] = inf, out[1] = 0). A caller that must not use an
// overflowed norm checks isfinite(out[0]) as well.
void mt_sumsq(TableView t, int64_t nchunks, DType d, float* out, hipStream_t s);
// embedding.hip: gw[V][D] += per-index sums of g [M][D] (fp32; V <= 8, D % 4 == 0)
bool emb_small_supported(int64_t V, int64_t D);
void emb_small_bwd(const int64_t* idx, const float* g, float* gw, int64_t M, int V, int D, hipStream_t s);

// In-place scale of every tensor: x *= scale_dev[0] (device scalar).
void mt_scale_by(TableView t, int64_t nchunks, DType d, const float* scale_dev, hipStream_t s);

// Layer-wise adaptive optimizers (LAMB / LARS): three launches over one table.
// A norm pass writes two fp32 partial sums per chunk, partials[2c] = Σp² and
// partials[2c + 1] = Σu² (LAMB: u = the Adam-style update; LARS: the scaled
// gradient), indexed by the global chunk number c, so the result does not
// depend on the grid; a reduce pass (one workgroup per tensor, fixed order, no
// atomics) turns them into the tensor's trust ratio, stored through
// `ratio_list`: a table list of one fp32 slot per tensor; the update pass
// reads it back. Every partial and slot is rewritten on each call. A group
// that does not adapt skips the norm pass and gets ratio 1.
struct LambParams {
  float lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale;
  // 1 - beta rounded from double: 1.f - 0.999f is off by 5e-5 relative, which
  // would scale v (and, without bias correction, u) by that much
  float omb1, omb2;
  bool maximize, adapt, shadow;
  // >= 0: table list of per-tensor device fp32 `step` scalars (capturable
  // mode, as mt_adam); < 0: bc1 / bc2_sqrt above are used
  int step_list;
  int ratio_list;
};
// lists: 0 param, 1 grad, 2 exp_avg, 3 exp_avg_sq, then (shadow) a bf16 copy of
// the updated parameter, then the step and ratio lists. clip: optional device
// fp32 scalar multiplied into grad_scale (nullptr = 1). partials: fp32 [2 * nchunks].
void mt_lamb(TableView t, int64_t nchunks, DType p, const LambParams& a, const float* clip, float* partials,
             hipStream_t s);

struct LarsParams {
  float lr, momentum, dampening, wd, grad_scale, trust, eps;
  bool nesterov, maximize, first_step, has_buf, adapt;
  int ratio_list;
};
// lists: 0 param, 1 grad, 2 momentum buffer (has_buf), then the ratio list.
void mt_lars(TableView t, int64_t nchunks, DType p, const LarsParams& a, float* partials, hipStream_t s);

// dst[i] = src[i], i < n, with the words carried in KERNEL ARGUMENTS (src is
// host memory read at launch / capture time; 256 words per launch). Used for
// table uploads inside a HIP-graph capture: a captured memcpy node is not
// reliably ordered before the kernel that reads the table, and a kernel
// node's arguments are stored in the graph itself.
void copy_words(const int64_t* src, int64_t* dst, int64_t n, hipStream_t s);

// Contention emulation of one collective on this GPU (multi_tensor.hip):
// `channels` workgroups move bytes_move bytes from src into scratch (both
// bytes_buf long, wrapping) and hold their CUs until `us` microseconds
// (≤ 50 ms) have passed since they started.
void comm_emulate(const void* src, void* scratch, int64_t bytes_buf, int64_t bytes_move, int channels, double us,
                  hipStream_t s);

// conv3_bwd.hip: backward of a bottleneck's conv3 (1x1, w -> 4w channels, w =
// 64 / 128) with BN3's backward apply as its prologue: dz3 = k1·(g − k2 −
// (z3 − μ3)·k3) (bn_bwd_apply_kernel's expression and rounding; stored once
// for the weight gradient), dy2 [M, w] = dz3 · W3 (wt = W3ᵀ bf16 [w][4w]) and
// the BN2+ReLU backward reduction of gemm_nt's RED epilogue into stats
// (zeroed fp32 [2w]) += (Σg2, Σg2·(x2 − μ2)). acc3 = (Σg, Σg·(z3 − μ3)) [2·4w].
void conv3_bwd_bf16(const void* g, const void* z3, const void* wt, const void* x2, void* dz3, void* dy2, int64_t M,
                    int w, const float* gamma3, const float* mean3, const float* invstd3, const float* acc3,
                    const float* gamma2, const float* beta2, const float* mean2, const float* invstd2, float* stats,
                    hipStream_t s);
// 0 = this shape stays on the unfused path; 1 = conv3_bwd_bf16 (gemm_tune
// "c3bwd" / "c3bwd64" / "c3bwd128"; "c3bwd_grid" caps the persistent grid)
int conv3_bwd_mode(int64_t M, int w);
// The same at a downsample block, relu(bn3(z3) + bn_d(zd)): both BNs' backward
// applies (bn_bwd_apply2_kernel's expressions and rounding) as the prologue;
// dz3 and dzd [M, 4w] are stored once. w = 64: also dxd [M, w] = dzd · Wd, the
// data gradient of the stride-1 downsample conv (wdt = Wdᵀ bf16 [w][4w]);
// w = 128: wdt / dxd unused (nullptr). accd = (Σg, Σg·(zd − μd)) [2·4w].
void conv3_bwd_ds_bf16(const void* g, const void* z3, const void* zd, const void* wt, const void* wdt, const void* x2,
                       void* dz3, void* dzd, void* dy2, void* dxd, int64_t M, int w, const float* gamma3,
                       const float* mean3, const float* invstd3, const float* acc3, const float* gammad,
                       const float* meand, const float* invstdd, const float* accd, const float* gamma2,
                       const float* beta2, const float* mean2, const float* invstd2, float* stats, hipStream_t s);
// 0 = a downsample block of this shape stays on bn_bwd_apply2; 1 = conv3_bwd_ds_bf16
// without dxd (w = 128); 2 = with it (w = 64). gemm_tune "c3bwd_ds" / "c3bwd_ds64" /
// "c3bwd_ds128"; 0 whenever conv3_bwd_mode is
int conv3_bwd_ds_mode(int64_t M, int w);
bool conv3_bwd_tune(const char* key, int value);  // false: not one of its keys
int conv3_bwd_tune_get(const char* key);          // -1: not one of its keys
// dgamma = Σg(x−μ)·invstd, dbeta = Σg from acc = (Σg, Σg·(x − μ)) [2C]
void bn_dparams(const float* acc, const float* invstd, float* dgamma, float* dbeta, int C, hipStream_t s);

// conv1_fwd.hip: forward of a block boundary with the next block's conv1 (1x1,
// K -> N channels; ⟨K, N⟩ = ⟨256, 64⟩, ⟨512, 128⟩, ⟨256, 128⟩) fed from the
// tile that forms y = relu(z3·scale + shift + r), r = res (rscale == nullptr)
// or res·rscale + rshift (the downsample BN inline); bn_apply_kernel's
// expression and rounding. Stores y [M, K], its mask bits (bit k of byte v =
// y[8v + k] > 0), z1 [M, N] = y · wᵀ (w bf16 [N][K]) and gemm_nt's STATS sums
// into stats (zeroed fp32 [2N]) += (Σz1, Σz1²) of the bf16-rounded z1.
void conv1_fwd_bf16(const void* z3, const void* res, const void* w, void* y, uint8_t* bits, void* z1, int64_t M, int K,
                    int N, const float* scale, const float* shift, const float* rscale, const float* rshift,
                    float* stats, hipStream_t s);
// 0 = this shape stays on the unfused path; 1 = conv1_fwd_bf16 (gemm_tune
// "c1fwd" / "c1fwd64" / "c1fwd128" / "c1fwd256x128"; "c1fwd_grid" caps the
// persistent grid)
int conv1_fwd_mode(int64_t M, int K, int N);
bool conv1_fwd_tune(const char* key, int value);  // false: not one of its keys
int conv1_fwd_tune_get(const char* key);          // -1: not one of its keys

}  // namespace kern
}  // namespace dcp
