// Torch op registrations for the mxllm HIP kernels (namespace torch.ops.mxllm).
//
// Kernels live in csrc/kernels/*.hip and expose plain C launchers
// (`mx_*`, taking raw pointers + hipStream_t); this file is the only one that
// includes torch headers, so kernel files compile in seconds and stay free of
// ATen.  Every op runs on the current HIP stream of the input's device.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>
#include "bindings.h"
#include <algorithm>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

namespace {

// On ROCm builds torch devices are DeviceType::CUDA backed by HIP: use the
// "masquerading" guard/stream so device indices and the current stream match torch's.
inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }
using DevGuard = c10::hip::HIPGuardMasqueradingAsCUDA;

#define MX_CHECK(cond, ...) TORCH_CHECK(cond, "mxllm: ", __VA_ARGS__)
#define MX_OK(call)                                                                              \
  do {                                                                                           \
    int _rc = (call);                                                                            \
    TORCH_CHECK(_rc == 0, "mxllm kernel launch failed (" #call ") rc=", _rc, " ",                 \
                hipGetErrorString((hipError_t)(_rc > 0 ? _rc : 1)));                             \
  } while (0)

inline const uint16_t* bf(const at::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
inline uint16_t* bfm(at::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

void check_bf16(const at::Tensor& t, const char* name) {
  MX_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  MX_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bfloat16");
  MX_CHECK(t.is_contiguous(), name, " must be contiguous");
}
// a 2-D row-strided bf16 view (rows may be the left part of a wider buffer)
int64_t check_rows_bf16(const at::Tensor& t, const char* name) {
  MX_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  MX_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bfloat16");
  MX_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) >= t.size(1) && t.stride(0) % 8 == 0, name,
           " must be a row-major [T, H] view with a row stride that is a multiple of 8");
  return t.stride(0);
}
// [T, H] output whose rows live in a [T, H + pad] buffer (pad extra columns left to the caller)
at::Tensor empty_rows(int64_t T, int64_t H, int64_t pad, const at::TensorOptions& o) {
  if (pad <= 0) return at::empty({T, H}, o);
  return at::empty({T, H + pad}, o).narrow(1, 0, H);
}
void check_f32(const at::Tensor& t, const char* name) {
  MX_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  MX_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  MX_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// ---------------------------------------------------------------- RMSNorm
// out_pad > 0: y is returned as the [T, H] left part of a [T, H + out_pad] buffer
std::tuple<at::Tensor, at::Tensor, at::Tensor> rmsnorm_fwd(const at::Tensor& x,
                                                           const c10::optional<at::Tensor>& res,
                                                           const at::Tensor& w, double eps, int64_t out_pad) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  DevGuard g(x.device());
  const int64_t H = x.size(-1);
  const int64_t T = x.numel() / H;
  MX_CHECK(w.numel() == H, "weight size mismatch");
  MX_CHECK(out_pad >= 0 && out_pad % 8 == 0, "out_pad must be a non-negative multiple of 8");
  at::Tensor y = out_pad > 0 ? empty_rows(T, H, out_pad, x.options()) : at::empty_like(x);
  auto rstd = at::empty({T}, x.options().dtype(at::kFloat));
  at::Tensor h;
  const uint16_t* rp = nullptr;
  uint16_t* hp = nullptr;
  if (res.has_value()) {
    check_bf16(*res, "res");
    MX_CHECK(res->sizes() == x.sizes(), "residual shape mismatch");
    h = at::empty_like(x);
    rp = bf(*res);
    hp = bfm(h);
  }
  if (T > 0)
    MX_OK(mx_rmsnorm_fwd(bf(x), rp, bf(w), bfm(y), hp, rstd.data_ptr<float>(), (int)T, (int)H, (int)(H + out_pad),
                         (float)eps, cur_stream()));
  if (!res.has_value()) h = x;
  return {y, rstd, h};
}

// returns (dx, dw_f32 or empty).  dres may be a row-strided [T, H] view;
// out_pad > 0: dx is the left part of a [T, H + out_pad] buffer.
std::tuple<at::Tensor, at::Tensor> rmsnorm_bwd(const at::Tensor& dy, const at::Tensor& x,
                                               const at::Tensor& w, const at::Tensor& rstd,
                                               const c10::optional<at::Tensor>& dres, bool need_dw,
                                               int64_t out_pad) {
  check_bf16(dy, "dy");
  check_bf16(x, "x");
  check_bf16(w, "w");
  check_f32(rstd, "rstd");
  DevGuard g(x.device());
  const int64_t H = x.size(-1);
  const int64_t T = x.numel() / H;
  MX_CHECK(out_pad >= 0 && out_pad % 8 == 0, "out_pad must be a non-negative multiple of 8");
  at::Tensor dx = out_pad > 0 ? empty_rows(T, H, out_pad, x.options()) : at::empty_like(x);
  const uint16_t* drp = nullptr;
  int64_t ldr = H;
  if (dres.has_value()) {
    if (dres->is_contiguous()) {
      check_bf16(*dres, "dres");
    } else {
      ldr = check_rows_bf16(*dres, "dres");
      MX_CHECK(dres->size(0) == T && dres->size(1) == H, "dres shape mismatch");
    }
    drp = bf(*dres);
  }
  // rows per block: keep >= ~2 blocks per CU on 256 CUs, amortise the dγ partial
  int rpb = 1;
  if (need_dw) {
    rpb = (int)std::max<int64_t>(1, T / 512);
    rpb = std::min(rpb, 32);
  }
  const int64_t nblk = (T + rpb - 1) / rpb;
  at::Tensor dwp, dw;
  float* dwpp = nullptr;
  if (need_dw) {
    dwp = at::empty({nblk, H}, x.options().dtype(at::kFloat));
    dw = at::empty({H}, x.options().dtype(at::kFloat));
    dwpp = dwp.data_ptr<float>();
  }
  if (T > 0) {
    MX_OK(mx_rmsnorm_bwd(bf(dy), bf(x), bf(w), rstd.data_ptr<float>(), drp, bfm(dx), dwpp, (int)T, (int)H,
                         (int)ldr, (int)(H + out_pad), rpb, cur_stream()));
    if (need_dw) MX_OK(mx_colsum_f32(dwpp, dw.data_ptr<float>(), (int)nblk, (int)H, cur_stream()));
  } else if (need_dw) {
    dw.zero_();
  }
  return {dx, need_dw ? dw : at::Tensor()};
}

// ---------------------------------------------------------------- misc
// desc: int64 [n, 9] on the device (see misc.hip); total_blocks = sum of per-descriptor blocks
void copy2d_batched(const at::Tensor& desc, int64_t total_blocks) {
  MX_CHECK(desc.is_cuda() && desc.scalar_type() == at::kLong && desc.dim() == 2 && desc.size(1) == 9 &&
               desc.is_contiguous(), "desc must be int64 [n, 9] on the GPU");
  DevGuard g(desc.device());
  MX_OK(mx_copy2d_batched(desc.data_ptr<int64_t>(), (int)desc.size(0), total_blocks, cur_stream()));
}

// out[C, R] = in[R, C]^T for a row-major (row-strided) 16-bit 2-D GPU tensor
// scale: optional f32 device scalar (bf16 input): out = bf16(in^T * scale)
at::Tensor transpose2d(const at::Tensor& in, const c10::optional<at::Tensor>& scale) {
  MX_CHECK(in.is_cuda() && in.dim() == 2 && in.element_size() == 2, "in must be a 2-D 16-bit GPU tensor");
  MX_CHECK(in.stride(1) == 1 && in.stride(0) >= in.size(1), "in must be a row-major (row-strided) view");
  const float* sc = nullptr;
  if (scale.has_value()) {
    MX_CHECK(in.scalar_type() == at::kBFloat16 && scale->scalar_type() == at::kFloat && scale->numel() == 1 &&
                 scale->device() == in.device(), "transpose2d scale: f32 scalar on the device, bf16 input");
    sc = scale->data_ptr<float>();
  }
  DevGuard g(in.device());
  const int64_t R = in.size(0), C = in.size(1);
  auto out = at::empty({C, R}, in.options());
  MX_OK(mx_transpose16(in.data_ptr(), out.data_ptr(), R, C, in.stride(0), R, sc, cur_stream()));
  return out;
}

// ---------------------------------------------------------------- gemm8 (csrc/kernels/gemm8.hip)
// The seven gemm8 ops share their argument handling: the helpers below check the tensors and fill the
// launch description (kernels/gemm8_args.h) that the launcher is then called from.  Every op returns
// false when nothing was launched: a layout the helpers do not take, or the launcher's -1
// (mx::g8_takes, the one operand check).

inline const uint16_t* g8p(const mx::G8Mat& m) { return static_cast<const uint16_t*>(m.p); }
inline uint16_t* g8pm(const mx::G8Mat& m) { return static_cast<uint16_t*>(const_cast<void*>(m.p)); }

// optional 1-element f32 scalar on `dev` -> its device pointer (nullptr when absent)
const float* f32_scalar(const char* what, const c10::optional<at::Tensor>& t, const at::Device& dev) {
  if (!t.has_value()) return nullptr;
  MX_CHECK(t->scalar_type() == at::kFloat && t->numel() == 1 && t->device() == dev, what,
           ": f32 scalar on the device");
  return t->data_ptr<float>();
}

// Operands a [M, K] (a_kc) / [K, M] and b [N, K] (b_kc) / [K, N], row-strided bf16 views, and -- when
// given -- the output [M, N] (bf16, or fp32 with f32_ok) into L.A / L.B / L.C, M, N, K, out_f32.
// False: a layout no launcher takes (an inner stride, a dimension past int).
bool g8_fill(const char* op, mx::G8Launch& L, const at::Tensor& a, bool a_kc, const at::Tensor& b, bool b_kc,
             const at::Tensor* out, bool f32_ok) {
  MX_CHECK(a.is_cuda() && b.is_cuda() && (!out || out->is_cuda()), op, ": GPU tensors");
  MX_CHECK(a.scalar_type() == at::kBFloat16 && b.scalar_type() == at::kBFloat16, op, ": bf16 operands");
  MX_CHECK(!out || out->scalar_type() == at::kBFloat16 || (f32_ok && out->scalar_type() == at::kFloat), op,
           f32_ok ? ": fp32 / bf16 output" : ": bf16 output");
  MX_CHECK(a.dim() == 2 && b.dim() == 2 && (!out || out->dim() == 2), op, ": 2-D operands");
  const int64_t M = a_kc ? a.size(0) : a.size(1), K = a_kc ? a.size(1) : a.size(0);
  const int64_t N = b_kc ? b.size(0) : b.size(1), Kb = b_kc ? b.size(1) : b.size(0);
  MX_CHECK(K == Kb && (!out || (out->size(0) == M && out->size(1) == N)), op, ": shape mismatch");
  if (a.stride(1) != 1 || b.stride(1) != 1 || (out && out->stride(1) != 1)) return false;
  if (M > INT32_MAX || N > INT32_MAX || K > INT32_MAX) return false;
  L.A = {a.data_ptr(), a.stride(0), a_kc ? 1 : 0};
  L.B = {b.data_ptr(), b.stride(0), b_kc ? 1 : 0};
  if (out) L.C = {out->data_ptr(), out->stride(0), 1};
  L.out_f32 = out && out->scalar_type() == at::kFloat ? 1 : 0;
  L.M = (int)M, L.N = (int)N, L.K = (int)K;
  return true;
}

// The RoPE epilogue block of gemm8_rope / gemm8_rope_tail: x [B*S, K] (row-strided), w [(Hq + 2 Hkv) *
// 128, K] -> q [B, Hq, S, 128], k / v [B, Hkv, S, 128] (preallocated, contiguous), rotated with the f32
// tables cos / sin [>= S, 64] at positions 0..S-1.  Fills the operands and L.ep.
bool g8_fill_rope(const char* op, mx::G8Launch& L, const at::Tensor& x, const at::Tensor& w, const at::Tensor& cos,
                  const at::Tensor& sin, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, at::Tensor& q, at::Tensor& k,
                  at::Tensor& v) {
  MX_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(0) == B * S, op, ": shapes");
  MX_CHECK(w.size(0) == (Hq + 2 * Hkv) * 128, op, ": head dim 128");
  MX_CHECK(cos.scalar_type() == at::kFloat && sin.scalar_type() == at::kFloat && cos.is_contiguous() &&
               sin.is_contiguous() && cos.size(-1) == 64 && cos.size(0) >= S && sin.sizes() == cos.sizes(),
           op, ": f32 [>= S, 64] tables");
  for (const at::Tensor* t : {&q, &k, &v})
    MX_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && t->is_contiguous(), op, ": bf16 outputs");
  MX_CHECK(q.numel() == B * Hq * S * 128 && k.numel() == B * Hkv * S * 128 && v.numel() == k.numel(), op,
           ": output sizes");
  if (!g8_fill(op, L, x, true, w, true, nullptr, false)) return false;
  L.epi = mx::G8_EPI_ROPE;
  L.ep.q = bfm(q), L.ep.k = bfm(k), L.ep.v = bfm(v);
  L.ep.cosb = cos.data_ptr<float>(), L.ep.sinb = sin.data_ptr<float>();
  L.ep.S = (int)S, L.ep.Hq = (int)Hq, L.ep.Hkv = (int)Hkv;
  return true;
}

// a launcher's return code -> the op's: false for -1 (nothing launched), an error for a HIP failure
bool g8_launched(const char* op, int rc) {
  if (rc == -1) return false;
  TORCH_CHECK(rc == 0, "mxllm kernel launch failed (", op, ") rc=", rc, " ", hipGetErrorString((hipError_t)(rc > 0 ? rc : 1)));
  return true;
}

// out[M, N] = beta * out + alpha * op(a) op(b); out fp32 or bf16; alpha = alpha_f * (the optional f32
// device scalar alpha_t).
bool gemm8(const at::Tensor& a, bool a_kc, const at::Tensor& b, bool b_kc, at::Tensor& out, double beta,
           const c10::optional<at::Tensor>& alpha_t, double alpha_f, int64_t ph) {
  mx::G8Launch L{};
  if (!g8_fill("gemm8", L, a, a_kc, b, b_kc, &out, true)) return false;
  const float* sc = f32_scalar("gemm8 alpha_t", alpha_t, a.device());
  DevGuard g(a.device());
  return g8_launched("mx_gemm8", mx_gemm8(g8p(L.A), L.A.ld, L.A.kc, g8p(L.B), L.B.ld, L.B.kc, out.data_ptr(), L.C.ld,
                                          L.out_f32, L.M, L.N, L.K, (float)beta, sc, (float)alpha_f, (int)ph,
                                          cur_stream()));
}

// out[M, N] (bf16, beta 0) = alpha op(a) op(b) that also writes one fp32 sum of squares of the stored
// values per 256 x 256 output tile into sq (>= (M / 256) * (N / 256) elements, row-major tile order):
// the gradient-clip norm's partials straight from the weight-gradient GEMMs.
bool gemm8_sq(const at::Tensor& a, bool a_kc, const at::Tensor& b, bool b_kc, at::Tensor& out, at::Tensor& sq,
              const c10::optional<at::Tensor>& alpha_t, double alpha_f) {
  MX_CHECK(sq.is_cuda() && sq.scalar_type() == at::kFloat, "gemm8_sq: f32 GPU partials");
  mx::G8Launch L{};
  if (!g8_fill("gemm8_sq", L, a, a_kc, b, b_kc, &out, false) || !sq.is_contiguous()) return false;
  if (L.M % 256 || L.N % 256) return false;
  MX_CHECK(sq.numel() >= (int64_t)(L.M / 256) * (L.N / 256), "gemm8_sq: partials buffer too small");
  const float* sc = f32_scalar("gemm8_sq alpha_t", alpha_t, a.device());
  DevGuard g(a.device());
  return g8_launched("mx_gemm8_sq", mx_gemm8_sq(g8p(L.A), L.A.ld, L.A.kc, g8p(L.B), L.B.ld, L.B.kc, g8pm(L.C), L.C.ld,
                                                L.M, L.N, L.K, sc, (float)alpha_f, sq.data_ptr<float>(),
                                                cur_stream()));
}

// out[M, N] (bf16) = op(a) op(b) with the tail-balanced launch (mx_gemm8_tail): the output split at
// `at` columns (rows when `rows`) -- whole waves of tiles before it, half-K workgroups summed through
// an fp32 workspace after it.  sq: one sum of squares per 256 x 256 tile (plain part's tiles, then the
// split part's).
bool gemm8_tail(const at::Tensor& a, bool a_kc, const at::Tensor& b, bool b_kc, at::Tensor& out, int64_t at,
                bool rows, int64_t ph, const c10::optional<at::Tensor>& sq) {
  mx::G8Launch L{};
  if (!g8_fill("gemm8_tail", L, a, a_kc, b, b_kc, &out, false)) return false;
  const int64_t lim = rows ? L.M : L.N;
  if (at <= 0 || at >= lim) return false;
  float* sqp = nullptr;
  if (sq.has_value()) {
    MX_CHECK(sq->scalar_type() == at::kFloat && sq->is_contiguous() && sq->device() == a.device(),
             "gemm8_tail sq: contiguous f32 on the device");
    if (L.M % 256 || L.N % 256) return false;
    MX_CHECK(sq->numel() >= (int64_t)(L.M / 256) * (L.N / 256), "gemm8_tail sq: partials buffer too small");
    sqp = sq->data_ptr<float>();
  }
  DevGuard g(a.device());
  auto ws = at::empty({2 * (lim - at) * (rows ? L.N : L.M)}, a.options().dtype(at::kFloat));
  return g8_launched("mx_gemm8_tail",
                     mx_gemm8_tail(g8p(L.A), L.A.ld, L.A.kc, g8p(L.B), L.B.ld, L.B.kc, g8pm(L.C), L.C.ld, L.M, L.N, L.K,
                                   rows ? 1 : 0, (int)at, ws.data_ptr<float>(), (int)ph, cur_stream(), sqp));
}

// Forward qkv projection with RoPE and the head split in the GEMM epilogue (G8_EPI_ROPE; g8_fill_rope).
bool gemm8_rope(const at::Tensor& x, const at::Tensor& w, const at::Tensor& cos, const at::Tensor& sin, int64_t B,
                int64_t S, int64_t Hq, int64_t Hkv, at::Tensor& q, at::Tensor& k, at::Tensor& v) {
  mx::G8Launch L{};
  if (!g8_fill_rope("gemm8_rope", L, x, w, cos, sin, B, S, Hq, Hkv, q, k, v)) return false;
  DevGuard g(x.device());
  return g8_launched("mx_gemm8_epi", mx_gemm8_epi(g8p(L.A), L.A.ld, g8p(L.B), L.B.ld, nullptr, 0, L.M, L.N, L.K,
                                                  mx::G8_EPI_ROPE, L.ep, cur_stream()));
}

// gemm8_rope on the tail-balanced schedule (mx_gemm8_rope_tail): columns [0, at) through the RoPE
// epilogue, the rest as half-K images summed, rotated and scattered by one pass -- bitwise
// gemm8_tail(at) followed by rope_split.
bool gemm8_rope_tail(const at::Tensor& x, const at::Tensor& w, const at::Tensor& cos, const at::Tensor& sin, int64_t B,
                     int64_t S, int64_t Hq, int64_t Hkv, at::Tensor& q, at::Tensor& k, at::Tensor& v, int64_t at) {
  mx::G8Launch L{};
  if (!g8_fill_rope("gemm8_rope_tail", L, x, w, cos, sin, B, S, Hq, Hkv, q, k, v) || at <= 0 || at >= L.N) return false;
  DevGuard g(x.device());
  auto ws = at::empty({2 * (int64_t)L.M * (L.N - at)}, x.options().dtype(at::kFloat));
  return g8_launched("mx_gemm8_rope_tail", mx_gemm8_rope_tail(g8p(L.A), L.A.ld, g8p(L.B), L.B.ld, L.M, L.N, L.K, (int)at,
                                                              ws.data_ptr<float>(), L.ep, cur_stream()));
}

// Forward gate-up projection with SwiGLU in the GEMM epilogue (G8_EPI_SWIGLU): x [T, K],
// w = [gate; up] [2F, K] -> gu [T, 2F] (the projection output, kept for the backward) and
// m = silu(gate) * up [T, F].
bool gemm8_swiglu(const at::Tensor& x, const at::Tensor& w, at::Tensor& gu, at::Tensor& m) {
  mx::G8Launch L{};
  const bool ok = g8_fill("gemm8_swiglu", L, x, true, w, true, &gu, false);
  MX_CHECK(m.scalar_type() == at::kBFloat16 && m.dim() == 2 && m.size(0) == x.size(0) && 2 * m.size(1) == w.size(0),
           "gemm8_swiglu: m [T, F] bf16");
  if (!ok || m.stride(1) != 1) return false;
  DevGuard g(x.device());
  L.ep.m = bfm(m);
  L.ep.ldm = m.stride(0);
  return g8_launched("mx_gemm8_epi", mx_gemm8_epi(g8p(L.A), L.A.ld, g8p(L.B), L.B.ld, g8pm(L.C), L.C.ld, L.M, L.N, L.K,
                                                  mx::G8_EPI_SWIGLU, L.ep, cur_stream()));
}

// The down projection's dX GEMM with the SwiGLU backward in its epilogue (G8_EPI_SWIGLU_BWD):
// dy [T, H] and w = W_down [H, F] -> dgu [T, 2F] from the forward's gu [T, 2F] (dm never reaches
// HBM), and with m given also m = silu(g) u [T, F] (the recompute path's dW input).
bool gemm8_swiglu_bwd(const at::Tensor& dy, const at::Tensor& w, const at::Tensor& gu, at::Tensor& dgu,
                      const c10::optional<at::Tensor>& m) {
  mx::G8Launch L{};
  const bool ok = g8_fill("gemm8_swiglu_bwd", L, dy, true, w, false, nullptr, false);
  MX_CHECK(gu.is_cuda() && gu.scalar_type() == at::kBFloat16 && dgu.scalar_type() == at::kBFloat16,
           "gemm8_swiglu_bwd: bf16 GPU tensors");
  MX_CHECK(gu.dim() == 2 && dgu.dim() == 2 && gu.size(0) == dy.size(0) && gu.size(1) == 2 * w.size(1) &&
               dgu.sizes() == gu.sizes(),
           "gemm8_swiglu_bwd: shapes");
  if (m) {
    MX_CHECK(m->scalar_type() == at::kBFloat16 && m->dim() == 2 && m->size(0) == dy.size(0) &&
                 m->size(1) == w.size(1),
             "gemm8_swiglu_bwd: m [T, F] bf16");
    if (m->stride(1) != 1) return false;
    L.ep.m = reinterpret_cast<uint16_t*>(m->data_ptr());
    L.ep.ldm = m->stride(0);
  }
  if (!ok || gu.stride(1) != 1 || dgu.stride(1) != 1) return false;
  DevGuard g(dy.device());
  L.ep.gu = bf(gu);
  L.ep.ldg = gu.stride(0);
  return g8_launched("mx_gemm8_epi", mx_gemm8_epi(g8p(L.A), L.A.ld, g8p(L.B), L.B.ld, bfm(dgu), dgu.stride(0), L.M, L.N,
                                                  L.K, mx::G8_EPI_SWIGLU_BWD, L.ep, cur_stream()));
}

// the gemm8 diagnostic build's cycle stamps (MXLLM_GEMM8_STAMPS): int64 [1024, 2, 80] on the host
at::Tensor gemm8_stamps() {
  auto out = at::empty({1024, 2, 80}, at::TensorOptions().dtype(at::kLong));
  MX_OK(mx_gemm8_stamps(reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>())));
  return out;
}

// A HIP stream confined to a subset of the device's CUs (hipExtStreamCreateWithCUMask):
// ``mask`` = one int per 32 CUs (bit i of word w = CU 32 w + i).  Returns the stream handle
// for torch.cuda.ExternalStream; the stream lives for the process (never destroyed).
int64_t cu_masked_stream(int64_t device, std::vector<int64_t> mask) {
  MX_CHECK(!mask.empty(), "cu_masked_stream: empty mask");
  DevGuard g(c10::Device(c10::DeviceType::CUDA, (c10::DeviceIndex)device));
  std::vector<uint32_t> w(mask.size());
  for (size_t i = 0; i < mask.size(); ++i) w[i] = (uint32_t)(mask[i] & 0xffffffffLL);
  hipStream_t s = nullptr;
  hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)(w.size() * 32), w.data());
  MX_CHECK(e == hipSuccess, "hipExtStreamCreateWithCUMask: ", hipGetErrorString(e));
  return (int64_t)reinterpret_cast<intptr_t>(s);
}

// read `t` once on the current stream (cache warm-up of a weight ahead of its consumer; misc.hip)
void prefetch(const at::Tensor& t, int64_t wgs) {
  MX_CHECK(t.is_cuda() && t.is_contiguous(), "prefetch: contiguous GPU tensor");
  DevGuard g(t.device());
  MX_OK(mx_prefetch(t.data_ptr(), t.numel() * t.element_size(), (int)wgs, cur_stream()));
}

at::Tensor segmented_mean(const at::Tensor& codes, const at::Tensor& offsets) {
  MX_CHECK(codes.is_cuda() && codes.scalar_type() == at::kInt, "codes must be int32 GPU");
  MX_CHECK(offsets.is_cuda() && offsets.scalar_type() == at::kLong, "offsets must be int64 GPU");
  DevGuard g(codes.device());
  const int64_t n = offsets.numel() - 1;
  auto out = at::empty({std::max<int64_t>(n, 0)}, codes.options().dtype(at::kFloat));
  if (n > 0)
    MX_OK(mx_segmented_mean_i32(codes.data_ptr<int32_t>(), offsets.data_ptr<int64_t>(),
                                out.data_ptr<float>(), (int)n, cur_stream()));
  return out;
}

// sum(x^2) of a contiguous f32 or bf16 GPU tensor -> f32 [1]; fixed-order reduction
at::Tensor sqnorm(const at::Tensor& x) {
  MX_CHECK(x.is_cuda() && x.is_contiguous(), "x must be a contiguous GPU tensor");
  MX_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "x must be float32 or bfloat16");
  DevGuard g(x.device());
  auto opts = x.options().dtype(at::kFloat);
  auto out = at::empty({1}, opts);
  auto work = at::empty({2048}, opts);
  MX_OK(mx_sqnorm(x.data_ptr(), x.scalar_type() == at::kBFloat16 ? 1 : 0, x.numel(), out.data_ptr<float>(),
                  work.data_ptr<float>(), cur_stream()));
  return out;
}

// ---------------------------------------------------------------- SwiGLU
// out_pad > 0: outputs are [T, n] views into [T, n + out_pad] buffers
at::Tensor swiglu_fwd(const at::Tensor& gu, int64_t out_pad) {
  check_bf16(gu, "gu");
  DevGuard g(gu.device());
  const int64_t F2 = gu.size(-1);
  MX_CHECK(F2 % 16 == 0, "2F must be a multiple of 16");
  MX_CHECK(out_pad >= 0 && out_pad % 8 == 0, "out_pad must be a non-negative multiple of 8");
  const int64_t T = gu.numel() / F2;
  at::Tensor m;
  if (out_pad > 0) {
    m = empty_rows(T, F2 / 2, out_pad, gu.options());
  } else {
    auto sizes = gu.sizes().vec();
    sizes.back() = F2 / 2;
    m = at::empty(sizes, gu.options());
  }
  if (T > 0) MX_OK(mx_swiglu_fwd(bf(gu), bfm(m), T, (int)(F2 / 2), F2 / 2 + out_pad, cur_stream()));
  return m;
}

at::Tensor swiglu_bwd(const at::Tensor& dm, const at::Tensor& gu, int64_t out_pad) {
  check_bf16(dm, "dm");
  check_bf16(gu, "gu");
  DevGuard g(gu.device());
  const int64_t F2 = gu.size(-1);
  const int64_t T = gu.numel() / F2;
  MX_CHECK(dm.numel() == T * (F2 / 2), "dm shape mismatch");
  MX_CHECK(out_pad >= 0 && out_pad % 8 == 0, "out_pad must be a non-negative multiple of 8");
  at::Tensor dgu = out_pad > 0 ? empty_rows(T, F2, out_pad, gu.options()) : at::empty_like(gu);
  if (T > 0) MX_OK(mx_swiglu_bwd(bf(dm), bf(gu), bfm(dgu), T, (int)(F2 / 2), F2 + out_pad, cur_stream()));
  return dgu;
}

// swiglu_bwd that also re-emits m = swiglu(gu) (bitwise the forward's) from the same read of gu:
// the backward of a linear whose input activation was recomputed instead of saved
std::vector<at::Tensor> swiglu_bwd_m(const at::Tensor& dm, const at::Tensor& gu) {
  check_bf16(dm, "dm");
  check_bf16(gu, "gu");
  DevGuard g(gu.device());
  const int64_t F2 = gu.size(-1);
  const int64_t T = gu.numel() / F2;
  MX_CHECK(dm.numel() == T * (F2 / 2), "dm shape mismatch");
  MX_CHECK(dm.is_contiguous() && gu.is_contiguous(), "swiglu_bwd_m: dense dm / gu");
  at::Tensor dgu = at::empty_like(gu);
  at::Tensor m = at::empty({T, F2 / 2}, gu.options());
  if (T > 0) MX_OK(mx_swiglu_bwd(bf(dm), bf(gu), bfm(dgu), T, (int)(F2 / 2), F2, cur_stream(), bfm(m)));
  return {dgu, m};
}

// SwiGLU fused with the LoRA tail of its augmented-GEMM neighbour (csrc/kernels/lora.hip):
// fwd: m [T, F] in a [T, F + pad] buffer, tail = alpha m v^T (v [>= 16 nrb, F] row view);
// bwd: dgu [T, 2F] in a [T, 2F + pad] buffer, tail = alpha dgu v^T (v [>= 16 nrb, 2F]).
at::Tensor swiglu_lora(const c10::optional<at::Tensor>& dm, const at::Tensor& gu, int64_t pad, const at::Tensor& v,
                       int64_t nrb, double alpha) {
  check_bf16(gu, "gu");
  const int64_t ldv = check_rows_bf16(v, "v");
  DevGuard g(gu.device());
  const bool bwd = dm.has_value();
  // the width first: F = F2 / 2 would take an odd F2 (rows then read with the wrong stride), and T divides by it
  MX_CHECK(gu.dim() == 2 && gu.size(1) > 0 && gu.size(1) % 256 == 0,
           "swiglu_lora: gu [T, 2F] with F % 128 == 0 (gate | up halves of equal width)");
  const int64_t F2 = gu.size(1), F = F2 / 2, T = gu.size(0);
  MX_CHECK(T % 16 == 0, "swiglu_lora: [T, 2F] with T % 16 == 0");
  MX_CHECK(nrb >= 1 && nrb <= 4 && pad >= 16 * nrb && pad % 8 == 0, "swiglu_lora: 16 nrb <= pad");
  MX_CHECK(v.size(0) >= 16 * nrb && v.size(1) == (bwd ? F2 : F), "swiglu_lora: v shape");
  if (bwd) {
    check_bf16(*dm, "dm");
    MX_CHECK(dm->numel() == T * F, "swiglu_lora: dm shape");
  }
  const int64_t W = bwd ? F2 : F;
  at::Tensor out = at::empty({T, W + pad}, gu.options());
  const int64_t nws = mx_swiglu_lora_ws((int)T, (int)F, (int)nrb);
  auto ws = at::empty({nws > 0 ? nws : 1}, gu.options().dtype(at::kFloat));
  if (T > 0)
    MX_OK(mx_swiglu_lora(bwd ? 1 : 0, bf(gu), bwd ? bf(*dm) : nullptr, bfm(out), W + pad, bf(v), ldv, (int)nrb,
                         (int)pad, (float)alpha, ws.data_ptr<float>(), (int)T, (int)F, cur_stream()));
  return out.narrow(1, 0, W);
}

// ---------------------------------------------------------------- AdamW
void adamw_step(const c10::optional<at::Tensor>& master, at::Tensor grad, at::Tensor m, at::Tensor v,
                const c10::optional<at::Tensor>& lowp, const c10::optional<at::Tensor>& lo, double lr, double b1,
                double b2, double eps, double wd, double bc1, double bc2, const c10::optional<at::Tensor>& scale_t,
                double scale_f, bool zero_grad) {
  // master: fp32, or absent with ``lo`` given (split master: lowp = high half, lo = int16 low half)
  MX_CHECK(master.has_value() != lo.has_value(), "give either the fp32 master or the split low half");
  check_f32(m, "m");
  check_f32(v, "v");
  MX_CHECK(grad.is_cuda() && grad.is_contiguous(), "grad must be contiguous GPU");
  MX_CHECK(grad.scalar_type() == at::kFloat || grad.scalar_type() == at::kBFloat16, "grad f32/bf16");
  const int64_t n = m.numel();
  MX_CHECK(grad.numel() == n && v.numel() == n, "adamw size mismatch");
  float* mp = nullptr;
  if (master.has_value()) {
    check_f32(*master, "master");
    MX_CHECK(master->numel() == n, "master size");
    mp = master->data_ptr<float>();
  }
  DevGuard g(m.device());
  uint16_t* lp = nullptr;
  if (lowp.has_value()) {
    check_bf16(*lowp, "lowp");
    MX_CHECK(lowp->numel() == n, "lowp size");
    lp = reinterpret_cast<uint16_t*>(lowp->data_ptr());
  }
  int16_t* lop = nullptr;
  if (lo.has_value()) {
    MX_CHECK(lo->is_cuda() && lo->is_contiguous() && lo->scalar_type() == at::kShort && lo->numel() == n,
             "lo must be a contiguous int16 GPU tensor of the master's size");
    MX_CHECK(lp != nullptr, "split master needs lowp (the high half)");
    lop = lo->data_ptr<int16_t>();
  }
  const float* st = nullptr;
  if (scale_t.has_value()) {
    check_f32(*scale_t, "scale_t");
    st = scale_t->data_ptr<float>();
  }
  MX_OK(mx_adamw(mp, grad.data_ptr(), grad.scalar_type() == at::kBFloat16 ? 1 : 0, m.data_ptr<float>(),
                 v.data_ptr<float>(), lp, lop, n, (float)lr, (float)b1, (float)b2, (float)eps, (float)wd, (float)bc1,
                 (float)bc2, st, (float)scale_f, zero_grad ? 1 : 0, cur_stream()));
}

// fp32 <-> split master halves (hi bf16 = bits rounded half-up, lo int16 = remainder)
void split_master(const at::Tensor& x, at::Tensor hi, at::Tensor lo) {
  check_f32(x, "x");
  check_bf16(hi, "hi");
  MX_CHECK(lo.is_cuda() && lo.is_contiguous() && lo.scalar_type() == at::kShort, "lo int16 contiguous GPU");
  MX_CHECK(hi.numel() == x.numel() && lo.numel() == x.numel(), "split_master size mismatch");
  DevGuard g(x.device());
  MX_OK(mx_split_master(x.data_ptr<float>(), reinterpret_cast<uint16_t*>(hi.data_ptr()), lo.data_ptr<int16_t>(),
                        x.numel(), cur_stream()));
}

void join_master(const at::Tensor& hi, const at::Tensor& lo, at::Tensor out) {
  check_bf16(hi, "hi");
  check_f32(out, "out");
  MX_CHECK(lo.is_cuda() && lo.is_contiguous() && lo.scalar_type() == at::kShort, "lo int16 contiguous GPU");
  MX_CHECK(hi.numel() == out.numel() && lo.numel() == out.numel(), "join_master size mismatch");
  DevGuard g(out.device());
  MX_OK(mx_join_master(reinterpret_cast<const uint16_t*>(hi.data_ptr()), lo.data_ptr<int16_t>(),
                       out.data_ptr<float>(), out.numel(), cur_stream()));
}

// ---------------------------------------------------------------- embedding
at::Tensor embedding_fwd(const at::Tensor& ids, const at::Tensor& w) {
  check_bf16(w, "weight");
  MX_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong, "ids must be int64 GPU");
  DevGuard g(w.device());
  auto idc = ids.contiguous();
  const int64_t T = idc.numel(), H = w.size(1), V = w.size(0);
  auto out = at::empty({T, H}, w.options());
  MX_OK(mx_embedding_fwd(idc.data_ptr<int64_t>(), bf(w), bfm(out), T, (int)H, V, cur_stream()));
  return out;
}

at::Tensor embedding_bwd(const at::Tensor& dy, const at::Tensor& ids, int64_t V) {
  check_bf16(dy, "dy");
  DevGuard g(dy.device());
  auto idc = ids.contiguous();
  const int64_t H = dy.size(-1), T = idc.numel();
  auto dw = at::zeros({V, H}, dy.options().dtype(at::kFloat));
  MX_OK(mx_embedding_bwd(idc.data_ptr<int64_t>(), bf(dy), dw.data_ptr<float>(), T, (int)H, V, cur_stream()));
  return dw;
}

// out[V, H] (bf16 or f32, contiguous) += the batch's rows of dW, computed from the stably
// sorted ids (sid) and their positions (perm): only touched rows read / written.
void embedding_bwd_sorted(const at::Tensor& dy, const at::Tensor& sid, const at::Tensor& perm, at::Tensor out) {
  check_bf16(dy, "dy");
  MX_CHECK(sid.scalar_type() == at::kLong && perm.scalar_type() == at::kLong && sid.is_contiguous() &&
               perm.is_contiguous() && sid.numel() == perm.numel(), "sid / perm: int64, same length");
  MX_CHECK(out.is_contiguous() && (out.scalar_type() == at::kFloat || out.scalar_type() == at::kBFloat16) &&
               out.dim() == 2 && out.size(1) == dy.size(-1) && dy.is_contiguous() &&
               dy.numel() == sid.numel() * dy.size(-1) && out.device() == dy.device(),
           "embedding_bwd_sorted: out [V, H] f32/bf16 contiguous, dy [T, H] contiguous");
  DevGuard g(dy.device());
  const int64_t T = sid.numel(), nch = (T + 63) / 64;
  auto ws = at::empty({std::max<int64_t>(1, 2 * nch * out.size(1))}, dy.options().dtype(at::kFloat));
  MX_OK(mx_embedding_bwd_sorted(bf(dy), sid.data_ptr<int64_t>(), perm.data_ptr<int64_t>(), T, (int)out.size(1),
                                out.size(0), out.data_ptr(), out.scalar_type() == at::kFloat ? 1 : 0,
                                ws.data_ptr<float>(), cur_stream()));
}

// ---------------------------------------------------------------- cross-entropy
// logits [T, V] bf16 is overwritten in place with d(mean loss)/d(logits).
std::tuple<at::Tensor, at::Tensor> ce_fwd_bwd(at::Tensor logits, const at::Tensor& labels, int64_t ignore) {
  check_bf16(logits, "logits");
  MX_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong, "labels must be int64 GPU");
  DevGuard g(logits.device());
  const int64_t V = logits.size(-1), T = logits.numel() / V;
  MX_CHECK(labels.numel() == T, "labels size mismatch");
  auto lab = labels.contiguous();
  auto losses = at::empty({T}, logits.options().dtype(at::kFloat));
  auto ws = at::empty({2}, logits.options().dtype(at::kFloat));
  auto loss = at::empty({}, logits.options().dtype(at::kFloat));
  MX_OK(mx_ce_fwd_bwd(bfm(logits), lab.data_ptr<int64_t>(), losses.data_ptr<float>(), ws.data_ptr<float>(),
                      loss.data_ptr<float>(), T, (int)V, ignore, cur_stream()));
  return {loss, losses};
}

// 1 / (number of rows the CE kernels count: label != ignore and inside [0, V)) as a 1-element f32
// device tensor (0 when none)
at::Tensor ce_inv_count(const at::Tensor& labels, int64_t ignore, int64_t V) {
  MX_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong, "labels must be int64 GPU");
  DevGuard g(labels.device());
  auto lab = labels.contiguous();
  auto inv = at::empty({1}, labels.options().dtype(at::kFloat));
  MX_OK(mx_ce_inv_count(lab.data_ptr<int64_t>(), lab.numel(), (int)V, ignore, inv.data_ptr<float>(), cur_stream()));
  return inv;
}

// one chunk of the chunked LM-head CE: per-row losses, logits <- (softmax - onehot) * inv_n in place
at::Tensor ce_chunk(at::Tensor logits, const at::Tensor& labels, int64_t ignore, const at::Tensor& inv_n) {
  check_bf16(logits, "logits");
  MX_CHECK(logits.is_contiguous(), "ce_chunk: contiguous logits");
  MX_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong, "labels must be int64 GPU");
  MX_CHECK(inv_n.scalar_type() == at::kFloat && inv_n.numel() == 1 && inv_n.device() == logits.device(),
           "ce_chunk: inv_n f32 device scalar");
  DevGuard g(logits.device());
  const int64_t V = logits.size(-1), T = logits.numel() / V;
  MX_CHECK(labels.numel() == T, "labels size mismatch");
  auto lab = labels.contiguous();
  auto losses = at::empty({T}, logits.options().dtype(at::kFloat));
  MX_OK(mx_ce_chunk(bfm(logits), lab.data_ptr<int64_t>(), losses.data_ptr<float>(), inv_n.data_ptr<float>(), T,
                    (int)V, ignore, cur_stream()));
  return losses;
}

// fp32-logits chunk: losses [T] returned, dl (bf16 [T, V]) <- (softmax - onehot) * inv_n
at::Tensor ce_chunk_f32(const at::Tensor& logits, at::Tensor dl, const at::Tensor& labels, int64_t ignore,
                        const at::Tensor& inv_n) {
  check_f32(logits, "logits");
  check_bf16(dl, "dl");
  MX_CHECK(logits.is_contiguous() && dl.is_contiguous() && dl.sizes() == logits.sizes(), "ce_chunk_f32: shapes");
  MX_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong, "labels must be int64 GPU");
  MX_CHECK(inv_n.scalar_type() == at::kFloat && inv_n.numel() == 1 && inv_n.device() == logits.device(),
           "ce_chunk_f32: inv_n f32 device scalar");
  DevGuard g(logits.device());
  const int64_t V = logits.size(-1), T = logits.numel() / V;
  MX_CHECK(labels.numel() == T, "labels size mismatch");
  auto lab = labels.contiguous();
  auto losses = at::empty({T}, logits.options());
  MX_OK(mx_ce_chunk_f32(logits.data_ptr<float>(), bfm(dl), lab.data_ptr<int64_t>(), losses.data_ptr<float>(),
                        inv_n.data_ptr<float>(), T, (int)V, ignore, cur_stream()));
  return losses;
}

// ---------------------------------------------------------------- RoPE split / merge
std::tuple<at::Tensor, at::Tensor, at::Tensor> rope_split(const at::Tensor& qkv, const at::Tensor& cos,
                                                          const at::Tensor& sin, int64_t B, int64_t S, int64_t Hq,
                                                          int64_t Hkv, int64_t D,
                                                          const c10::optional<at::Tensor>& positions) {
  check_bf16(qkv, "qkv");
  check_f32(cos, "cos");
  check_f32(sin, "sin");
  MX_CHECK(qkv.numel() == B * S * (Hq + 2 * Hkv) * D, "qkv shape mismatch");
  MX_CHECK(cos.size(-1) == D / 2, "rope table width");
  DevGuard g(qkv.device());
  const int32_t* pos = nullptr;
  if (positions.has_value()) {
    MX_CHECK(positions->scalar_type() == at::kInt && positions->numel() == B * S, "positions int32 [B*S]");
    pos = positions->data_ptr<int32_t>();
  } else {
    MX_CHECK(cos.size(0) >= S, "rope table too short");
  }
  auto q = at::empty({B, Hq, S, D}, qkv.options());
  auto k = at::empty({B, Hkv, S, D}, qkv.options());
  auto v = at::empty({B, Hkv, S, D}, qkv.options());
  MX_OK(mx_rope_split(bf(qkv), cos.data_ptr<float>(), sin.data_ptr<float>(), pos, bfm(q), bfm(k), bfm(v), (int)B,
                      (int)S, (int)Hq, (int)Hkv, (int)D, cur_stream()));
  return {q, k, v};
}

at::Tensor rope_merge_bwd(const at::Tensor& dq, const at::Tensor& dkp, const at::Tensor& dvp, const at::Tensor& cos,
                          const at::Tensor& sin, int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D,
                          int64_t out_pad) {
  check_f32(dq, "dq");
  check_f32(dkp, "dkp");
  check_f32(dvp, "dvp");
  DevGuard g(dq.device());
  const int64_t kvin = dkp.size(1);
  MX_CHECK(dkp.dim() == 4 && dkp.size(0) == B && dkp.size(2) == S && dkp.size(3) == D, "dk partial shape");
  MX_CHECK(out_pad >= 0 && out_pad % 8 == 0, "out_pad must be a non-negative multiple of 8");
  const int64_t NHD = (Hq + 2 * Hkv) * D;
  auto dqkv = empty_rows(B * S, NHD, out_pad, dq.options().dtype(at::kBFloat16));
  MX_OK(mx_rope_merge_bwd(dq.data_ptr<float>(), dkp.data_ptr<float>(), dvp.data_ptr<float>(), cos.data_ptr<float>(),
                          sin.data_ptr<float>(), bfm(dqkv), (int)B, (int)S, (int)Hq, (int)Hkv, (int)kvin, (int)D,
                          NHD + out_pad, cur_stream(), 0));
  return dqkv;
}

// ---------------------------------------------------------------- attention
// Operand checks of attn_fwd, attn_bwd and attn_bwd_rope: all run before anything is allocated or written;
// the shape rules themselves are mx::af_takes / mx::ab_takes (kernels/attn_args.h).
typedef c10::optional<at::Tensor> OptTensor;
static void attn_operand(const char* op, const char* name, const at::Tensor& t, at::Device dev, at::ScalarType dt) {
  MX_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == dt && t.is_contiguous(), op, ": ", name,
           " must be a contiguous ", c10::toString(dt), " GPU tensor on q's device");
}
// rc of a launcher (or of a check) that was handed L: -1 is a refusal (nothing was launched), > 0 a HIP error
static void attn_launched(const char* op, int rc, const mx::AbLaunch& L) {
  MX_CHECK(rc != -1, op, ": the kernels do not take this call (mx::af_takes / mx::ab_takes, kernels/attn_args.h): B ",
           L.B, ", Hq ", L.Hq, ", Hkv ", L.Hkv, ", S ", L.S, ", Sk ", L.Sk, ", D ", L.D, ", causal ", L.causal,
           ", dq_mode ", L.dq_mode, ", row strides o ", L.ldo, ", dqkv ", L.ldq);
  TORCH_CHECK(rc == 0, "mxllm kernel launch failed (", op, ") rc=", rc, " ", hipGetErrorString((hipError_t)rc));
}
// The description of a call from its tensors: q [B,Hq,S,D], k / v [B,Hkv,Sk,D] on one device; for the
// backward (dout given) also o, dout, lse, the RoPE tables, preallocated outputs, L.hpw and the shape rules.
static mx::AbLaunch attn_fill(const char* op, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                              bool causal, int64_t dq_mode = 3, const at::Tensor* o = nullptr,
                              const at::Tensor* dout = nullptr, const at::Tensor* lse = nullptr,
                              const at::Tensor* cos = nullptr, const at::Tensor* sin = nullptr,
                              const OptTensor& dq_out = c10::nullopt, const OptTensor& dk_out = c10::nullopt,
                              const OptTensor& dv_out = c10::nullopt) {
  MX_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, op, ": q [B,Hq,S,D], k/v [B,Hkv,Sk,D]");
  const at::Device dev = q.device();
  for (auto [n, t] : {std::pair{"q", &q}, {"k", &k}, {"v", &v}}) attn_operand(op, n, *t, dev, at::kBFloat16);
  mx::AbLaunch L{};
  L.B = q.size(0), L.Hq = q.size(1), L.S = q.size(2), L.D = q.size(3), L.Hkv = k.size(1), L.Sk = k.size(2);
  MX_CHECK(k.size(0) == L.B && k.size(3) == L.D && v.sizes() == k.sizes(), op, ": k ", k.sizes(), " and v ", v.sizes(),
           " must be [B,Hkv,Sk,D] for q ", q.sizes());
  L.q = q.data_ptr(), L.k = k.data_ptr(), L.v = v.data_ptr(), L.q_bf16 = L.kv_bf16 = 1;
  L.causal = causal ? 1 : 0, L.dq_mode = (int)dq_mode, L.ldo = L.Hq * L.D, L.hpw = 1;
  if (!dout) return L;
  MX_CHECK(dq_mode >= 1 && dq_mode <= 3, op, ": dq_mode must be 1, 2 or 3");
  attn_operand(op, "dout", *dout, dev, at::kBFloat16);
  attn_operand(op, "lse", *lse, dev, at::kFloat);
  MX_CHECK(dout->numel() == q.numel() && o->numel() == dout->numel(), op, ": dout/o shape");
  MX_CHECK(lse->numel() == L.B * L.Hq * L.S, op, ": lse must be [B,Hq,S], got ", lse->sizes());
  if (o->is_contiguous()) {
    attn_operand(op, "o", *o, dev, at::kBFloat16);
  } else {  // token rows with a row stride (the padded attention output)
    MX_CHECK(o->is_cuda() && o->device() == dev && o->scalar_type() == at::kBFloat16 && o->dim() == 3 &&
                 o->stride(2) == 1 && o->size(2) == L.Hq * L.D && o->stride(0) == L.S * o->stride(1) &&
                 o->stride(1) % 8 == 0, op, ": o must be [B, S, Hq*D] with unit inner stride");
    L.ldo = o->stride(1);
  }
  L.o = o->data_ptr(), L.dout = dout->data_ptr(), L.lse = lse->data_ptr();
  L.o_bf16 = L.dout_bf16 = L.lse_f32 = L.out_f32 = 1;
  if (cos) {  // the backward that writes d(qkv) itself
    MX_CHECK(mx::ab_takes_rope(dq_mode, L.D, L.S, L.Sk), op, ": D = 128 self-attention in the split mode");
    for (auto [n, t] : {std::pair{"cos", cos}, {"sin", sin}}) attn_operand(op, n, *t, dev, at::kFloat);
    MX_CHECK(L.D >= 2 && cos->numel() >= L.S * (L.D / 2) && sin->numel() >= L.S * (L.D / 2), op,
             ": cos / sin: [>= S, D/2] contiguous f32");
    L.cos = cos->data_ptr(), L.sin = sin->data_ptr();
    L.cos_rows = std::min(cos->numel(), sin->numel()) / (L.D / 2);
  }
  const int64_t P = mx_attn_bwd_partial_heads(L);  // dK / dV partials [B, P, Sk, D], a KV head's consecutive
  if (dq_out.has_value() || dk_out.has_value() || dv_out.has_value()) {
    MX_CHECK(dq_out.has_value() && dk_out.has_value() && dv_out.has_value() && dq_mode == 3, op,
             ": preallocated outputs need all three and the split mode");
    for (auto [n, t] : {std::pair{"dq_out", &*dq_out}, {"dk_out", &*dk_out}, {"dv_out", &*dv_out}})
      attn_operand(op, n, *t, dev, at::kFloat);
    MX_CHECK(dq_out->numel() == q.numel() && dk_out->numel() == L.B * P * L.Sk * L.D &&
                 dv_out->numel() == L.B * P * L.Sk * L.D, op, ": output sizes");
  }
  attn_launched(op, mx::ab_shape_takes(L) ? 0 : -1, L);
  return L;
}

// out_pad > 0: o [B, S, Hq*D] is a view into [B, S, Hq*D + out_pad] (row stride Hq*D + out_pad)
std::tuple<at::Tensor, at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                            bool causal, double scale, int64_t out_pad) {
  mx::AbLaunch S = attn_fill("attn_fwd", q, k, v, causal);
  MX_CHECK(out_pad >= 0 && out_pad % 8 == 0, "out_pad must be a non-negative multiple of 8");
  S.ldo += out_pad;
  DevGuard g(q.device());
  auto o = at::empty({S.B, S.S, S.ldo}, q.options()).narrow(2, 0, S.Hq * S.D);  // (the whole of it without out_pad)
  auto lse = at::empty({S.B, S.Hq, S.S}, q.options().dtype(at::kFloat));
  mx::AfLaunch L{S.q, S.k, S.v, o.data_ptr(), lse.data_ptr(), 1, 1, 1, 1, S.B, S.Hq, S.Hkv, S.S, S.Sk, S.D, S.ldo};
  L.causal = S.causal;
  attn_launched("attn_fwd", mx_attn_fwd(L, (float)scale, cur_stream()), S);
  return {o, lse};
}

// dq_mode: mx::AbLaunch.  dq_out / dk_out / dv_out (optional, split mode only): preallocated f32 dq [B, Hq, S, D]
// and dK / dV partials [B, P, Sk, D] to write into (head-range views of larger tensors: the chunked long-context
// backward, mxllm/ops/attention.py).  dqkv (attn_bwd_rope): d(qkv) rows whose q columns the dQ kernel writes.
static std::tuple<at::Tensor, at::Tensor, at::Tensor> attn_bwd_impl(
    const char* op, const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
    const at::Tensor& o, const at::Tensor& lse, bool causal, double scale, int64_t dq_mode, const OptTensor& dq_out,
    const OptTensor& dk_out, const OptTensor& dv_out, at::Tensor* dqkv = nullptr, int64_t dqkv_pad = 0,
    const at::Tensor* cos = nullptr, const at::Tensor* sin = nullptr) {
  mx::AbLaunch L = attn_fill(op, q, k, v, causal, dq_mode, &o, &dout, &lse, cos, sin, dq_out, dk_out, dv_out);
  DevGuard g(q.device());
  const auto f32 = q.options().dtype(at::kFloat);
  const bool outs = dq_out.has_value();
  const int64_t P = L.Hq / L.hpw, S_pad = mx::ab_s_pad(L.S);  // P partial heads: mx::ab_hpw
  auto dkp = outs ? *dk_out : at::empty({L.B, P, L.Sk, L.D}, f32);
  auto dvp = outs ? *dv_out : at::empty({L.B, P, L.Sk, L.D}, f32);
  auto delta = at::empty({L.B, L.Hq, L.S}, f32);
  auto work = at::empty({mx::ab_work_bytes(L)}, q.options().dtype(at::kByte));
  // mode 1: a zeroed dQ padded to whole q tiles (the tail tile's atomics need no guard)
  auto dq = outs ? *dq_out
                 : (dq_mode == 1 ? at::zeros({L.B, L.Hq, S_pad, L.D}, f32)
                                 : at::empty({dqkv ? 0 : L.B, L.Hq, L.S, L.D}, f32));
  L.delta = delta.data_ptr(), L.dq = dq.data_ptr(), L.dkp = dkp.data_ptr(), L.dvp = dvp.data_ptr();
  if (dq_mode != 1) L.work = work.data_ptr();
  if (dqkv) *dqkv = empty_rows(L.B * L.S, (L.Hq + 2 * L.Hkv) * L.D, dqkv_pad, q.options());
  if (dqkv) L.dqkv = dqkv->data_ptr(), L.ldq = dqkv->stride(0), L.dqkv_bf16 = 1;
  attn_launched(op, mx_attn_bwd(L, (float)scale, cur_stream()), L);
  if (dq_mode == 1 && S_pad != L.S) dq = dq.narrow(2, 0, L.S).contiguous();
  return {dq, dkp, dvp};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> attn_bwd(
    const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const at::Tensor& o,
    const at::Tensor& lse, bool causal, double scale, int64_t dq_mode, const OptTensor& dq_out, const OptTensor& dk_out,
    const OptTensor& dv_out) {
  return attn_bwd_impl("attn_bwd", dout, q, k, v, o, lse, causal, scale, dq_mode, dq_out, dk_out, dv_out);
}

// The attention backward straight into d(qkv) [B*S, (Hq+2Hkv)*D (+out_pad)] bf16 (D = 128, split mode):
// the dQ kernel writes the q columns with the inverse RoPE applied, rope_merge_bwd only the k / v
// columns from the dK / dV partials -- the fp32 dQ never reaches HBM (mxllm/ops/attention.py).
at::Tensor attn_bwd_rope(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                         const at::Tensor& o, const at::Tensor& lse, bool causal, double scale, const at::Tensor& cos,
                         const at::Tensor& sin, int64_t out_pad) {
  MX_CHECK(out_pad >= 0 && out_pad % 8 == 0, "out_pad must be a non-negative multiple of 8");
  at::Tensor dqkv;
  auto [dq, dkp, dvp] = attn_bwd_impl("attn_bwd_rope", dout, q, k, v, o, lse, causal, scale, 3, c10::nullopt,
                                      c10::nullopt, c10::nullopt, &dqkv, out_pad, &cos, &sin);
  DevGuard g(q.device());
  const int64_t B = q.size(0), Hq = q.size(1), S = q.size(2), D = q.size(3), Hkv = k.size(1);
  MX_OK(mx_rope_merge_bwd(nullptr, dkp.data_ptr<float>(), dvp.data_ptr<float>(), cos.data_ptr<float>(),
                          sin.data_ptr<float>(), bfm(dqkv), (int)B, (int)S, (int)Hq, (int)Hkv, (int)dkp.size(1), (int)D,
                          dqkv.stride(0), cur_stream(), (int)Hq));
  return dqkv;
}

// ---------------------------------------------------------------- decode
// Paged KV caches: k_cache/v_cache [blocks, Hkv, block, D] + block_table int32 [slots, maxb]
// (token p of slot s in block block_table[s][p / block]); without a block table the caches
// are [slots, Hkv, max_seq, D].
struct KvPages {
  const int32_t* bt = nullptr;
  int maxb = 0;
};
static KvPages kv_pages(const c10::optional<at::Tensor>& block_table, const at::Tensor& k_cache) {
  KvPages pg;
  if (block_table.has_value() && block_table->defined()) {
    const at::Tensor& t = *block_table;
    MX_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.dim() == 2 && t.is_contiguous(),
             "block_table int32 [slots, max_blocks] contiguous GPU");
    MX_CHECK(k_cache.size(2) % 256 == 0, "paged KV: the block size must be a multiple of 256 tokens");
    pg.bt = t.data_ptr<int32_t>();
    pg.maxb = (int)t.size(1);
  }
  return pg;
}

// Operand checks of the decode ops, bf16 and kv8 caches alike.  Every check runs before anything is
// allocated or written.
//
// K and V pools of one layer: [rows, Hkv, SEQ, D] of one element type, equal in shape
static void check_kv_pools(const at::Tensor& k, const at::Tensor& v, at::ScalarType dt, int64_t D,
                           const at::Device& dev, int64_t Hkv, const char* op) {
  for (const at::Tensor* c : {&k, &v})
    MX_CHECK(c->device() == dev && c->scalar_type() == dt && c->is_contiguous() && c->dim() == 4, op,
             ": K and V pools must be contiguous ", c10::toString(dt), " [rows, Hkv, SEQ, D] on the query's device");
  MX_CHECK(k.size(3) == D, op, ": the pools' last dimension is ", k.size(3), ", expected head_dim ", D);
  MX_CHECK(k.size(1) == Hkv, op, ": the pools hold ", k.size(1), " KV heads, expected ", Hkv);
  MX_CHECK(v.sizes() == k.sizes(), op, ": the K and V pools differ in shape");
}
// lens / pos / slots: one int32 per sequence (nullptr for an optional tensor that is not given)
static const int32_t* check_rows_i32(const c10::optional<at::Tensor>& t, const at::Device& dev, int64_t B,
                                     const char* op, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  MX_CHECK(t->device() == dev && t->scalar_type() == at::kInt && t->is_contiguous() && t->numel() == B, op, ": ", name,
           " must be a contiguous int32 [B] tensor on the query's device");
  return t->data_ptr<int32_t>();
}
static void check_gqa(int64_t Hq, int64_t Hkv, const char* op) {
  MX_CHECK(Hkv > 0 && Hq % Hkv == 0 && Hq / Hkv <= 16, op, ": ", Hq, " q-heads over ", Hkv,
           " KV heads: the group size must be a whole number of at most 16");
}

// The split plan of a decode-attention call: one split per 256 positions that a sequence of at
// most max_len tokens can hold, and the partials (m, l) [B, Hq, nsplit, 2], o [B, Hq, nsplit, D]
struct DecodeSplits {
  int64_t nsplit;
  at::Tensor ml, po;
};
static DecodeSplits decode_splits(const at::Tensor& q, int64_t max_seq, int64_t max_len, const KvPages& pg) {
  const int64_t cap = pg.bt ? (int64_t)pg.maxb * max_seq : max_seq;  // positions a sequence can hold
  const int64_t nsplit = std::max<int64_t>(1, (std::min(max_len, cap) + 255) / 256);
  const auto f32 = q.options().dtype(at::kFloat);
  return {nsplit, at::empty({q.size(0), q.size(1), nsplit, 2}, f32),
          at::empty({q.size(0), q.size(1), nsplit, q.size(2)}, f32)};
}

// qkv [B, NH*D]; k_cache/v_cache [slots, Hkv, max_seq, D] (or paged); pos/slots int32 [B]
at::Tensor rope_append(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin, const at::Tensor& pos,
                       const c10::optional<at::Tensor>& slots, at::Tensor k_cache, at::Tensor v_cache, int64_t Hq,
                       int64_t Hkv, int64_t D, const c10::optional<at::Tensor>& block_table) {
  check_bf16(qkv, "qkv");
  MX_CHECK(qkv.dim() == 2 && Hq > 0 && Hkv > 0 && qkv.size(1) == (Hq + 2 * Hkv) * D,
           "rope_append: qkv must be [B, (Hq + 2 Hkv) * D]");
  const int64_t B = qkv.size(0);
  check_kv_pools(k_cache, v_cache, at::kBFloat16, D, qkv.device(), Hkv, "rope_append");
  MX_CHECK(pos.defined(), "rope_append: pos");
  const int32_t* pp = check_rows_i32(pos, qkv.device(), B, "rope_append", "pos");
  const int32_t* sl = check_rows_i32(slots, qkv.device(), B, "rope_append", "slots");
  DevGuard g(qkv.device());
  const KvPages pg = kv_pages(block_table, k_cache);
  auto q = at::empty({B, Hq, D}, qkv.options());
  MX_OK(mx_rope_append(bf(qkv), cos.data_ptr<float>(), sin.data_ptr<float>(), pp, sl, bfm(q), bfm(k_cache),
                       bfm(v_cache), (int)B, (int)Hq, (int)Hkv, (int)D, (int)k_cache.size(2), pg.bt, pg.maxb,
                       cur_stream()));
  return q;
}

// The operand checks of decode_attn and decode_attn_partials (op: the caller's name) and what the
// launch takes from the operands
struct DecodeCall {
  int64_t B, Hq, Hkv, D, max_seq;
  const int32_t *lens, *slots;
  KvPages pg;
};
static DecodeCall check_decode_attn(const char* op, const at::Tensor& q, const at::Tensor& k_cache,
                                    const at::Tensor& v_cache, const at::Tensor& lens,
                                    const c10::optional<at::Tensor>& slots,
                                    const c10::optional<at::Tensor>& block_table) {
  check_bf16(q, "q");
  MX_CHECK(q.dim() == 3, op, ": q must be [B, Hq, D]");
  MX_CHECK(k_cache.dim() == 4, op, ": the caches must be bf16 [rows, Hkv, SEQ, D]");
  DecodeCall c{q.size(0), q.size(1), k_cache.size(1), q.size(2), k_cache.size(2), nullptr, nullptr, {}};
  check_kv_pools(k_cache, v_cache, at::kBFloat16, c.D, q.device(), c.Hkv, op);
  check_gqa(c.Hq, c.Hkv, op);
  MX_CHECK(lens.defined(), op, ": lens");
  c.lens = check_rows_i32(lens, q.device(), c.B, op, "lens");
  c.slots = check_rows_i32(slots, q.device(), c.B, op, "slots");
  c.pg = kv_pages(block_table, k_cache);
  return c;
}

at::Tensor decode_attn(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                       const at::Tensor& lens, const c10::optional<at::Tensor>& slots, int64_t max_len, double scale,
                       int64_t len_off, const c10::optional<at::Tensor>& block_table,
                       const c10::optional<at::Tensor>& counters) {
  const DecodeCall c = check_decode_attn("decode_attn", q, k_cache, v_cache, lens, slots, block_table);
  // counters: int32 [>= B * Hkv], zero, owned by the caller (a decode engine): the split
  // partials are merged in-launch by the last workgroup of each (seq, kv-head), which
  // resets its counter -> no combine launch (head_dim 128)
  unsigned int* cnt = nullptr;
  if (counters.has_value() && c.D == 128) {
    MX_CHECK(counters->scalar_type() == at::kInt && counters->is_contiguous() && counters->numel() >= c.B * c.Hkv &&
                 counters->device() == q.device(),
             "decode_attn: counters must be a contiguous int32 tensor of >= B * Hkv zeros on q's device");
    cnt = reinterpret_cast<unsigned int*>(counters->data_ptr<int32_t>());
  }
  DevGuard g(q.device());
  DecodeSplits sp = decode_splits(q, c.max_seq, max_len, c.pg);
  auto out = at::empty({c.B, c.Hq * c.D}, q.options());
  MX_OK(mx_decode_attn(bf(q), bf(k_cache), bf(v_cache), c.lens, (int)len_off, c.slots, sp.ml.data_ptr<float>(),
                       sp.po.data_ptr<float>(), bfm(out), (int)c.B, (int)c.Hq, (int)c.Hkv, (int)c.D, (int)c.max_seq,
                       (int)sp.nsplit, (float)scale, c.pg.bt, c.pg.maxb, cnt, cur_stream()));
  return out;
}

// ---------------------------------------------------------------- paged-KV prefill attention
// Causal attention of query segments over the paged bf16 cache (csrc/kernels/prefill_paged.hip):
// q [T, Hq, 128], pools [blocks, Hkv, blk, 128], block_table int32 [slots, maxb], segs int32 [nseg, 4]
// = (first q row, n, slot, p0) -> out [T, Hq * 128]; rows outside every segment are not written.
// The segments come from host lists: mx::pp_takes (kernels/prefill_paged_args.h) checks the host copy
// before anything is enqueued, so a refused call writes nothing.  The device copy of the segment and
// work tables is kept for the next call with the same segments (every layer of one prefill pass).
at::Tensor prefill_attn_paged(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                              const at::Tensor& block_table, const at::Tensor& segs, double scale,
                              const c10::optional<at::Tensor>& out) {
  const char* op = "prefill_attn_paged";
  MX_CHECK(q.is_cuda() && q.dim() == 3 && q.is_contiguous(), op, ": q must be a contiguous GPU tensor [T, Hq, D]");
  MX_CHECK(k_cache.dim() == 4 && v_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes() &&
               k_cache.is_contiguous() && v_cache.is_contiguous() && k_cache.device() == q.device() &&
               v_cache.device() == q.device() && k_cache.scalar_type() == v_cache.scalar_type(),
           op, ": K and V pools must be contiguous [blocks, Hkv, blk, D] tensors of one shape and type on q's device");
  MX_CHECK(block_table.device() == q.device() && block_table.scalar_type() == at::kInt && block_table.dim() == 2 &&
               block_table.is_contiguous(),
           op, ": block_table must be a contiguous int32 [slots, max_blocks] tensor on q's device");
  MX_CHECK(segs.scalar_type() == at::kInt && segs.dim() == 2 && segs.size(1) == 4, op,
           ": segs must be int32 [nseg, 4] = (first q row, n, slot, p0)");
  MX_CHECK(k_cache.size(3) == q.size(2), op, ": the pools' last dimension is ", k_cache.size(3), ", q's is ", q.size(2));
  const int64_t T = q.size(0), Hq = q.size(1), D = q.size(2);
  if (out.has_value() && out->defined())
    MX_CHECK(out->device() == q.device() && out->dim() == 2 && out->size(0) == T && out->size(1) == Hq * D &&
                 out->stride(1) == 1,
             op, ": out must be [T, Hq * D] rows on q's device");
  const at::Tensor sh = segs.cpu().contiguous();
  const int64_t nseg = sh.size(0);
  DevGuard g(q.device());
  at::Tensor o = out.has_value() && out->defined() ? *out : at::empty({T, Hq * D}, q.options());
  if (nseg == 0 || T == 0) return o;
  const auto* sp = reinterpret_cast<const mx::PpSeg*>(sh.data_ptr<int32_t>());

  mx::PpLaunch L{};
  L.q = q.data_ptr();
  L.k_pool = k_cache.data_ptr();
  L.v_pool = v_cache.data_ptr();
  L.o = o.data_ptr();
  L.bt = block_table.data_ptr<int32_t>();
  L.segs_host = sp;
  L.q_bf16 = q.scalar_type() == at::kBFloat16;
  L.kv_bf16 = k_cache.scalar_type() == at::kBFloat16;
  L.o_bf16 = o.scalar_type() == at::kBFloat16;
  L.T = T, L.Hq = Hq, L.Hkv = k_cache.size(1), L.D = D;
  L.blocks = k_cache.size(0), L.blk = k_cache.size(2), L.slots = block_table.size(0), L.maxb = block_table.size(1);
  L.nseg = nseg, L.nwork = mx::pp_work_count(sp, nseg), L.ldo = o.stride(0);
  // the check runs on placeholders of the two device tables first: nothing is uploaded for a refused call
  L.segs = L.work = L.bt;
  MX_CHECK(mx::pp_takes(L), op, ": the kernel does not take this call (mx::pp_takes, csrc/kernels/prefill_paged_args.h): T ",
           T, ", Hq ", Hq, ", Hkv ", L.Hkv, ", D ", D, ", blk ", L.blk, ", slots ", L.slots, ", maxb ", L.maxb, ", ", nseg,
           " segments");

  static std::mutex mu;
  static std::vector<int32_t> host_key;
  static at::Tensor dev_tab;
  at::Tensor tab;
  {
    std::lock_guard<std::mutex> lk(mu);
    std::vector<int32_t> key((size_t)(4 * nseg + 2 * L.nwork));
    std::memcpy(key.data(), sp, sizeof(int32_t) * 4 * (size_t)nseg);
    mx::pp_fill_work(sp, nseg, key.data() + 4 * nseg);
    if (!dev_tab.defined() || dev_tab.device() != q.device() || key != host_key) {
      at::Tensor ht = at::empty({(int64_t)key.size()}, at::TensorOptions().dtype(at::kInt));
      std::memcpy(ht.data_ptr<int32_t>(), key.data(), sizeof(int32_t) * key.size());
      dev_tab = ht.to(q.device());
      host_key = std::move(key);
    }
    tab = dev_tab;
  }
  L.segs = tab.data_ptr<int32_t>();
  L.work = L.segs + 4 * nseg;
  MX_OK(mx_prefill_attn_paged(L, (float)scale, cur_stream()));
  return o;
}

// ---------------------------------------------------------------- kv8: fp8 (e4m3) KV cache, head_dim 128
// Pools of one layer: codes uint8 [rows, Hkv, SEQ, 128] and scales f32 [rows, Hkv, SEQ] for K and
// for V (contiguous or paged like the bf16 caches).
static void check_kv8_pools(const at::Tensor& k_codes, const at::Tensor& k_scale, const at::Tensor& v_codes,
                            const at::Tensor& v_scale, const at::Device& dev, int64_t Hkv, const char* op) {
  check_kv_pools(k_codes, v_codes, at::kByte, 128, dev, Hkv, op);
  for (const at::Tensor* s : {&k_scale, &v_scale})
    MX_CHECK(s->device() == dev && s->scalar_type() == at::kFloat && s->is_contiguous() && s->dim() == 3 &&
                 s->size(0) == k_codes.size(0) && s->size(1) == Hkv && s->size(2) == k_codes.size(2),
             op, ": scale pools must be contiguous float32 [rows, Hkv, SEQ] matching the code pools");
}

// x [R, 128] bf16 rows (row stride a multiple of 8) -> (codes uint8 [R, 128], scale f32 [R])
std::tuple<at::Tensor, at::Tensor> kv8_quant_rows(const at::Tensor& x) {
  MX_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.size(1) == 128 &&
               (x.size(0) <= 1 || (x.stride(0) >= 128 && x.stride(0) % 8 == 0)) && x.stride(1) == 1,
           "kv8_quant_rows: x must be bf16 [R, 128] rows on the GPU with a row stride that is a multiple of 8");
  DevGuard g(x.device());
  const int64_t R = x.size(0);
  auto q = at::empty({R, 128}, x.options().dtype(at::kByte));
  auto s = at::empty({R}, x.options().dtype(at::kFloat));
  MX_OK(mx_kv8_quant_rows(bf(x), R <= 1 ? 128 : x.stride(0), q.data_ptr<uint8_t>(), s.data_ptr<float>(), R,
                          cur_stream()));
  return {q, s};
}

// rope_append into kv8 pools; returns the rotated q [B, Hq, 128] (rope_append's q)
at::Tensor rope_append_kv8(const at::Tensor& qkv, const at::Tensor& cos, const at::Tensor& sin, const at::Tensor& pos,
                           const c10::optional<at::Tensor>& slots, at::Tensor k_codes, at::Tensor k_scale,
                           at::Tensor v_codes, at::Tensor v_scale, int64_t Hq, int64_t Hkv,
                           const c10::optional<at::Tensor>& block_table) {
  check_bf16(qkv, "qkv");
  MX_CHECK(qkv.dim() == 2 && Hq > 0 && Hkv > 0 && qkv.size(1) == (Hq + 2 * Hkv) * 128,
           "rope_append_kv8: qkv must be [B, (Hq + 2 Hkv) * 128] (head_dim 128 only)");
  const int64_t B = qkv.size(0);
  check_kv8_pools(k_codes, k_scale, v_codes, v_scale, qkv.device(), Hkv, "rope_append_kv8");
  for (const at::Tensor* t : {&cos, &sin})
    MX_CHECK(t->device() == qkv.device() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 2 &&
                 t->size(1) == 64,
             "rope_append_kv8: cos / sin must be contiguous float32 [positions, 64] on qkv's device");
  MX_CHECK(pos.defined(), "rope_append_kv8: pos");
  const int32_t* pp = check_rows_i32(pos, qkv.device(), B, "rope_append_kv8", "pos");
  const int32_t* sl = check_rows_i32(slots, qkv.device(), B, "rope_append_kv8", "slots");
  DevGuard g(qkv.device());
  const KvPages pg = kv_pages(block_table, k_codes);
  auto q = at::empty({B, Hq, 128}, qkv.options());
  MX_OK(mx_rope_append_kv8(bf(qkv), cos.data_ptr<float>(), sin.data_ptr<float>(), pp, sl, bfm(q),
                           k_codes.data_ptr<uint8_t>(), k_scale.data_ptr<float>(), v_codes.data_ptr<uint8_t>(),
                           v_scale.data_ptr<float>(), (int)B, (int)Hq, (int)Hkv, (int)k_codes.size(2), pg.bt, pg.maxb,
                           cur_stream()));
  return q;
}

// decode_attn over kv8 pools: q [B, Hq, 128] -> out [B, Hq * 128]
at::Tensor decode_attn_kv8(const at::Tensor& q, const at::Tensor& k_codes, const at::Tensor& k_scale,
                           const at::Tensor& v_codes, const at::Tensor& v_scale, const at::Tensor& lens,
                           const c10::optional<at::Tensor>& slots, int64_t max_len, double scale, int64_t len_off,
                           const c10::optional<at::Tensor>& block_table) {
  check_bf16(q, "q");
  MX_CHECK(q.dim() == 3 && q.size(2) == 128, "decode_attn_kv8: q must be [B, Hq, 128] (head_dim 128 only)");
  const int64_t B = q.size(0), Hq = q.size(1);
  MX_CHECK(k_codes.dim() == 4, "decode_attn_kv8: code pools must be uint8 [rows, Hkv, SEQ, 128]");
  const int64_t Hkv = k_codes.size(1), max_seq = k_codes.size(2);
  check_kv8_pools(k_codes, k_scale, v_codes, v_scale, q.device(), Hkv, "decode_attn_kv8");
  check_gqa(Hq, Hkv, "decode_attn_kv8");
  MX_CHECK(lens.defined(), "decode_attn_kv8: lens");
  const int32_t* lp = check_rows_i32(lens, q.device(), B, "decode_attn_kv8", "lens");
  const int32_t* sl = check_rows_i32(slots, q.device(), B, "decode_attn_kv8", "slots");
  DevGuard g(q.device());
  const KvPages pg = kv_pages(block_table, k_codes);
  DecodeSplits sp = decode_splits(q, max_seq, max_len, pg);
  auto out = at::empty({B, Hq * 128}, q.options());
  MX_OK(mx_decode_attn_kv8(bf(q), k_codes.data_ptr<uint8_t>(), k_scale.data_ptr<float>(), v_codes.data_ptr<uint8_t>(),
                           v_scale.data_ptr<float>(), lp, (int)len_off, sl, sp.ml.data_ptr<float>(),
                           sp.po.data_ptr<float>(), bfm(out), (int)B, (int)Hq, (int)Hkv, (int)max_seq, (int)sp.nsplit,
                           (float)scale, pg.bt, pg.maxb, cur_stream()));
  return out;
}

// The split-K partials without the combine: (part_ml [B, Hq, nsplit, 2], part_o [B, Hq, nsplit, D]),
// merged by the o-projection's prologue (skinny_merge_linear).  D = 128.
std::tuple<at::Tensor, at::Tensor> decode_attn_partials(const at::Tensor& q, const at::Tensor& k_cache,
                                                        const at::Tensor& v_cache, const at::Tensor& lens,
                                                        const c10::optional<at::Tensor>& slots, int64_t max_len,
                                                        double scale, int64_t len_off,
                                                        const c10::optional<at::Tensor>& block_table) {
  const DecodeCall c = check_decode_attn("decode_attn_partials", q, k_cache, v_cache, lens, slots, block_table);
  MX_CHECK(c.D == 128, "decode_attn_partials: head_dim 128");
  DevGuard g(q.device());
  DecodeSplits sp = decode_splits(q, c.max_seq, max_len, c.pg);
  MX_OK(mx_decode_attn(bf(q), bf(k_cache), bf(v_cache), c.lens, (int)len_off, c.slots, sp.ml.data_ptr<float>(),
                       sp.po.data_ptr<float>(), nullptr, (int)c.B, (int)c.Hq, (int)c.Hkv, (int)c.D, (int)c.max_seq,
                       (int)sp.nsplit, (float)scale, c.pg.bt, c.pg.maxb, nullptr, cur_stream()));
  return {sp.ml, sp.po};
}

// ---------------------------------------------------------------- verify attention (speculative decoding)
// Decode attention for n consecutive query rows per sequence (csrc/kernels/decode.hip verify_attn):
// q [B * n, Hq, 128], row b * n + j at position lens[b] + j of slot slots[b], j < nq[b]; the rows' K/V
// are in the cache already -> out [B * n, Hq * 128]; rows j >= nq[b] are zeros.  `out` given: its first
// B * n rows are written, the rest is left alone.  Pools: bf16 caches, or kv8 code pools with their
// scale pools.  mx::vf_takes (kernels/verify_args.h) is THE check: it
// runs before anything is allocated or enqueued, so a refused call writes nothing.
static at::Tensor verify_attn_call(const char* op, const at::Tensor& q, const at::Tensor& k_pool,
                                   const c10::optional<at::Tensor>& k_scale, const at::Tensor& v_pool,
                                   const c10::optional<at::Tensor>& v_scale, const at::Tensor& lens,
                                   const at::Tensor& nq, const c10::optional<at::Tensor>& slots, int64_t n,
                                   int64_t max_len, double scale, const c10::optional<at::Tensor>& block_table,
                                   const c10::optional<at::Tensor>& out_) {
  const bool kv8 = k_scale.has_value();
  MX_CHECK(q.is_cuda() && q.dim() == 3 && q.is_contiguous(), op, ": q must be a contiguous GPU tensor [B * n, Hq, D]");
  MX_CHECK(n >= 1 && q.size(0) % n == 0, op, ": q has ", q.size(0), " rows, not a multiple of n = ", n);
  const int64_t B = q.size(0) / n, Hq = q.size(1), D = q.size(2);
  MX_CHECK(k_pool.dim() == 4 && v_pool.dim() == 4 && k_pool.sizes() == v_pool.sizes() && k_pool.is_contiguous() &&
               v_pool.is_contiguous() && k_pool.device() == q.device() && v_pool.device() == q.device() &&
               k_pool.scalar_type() == v_pool.scalar_type() && k_pool.size(3) == D,
           op, ": K and V pools must be contiguous [rows, Hkv, SEQ, D] tensors of one shape and type on q's device");
  const int64_t Hkv = k_pool.size(1), max_seq = k_pool.size(2);
  if (kv8)
    for (const at::Tensor* s : {&*k_scale, &*v_scale})
      MX_CHECK(s->device() == q.device() && s->is_contiguous() && s->dim() == 3 && s->size(0) == k_pool.size(0) &&
                   s->size(1) == Hkv && s->size(2) == max_seq && s->scalar_type() == at::kFloat,
               op, ": scale pools must be contiguous float32 [rows, Hkv, SEQ] matching the code pools");
  MX_CHECK(lens.defined() && nq.defined(), op, ": lens and nq");
  mx::VfLaunch L{};
  L.lens = check_rows_i32(lens, q.device(), B, op, "lens");
  L.nq = check_rows_i32(nq, q.device(), B, op, "nq");
  L.slots = check_rows_i32(slots, q.device(), B, op, "slots");
  if (block_table.has_value() && block_table->defined()) {
    const at::Tensor& t = *block_table;
    MX_CHECK(t.device() == q.device() && t.scalar_type() == at::kInt && t.dim() == 2 && t.is_contiguous(), op,
             ": block_table must be a contiguous int32 [slots, max_blocks] tensor on q's device");
    L.bt = t.data_ptr<int32_t>();
    L.maxb = t.size(1);
  }
  L.q = q.data_ptr();
  L.k_pool = k_pool.data_ptr();
  L.v_pool = v_pool.data_ptr();
  L.k_scale = kv8 ? k_scale->data_ptr<float>() : nullptr;
  L.v_scale = kv8 ? v_scale->data_ptr<float>() : nullptr;
  const bool has_out = out_.has_value() && out_->defined();
  if (has_out)
    MX_CHECK(out_->device() == q.device() && out_->dim() == 2 && out_->is_contiguous() && out_->size(0) >= q.size(0) &&
                 out_->size(1) == Hq * D,
             op, ": out must be contiguous [>= B * n, Hq * D] rows on q's device");
  L.q_bf16 = q.scalar_type() == at::kBFloat16;
  L.out_bf16 = has_out ? out_->scalar_type() == at::kBFloat16 : L.q_bf16;
  L.kv_bf16 = k_pool.scalar_type() == at::kBFloat16;
  L.kv_u8 = k_pool.scalar_type() == at::kByte;
  L.B = B, L.n = n, L.Hq = Hq, L.Hkv = Hkv, L.D = D;
  L.rows = k_pool.size(0), L.max_seq = max_seq;
  const int64_t cap = L.bt ? L.maxb * max_seq : max_seq;  // positions a sequence can hold
  L.nsplit = std::max<int64_t>(1, (std::min(max_len, cap) + 255) / 256);  // decode_splits' plan
  // the check runs on placeholders of the partials and the output first: nothing is allocated for a refused call
  L.part_ml = L.part_o = reinterpret_cast<float*>(q.data_ptr());
  L.out = q.data_ptr();
  MX_CHECK(B > 0 && mx::vf_takes(L), op, ": the kernel does not take this call (mx::vf_takes, csrc/kernels/verify_args.h): B ",
           B, ", n ", n, ", Hq ", Hq, ", Hkv ", Hkv, ", D ", D, ", SEQ ", max_seq, ", maxb ", L.maxb, ", nsplit ", L.nsplit,
           kv8 ? ", kv8 pools" : ", pools of q's type");
  DevGuard g(q.device());
  const auto f32 = q.options().dtype(at::kFloat);
  at::Tensor ml = at::empty({B * n, Hq, L.nsplit, 2}, f32), po = at::empty({B * n, Hq, L.nsplit, D}, f32);
  at::Tensor out = has_out ? *out_ : at::empty({B * n, Hq * D}, q.options());
  L.part_ml = ml.data_ptr<float>();
  L.part_o = po.data_ptr<float>();
  L.out = out.data_ptr();
  MX_OK(mx_verify_attn(L, (float)scale, cur_stream()));
  return out;
}

at::Tensor verify_attn(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache, const at::Tensor& lens,
                       const at::Tensor& nq, const c10::optional<at::Tensor>& slots, int64_t n, int64_t max_len,
                       double scale, const c10::optional<at::Tensor>& block_table,
                       const c10::optional<at::Tensor>& out) {
  MX_CHECK(k_cache.scalar_type() != at::kByte, "verify_attn: u8 code pools need their scale pools (verify_attn_kv8)");
  return verify_attn_call("verify_attn", q, k_cache, c10::nullopt, v_cache, c10::nullopt, lens, nq, slots, n, max_len,
                          scale, block_table, out);
}

at::Tensor verify_attn_kv8(const at::Tensor& q, const at::Tensor& k_codes, const at::Tensor& k_scale,
                           const at::Tensor& v_codes, const at::Tensor& v_scale, const at::Tensor& lens,
                           const at::Tensor& nq, const c10::optional<at::Tensor>& slots, int64_t n, int64_t max_len,
                           double scale, const c10::optional<at::Tensor>& block_table,
                           const c10::optional<at::Tensor>& out) {
  MX_CHECK(k_codes.scalar_type() == at::kByte, "verify_attn_kv8: code pools must be uint8 [rows, Hkv, SEQ, 128]");
  return verify_attn_call("verify_attn_kv8", q, k_codes, k_scale, v_codes, v_scale, lens, nq, slots, n, max_len, scale,
                          block_table, out);
}

at::Tensor sample(const at::Tensor& logits, double temperature, int64_t seed, int64_t step) {
  MX_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, "logits [B, V] contiguous GPU");
  MX_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16/f32");
  DevGuard g(logits.device());
  auto out = at::empty({logits.size(0)}, logits.options().dtype(at::kLong));
  auto ws = at::empty({std::max<int64_t>(1, mx_sample_ws_floats((int)logits.size(0)))},
                      logits.options().dtype(at::kFloat));  // per-call partials (stream-ordered allocator)
  MX_OK(mx_sample(logits.data_ptr(), logits.scalar_type() == at::kBFloat16 ? 1 : 0, out.data_ptr<int64_t>(),
                  (int)logits.size(0), (int)logits.size(1), (float)temperature, (uint32_t)seed, (uint32_t)step,
                  ws.data_ptr<float>(), cur_stream()));
  return out;
}

// per-row temperature / seed / step without top-k / top-p (the split-vocabulary kernel of
// decode.hip; same draws as sample_rows for such rows)
at::Tensor sample_temp_rows(const at::Tensor& logits, const at::Tensor& temps, const at::Tensor& seeds,
                            const at::Tensor& steps) {
  MX_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, "logits [B, V] contiguous GPU");
  MX_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16/f32");
  const int64_t B = logits.size(0);
  auto chk = [&](const at::Tensor& t, at::ScalarType st, const char* name) {
    MX_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == st && t.numel() == B, name);
  };
  chk(temps, at::kFloat, "temps f32 [B]");
  chk(seeds, at::kLong, "seeds i64 [B]");
  chk(steps, at::kInt, "steps i32 [B]");
  DevGuard g(logits.device());
  auto out = at::empty({B}, logits.options().dtype(at::kLong));
  auto ws = at::empty({std::max<int64_t>(1, mx_sample_ws_floats((int)B))}, logits.options().dtype(at::kFloat));
  MX_OK(mx_sample_temp_rows(logits.data_ptr(), logits.scalar_type() == at::kBFloat16 ? 1 : 0,
                            out.data_ptr<int64_t>(), (int)B, (int)logits.size(1), temps.data_ptr<float>(),
                            seeds.data_ptr<int64_t>(), steps.data_ptr<int32_t>(), ws.data_ptr<float>(),
                            cur_stream()));
  return out;
}

at::Tensor sample_rows(const at::Tensor& logits, const at::Tensor& temps, const at::Tensor& top_p,
                       const at::Tensor& top_k, const at::Tensor& seeds, const at::Tensor& steps) {
  MX_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, "logits [B, V] contiguous GPU");
  MX_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16/f32");
  const int64_t B = logits.size(0);
  auto chk = [&](const at::Tensor& t, at::ScalarType st, const char* name) {
    MX_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == st && t.numel() == B, name);
  };
  chk(temps, at::kFloat, "temps f32 [B]");
  chk(top_p, at::kFloat, "top_p f32 [B]");
  chk(top_k, at::kInt, "top_k i32 [B]");
  chk(seeds, at::kLong, "seeds i64 [B]");
  chk(steps, at::kInt, "steps i32 [B]");
  DevGuard g(logits.device());
  auto out = at::empty({B}, logits.options().dtype(at::kLong));
  MX_OK(mx_sample_rows(logits.data_ptr(), logits.scalar_type() == at::kBFloat16 ? 1 : 0, out.data_ptr<int64_t>(),
                       (int)B, (int)logits.size(1), temps.data_ptr<float>(), top_p.data_ptr<float>(),
                       top_k.data_ptr<int32_t>(), seeds.data_ptr<int64_t>(), steps.data_ptr<int32_t>(),
                       cur_stream()));
  return out;
}

// acceptance of deterministic drafts (sampling.hip spec_accept_kernel): drawn, tokens int64 [B, n],
// nq int32 [B] -> int32 [B, n + 1] = (accepted drafts, the emitted tokens, -1 padding)
at::Tensor spec_accept(const at::Tensor& drawn, const at::Tensor& tokens, const at::Tensor& nq) {
  MX_CHECK(drawn.is_cuda() && drawn.is_contiguous() && drawn.dim() == 2 && drawn.scalar_type() == at::kLong &&
               drawn.size(1) >= 1,
           "spec_accept: drawn must be a contiguous int64 [B, n] GPU tensor");
  MX_CHECK(tokens.device() == drawn.device() && tokens.is_contiguous() && tokens.scalar_type() == at::kLong &&
               tokens.sizes() == drawn.sizes(),
           "spec_accept: tokens must be a contiguous int64 [B, n] tensor on drawn's device");
  const int64_t B = drawn.size(0), n = drawn.size(1);
  MX_CHECK(B <= 0x7fffffff / (n + 1), "spec_accept: B * (n + 1) must fit 31 bits");
  MX_CHECK(nq.defined(), "spec_accept: nq");
  const int32_t* np = check_rows_i32(nq, drawn.device(), B, "spec_accept", "nq");
  DevGuard g(drawn.device());
  auto out = at::empty({B, n + 1}, drawn.options().dtype(at::kInt));
  MX_OK(mx_spec_accept(drawn.data_ptr<int64_t>(), tokens.data_ptr<int64_t>(), np, out.data_ptr<int32_t>(), (int)B,
                       (int)n, cur_stream()));
  return out;
}

// sampling penalties + logit_bias on the logits (logits_proc.hip): f32 [B, V].  state int32
// [n_slots, V] / bias f32 [n_slots, V] may be absent; slots < 0: plain conversion
at::Tensor logits_adjust_rows(const at::Tensor& logits, const c10::optional<at::Tensor>& state,
                              const at::Tensor& slots, const at::Tensor& presence, const at::Tensor& frequency,
                              const at::Tensor& repetition, const c10::optional<at::Tensor>& bias) {
  MX_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, "logits [B, V] contiguous GPU");
  MX_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16/f32");
  const int64_t B = logits.size(0), V = logits.size(1);
  auto chk = [&](const at::Tensor& t, at::ScalarType st, const char* name) {
    MX_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == st && t.numel() == B, name);
  };
  chk(slots, at::kInt, "slots i32 [B]");
  chk(presence, at::kFloat, "presence f32 [B]");
  chk(frequency, at::kFloat, "frequency f32 [B]");
  chk(repetition, at::kFloat, "repetition f32 [B]");
  int64_t n_slots = -1;
  auto table = [&](const c10::optional<at::Tensor>& t, at::ScalarType st, const char* name) {
    if (!t.has_value()) return;
    MX_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == st && t->dim() == 2 && t->size(1) == V &&
                 (n_slots < 0 || t->size(0) == n_slots), name);
    n_slots = t->size(0);
  };
  table(state, at::kInt, "state i32 [n_slots, V]");
  table(bias, at::kFloat, "bias f32 [n_slots, V]");
  DevGuard g(logits.device());
  auto out = at::empty({B, V}, logits.options().dtype(at::kFloat));
  MX_OK(mx_logits_adjust_rows(logits.data_ptr(), logits.scalar_type() == at::kBFloat16 ? 1 : 0,
                              out.data_ptr<float>(), (int)B, (int)V,
                              state.has_value() ? state->data_ptr<int32_t>() : nullptr, slots.data_ptr<int32_t>(),
                              (int)std::max<int64_t>(n_slots, 0), presence.data_ptr<float>(),
                              frequency.data_ptr<float>(), repetition.data_ptr<float>(),
                              bias.has_value() ? bias->data_ptr<float>() : nullptr, cur_stream()));
  return out;
}

// state[slots[b], ids[b]] += 1 in place (slots < 0 skipped)
void token_state_update(at::Tensor state, const at::Tensor& slots, const at::Tensor& ids) {
  MX_CHECK(state.is_cuda() && state.is_contiguous() && state.scalar_type() == at::kInt && state.dim() == 2,
           "state i32 [n_slots, V] contiguous GPU");
  const int64_t B = slots.numel();
  MX_CHECK(slots.is_cuda() && slots.is_contiguous() && slots.scalar_type() == at::kInt, "slots i32 [B]");
  MX_CHECK(ids.is_cuda() && ids.is_contiguous() && ids.scalar_type() == at::kLong && ids.numel() == B, "ids i64 [B]");
  DevGuard g(state.device());
  MX_OK(mx_token_state_update(state.data_ptr<int32_t>(), slots.data_ptr<int32_t>(), ids.data_ptr<int64_t>(), (int)B,
                              (int)state.size(1), (int)state.size(0), cur_stream()));
}

// log-probabilities of the chosen and the n_top[b] most likely tokens of every row (logits_proc.hip)
std::tuple<at::Tensor, at::Tensor, at::Tensor> logprob_rows(const at::Tensor& logits, const at::Tensor& ids,
                                                            const at::Tensor& n_top) {
  MX_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, "logits [B, V] contiguous GPU");
  MX_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, "logits bf16/f32");
  const int64_t B = logits.size(0);
  MX_CHECK(ids.is_cuda() && ids.is_contiguous() && ids.scalar_type() == at::kLong && ids.numel() == B, "ids i64 [B]");
  MX_CHECK(n_top.is_cuda() && n_top.is_contiguous() && n_top.scalar_type() == at::kInt && n_top.numel() == B,
           "n_top i32 [B]");
  DevGuard g(logits.device());
  auto chosen = at::empty({B}, logits.options().dtype(at::kFloat));
  auto top_ids = at::empty({B, 20}, logits.options().dtype(at::kInt));
  auto top_lp = at::empty({B, 20}, logits.options().dtype(at::kFloat));
  MX_CHECK(B <= 65535 && logits.size(1) <= 2048 * 400, "logprob_rows: at most 65535 rows of at most 819200 logits");
  // per-call slice candidates / partial sums (stream-ordered allocator)
  auto ws = at::empty({std::max<int64_t>(1, (mx_logprob_ws_bytes((int)B, (int)logits.size(1)) + 7) / 8)},
                      logits.options().dtype(at::kLong));
  MX_OK(mx_logprob_rows(logits.data_ptr(), logits.scalar_type() == at::kBFloat16 ? 1 : 0, ids.data_ptr<int64_t>(),
                        n_top.data_ptr<int32_t>(), chosen.data_ptr<float>(), top_ids.data_ptr<int32_t>(),
                        top_lp.data_ptr<float>(), (int)B, (int)logits.size(1), ws.data_ptr(), cur_stream()));
  return {chosen, top_ids, top_lp};
}

}  // namespace


// ---------------------------------------------------------------- skinny decode GEMMs (serving)
// y[M, N] = x[M, K] . w[N, K]^T for decode-sized M on the weight-streaming HIP kernels
// (csrc/kernels/skinny_gemm.hip; fp8 weights: fp8_gemm.hip).  The helpers check what the ops are handed
// (type, rank, device) before anything is allocated; which shapes and strides a kernel takes is
// mx::sk_takes (csrc/kernels/skinny_args.h), asked by the launcher before it enqueues anything.
// a 2-D bf16 row view (unit inner stride, any row stride) on `dev`
static void sk_rows(const char* op, const char* name, const at::Tensor& t, const at::Device& dev) {
  MX_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == at::kBFloat16 && t.dim() == 2 && t.stride(1) == 1, op,
           ": ", name, " must be bf16 [rows, cols] GPU rows with a unit inner stride, on one device with the others");
}
static bool sk_ints(int64_t M, int64_t N, int64_t K) {
  const int64_t lim = std::numeric_limits<int>::max();
  return M <= lim && N <= lim && K <= lim;
}
// The operands every op shares, M rows of K (x [M, K], M >= 1, unless the op builds them) against w [N, K]
// on one device: entry, X, W, M, N, K of the description
static mx::SkLaunch sk_fill(const char* op, mx::SkEntry entry, const at::Tensor* x, const at::Tensor& w,
                            const at::Device& dev, int64_t M, int64_t K) {
  if (x) sk_rows(op, "x", *x, dev);
  sk_rows(op, "w", w, dev);
  MX_CHECK(w.size(1) == K && (!x || M >= 1) && sk_ints(M, w.size(0), K), op, ": ", M, " rows of ", K, " against w ",
           w.sizes());
  mx::SkLaunch L{};
  L.entry = entry, L.W = {w.data_ptr(), w.stride(0)}, L.M = (int)M, L.N = (int)w.size(0), L.K = (int)K;
  if (x) L.X = {x->data_ptr(), x->stride(0)};
  return L;
}
static mx::SkLaunch sk_fill(const char* op, mx::SkEntry entry, const at::Tensor& x, const at::Tensor& w) {
  MX_CHECK(x.dim() == 2, op, ": x must be [M, K]");
  return sk_fill(op, entry, &x, w, x.device(), x.size(0), x.size(1));
}
// The RMSNorm prologue's operands into L.na: gamma [K], optionally delta [M, K] rows.  Returns the new
// residual: h + delta (allocated here, written by the kernel), h itself without delta.
static at::Tensor sk_norm(const char* op, mx::SkLaunch& L, const at::Tensor& h, const c10::optional<at::Tensor>& delta,
                          const at::Tensor& gamma, double eps) {
  MX_CHECK(gamma.device() == h.device() && gamma.scalar_type() == at::kBFloat16 && gamma.is_contiguous() &&
               gamma.numel() == L.K, op, ": gamma must be contiguous bf16 [K] on h's device");
  L.na.gamma = bf(gamma);
  L.na.eps = (float)eps;
  if (!delta.has_value() || !delta->defined()) return h;
  sk_rows(op, "delta", *delta, h.device());
  MX_CHECK(delta->size(0) == L.M && delta->size(1) == L.K, op, ": delta must have h's shape");
  at::Tensor h_out = at::empty({L.M, L.K}, h.options());
  L.na.delta = bf(*delta), L.na.ldd = delta->stride(0), L.na.h_out = bfm(h_out);
  return h_out;
}
// The RoPE / KV-append epilogue's operands into L.rp (q: by the caller), as rope_append checks them
static void sk_rope(const char* op, mx::SkLaunch& L, const at::Tensor& h, const at::Tensor& cosb, const at::Tensor& sinb,
                    const at::Tensor& pos, const c10::optional<at::Tensor>& slots, at::Tensor& k_cache,
                    at::Tensor& v_cache, int64_t Hq, int64_t Hkv, const c10::optional<at::Tensor>& block_table) {
  MX_CHECK(Hq > 0 && Hkv > 0 && sk_ints(Hq, Hkv, 0), op, ": Hq, Hkv");
  check_kv_pools(k_cache, v_cache, at::kBFloat16, 128, h.device(), Hkv, op);
  for (const at::Tensor* t : {&cosb, &sinb})
    MX_CHECK(t->device() == h.device() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 2 &&
                 t->size(1) == 64, op, ": cos / sin must be contiguous float32 [positions, 64] on h's device");
  MX_CHECK(pos.defined(), op, ": pos");
  const int32_t* pp = check_rows_i32(pos, h.device(), L.M, op, "pos");
  const int32_t* sl = check_rows_i32(slots, h.device(), L.M, op, "slots");
  const KvPages pg = kv_pages(block_table, k_cache);
  L.rp = {cosb.data_ptr<float>(), sinb.data_ptr<float>(), pp, sl, nullptr, bfm(k_cache), bfm(v_cache), (int)Hq,
          (int)Hkv, (int)k_cache.size(2), pg.bt, pg.maxb};
}
// rc of a launcher that was handed L: -1 is sk_takes' refusal (nothing was launched), > 0 a HIP error
static void sk_launched(const char* op, int rc, const mx::SkLaunch& L) {
  MX_CHECK(rc != -1, op, ": the kernel does not take this call (mx::sk_takes, csrc/kernels/skinny_args.h): M ", L.M,
           ", N ", L.N, ", K ", L.K, ", row strides x ", L.X.ld, ", w ", L.W.ld, ", y ", L.Y.ld, ", delta ", L.na.ldd);
  TORCH_CHECK(rc == 0, "mxllm kernel launch failed (", op, ") rc=", rc, " ", hipGetErrorString((hipError_t)rc));
}
// y [M, cols] allocated like `t` (under the caller's device guard), the launch, its report
static at::Tensor sk_run(const char* op, mx::SkLaunch& L, const at::Tensor& t, int64_t cols) {
  auto y = at::empty({L.M, cols}, t.options());
  L.Y = {y.data_ptr(), cols};
  sk_launched(op, mx_skinny(L, cur_stream()), L);
  return y;
}

at::Tensor skinny_linear(const at::Tensor& x, const at::Tensor& w) {
  mx::SkLaunch L = sk_fill("skinny_linear", mx::SK_PLAIN, x, w);
  DevGuard g(x.device());
  return sk_run("skinny_linear", L, x, L.N);
}

// y[M, F] = swiglu(x . w^T), w = [gate; up] [2F, K] rows: the decode MLP's first projection with the
// SwiGLU in the GEMM epilogue
at::Tensor skinny_linear_swiglu(const at::Tensor& x, const at::Tensor& w) {
  mx::SkLaunch L = sk_fill("skinny_linear_swiglu", mx::SK_SWIGLU, x, w);
  DevGuard g(x.device());
  return sk_run("skinny_linear_swiglu", L, x, L.N / 2);
}

// Decode rows: y = rmsnorm(h + delta) . w^T with the RMSNorm (and residual add) in the GEMM prologue;
// swiglu: w = [gate; up], y = silu(g) * u.  Returns (y, h + delta) -- the new residual is h itself
// when delta is absent.
std::tuple<at::Tensor, at::Tensor> skinny_norm_linear(const at::Tensor& h, const c10::optional<at::Tensor>& delta,
                                                      const at::Tensor& gamma, double eps, const at::Tensor& w,
                                                      bool swiglu) {
  mx::SkLaunch L = sk_fill("skinny_norm_linear", mx::SK_NORM, h, w);
  L.swiglu = swiglu ? 1 : 0;
  DevGuard g(h.device());
  at::Tensor h_out = sk_norm("skinny_norm_linear", L, h, delta, gamma, eps);
  return {sk_run("skinny_norm_linear", L, h, swiglu ? L.N / 2 : L.N), h_out};
}

// Decode QKV projection with the RoPE / KV-cache append in the GEMM epilogue and, when gamma is
// given, the (residual-add +) RMSNorm in its prologue (delta counts only then).
// Returns (q [M, Hq, 128] rotated, new residual); K/V rows land in the caches at (slot, pos).
std::tuple<at::Tensor, at::Tensor> skinny_qkv_rope(const at::Tensor& h, const c10::optional<at::Tensor>& delta,
                                                   const c10::optional<at::Tensor>& gamma, double eps,
                                                   const at::Tensor& w, const at::Tensor& cosb, const at::Tensor& sinb,
                                                   const at::Tensor& pos, const c10::optional<at::Tensor>& slots,
                                                   at::Tensor& k_cache, at::Tensor& v_cache, int64_t Hq, int64_t Hkv,
                                                   const c10::optional<at::Tensor>& block_table) {
  mx::SkLaunch L = sk_fill("skinny_qkv_rope", mx::SK_ROPE, h, w);
  sk_rope("skinny_qkv_rope", L, h, cosb, sinb, pos, slots, k_cache, v_cache, Hq, Hkv, block_table);
  L.norm = gamma.has_value() && gamma->defined();
  DevGuard g(h.device());
  at::Tensor h_out = L.norm ? sk_norm("skinny_qkv_rope", L, h, delta, *gamma, eps) : h;
  auto q = at::empty({L.M, Hq, 128}, h.options());
  L.rp.q = bfm(q);
  sk_launched("skinny_qkv_rope", mx_skinny(L, cur_stream()), L);
  return {q, h_out};
}

// y [M, N] = merge(part_ml, part_o) . w^T: the decode o-projection with the split merge of
// decode_attn_partials in its prologue
at::Tensor skinny_merge_linear(const at::Tensor& ml, const at::Tensor& po, const at::Tensor& w) {
  MX_CHECK(ml.is_cuda() && ml.scalar_type() == at::kFloat && ml.is_contiguous() && ml.dim() == 4 && ml.size(3) == 2,
           "skinny_merge_linear: part_ml f32 [M, Hq, nsplit, 2]");
  MX_CHECK(po.device() == ml.device() && po.scalar_type() == at::kFloat && po.is_contiguous() && po.dim() == 4 &&
               po.size(0) == ml.size(0) && po.size(1) == ml.size(1) && po.size(2) == ml.size(2) && po.size(3) == 128,
           "skinny_merge_linear: part_o f32 [M, Hq, nsplit, 128]");
  mx::SkLaunch L = sk_fill("skinny_merge_linear", mx::SK_MERGE, nullptr, w, ml.device(), ml.size(0), ml.size(1) * 128);
  MX_CHECK(sk_ints(ml.size(2), 0, 0), "skinny_merge_linear: nsplit");
  L.mg = {ml.data_ptr<float>(), po.data_ptr<float>(), (int)ml.size(2)};
  DevGuard g(w.device());
  return sk_run("skinny_merge_linear", L, w, L.N);
}

// ---------------------------------------------------------------- fp8 weights (serving)
// y[M, N] = x[M, K] . (scale[:, None] * q[N, K])^T ; q: e4m3 codes (uint8), scale f32 [N].
// Calls the fused weight-streaming kernel takes (mx::sk_takes, SK_W8) run on it; the others
// dequantise to bf16 and run the hipBLASLt GEMM.  mxllm/serve/quant.py calls this only up to
// SMALL_M (8) tokens and routes larger calls to the fp8 x fp8 hipBLASLt GEMM.
at::Tensor w8_linear(const at::Tensor& x, const at::Tensor& q, const at::Tensor& scale) {
  sk_rows("w8_linear", "x", x, x.device());
  MX_CHECK(q.is_cuda() && q.scalar_type() == at::kByte && q.dim() == 2 && q.is_contiguous(), "q: uint8 [N, K]");
  check_f32(scale, "scale");
  const int64_t M = x.size(0), K = x.size(1), N = q.size(0);
  MX_CHECK(q.size(1) == K && scale.numel() == N, "w8_linear shapes");
  DevGuard g(x.device());
  auto y = at::empty({M, N}, x.options());
  mx::SkLaunch L{};
  L.entry = mx::SK_W8, L.X = {x.data_ptr(), x.stride(0)}, L.W = {q.data_ptr(), K}, L.Y = {y.data_ptr(), N};
  L.M = (int)M, L.N = (int)N, L.K = (int)K, L.scale = scale.data_ptr<float>();
  if (M == 0 || (sk_ints(M, N, K) && mx::sk_takes(L))) {  // no rows: an empty launch
    sk_launched("w8_linear", mx_w8a16_gemm(bf(x), x.stride(0), q.data_ptr<uint8_t>(), L.scale, bfm(y), N, L.M, L.N,
                                           L.K, cur_stream()), L);
    return y;
  }
  auto w = at::empty({N, K}, x.options());
  MX_OK(mx_w8_dequant(q.data_ptr<uint8_t>(), scale.data_ptr<float>(), bfm(w), N, (int)K, cur_stream()));
  return at::mm(x, w.t());
}

// per-token e4m3 quantisation of bf16 rows: (codes uint8 [M, K], scale f32 [M, 1])
std::tuple<at::Tensor, at::Tensor> quant_rows_e4m3(const at::Tensor& x) {
  MX_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.stride(1) == 1, "x: bf16 [M, K] rows");
  DevGuard g(x.device());
  const int64_t M = x.size(0), K = x.size(1);
  auto q = at::empty({M, K}, x.options().dtype(at::kByte));
  auto s = at::empty({M, 1}, x.options().dtype(at::kFloat));
  MX_OK(mx_quant_rows_e4m3(bf(x), x.stride(0), q.data_ptr<uint8_t>(), s.data_ptr<float>(), M, (int)K,
                           cur_stream()));
  return {q, s};
}

at::Tensor w8_dequant(const at::Tensor& q, const at::Tensor& scale) {
  MX_CHECK(q.is_cuda() && q.scalar_type() == at::kByte && q.dim() == 2 && q.is_contiguous(), "q: uint8 [N, K]");
  check_f32(scale, "scale");
  DevGuard g(q.device());
  auto w = at::empty({q.size(0), q.size(1)}, q.options().dtype(at::kBFloat16));
  MX_OK(mx_w8_dequant(q.data_ptr<uint8_t>(), scale.data_ptr<float>(), bfm(w), q.size(0), (int)q.size(1),
                      cur_stream()));
  return w;
}

// ---------------------------------------------------------------- MXFP4 weights (serving)
// codes u8 [N, K/2] (two e2m1 codes per byte, even k low), scales u8 [N, K/32] (e8m0): mxllm/serve/quant.py
static void w4_weights(const char* op, const at::Tensor& codes, const at::Tensor& scales, const at::Device& dev) {
  MX_CHECK(codes.is_cuda() && codes.device() == dev && codes.scalar_type() == at::kByte && codes.dim() == 2 &&
               codes.is_contiguous(), op, ": codes must be contiguous uint8 [N, K/2] on the GPU");
  MX_CHECK(scales.device() == dev && scales.scalar_type() == at::kByte && scales.dim() == 2 && scales.is_contiguous() &&
               scales.size(0) == codes.size(0) && codes.size(1) % 16 == 0 && scales.size(1) == codes.size(1) / 16,
           op, ": scales must be contiguous uint8 [N, K/32] beside codes [N, K/2], K % 32 == 0");
}

at::Tensor w4_dequant(const at::Tensor& codes, const at::Tensor& scales) {
  w4_weights("w4_dequant", codes, scales, codes.device());
  DevGuard g(codes.device());
  const int64_t N = codes.size(0), K = 2 * codes.size(1);
  auto w = at::empty({N, K}, codes.options().dtype(at::kBFloat16));
  MX_OK(mx_w4_dequant(codes.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>(), bfm(w), N, K, cur_stream()));
  return w;
}

// y[M, N] = x[M, K] . dequant(codes, scales)^T.  Up to 32 rows: one launch of the weight-streaming
// kernel.  33 .. stream_m rows: ceil(M / 32) launches over 32-row slices of x and y (the 4-bit weights
// are streamed that many times: at 64 rows as many bytes as one fp8 pass).  More rows, or a shape
// mx::w4_takes refuses: dequantise into a bf16 temporary and run the hipBLASLt GEMM.  Nothing here
// synchronises with the host, so all of it can be captured into a hipGraph.
at::Tensor w4_linear(const at::Tensor& x, const at::Tensor& codes, const at::Tensor& scales, int64_t stream_m) {
  sk_rows("w4_linear", "x", x, x.device());
  w4_weights("w4_linear", codes, scales, x.device());
  const int64_t M = x.size(0), K = x.size(1), N = codes.size(0);
  MX_CHECK(2 * codes.size(1) == K, "w4_linear: x has ", K, " columns, the codes ", 2 * codes.size(1));
  DevGuard g(x.device());
  auto y = at::empty({M, N}, x.options());
  if (M == 0 || N == 0) return y;
  const int64_t ldx = M <= 1 ? K : x.stride(0);  // the stride of a one-row view is arbitrary
  mx::W4Launch L{};
  L.x = x.data_ptr(), L.ldx = ldx, L.codes = codes.data_ptr(), L.scales = scales.data_ptr();
  L.y = y.data_ptr(), L.ldy = N;
  L.M = std::min<int64_t>(M, mx::W4_MAX_M), L.N = N, L.K = K;
  if (M <= std::max<int64_t>(stream_m, mx::W4_MAX_M) && mx::w4_takes(L)) {
    for (int64_t m0 = 0; m0 < M; m0 += mx::W4_MAX_M) {
      L.x = bf(x) + m0 * ldx, L.y = bfm(y) + m0 * N, L.M = std::min<int64_t>(M - m0, mx::W4_MAX_M);
      const int rc = mx_w4a16_gemm(L, cur_stream());
      MX_CHECK(rc != -1, "w4_linear: the kernel does not take this call (mx::w4_takes, csrc/kernels/w4_args.h): M ", L.M,
               ", N ", N, ", K ", K, ", row stride x ", ldx);
      TORCH_CHECK(rc == 0, "mxllm kernel launch failed (w4_linear) rc=", rc, " ", hipGetErrorString((hipError_t)rc));
    }
    return y;
  }
  auto w = at::empty({N, K}, x.options());
  MX_OK(mx_w4_dequant(codes.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>(), bfm(w), N, K, cur_stream()));
  return at::mm(x, w.t());
}

// ---------------------------------------------------------------- LoRA rank-r GEMMs
// out[:, 0:Vrows] = alpha * x . v^T (x [M, K], v [Vrows, K] row views, Vrows % 64 == 0):
// the forward s x A^T / backward s dy B products written into the augmented-GEMM tails.
// rows > 0: only v's first `rows` rows are non-zero (the adapter; the rest is padding).
void lora_xwt(const at::Tensor& x, const at::Tensor& v, at::Tensor& out, double alpha, int64_t rows) {
  const int64_t ldx = check_rows_bf16(x, "x"), ldv = check_rows_bf16(v, "v"), ldo = check_rows_bf16(out, "out");
  const int64_t M = x.size(0), K = x.size(1), Vr = v.size(0);
  MX_CHECK(v.size(1) == K && out.size(0) == M && out.size(1) >= Vr, "lora_xwt shapes");
  MX_CHECK(rows >= 0 && rows <= Vr, "lora_xwt: rows <= rows(v)");
  MX_CHECK(M % 16 == 0 && K % 64 == 0 && Vr % 64 == 0 && ldo % 4 == 0,
           "lora_xwt: M % 16, K % 64, rows(v) % 64");
  DevGuard g(x.device());
  const int64_t nws = mx_lora_xwt_ws((int)M, (int)K, (int)rows);
  auto ws = at::empty({nws > 0 ? nws : 1}, x.options().dtype(at::kFloat));
  MX_OK(mx_lora_xwt(bf(x), ldx, bf(v), ldv, (int)Vr, bfm(out), ldo, ws.data_ptr<float>(), (int)M, (int)K, (float)alpha,
                    (int)rows, cur_stream()));
}

// LoRA adapter gradients in ONE launch: ga [R, K] (+)= g^T x and the diagonal blocks
// gb[off_i : off_i + n_i, i r : (i + 1) r] (+)= dy_i^T st_i.  x [T, K], dy [T, N], and the
// tails g [T, >= 64], st [T, >= 64] (row views); r % 16 == 0.
void lora_grads(const at::Tensor& x, const at::Tensor& dy, const at::Tensor& g, const at::Tensor& st, at::Tensor& ga,
                at::Tensor& gb, at::IntArrayRef splits, int64_t r, bool accumulate) {
  const int64_t ldx = check_rows_bf16(x, "x"), ldd = check_rows_bf16(dy, "dy");
  const int64_t ldg = check_rows_bf16(g, "g"), lds = check_rows_bf16(st, "st");
  check_bf16(ga, "ga");
  check_bf16(gb, "gb");
  const int64_t T = x.size(0), K = x.size(1), N = dy.size(1), n = (int64_t)splits.size(), R = n * r;
  MX_CHECK(dy.size(0) == T && g.size(0) == T && st.size(0) == T, "lora_grads: token counts differ");
  MX_CHECK(ga.size(0) == R && ga.size(1) == K && gb.size(0) == N && gb.size(1) == R, "lora_grads: grad shapes");
  MX_CHECK(T % 64 == 0 && K % 64 == 0 && r % 16 == 0 && r <= 64, "lora_grads: T, K multiples of 64, r of 16");
  std::vector<int64_t> desc;
  auto add = [&](const uint16_t* X, int64_t lx, const uint16_t* G, int64_t lg, int64_t gw, uint16_t* out, int64_t os_n,
                 int64_t os_j, int64_t Nx, int64_t jb0, int64_t JB) {
    MX_CHECK(16 * (jb0 + JB) <= gw, "lora_grads: operand tail too narrow");
    MX_CHECK(Nx % 64 == 0, "lora_grads: split sizes must be multiples of 64");
    // JB > 1 reads a 64-column G window starting at column 16 jb0.  Where that window would run past the
    // tail (two splits of r = 32 in a 64-column pad: the second split's blocks are columns 32..63), the
    // blocks go as JB problems of one block each: the one-block form reads its 16 columns only
    if (JB > 1 && 16 * jb0 + 64 > gw) {
      for (int64_t j = 0; j < JB; ++j)
        desc.insert(desc.end(), {(int64_t)X, (int64_t)G, (int64_t)(out + 16 * j * os_j), lx, lg, os_n, os_j, Nx,
                                 jb0 + j, (int64_t)1});
      return;
    }
    desc.insert(desc.end(), {(int64_t)X, (int64_t)G, (int64_t)out, lx, lg, os_n, os_j, Nx, jb0, JB});
  };
  // dA: R columns of g in chunks of <= 4 blocks
  for (int64_t j0 = 0; j0 < R; j0 += 64) {
    const int64_t jb = std::min<int64_t>(4, (R - j0) / 16);
    add(bf(x), ldx, bf(g), ldg, g.size(1), bfm(ga) + j0 * K, 1, K, K, j0 / 16, jb);
  }
  int64_t off = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t ni = splits[i];
    add(bf(dy) + off, ldd, bf(st), lds, st.size(1), bfm(gb) + off * R + i * r, R, 1, ni, i * r / 16, r / 16);
    off += ni;
  }
  MX_CHECK(off == N, "lora_grads: splits do not sum to dy's width");
  const int np = (int)(desc.size() / 10);
  MX_CHECK(np <= 8, "lora_grads: too many problems");
  int64_t ntiles = 0;
  for (int i = 0; i < np; ++i) ntiles += desc[i * 10 + 7] / 64;
  DevGuard gd(x.device());
  const int64_t nws = mx_lora_xtg_ws((int)ntiles, (int)T);
  auto ws = at::empty({nws > 0 ? nws : 1}, x.options().dtype(at::kFloat));
  MX_OK(mx_lora_xtg(desc.data(), np, (int)T, 1.0f, accumulate ? 1 : 0, ws.data_ptr<float>(), cur_stream()));
}

// ---------------------------------------------------------------- multi-adapter LoRA for serving (lora_serve.hip)
// The operand check of lora_gather_shrink and lora_gather_expand_add_ (op: the caller's name): the
// rows (x or y), the per-row adapter ids, the table those rows gather from and the partials
// between the two launches.  Every check runs before anything is launched or written.
struct LoraServeCall {
  int64_t M, W, ld, n_adapters, KS, R;  // W: the rows' width (K of x, N of y)
  const int32_t* ids;
};
static LoraServeCall check_lora_serve(const char* op, const at::Tensor& rows, const char* rows_name,
                                      const at::Tensor& ids, const at::Tensor& tab, int64_t tab_w_dim,
                                      const at::Tensor& partials, int64_t K) {
  MX_CHECK(rows.is_cuda() && rows.scalar_type() == at::kBFloat16 && rows.dim() == 2 && rows.size(0) >= 1, op, ": ",
           rows_name, " must be a bfloat16 [M, ", tab_w_dim == 2 ? "K" : "N", "] GPU tensor with M >= 1");
  MX_CHECK(rows.stride(1) == 1 && rows.stride(0) >= rows.size(1) && rows.stride(0) % 8 == 0 &&
               reinterpret_cast<uintptr_t>(rows.data_ptr()) % 16 == 0,
           op, ": ", rows_name, " must be a 16-byte aligned row-major view with a row stride that is a multiple of 8");
  LoraServeCall c{rows.size(0), rows.size(1), rows.stride(0), 0, 0, 0, nullptr};
  MX_CHECK(c.W >= 8 && c.W % 8 == 0, op, ": ", rows_name, " has ", c.W, " columns, not a positive multiple of 8");
  MX_CHECK(c.M < (int64_t(1) << 31) && c.ld < (int64_t(1) << 31), op, ": ", rows_name, " is too large");
  c.ids = check_rows_i32(ids, rows.device(), c.M, op, "ids");
  MX_CHECK(c.ids != nullptr, op, ": ids");
  MX_CHECK(tab.device() == rows.device() && tab.scalar_type() == at::kBFloat16 && tab.is_contiguous() &&
               tab.dim() == 3 && tab.size(0) >= 1 && tab.size(tab_w_dim) == c.W,
           op, ": the table must be a contiguous bfloat16 ", tab_w_dim == 2 ? "[n_adapters, R, K]" : "[n_adapters, N, r_max]",
           " tensor on ", rows_name, "'s device whose ", tab_w_dim == 2 ? "K" : "N", " is ", c.W);
  c.n_adapters = tab.size(0);
  c.KS = mx_lora_serve_ksplits((int)(tab_w_dim == 2 ? c.W : K));
  MX_CHECK(partials.device() == rows.device() && partials.scalar_type() == at::kFloat && partials.is_contiguous() &&
               partials.dim() == 3 && partials.size(0) == c.KS && partials.size(1) == c.M,
           op, ": partials must be a contiguous float32 [", c.KS, ", ", c.M, ", R] tensor on ", rows_name, "'s device");
  c.R = partials.size(2);
  return c;
}

// x [M, K] -> partials [ceil(K / 512), M, R] (written for the rows whose id is >= 0)
void lora_gather_shrink(const at::Tensor& x, const at::Tensor& ids, const at::Tensor& a_tab, at::Tensor partials) {
  const LoraServeCall c = check_lora_serve("lora_gather_shrink", x, "x", ids, a_tab, 2, partials, 0);
  MX_CHECK(a_tab.size(1) == c.R && c.R % 8 == 0 && c.R >= 8 && c.R <= 192, "lora_gather_shrink: A_tab holds ",
           a_tab.size(1), " rows per adapter and partials ", c.R, "; both must be n_splits * r_max <= 192");
  DevGuard g(x.device());
  MX_OK(mx_lora_gather_shrink(bf(x), c.ld, c.ids, bf(a_tab), partials.data_ptr<float>(), (int)c.M, (int)c.W, (int)c.R,
                              (int)c.n_adapters, cur_stream()));
}

// y [M, N] += s * t B^T per row, t = the sum of the partials over the K splits of a projection of K inputs
void lora_gather_expand_add_(at::Tensor y, const at::Tensor& partials, const at::Tensor& ids, const at::Tensor& b_tab,
                             const at::Tensor& s_tab, at::IntArrayRef splits, int64_t K) {
  const char* op = "lora_gather_expand_add_";
  MX_CHECK(K >= 8 && K % 8 == 0 && K < (int64_t(1) << 31), op, ": K must be a positive multiple of 8");
  const LoraServeCall c = check_lora_serve(op, y, "y", ids, b_tab, 1, partials, K);
  const int64_t r_max = b_tab.size(2), ns = (int64_t)splits.size();
  MX_CHECK(r_max == 8 || r_max == 16 || r_max == 32 || r_max == 64, op, ": r_max must be 8, 16, 32 or 64, got ", r_max);
  MX_CHECK(ns >= 1 && ns <= 3, op, ": 1 to 3 splits, got ", ns);
  int sp[3] = {0, 0, 0};
  int64_t sum = 0;
  for (int64_t i = 0; i < ns; ++i) {
    MX_CHECK(splits[i] >= 8 && splits[i] % 8 == 0, op, ": every split must be a positive multiple of 8, got ", splits[i]);
    sp[i] = (int)splits[i];
    sum += splits[i];
  }
  MX_CHECK(sum == c.W, op, ": the splits sum to ", sum, ", y has ", c.W, " columns");
  MX_CHECK(c.R == ns * r_max, op, ": partials hold ", c.R, " columns, expected n_splits * r_max = ", ns * r_max);
  MX_CHECK(s_tab.device() == y.device() && s_tab.scalar_type() == at::kFloat && s_tab.is_contiguous() &&
               s_tab.dim() == 1 && s_tab.size(0) == c.n_adapters,
           op, ": s_tab must be a contiguous float32 [n_adapters] tensor on y's device");
  DevGuard g(y.device());
  MX_OK(mx_lora_gather_expand_add(bfm(y), c.ld, partials.data_ptr<float>(), c.ids, bf(b_tab), s_tab.data_ptr<float>(),
                                  (int)c.M, (int)c.W, (int)c.KS, (int)r_max, sp, (int)ns, (int)c.n_adapters,
                                  cur_stream()));
}

TORCH_LIBRARY(mxllm, m) {
  m.def("rmsnorm_fwd(Tensor x, Tensor? res, Tensor w, float eps, int out_pad=0) -> (Tensor, Tensor, Tensor)");
  m.def("rmsnorm_bwd(Tensor dy, Tensor x, Tensor w, Tensor rstd, Tensor? dres, bool need_dw, int out_pad=0) -> (Tensor, Tensor)");
  m.def("segmented_mean(Tensor codes, Tensor offsets) -> Tensor");
  m.def("copy2d_batched(Tensor desc, int total_blocks) -> ()");
  m.def("transpose2d(Tensor x, Tensor? scale=None) -> Tensor");
  m.def("gemm8(Tensor a, bool a_kc, Tensor b, bool b_kc, Tensor(a!) out, float beta, Tensor? alpha_t=None, float alpha=1.0, int ph=8) -> bool");
  m.def("prefetch(Tensor t, int wgs) -> ()");
  m.def("cu_masked_stream(int device, int[] mask) -> int", &cu_masked_stream);  // no tensor args: catch-all
  m.def("gemm8_stamps() -> Tensor", &gemm8_stamps);
  m.def("gemm8_tail(Tensor a, bool a_kc, Tensor b, bool b_kc, Tensor(a!) out, int at, bool rows=False, int ph=4, Tensor(b!)? sq=None) -> bool");
  m.def("gemm8_rope(Tensor x, Tensor w, Tensor cos, Tensor sin, int B, int S, int Hq, int Hkv, Tensor(a!) q, Tensor(b!) k, Tensor(c!) v) -> bool");
  m.def("gemm8_rope_tail(Tensor x, Tensor w, Tensor cos, Tensor sin, int B, int S, int Hq, int Hkv, Tensor(a!) q, Tensor(b!) k, Tensor(c!) v, int at) -> bool");
  m.def("gemm8_swiglu(Tensor x, Tensor w, Tensor(a!) gu, Tensor(b!) m) -> bool");
  m.def("gemm8_sq(Tensor a, bool a_kc, Tensor b, bool b_kc, Tensor(a!) out, Tensor(b!) sq, Tensor? alpha_t=None, float alpha=1.0) -> bool");
  m.def("gemm8_swiglu_bwd(Tensor dy, Tensor w, Tensor gu, Tensor(a!) dgu, Tensor(b!)? m=None) -> bool");
  m.def("sqnorm(Tensor x) -> Tensor");
  m.def("swiglu_fwd(Tensor gu, int out_pad=0) -> Tensor");
  m.def("swiglu_bwd(Tensor dm, Tensor gu, int out_pad=0) -> Tensor");
  m.def("swiglu_bwd_m(Tensor dm, Tensor gu) -> Tensor[]");
  m.def("adamw_step(Tensor(a!)? master, Tensor(e!) grad, Tensor(b!) m, Tensor(c!) v, Tensor(d!)? lowp, Tensor(f!)? lo, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, Tensor? scale_t, float scale_f, bool zero_grad=False) -> ()");
  m.def("split_master(Tensor x, Tensor(a!) hi, Tensor(b!) lo) -> ()");
  m.def("join_master(Tensor hi, Tensor lo, Tensor(a!) out) -> ()");
  m.def("embedding_fwd(Tensor ids, Tensor w) -> Tensor");
  m.def("embedding_bwd(Tensor dy, Tensor ids, int V) -> Tensor");
  m.def("embedding_bwd_sorted(Tensor dy, Tensor sid, Tensor perm, Tensor(a!) out) -> ()");
  m.def("ce_fwd_bwd(Tensor(a!) logits, Tensor labels, int ignore_index) -> (Tensor, Tensor)");
  m.def("ce_inv_count(Tensor labels, int ignore_index, int vocab) -> Tensor");
  m.def("ce_chunk(Tensor(a!) logits, Tensor labels, int ignore_index, Tensor inv_n) -> Tensor");
  m.def("ce_chunk_f32(Tensor logits, Tensor(a!) dl, Tensor labels, int ignore_index, Tensor inv_n) -> Tensor");
  m.def("rope_split(Tensor qkv, Tensor cos, Tensor sin, int B, int S, int Hq, int Hkv, int D, Tensor? positions=None) -> (Tensor, Tensor, Tensor)");
  m.def("rope_merge_bwd(Tensor dq, Tensor dkp, Tensor dvp, Tensor cos, Tensor sin, int B, int S, int Hq, int Hkv, int D, int out_pad=0) -> Tensor");
  m.def("attn_fwd(Tensor q, Tensor k, Tensor v, bool causal, float scale, int out_pad=0) -> (Tensor, Tensor)");
  m.def("rope_append(Tensor qkv, Tensor cos, Tensor sin, Tensor pos, Tensor? slots, Tensor(a!) k_cache, Tensor(b!) v_cache, int Hq, int Hkv, int D, Tensor? block_table=None) -> Tensor");
  m.def("decode_attn(Tensor q, Tensor k_cache, Tensor v_cache, Tensor lens, Tensor? slots, int max_len, float scale, int len_off=0, Tensor? block_table=None, Tensor? counters=None) -> Tensor");
  m.def("decode_attn_partials(Tensor q, Tensor k_cache, Tensor v_cache, Tensor lens, Tensor? slots, int max_len, float scale, int len_off=0, Tensor? block_table=None) -> (Tensor, Tensor)");
  m.def("prefill_attn_paged(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, Tensor segs, float scale, Tensor? out=None) -> Tensor");
  m.def("kv8_quant_rows(Tensor x) -> (Tensor, Tensor)");
  m.def("rope_append_kv8(Tensor qkv, Tensor cos, Tensor sin, Tensor pos, Tensor? slots, Tensor(a!) k_codes, Tensor(b!) k_scale, Tensor(c!) v_codes, Tensor(d!) v_scale, int Hq, int Hkv, Tensor? block_table=None) -> Tensor");
  m.def("decode_attn_kv8(Tensor q, Tensor k_codes, Tensor k_scale, Tensor v_codes, Tensor v_scale, Tensor lens, Tensor? slots, int max_len, float scale, int len_off=0, Tensor? block_table=None) -> Tensor");
  m.def("verify_attn(Tensor q, Tensor k_cache, Tensor v_cache, Tensor lens, Tensor nq, Tensor? slots, int n, int max_len, float scale, Tensor? block_table=None, Tensor? out=None) -> Tensor");
  m.def("verify_attn_kv8(Tensor q, Tensor k_codes, Tensor k_scale, Tensor v_codes, Tensor v_scale, Tensor lens, Tensor nq, Tensor? slots, int n, int max_len, float scale, Tensor? block_table=None, Tensor? out=None) -> Tensor");
  m.def("spec_accept(Tensor drawn, Tensor tokens, Tensor nq) -> Tensor");
  m.def("skinny_merge_linear(Tensor ml, Tensor po, Tensor w) -> Tensor");
  m.def("sample(Tensor logits, float temperature, int seed, int step) -> Tensor");
  m.def("sample_rows(Tensor logits, Tensor temps, Tensor top_p, Tensor top_k, Tensor seeds, Tensor steps) -> Tensor");
  m.def("sample_temp_rows(Tensor logits, Tensor temps, Tensor seeds, Tensor steps) -> Tensor");
  m.def("logits_adjust_rows(Tensor logits, Tensor? state, Tensor slots, Tensor presence, Tensor frequency, "
        "Tensor repetition, Tensor? bias) -> Tensor");
  m.def("token_state_update(Tensor(a!) state, Tensor slots, Tensor ids) -> ()");
  m.def("logprob_rows(Tensor logits, Tensor ids, Tensor n_top) -> (Tensor, Tensor, Tensor)");
  m.def("w8_linear(Tensor x, Tensor q, Tensor scale) -> Tensor");
  m.def("skinny_linear(Tensor x, Tensor w) -> Tensor");
  m.def("skinny_linear_swiglu(Tensor x, Tensor w) -> Tensor");
  m.def("skinny_qkv_rope(Tensor h, Tensor? delta, Tensor? gamma, float eps, Tensor w, Tensor cos, Tensor sin, Tensor pos, Tensor? slots, Tensor(a!) k_cache, Tensor(b!) v_cache, int Hq, int Hkv, Tensor? block_table=None) -> (Tensor, Tensor)");
  m.def("skinny_norm_linear(Tensor h, Tensor? delta, Tensor gamma, float eps, Tensor w, bool swiglu) -> (Tensor, Tensor)");
  m.def("w8_dequant(Tensor q, Tensor scale) -> Tensor");
  m.def("w4_linear(Tensor x, Tensor codes, Tensor scales, int stream_m) -> Tensor");
  m.def("w4_dequant(Tensor codes, Tensor scales) -> Tensor");
  m.def("quant_rows_e4m3(Tensor x) -> (Tensor, Tensor)");
  m.def("lora_xwt(Tensor x, Tensor v, Tensor(a!) out, float alpha, int rows=0) -> ()");
  m.def("swiglu_lora(Tensor? dm, Tensor gu, int pad, Tensor v, int nrb, float alpha) -> Tensor");
  m.def("lora_grads(Tensor x, Tensor dy, Tensor g, Tensor st, Tensor(a!) ga, Tensor(b!) gb, int[] splits, int r, bool accumulate) -> ()");
  m.def("lora_gather_shrink(Tensor x, Tensor ids, Tensor a_tab, Tensor(a!) partials) -> ()");
  m.def("lora_gather_expand_add_(Tensor(a!) y, Tensor partials, Tensor ids, Tensor b_tab, Tensor s_tab, int[] splits, int K) -> ()");
  m.def("attn_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, bool causal, float scale, int dq_mode=3, Tensor? dq_out=None, Tensor? dk_out=None, Tensor? dv_out=None) -> (Tensor, Tensor, Tensor)");
  m.def("attn_bwd_rope(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, bool causal, float scale, Tensor cos, Tensor sin, int out_pad=0) -> Tensor");
}

TORCH_LIBRARY_IMPL(mxllm, CUDA, m) {
  m.impl("rmsnorm_fwd", &rmsnorm_fwd);
  m.impl("rmsnorm_bwd", &rmsnorm_bwd);
  m.impl("segmented_mean", &segmented_mean);
  m.impl("copy2d_batched", &copy2d_batched);
  m.impl("transpose2d", &transpose2d);
  m.impl("gemm8", &gemm8);
  m.impl("gemm8_tail", &gemm8_tail);
  m.impl("gemm8_rope", &gemm8_rope);
  m.impl("gemm8_rope_tail", &gemm8_rope_tail);
  m.impl("gemm8_swiglu", &gemm8_swiglu);
  m.impl("gemm8_sq", &gemm8_sq);
  m.impl("gemm8_swiglu_bwd", &gemm8_swiglu_bwd);
  m.impl("ce_inv_count", &ce_inv_count);
  m.impl("ce_chunk", &ce_chunk);
  m.impl("ce_chunk_f32", &ce_chunk_f32);
  m.impl("prefetch", &prefetch);
  m.impl("sqnorm", &sqnorm);
  m.impl("swiglu_fwd", &swiglu_fwd);
  m.impl("swiglu_bwd", &swiglu_bwd);
  m.impl("swiglu_bwd_m", &swiglu_bwd_m);
  m.impl("adamw_step", &adamw_step);
  m.impl("split_master", &split_master);
  m.impl("join_master", &join_master);
  m.impl("embedding_fwd", &embedding_fwd);
  m.impl("embedding_bwd", &embedding_bwd);
  m.impl("embedding_bwd_sorted", &embedding_bwd_sorted);
  m.impl("ce_fwd_bwd", &ce_fwd_bwd);
  m.impl("rope_split", &rope_split);
  m.impl("rope_merge_bwd", &rope_merge_bwd);
  m.impl("attn_fwd", &attn_fwd);
  m.impl("attn_bwd", &attn_bwd);
  m.impl("attn_bwd_rope", &attn_bwd_rope);
  m.impl("rope_append", &rope_append);
  m.impl("decode_attn_partials", &decode_attn_partials);
  m.impl("skinny_merge_linear", &skinny_merge_linear);
  m.impl("decode_attn", &decode_attn);
  m.impl("prefill_attn_paged", &prefill_attn_paged);
  m.impl("kv8_quant_rows", &kv8_quant_rows);
  m.impl("rope_append_kv8", &rope_append_kv8);
  m.impl("decode_attn_kv8", &decode_attn_kv8);
  m.impl("spec_accept", &spec_accept);
  m.impl("verify_attn", &verify_attn);
  m.impl("verify_attn_kv8", &verify_attn_kv8);
  m.impl("sample", &sample);
  m.impl("sample_rows", &sample_rows);
  m.impl("sample_temp_rows", &sample_temp_rows);
  m.impl("logits_adjust_rows", &logits_adjust_rows);
  m.impl("token_state_update", &token_state_update);
  m.impl("logprob_rows", &logprob_rows);
  m.impl("w8_linear", &w8_linear);
  m.impl("skinny_linear", &skinny_linear);
  m.impl("skinny_linear_swiglu", &skinny_linear_swiglu);
  m.impl("skinny_qkv_rope", &skinny_qkv_rope);
  m.impl("skinny_norm_linear", &skinny_norm_linear);
  m.impl("w8_dequant", &w8_dequant);
  m.impl("w4_linear", &w4_linear);
  m.impl("w4_dequant", &w4_dequant);
  m.impl("quant_rows_e4m3", &quant_rows_e4m3);
  m.impl("lora_xwt", &lora_xwt);
  m.impl("swiglu_lora", &swiglu_lora);
  m.impl("lora_grads", &lora_grads);
  m.impl("lora_gather_shrink", &lora_gather_shrink);
  m.impl("lora_gather_expand_add_", &lora_gather_expand_add_);
}
