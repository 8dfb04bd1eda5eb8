// PyTorch-ROCm custom ops over the kwhisper C ABI (include/kwhisper.h): torch.ops.kw.*
//
// "Torch custom ops (torch.ops.kw.*) wrap the ABI".  Each op takes device tensors plus
// plain integers, fills the ABI's argument block, and launches on torch's CURRENT HIP stream (so the
// kernels order with torch's own work and are captured by torch.cuda.graph like any torch op).  The ops
// mutate their output tensors in place (schema annotations Tensor(a!)) and return nothing; there is no
// CPU kernel and no fallback: a non-HIP tensor is rejected.  Error behaviour mirrors the ctypes binding:
// KW_EINVAL -> ValueError, any other code -> RuntimeError, both with kw_last_error()'s message.
//
// The C ABI stays the boundary beneath (libkwhisper.so, linked, not re-implemented here).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <cstdint>
#include <string>
#include <vector>

#include "kwhisper.h"

namespace {

using at::Tensor;
using std::optional;

void* stream_of(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

void check(int rc, const char* what) {
  if (rc == KW_OK) return;
  const char* msg = kw_last_error();
  TORCH_CHECK_VALUE(rc != KW_EINVAL, what, ": ", msg ? msg : "");
  TORCH_CHECK(false, what, " failed (code ", rc, "): ", msg ? msg : "");
}

void dev(const Tensor& t, const char* what) {
  TORCH_CHECK_VALUE(t.is_cuda(), what, ": kwhisper ops take device (HIP) tensors");
}
void dev(const optional<Tensor>& t, const char* what) {
  if (t.has_value()) dev(*t, what);
}

int dt_of(const Tensor& t) {
  if (t.scalar_type() == at::kFloat) return KW_DT_F32;
  if (t.scalar_type() == at::kBFloat16) return KW_DT_BF16;
  TORCH_CHECK_VALUE(false, "unsupported dtype ", t.scalar_type(), "; expected float32 or bfloat16");
}

template <typename T = void>
T* ptr(const Tensor& t, int64_t offset_elems = 0) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(t.data_ptr()) + offset_elems * t.element_size());
}
template <typename T = void>
T* optr(const optional<Tensor>& t) {
  return t.has_value() ? ptr<T>(*t) : nullptr;
}

int64_t at_(const std::vector<int64_t>& v, size_t i, const char* what) {
  TORCH_CHECK_VALUE(i < v.size(), what, ": argument list too short");
  return v[i];
}

// ---- a1 log-mel ---------------------------------------------------------------------------------------
void log_mel(const Tensor& audio, const Tensor& mel_filters, Tensor& out, Tensor& workspace) {
  dev(audio, "kw_log_mel");
  dev(mel_filters, "kw_log_mel");
  dev(out, "kw_log_mel");
  dev(workspace, "kw_log_mel");
  TORCH_CHECK_VALUE(audio.dim() == 2 && audio.scalar_type() == at::kFloat && audio.stride(1) == 1,
                    "audio must be a (B, n_samples) float32 tensor with unit inner stride");
  c10::DeviceGuard g(audio.device());
  check(kw_log_mel(ptr<const float>(audio), audio.size(0), audio.size(1), audio.stride(0), ptr<const float>(mel_filters),
                   (int)mel_filters.size(1), ptr<float>(out), ptr(workspace), stream_of(audio)),
        "kw_log_mel");
}

void mel_to_time_major(const Tensor& mel, int64_t c_pad, Tensor& out) {
  dev(mel, "kw_mel_to_time_major");
  dev(out, "kw_mel_to_time_major");
  TORCH_CHECK_VALUE(mel.dim() == 3 && mel.is_contiguous() && mel.scalar_type() == at::kFloat,
                    "mel must be a contiguous (B, C, T) float32 tensor");
  c10::DeviceGuard g(mel.device());
  check(kw_mel_to_time_major(ptr<const float>(mel), mel.size(0), mel.size(1), mel.size(2), c_pad, ptr(out), dt_of(out),
                             stream_of(mel)),
        "kw_mel_to_time_major");
}

// ---- linear / conv-as-GEMM ----------------------------------------------------------------------------
// geo = [a_offset, lda, a_rows_per_batch, a_batch_stride, c_offset, ldc, c_rows_per_batch, c_batch_stride,
//        M, N, K, epilogue, gelu, scale_cols, row_add_period, hs_seq, hs_heads, hs_head_dim]
void gemm(const Tensor& A, const Tensor& W, const optional<Tensor>& bias, Tensor& C, const optional<Tensor>& row_add,
          std::vector<int64_t> geo, double scale, int64_t dtype) {
  const char* w = "kw_gemm";
  dev(A, w), dev(W, w), dev(bias, w), dev(C, w), dev(row_add, w);
  TORCH_CHECK_VALUE(geo.size() == 18, "kw_gemm: geo must hold 18 integers");
  kw_gemm_args a{};
  a.dtype = dtype >= 0 ? (int)dtype : dt_of(W);
  a.c_dtype = dt_of(C);
  a.A = ptr(A, geo[0]);
  a.lda = geo[1], a.a_rows_per_batch = geo[2], a.a_batch_stride = geo[3];
  a.W = ptr(W);
  a.bias = optr<const float>(bias);
  a.C = ptr(C, geo[4]);
  a.ldc = geo[5], a.c_rows_per_batch = geo[6], a.c_batch_stride = geo[7];
  a.M = geo[8], a.N = geo[9], a.K = geo[10];
  a.epilogue = (int)geo[11];
  a.gelu = (int)geo[12];
  a.scale = (float)scale;
  a.scale_cols = geo[13];
  a.row_add = optr<const float>(row_add);
  a.row_add_period = geo[14];
  a.hs_seq = geo[15], a.hs_heads = geo[16], a.hs_head_dim = geo[17];
  c10::DeviceGuard g(W.device());
  check(kw_gemm(&a, stream_of(W)), w);
}

// ---- decode-step linear over packed weights -----------------------------------------------------------
// geo = [x_offset, ldx, ln, c_offset, ldc, gelu, scale_cols, resid_row0, ldh, M, N, K (, epilogue flags: KW_EPI_HB_TILED)]
void dec_linear(const Tensor& x, const Tensor& W, const optional<Tensor>& bias, const optional<Tensor>& ln_colsum,
                optional<Tensor> C, optional<Tensor> h, optional<Tensor> hb, Tensor& workspace,
                std::vector<int64_t> geo, double ln_eps, double scale) {
  const char* w = "kw_dec_linear";
  dev(x, w), dev(W, w), dev(bias, w), dev(ln_colsum, w), dev(C, w), dev(h, w), dev(hb, w), dev(workspace, w);
  TORCH_CHECK_VALUE(geo.size() == 12 || geo.size() == 13, "kw_dec_linear: geo must hold 12 or 13 integers");
  TORCH_CHECK_VALUE(x.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16,
                    "kw_dec_linear takes bf16 activations and packed bf16 weights");
  kw_dec_linear_args a{};
  a.x = ptr(x, geo[0]);
  a.ldx = geo[1];
  a.ln = (int)geo[2];
  a.ln_eps = (float)ln_eps;
  a.ln_colsum = optr<const float>(ln_colsum);
  a.W = ptr(W);
  a.bias = optr<const float>(bias);
  if (h.has_value()) {
    TORCH_CHECK_VALUE(hb.has_value() && h->scalar_type() == at::kFloat && hb->scalar_type() == at::kBFloat16,
                      "RESID needs an f32 residual and a bf16 mirror");
    a.epilogue = KW_EPI_RESID | (geo.size() > 12 ? (int)geo[12] : 0);
    a.h = ptr<float>(*h, geo[7] * geo[8]);
    a.hb = ptr(*hb, geo[7] * geo[8]);
    a.ldh = geo[8];
  } else {
    TORCH_CHECK_VALUE(C.has_value(), "STORE needs C");
    a.epilogue = KW_EPI_STORE;
    a.C = ptr(*C, geo[3]);
    a.ldc = geo[4];
    a.c_dtype = dt_of(*C);
  }
  a.gelu = (int)geo[5];
  a.scale = (float)scale;
  a.scale_cols = geo[6];
  a.M = geo[9], a.N = geo[10], a.K = geo[11];
  a.workspace = ptr(workspace);
  a.ws_bytes = (size_t)workspace.numel() * workspace.element_size();
  c10::DeviceGuard g(W.device());
  check(kw_dec_linear(&a, stream_of(W)), w);
}

void pack_weight(const Tensor& W, Tensor& out) {
  dev(W, "kw_pack_weight");
  dev(out, "kw_pack_weight");
  TORCH_CHECK_VALUE(W.dim() == 2 && W.is_contiguous() && W.scalar_type() == at::kBFloat16,
                    "pack_weight expects a contiguous 2-D bfloat16 tensor");
  TORCH_CHECK_VALUE((size_t)out.numel() * out.element_size() >= kw_packed_weight_bytes(W.size(0), W.size(1)),
                    "pack_weight: output too small");
  c10::DeviceGuard g(W.device());
  check(kw_pack_weight(ptr(W), W.size(0), W.size(1), ptr(out), stream_of(W)), "kw_pack_weight");
}

// ---- LayerNorm (residual stream f32 or bf16) ----------------------------------------------------------
void layernorm(Tensor& x, const Tensor& gamma, const Tensor& beta, double eps, Tensor& y, const optional<Tensor>& delta) {
  const char* w = "kw_layernorm";
  dev(x, w), dev(gamma, w), dev(beta, w), dev(y, w), dev(delta, w);
  TORCH_CHECK_VALUE(x.is_contiguous() && (x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16),
                    "layernorm input must be contiguous float32 or bfloat16");
  const int64_t dim = x.dim() ? x.size(-1) : 0, rows = dim ? x.numel() / dim : 0;
  for (const Tensor* t : {&gamma, &beta})
    TORCH_CHECK_VALUE(t->scalar_type() == at::kFloat && t->numel() == dim && t->is_contiguous(),
                      "layernorm gamma and beta must be contiguous float32 tensors of x's last dimension");
  TORCH_CHECK_VALUE((y.scalar_type() == at::kFloat || y.scalar_type() == at::kBFloat16) && y.numel() == x.numel() &&
                        y.is_contiguous(),
                    "layernorm out must be a contiguous float32 or bfloat16 tensor of x's size");
  TORCH_CHECK_VALUE(!delta.has_value() || (delta->scalar_type() == at::kBFloat16 && delta->numel() == x.numel() &&
                                           delta->is_contiguous()),
                    "layernorm delta must be a contiguous bf16 tensor of x's size");
  if (rows == 0) return;  // nothing to launch (an empty tensor has no address to pass either)
  c10::DeviceGuard g(x.device());
  if (x.scalar_type() == at::kBFloat16)
    check(kw_layernorm_bf16res(ptr(x), rows, dim, ptr<const float>(gamma), ptr<const float>(beta), (float)eps, ptr(y),
                               dt_of(y), optr<const void>(delta), stream_of(x)),
          "kw_layernorm_bf16res");
  else
    check(kw_layernorm(ptr<float>(x), rows, dim, ptr<const float>(gamma), ptr<const float>(beta), (float)eps, ptr(y),
                       dt_of(y), optr<const void>(delta), stream_of(x)),
          w);
}

// ---- attention ----------------------------------------------------------------------------------------
void attention(const Tensor& qkv, int64_t B, int64_t H, int64_t T, int64_t hd, Tensor& out, int64_t flags) {
  dev(qkv, "kw_attention");
  dev(out, "kw_attention");
  c10::DeviceGuard g(qkv.device());
  check(kw_attention(dt_of(qkv) | (int)flags, ptr(qkv), B, H, T, hd, ptr(out), stream_of(qkv)), "kw_attention");
}

void embed(const Tensor& ids, int64_t B, int64_t q_len, const Tensor& cur_len, const Tensor& tok_emb,
           const Tensor& pos_emb, Tensor& h, optional<Tensor> hb, int64_t flags) {
  const char* w = "kw_embed";
  dev(ids, w), dev(cur_len, w), dev(tok_emb, w), dev(pos_emb, w), dev(h, w), dev(hb, w);
  c10::DeviceGuard g(ids.device());
  check(kw_embed(dt_of(tok_emb) | (int)flags, ptr<const int64_t>(ids), ids.stride(0), B, q_len, ptr<const int32_t>(cur_len),
                 ptr(tok_emb), ptr(pos_emb), tok_emb.size(1), ptr<float>(h), optr<void>(hb), stream_of(ids)),
        w);
}

void self_attn_step(const Tensor& qkv, int64_t B, int64_t q_len, int64_t H, int64_t hd, Tensor& k_cache,
                    Tensor& v_cache, int64_t t_max, const Tensor& cur_len, Tensor& out, optional<Tensor> workspace,
                    const optional<Tensor>& bp) {
  const char* w = "kw_self_attn_step";
  dev(qkv, w), dev(k_cache, w), dev(v_cache, w), dev(cur_len, w), dev(out, w), dev(workspace, w), dev(bp, w);
  const size_t nb = workspace.has_value() ? (size_t)workspace->numel() * workspace->element_size() : 0;
  c10::DeviceGuard g(qkv.device());
  check(kw_self_attn_step(dt_of(qkv), ptr(qkv), B, q_len, H, hd, ptr(k_cache), ptr(v_cache), t_max,
                          ptr<const int32_t>(cur_len), optr<const int32_t>(bp), bp.has_value() ? bp->stride(0) : 0,
                          ptr(out), optr<void>(workspace), nb, stream_of(qkv)),
        w);
}

void self_attn_step_masked(const Tensor& qkv, int64_t B, int64_t q_len, int64_t H, int64_t hd, Tensor& k_cache,
                           Tensor& v_cache, int64_t t_max, const Tensor& cur_len, const Tensor& key_start, Tensor& out,
                           optional<Tensor> workspace, const optional<Tensor>& bp, int64_t flags) {
  const char* w = "kw_self_attn_step_masked";
  dev(qkv, w), dev(k_cache, w), dev(v_cache, w), dev(cur_len, w), dev(key_start, w), dev(out, w), dev(workspace, w), dev(bp, w);
  TORCH_CHECK_VALUE(key_start.scalar_type() == at::kInt && key_start.is_contiguous() && key_start.numel() >= B, w,
                    ": key_start must be a contiguous int32 tensor of B elements");
  const size_t nb = workspace.has_value() ? (size_t)workspace->numel() * workspace->element_size() : 0;
  c10::DeviceGuard g(qkv.device());
  check(kw_self_attn_step_masked(dt_of(qkv) | (int)flags, ptr(qkv), B, q_len, H, hd, ptr(k_cache), ptr(v_cache), t_max,
                                 ptr<const int32_t>(cur_len), ptr<const int32_t>(key_start), optr<const int32_t>(bp),
                                 bp.has_value() ? bp->stride(0) : 0, ptr(out), optr<void>(workspace), nb, stream_of(qkv)),
        w);
}

// ---- fused decode cross-attention query + step -----------------------------------------------------------
// dims = [ldx, M, d, H, S]
void dec_xq_cross(const Tensor& x, const Tensor& W, const optional<Tensor>& bias, const Tensor& ln_colsum,
                  const Tensor& k, const Tensor& v, Tensor& out, Tensor& workspace, std::vector<int64_t> dims,
                  double ln_eps, double scale) {
  const char* w = "kw_dec_xq_cross";
  dev(x, w), dev(W, w), dev(bias, w), dev(ln_colsum, w), dev(k, w), dev(v, w), dev(out, w), dev(workspace, w);
  TORCH_CHECK_VALUE(dims.size() == 5, "kw_dec_xq_cross: dims must hold 5 integers");
  TORCH_CHECK_VALUE(x.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16 &&
                        out.scalar_type() == at::kBFloat16 && k.scalar_type() == at::kBFloat16 &&
                        v.scalar_type() == at::kBFloat16,
                    "kw_dec_xq_cross takes bf16 activations, packed bf16 weights, bf16 K / V and output");
  kw_dec_xq_cross_args a{};
  a.x = ptr(x);
  a.ldx = dims[0];
  a.ln_eps = (float)ln_eps;
  a.ln_colsum = ptr<const float>(ln_colsum);
  a.W = ptr(W);
  a.bias = optr<const float>(bias);
  a.scale = (float)scale;
  a.M = dims[1], a.d = dims[2], a.H = dims[3];
  a.k = ptr(k);
  a.v = ptr(v);
  a.S = dims[4];
  a.out = ptr(out);
  a.workspace = ptr(workspace);
  a.ws_bytes = (size_t)workspace.numel() * workspace.element_size();
  c10::DeviceGuard g(x.device());
  check(kw_dec_xq_cross(&a, stream_of(x)), w);
}

// ---- fp8 cross K/V: quantisation, step, fused query + step ------------------------------------------------
void cross_kv_quant(const Tensor& x, int64_t n, int64_t S, int64_t hd, Tensor& codes, Tensor& scales) {
  const char* w = "kw_cross_kv_quant";
  dev(x, w), dev(codes, w), dev(scales, w);
  TORCH_CHECK_VALUE(x.scalar_type() == at::kBFloat16 && codes.scalar_type() == at::kByte && scales.scalar_type() == at::kFloat &&
                        x.numel() >= n * S * hd && codes.numel() >= n * S * hd && scales.numel() >= n * hd,
                    "kw_cross_kv_quant: x bf16 [n][S][hd], codes uint8 [n][S][hd], scales f32 [n][hd]");
  c10::DeviceGuard g(x.device());
  check(kw_cross_kv_quant(ptr(x), n, S, hd, ptr(codes), ptr<float>(scales), stream_of(x)), w);
}

void cross_attn_step_fp8(const Tensor& q, int64_t B, int64_t q_len, int64_t H, int64_t hd, const Tensor& k, const Tensor& v,
                         const Tensor& k_scale, const Tensor& v_scale, int64_t S, Tensor& out) {
  const char* w = "kw_cross_attn_step_fp8";
  dev(q, w), dev(k, w), dev(v, w), dev(k_scale, w), dev(v_scale, w), dev(out, w);
  TORCH_CHECK_VALUE(q.scalar_type() == at::kBFloat16 && out.scalar_type() == at::kBFloat16 && k.scalar_type() == at::kByte &&
                        v.scalar_type() == at::kByte && k_scale.scalar_type() == at::kFloat && v_scale.scalar_type() == at::kFloat,
                    "kw_cross_attn_step_fp8 takes a bf16 query and output, uint8 (e4m3) K / V and f32 scales");
  c10::DeviceGuard g(q.device());
  check(kw_cross_attn_step_fp8(ptr(q), B, q_len, H, hd, ptr(k), ptr(v), ptr<const float>(k_scale), ptr<const float>(v_scale), S,
                               ptr(out), stream_of(q)),
        w);
}

// dims = [ldx, M, d, H, S]
void dec_xq_cross_fp8(const Tensor& x, const Tensor& W, const optional<Tensor>& bias, const Tensor& ln_colsum,
                      const Tensor& k, const Tensor& v, const Tensor& k_scale, const Tensor& v_scale, Tensor& out,
                      Tensor& workspace, std::vector<int64_t> dims, double ln_eps, double scale) {
  const char* w = "kw_dec_xq_cross_fp8";
  dev(x, w), dev(W, w), dev(bias, w), dev(ln_colsum, w), dev(k, w), dev(v, w), dev(k_scale, w), dev(v_scale, w), dev(out, w),
      dev(workspace, w);
  TORCH_CHECK_VALUE(dims.size() == 5, "kw_dec_xq_cross_fp8: dims must hold 5 integers");
  TORCH_CHECK_VALUE(x.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16 &&
                        out.scalar_type() == at::kBFloat16 && k.scalar_type() == at::kByte && v.scalar_type() == at::kByte &&
                        k_scale.scalar_type() == at::kFloat && v_scale.scalar_type() == at::kFloat,
                    "kw_dec_xq_cross_fp8 takes bf16 activations, packed bf16 weights, uint8 (e4m3) K / V, f32 scales and "
                    "a bf16 output");
  kw_dec_xq_cross_fp8_args a{};
  a.x = ptr(x);
  a.ldx = dims[0];
  a.ln_eps = (float)ln_eps;
  a.ln_colsum = ptr<const float>(ln_colsum);
  a.W = ptr(W);
  a.bias = optr<const float>(bias);
  a.scale = (float)scale;
  a.M = dims[1], a.d = dims[2], a.H = dims[3];
  a.k = ptr(k);
  a.v = ptr(v);
  a.k_scale = ptr<const float>(k_scale);
  a.v_scale = ptr<const float>(v_scale);
  a.S = dims[4];
  a.out = ptr(out);
  a.workspace = ptr(workspace);
  a.ws_bytes = (size_t)workspace.numel() * workspace.element_size();
  c10::DeviceGuard g(x.device());
  check(kw_dec_xq_cross_fp8(&a, stream_of(x)), w);
}

// ---- fused decode self-attention block (LayerNorm-fused QKV projection + self-attention step) ------------
// dims = [ldx, M, d, H, t_max]
void dec_qkv_self(const Tensor& x, const Tensor& W, const optional<Tensor>& bias, const Tensor& ln_colsum,
                  Tensor& k_cache, Tensor& v_cache, const Tensor& cur_len, Tensor& out, Tensor& workspace,
                  std::vector<int64_t> dims, double ln_eps, double scale) {
  const char* w = "kw_dec_qkv_self";
  dev(x, w), dev(W, w), dev(bias, w), dev(ln_colsum, w), dev(k_cache, w), dev(v_cache, w), dev(cur_len, w),
      dev(out, w), dev(workspace, w);
  TORCH_CHECK_VALUE(dims.size() == 5, "kw_dec_qkv_self: dims must hold 5 integers");
  TORCH_CHECK_VALUE(x.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16 &&
                        out.scalar_type() == at::kBFloat16 && k_cache.scalar_type() == at::kBFloat16,
                    "kw_dec_qkv_self takes bf16 activations, packed bf16 weights, bf16 caches and output");
  kw_dec_qkv_self_args a{};
  a.x = ptr(x);
  a.ldx = dims[0];
  a.ln_eps = (float)ln_eps;
  a.ln_colsum = ptr<const float>(ln_colsum);
  a.W = ptr(W);
  a.bias = optr<const float>(bias);
  a.scale = (float)scale;
  a.M = dims[1], a.d = dims[2], a.H = dims[3];
  a.k_cache = ptr(k_cache);
  a.v_cache = ptr(v_cache);
  a.t_max = dims[4];
  a.cur_len = ptr<const int32_t>(cur_len);
  a.out = ptr(out);
  a.workspace = ptr(workspace);
  a.ws_bytes = (size_t)workspace.numel() * workspace.element_size();
  c10::DeviceGuard g(x.device());
  check(kw_dec_qkv_self(&a, stream_of(x)), w);
}

void cross_attn_step(const Tensor& q, int64_t B, int64_t q_len, int64_t H, int64_t hd, const Tensor& k, const Tensor& v,
                     int64_t S, Tensor& out, Tensor& workspace) {
  const char* w = "kw_cross_attn_step";
  dev(q, w), dev(k, w), dev(v, w), dev(out, w), dev(workspace, w);
  c10::DeviceGuard g(q.device());
  check(kw_cross_attn_step(dt_of(q), ptr(q), B, q_len, H, hd, ptr(k), ptr(v), S, ptr(out), ptr(workspace),
                           (size_t)workspace.numel() * workspace.element_size(), stream_of(q)),
        w);
}

// ---- greedy step (processors + argmax + stopping) -----------------------------------------------------
// cfg = [return_timestamps, ts_begin, no_ts_id, eos_id, pad_id, max_initial_ts, max_length, begin_index]
void greedy_step(Tensor& logits, const Tensor& suppress_mask, const optional<Tensor>& begin_suppress, Tensor& ids,
                 Tensor& cur_len, Tensor& unfinished, Tensor& counter, Tensor& n_unfinished, optional<Tensor> scores_out,
                 optional<Tensor> workspace, std::vector<int64_t> cfg) {
  const char* w = "kw_greedy_step";
  dev(logits, w), dev(suppress_mask, w), dev(begin_suppress, w), dev(ids, w), dev(cur_len, w), dev(unfinished, w);
  dev(counter, w), dev(n_unfinished, w), dev(scores_out, w), dev(workspace, w);
  TORCH_CHECK_VALUE(cfg.size() == 8, "kw_greedy_step: cfg must hold 8 integers");
  kw_sampler_args a{};
  a.logits = ptr<float>(logits);
  a.B = logits.size(0), a.V = logits.size(1);
  a.suppress_mask = ptr<const uint8_t>(suppress_mask);
  a.begin_suppress = optr<const int32_t>(begin_suppress);
  a.n_begin_suppress = begin_suppress.has_value() ? (int32_t)begin_suppress->numel() : 0;
  a.return_timestamps = (int32_t)cfg[0];
  a.ts_begin = (int32_t)cfg[1], a.no_ts_id = (int32_t)cfg[2], a.eos_id = (int32_t)cfg[3], a.pad_id = (int32_t)cfg[4];
  a.max_initial_ts = (int32_t)cfg[5];
  a.ids = ptr<int64_t>(ids);
  a.ids_stride = ids.stride(0);
  a.cur_len = ptr<int32_t>(cur_len);
  a.max_length = (int32_t)cfg[6], a.begin_index = (int32_t)cfg[7];
  a.unfinished = ptr<int32_t>(unfinished);
  a.counter = ptr<int32_t>(counter);
  a.n_unfinished = ptr<int32_t>(n_unfinished);
  a.scores_out = optr<float>(scores_out);
  a.workspace = optr<void>(workspace);
  a.ws_bytes = workspace.has_value() ? (size_t)workspace->numel() * workspace->element_size() : 0;
  c10::DeviceGuard g(logits.device());
  check(kw_greedy_step(&a, stream_of(logits)), w);
}

// ---- sampling step with running log-probabilities -------------------------------------------------------
// cfg = [return_timestamps, ts_begin, no_ts_id, eos_id, pad_id, max_initial_ts, max_length, begin_index];
// inv_temperature f32 [1], seed int64 [1] (its 64 bits are the key), attempt int32 [1]
void sample_step(const Tensor& logits, const Tensor& suppress_mask, const optional<Tensor>& begin_suppress, Tensor& ids,
                 Tensor& cur_len, Tensor& unfinished, Tensor& counter, Tensor& n_unfinished, const Tensor& inv_temperature,
                 const Tensor& seed, const Tensor& attempt, Tensor& sum_logprob, Tensor& n_tokens,
                 const optional<Tensor>& active, optional<Tensor> noise_out, Tensor& workspace, std::vector<int64_t> cfg) {
  const char* w = "kw_sample_step";
  dev(logits, w), dev(suppress_mask, w), dev(begin_suppress, w), dev(ids, w), dev(cur_len, w), dev(unfinished, w);
  dev(counter, w), dev(n_unfinished, w), dev(inv_temperature, w), dev(seed, w), dev(attempt, w), dev(sum_logprob, w);
  dev(n_tokens, w), dev(active, w), dev(noise_out, w), dev(workspace, w);
  TORCH_CHECK_VALUE(cfg.size() == 8, "kw_sample_step: cfg must hold 8 integers");
  TORCH_CHECK_VALUE(logits.dim() == 2 && logits.is_contiguous() && logits.scalar_type() == at::kFloat,
                    "kw_sample_step: logits must be a contiguous (B, V) float32 tensor");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK_VALUE(inv_temperature.scalar_type() == at::kFloat && seed.scalar_type() == at::kLong &&
                        attempt.scalar_type() == at::kInt && sum_logprob.scalar_type() == at::kFloat &&
                        n_tokens.scalar_type() == at::kInt && sum_logprob.numel() >= B && n_tokens.numel() >= B,
                    "kw_sample_step: inv_temperature f32 [1], seed int64 [1], attempt int32 [1], sum_logprob f32 [B], "
                    "n_tokens int32 [B]");
  TORCH_CHECK_VALUE(!active.has_value() || (active->scalar_type() == at::kByte && active->numel() >= B),
                    "kw_sample_step: active must be uint8 [B]");
  TORCH_CHECK_VALUE(!noise_out.has_value() || (noise_out->scalar_type() == at::kFloat && noise_out->is_contiguous() &&
                                               noise_out->numel() >= B * V),
                    "kw_sample_step: noise_out must be a contiguous float32 [B][V] tensor");
  TORCH_CHECK_VALUE(suppress_mask.numel() >= V && unfinished.numel() >= B && ids.size(0) >= B && ids.stride(1) == 1 &&
                        ids.size(1) > cfg[6] - 1,
                    "kw_sample_step: suppress_mask [V], unfinished [B], ids [B][>= max_length]");
  kw_sample_args a{};
  a.logits = ptr<const float>(logits);
  a.B = B, a.V = V;
  a.suppress_mask = ptr<const uint8_t>(suppress_mask);
  a.begin_suppress = optr<const int32_t>(begin_suppress);
  a.n_begin_suppress = begin_suppress.has_value() ? (int32_t)begin_suppress->numel() : 0;
  a.return_timestamps = (int32_t)cfg[0];
  a.ts_begin = (int32_t)cfg[1], a.no_ts_id = (int32_t)cfg[2], a.eos_id = (int32_t)cfg[3], a.pad_id = (int32_t)cfg[4];
  a.max_initial_ts = (int32_t)cfg[5];
  a.ids = ptr<int64_t>(ids);
  a.ids_stride = ids.stride(0);
  a.cur_len = ptr<int32_t>(cur_len);
  a.max_length = (int32_t)cfg[6], a.begin_index = (int32_t)cfg[7];
  a.unfinished = ptr<int32_t>(unfinished);
  a.counter = ptr<int32_t>(counter);
  a.n_unfinished = ptr<int32_t>(n_unfinished);
  a.inv_temperature = ptr<const float>(inv_temperature);
  a.seed = ptr<const uint64_t>(seed);
  a.attempt = ptr<const uint32_t>(attempt);
  a.sum_logprob = ptr<float>(sum_logprob);
  a.n_tokens = ptr<int32_t>(n_tokens);
  a.active = optr<const uint8_t>(active);
  a.noise_out = optr<float>(noise_out);
  a.workspace = ptr(workspace);
  a.ws_bytes = (size_t)workspace.numel() * workspace.element_size();
  c10::DeviceGuard g(logits.device());
  check(kw_sample_step(&a, stream_of(logits)), w);
}

// ---- speculative decoding: the accept step ----------------------------------------------------------------
// cfg = [return_timestamps, ts_begin, no_ts_id, eos_id, pad_id, max_initial_ts, max_length, begin_index, K];
// logits f32 [K + 1][V]; ids int64: the row (1-D, or row 0 of a 2-D tensor)
void spec_accept(const Tensor& logits, const Tensor& suppress_mask, const optional<Tensor>& begin_suppress, Tensor& ids,
                 Tensor& cur_len, Tensor& unfinished, Tensor& n_unfinished, optional<Tensor> asst_cur_len,
                 optional<Tensor> asst_unfinished, optional<Tensor> verify_len, optional<Tensor> stats, Tensor& workspace,
                 std::vector<int64_t> cfg) {
  const char* w = "kw_spec_accept";
  dev(logits, w), dev(suppress_mask, w), dev(begin_suppress, w), dev(ids, w), dev(cur_len, w), dev(unfinished, w);
  dev(n_unfinished, w), dev(asst_cur_len, w), dev(asst_unfinished, w), dev(verify_len, w), dev(stats, w), dev(workspace, w);
  TORCH_CHECK_VALUE(cfg.size() == 9, "kw_spec_accept: cfg must hold 9 integers");
  const int64_t K = cfg[8];
  TORCH_CHECK_VALUE(logits.dim() == 2 && logits.is_contiguous() && logits.scalar_type() == at::kFloat &&
                        logits.size(0) == K + 1,
                    "kw_spec_accept: logits must be a contiguous (K + 1, V) float32 tensor");
  const int64_t V = logits.size(1);
  auto i32 = [](const Tensor& t, int64_t n) { return t.scalar_type() == at::kInt && t.numel() >= n; };
  TORCH_CHECK_VALUE(i32(cur_len, 1) && i32(unfinished, 1) && i32(n_unfinished, 1) &&
                        (!asst_cur_len.has_value() || i32(*asst_cur_len, 1)) &&
                        (!asst_unfinished.has_value() || i32(*asst_unfinished, 1)) &&
                        (!verify_len.has_value() || i32(*verify_len, 1)) && (!stats.has_value() || i32(*stats, 3)),
                    "kw_spec_accept: cur_len, unfinished, n_unfinished, asst_cur_len, asst_unfinished, verify_len int32 "
                    "[1], stats int32 [3]");
  TORCH_CHECK_VALUE(ids.scalar_type() == at::kLong && ids.stride(-1) == 1 && ids.size(-1) >= cfg[6] &&
                        suppress_mask.scalar_type() == at::kByte && suppress_mask.numel() >= V,
                    "kw_spec_accept: ids int64 [>= max_length], suppress_mask uint8 [V]");
  kw_spec_accept_args a{};
  a.logits = ptr<const float>(logits);
  a.V = V, a.K = (int32_t)K;
  a.suppress_mask = ptr<const uint8_t>(suppress_mask);
  a.begin_suppress = optr<const int32_t>(begin_suppress);
  a.n_begin_suppress = begin_suppress.has_value() ? (int32_t)begin_suppress->numel() : 0;
  a.return_timestamps = (int32_t)cfg[0];
  a.ts_begin = (int32_t)cfg[1], a.no_ts_id = (int32_t)cfg[2], a.eos_id = (int32_t)cfg[3], a.pad_id = (int32_t)cfg[4];
  a.max_initial_ts = (int32_t)cfg[5];
  a.ids = ptr<int64_t>(ids);
  a.ids_stride = ids.size(-1);
  a.cur_len = ptr<int32_t>(cur_len);
  a.max_length = (int32_t)cfg[6], a.begin_index = (int32_t)cfg[7];
  a.unfinished = ptr<int32_t>(unfinished);
  a.n_unfinished = ptr<int32_t>(n_unfinished);
  a.asst_cur_len = optr<int32_t>(asst_cur_len);
  a.asst_unfinished = optr<int32_t>(asst_unfinished);
  a.verify_len = optr<int32_t>(verify_len);
  a.stats = optr<int32_t>(stats);
  a.workspace = ptr(workspace);
  a.ws_bytes = (size_t)workspace.numel() * workspace.element_size();
  c10::DeviceGuard g(logits.device());
  check(kw_spec_accept(&a, stream_of(logits)), w);
}

// ---- LM head + greedy step in one launch (no timestamps) ------------------------------------------------
// lm_geo = [x_offset, ldx, M, N, K]; cfg = [eos_id, pad_id, max_length, begin_index]
void dec_lm_greedy(const Tensor& x, const Tensor& W, const optional<Tensor>& bias, const Tensor& ln_colsum,
                   optional<Tensor> logits, const Tensor& suppress_mask, const optional<Tensor>& begin_suppress,
                   Tensor& ids, Tensor& cur_len, Tensor& unfinished, Tensor& n_unfinished, Tensor& workspace,
                   std::vector<int64_t> lm_geo, double ln_eps, std::vector<int64_t> cfg) {
  const char* w = "kw_dec_lm_greedy";
  dev(x, w), dev(W, w), dev(bias, w), dev(ln_colsum, w), dev(logits, w), dev(suppress_mask, w), dev(begin_suppress, w);
  dev(ids, w), dev(cur_len, w), dev(unfinished, w), dev(n_unfinished, w), dev(workspace, w);
  TORCH_CHECK_VALUE(lm_geo.size() == 5 && cfg.size() == 4, "kw_dec_lm_greedy: lm_geo holds 5, cfg 4 integers");
  TORCH_CHECK_VALUE(x.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16,
                    "kw_dec_lm_greedy takes bf16 activations and packed bf16 weights");
  kw_dec_linear_args a{};
  a.x = ptr(x, lm_geo[0]);
  a.ldx = lm_geo[1];
  a.ln = 1;
  a.ln_eps = (float)ln_eps;
  a.ln_colsum = ptr<const float>(ln_colsum);
  a.W = ptr(W);
  a.bias = optr<const float>(bias);
  a.epilogue = KW_EPI_STORE;
  a.C = optr<void>(logits);
  a.ldc = logits.has_value() ? logits->stride(0) : lm_geo[3];
  a.c_dtype = KW_DT_F32;
  a.scale = 1.f;
  a.M = lm_geo[2], a.N = lm_geo[3], a.K = lm_geo[4];
  kw_sampler_args g{};
  g.B = a.M, g.V = a.N;
  g.suppress_mask = ptr<const uint8_t>(suppress_mask);
  g.begin_suppress = optr<const int32_t>(begin_suppress);
  g.n_begin_suppress = begin_suppress.has_value() ? (int32_t)begin_suppress->numel() : 0;
  g.eos_id = (int32_t)cfg[0], g.pad_id = (int32_t)cfg[1], g.max_length = (int32_t)cfg[2], g.begin_index = (int32_t)cfg[3];
  g.max_initial_ts = -1;
  g.ids = ptr<int64_t>(ids);
  g.ids_stride = ids.stride(0);
  g.cur_len = ptr<int32_t>(cur_len);
  g.unfinished = ptr<int32_t>(unfinished);
  g.n_unfinished = ptr<int32_t>(n_unfinished);
  g.workspace = ptr(workspace);
  g.ws_bytes = (size_t)workspace.numel() * workspace.element_size();
  c10::DeviceGuard dg(x.device());
  check(kw_dec_lm_greedy(&a, &g, stream_of(x)), w);
}

// ---- beam search step ---------------------------------------------------------------------------------
// cfg = [return_timestamps, ts_begin, no_ts_id, eos_id, max_initial_ts, begin_index, k]
// A kw_seq_bias_table from its five device arrays [tokens, seq_off, values, group_off, group_tok] (an empty list: no
// table, n_seq 0) and the longest entry's token count.
kw_seq_bias_table seq_table(const std::vector<Tensor>& t, int64_t max_len, const char* w) {
  kw_seq_bias_table o{};
  if (t.empty()) return o;
  TORCH_CHECK_VALUE(t.size() == 5, w, ": a sequence table is [tokens, seq_off, values, group_off, group_tok]");
  for (const Tensor& x : t) {
    dev(x, w);
    TORCH_CHECK_VALUE(x.dim() == 1 && x.is_contiguous(), w, ": sequence table arrays must be contiguous vectors");
  }
  TORCH_CHECK_VALUE(t[0].scalar_type() == at::kInt && t[1].scalar_type() == at::kInt &&
                        t[2].scalar_type() == at::kFloat && t[3].scalar_type() == at::kInt &&
                        t[4].scalar_type() == at::kInt,
                    w, ": sequence table arrays are int32 but the float32 values");
  const int64_t n_seq = t[2].numel(), n_groups = t[4].numel();
  TORCH_CHECK_VALUE(n_seq >= 1 && n_seq <= INT32_MAX && t[1].numel() == n_seq + 1 && t[3].numel() == n_groups + 1 &&
                        t[0].numel() >= n_seq && max_len >= 1 && max_len <= INT32_MAX,
                    w, ": sequence table arrays disagree in length");
  o.tokens = ptr<const int32_t>(t[0]);
  o.seq_off = ptr<const int32_t>(t[1]);
  o.values = ptr<const float>(t[2]);
  o.group_off = ptr<const int32_t>(t[3]);
  o.group_tok = ptr<const int32_t>(t[4]);
  o.n_seq = (int32_t)n_seq, o.n_groups = (int32_t)n_groups, o.max_len = (int32_t)max_len;
  return o;
}

// (penalty / ngram: kw_beam_logprobs_rep when rep, else kw_beam_logprobs; sb / bw: kw_beam_logprobs_proc)
void beam_logprobs_impl(const char* w, bool rep, const Tensor& logits, const Tensor& suppress_mask,
                        const optional<Tensor>& begin_suppress, const Tensor& ids, const Tensor& cur_len, Tensor& cand_val,
                        Tensor& cand_idx, const Tensor& done, optional<Tensor> workspace, std::vector<int64_t> cfg,
                        double penalty, int64_t ngram, const kw_seq_bias_table* sb = nullptr,
                        const kw_seq_bias_table* bw = nullptr) {
  dev(logits, w), dev(suppress_mask, w), dev(begin_suppress, w), dev(ids, w), dev(cur_len, w);
  dev(cand_val, w), dev(cand_idx, w), dev(done, w), dev(workspace, w);
  TORCH_CHECK_VALUE(cfg.size() == 7, w, ": cfg must hold 7 integers");
  kw_beam_logprobs_args a{};
  a.logits = ptr<const float>(logits);
  a.R = logits.size(0), a.V = logits.size(1);
  a.suppress_mask = ptr<const uint8_t>(suppress_mask);
  a.begin_suppress = optr<const int32_t>(begin_suppress);
  a.n_begin_suppress = begin_suppress.has_value() ? (int32_t)begin_suppress->numel() : 0;
  a.return_timestamps = (int32_t)cfg[0];
  a.ts_begin = (int32_t)cfg[1], a.no_ts_id = (int32_t)cfg[2], a.eos_id = (int32_t)cfg[3];
  a.max_initial_ts = (int32_t)cfg[4];
  a.ids = ptr<const int64_t>(ids);
  a.ids_stride = ids.stride(0);
  a.cur_len = ptr<const int32_t>(cur_len);
  a.begin_index = (int32_t)cfg[5];
  a.k = (int32_t)cfg[6];
  a.cand_val = ptr<float>(cand_val);
  a.cand_idx = ptr<int32_t>(cand_idx);
  a.done = ptr<const int32_t>(done);
  a.workspace = optr<void>(workspace);
  a.ws_bytes = workspace.has_value() ? (size_t)workspace->numel() * workspace->element_size() : 0;
  c10::DeviceGuard g(logits.device());
  if (sb) {
    TORCH_CHECK_VALUE(ngram >= INT32_MIN && ngram <= INT32_MAX, w, ": ngram out of range");
    check(kw_beam_logprobs_proc(&a, (float)penalty, (int32_t)ngram, sb, bw, stream_of(logits)), w);
  } else if (rep) {
    TORCH_CHECK_VALUE(ngram >= INT32_MIN && ngram <= INT32_MAX, w, ": ngram out of range");
    check(kw_beam_logprobs_rep(&a, (float)penalty, (int32_t)ngram, stream_of(logits)), w);
  } else {
    check(kw_beam_logprobs(&a, stream_of(logits)), w);
  }
}

void beam_logprobs(const Tensor& logits, const Tensor& suppress_mask, const optional<Tensor>& begin_suppress,
                   const Tensor& ids, const Tensor& cur_len, Tensor& cand_val, Tensor& cand_idx, const Tensor& done,
                   optional<Tensor> workspace, std::vector<int64_t> cfg) {
  beam_logprobs_impl("kw_beam_logprobs", false, logits, suppress_mask, begin_suppress, ids, cur_len, cand_val, cand_idx,
                     done, workspace, cfg, 1.0, 0);
}

// kw_beam_logprobs with repetition_penalty / no_repeat_ngram_size on the log-probs (cfg as beam_logprobs)
void beam_logprobs_rep(const Tensor& logits, const Tensor& suppress_mask, const optional<Tensor>& begin_suppress,
                       const Tensor& ids, const Tensor& cur_len, Tensor& cand_val, Tensor& cand_idx, const Tensor& done,
                       optional<Tensor> workspace, std::vector<int64_t> cfg, double penalty, int64_t ngram) {
  beam_logprobs_impl("kw_beam_logprobs_rep", true, logits, suppress_mask, begin_suppress, ids, cur_len, cand_val,
                     cand_idx, done, workspace, cfg, penalty, ngram);
}

// kw_beam_logprobs_rep between sequence_bias and bad_words_ids (tables as seq_table takes them)
void beam_logprobs_proc(const Tensor& logits, const Tensor& suppress_mask, const optional<Tensor>& begin_suppress,
                        const Tensor& ids, const Tensor& cur_len, Tensor& cand_val, Tensor& cand_idx, const Tensor& done,
                        optional<Tensor> workspace, std::vector<int64_t> cfg, double penalty, int64_t ngram,
                        std::vector<Tensor> bias, int64_t bias_max_len, std::vector<Tensor> bad_words,
                        int64_t bad_max_len) {
  const char* w = "kw_beam_logprobs_proc";
  const kw_seq_bias_table sb = seq_table(bias, bias_max_len, w), bw = seq_table(bad_words, bad_max_len, w);
  beam_logprobs_impl(w, true, logits, suppress_mask, begin_suppress, ids, cur_len, cand_val, cand_idx, done, workspace,
                     cfg, penalty, ngram, &sb, &bw);
}

// ---- sequence_bias / bad_words_ids in place on f32 scores [R][V] -------------------------------------------
void seq_bias_process(Tensor& scores, const Tensor& ids, const Tensor& cur_len, std::vector<Tensor> table,
                      int64_t max_len) {
  const char* w = "kw_seq_bias_process";
  dev(scores, w), dev(ids, w), dev(cur_len, w);
  TORCH_CHECK_VALUE(scores.dim() == 2 && scores.is_contiguous() && scores.scalar_type() == at::kFloat,
                    "kw_seq_bias_process: scores must be a contiguous (R, V) float32 tensor");
  TORCH_CHECK_VALUE(ids.dim() == 2 && ids.scalar_type() == at::kLong && ids.stride(1) == 1 &&
                        ids.size(0) >= scores.size(0) && cur_len.scalar_type() == at::kInt && cur_len.numel() >= 1,
                    "kw_seq_bias_process: ids int64 [R][ids_stride], cur_len int32 [1]");
  const kw_seq_bias_table t = seq_table(table, max_len, w);
  c10::DeviceGuard g(scores.device());
  check(kw_seq_bias_process(ptr<float>(scores), scores.size(0), scores.size(1), ptr<const int64_t>(ids), ids.stride(0),
                            ptr<const int32_t>(cur_len), &t, stream_of(scores)),
        w);
}

// ---- repetition_penalty / no_repeat_ngram_size in place on f32 scores [R][V] ------------------------------
void repeat_process(Tensor& scores, const Tensor& ids, const Tensor& cur_len, double penalty, int64_t ngram) {
  const char* w = "kw_repeat_process";
  dev(scores, w), dev(ids, w), dev(cur_len, w);
  TORCH_CHECK_VALUE(scores.dim() == 2 && scores.is_contiguous() && scores.scalar_type() == at::kFloat,
                    "kw_repeat_process: scores must be a contiguous (R, V) float32 tensor");
  TORCH_CHECK_VALUE(ids.dim() == 2 && ids.scalar_type() == at::kLong && ids.stride(1) == 1 &&
                        ids.size(0) >= scores.size(0) && cur_len.scalar_type() == at::kInt && cur_len.numel() >= 1,
                    "kw_repeat_process: ids int64 [R][ids_stride], cur_len int32 [1]");
  TORCH_CHECK_VALUE(ngram >= INT32_MIN && ngram <= INT32_MAX, "kw_repeat_process: ngram out of range");
  c10::DeviceGuard g(scores.device());
  // (the kernel reads ids[r][0 .. min(*cur_len, row length)): the row length, not the stride, bounds the history)
  check(kw_repeat_process(ptr<float>(scores), scores.size(0), scores.size(1), ptr<const int64_t>(ids), ids.stride(0),
                          ptr<const int32_t>(cur_len), (float)penalty, (int32_t)ngram, stream_of(scores)),
        w);
}

// ---- distillation loss: temperature KL of teacher / student logits, forward + student gradient ------------
void kd_loss(const Tensor& teacher, const Tensor& student, const Tensor& labels, double temperature, Tensor& row_kl,
             Tensor& loss, optional<Tensor> grad, Tensor& workspace) {
  const char* w = "kw_kd_loss";
  dev(teacher, w), dev(student, w), dev(labels, w), dev(row_kl, w), dev(loss, w), dev(grad, w), dev(workspace, w);
  TORCH_CHECK_VALUE(teacher.dim() == 2 && teacher.scalar_type() == at::kFloat && teacher.stride(1) == 1,
                    "kw_kd_loss: teacher must be an (N, V) float32 tensor with unit inner stride");
  const int64_t N = teacher.size(0), V = teacher.size(1);
  TORCH_CHECK_VALUE(student.dim() == 2 && student.size(0) == N && student.size(1) == V && student.stride(1) == 1,
                    "kw_kd_loss: student must be an (N, V) tensor like teacher, with unit inner stride");
  const int sdt = dt_of(student);
  TORCH_CHECK_VALUE(labels.dim() == 1 && labels.size(0) == N && labels.scalar_type() == at::kLong &&
                        labels.is_contiguous(),
                    "kw_kd_loss: labels must be a contiguous int64 [N] tensor");
  TORCH_CHECK_VALUE(row_kl.scalar_type() == at::kFloat && row_kl.is_contiguous() && row_kl.numel() == N &&
                        loss.scalar_type() == at::kFloat && loss.numel() == 1,
                    "kw_kd_loss: row_kl float32 [N], loss float32 [1]");
  if (grad.has_value())
    TORCH_CHECK_VALUE(grad->dim() == 2 && grad->size(0) == N && grad->size(1) == V && grad->stride(1) == 1 &&
                          grad->scalar_type() == student.scalar_type(),
                      "kw_kd_loss: grad must be an (N, V) tensor of the student's dtype with unit inner stride");
  // (a one-row tensor's stride(0) is arbitrary: V serves)
  auto ld = [&](const Tensor& t) { return N == 1 ? V : t.stride(0); };
  kw_kd_loss_args a{};
  a.teacher = ptr<const float>(teacher), a.ldt = ld(teacher);
  a.student = ptr(student), a.lds = ld(student), a.s_dtype = sdt;
  a.labels = ptr<const int64_t>(labels);
  a.N = N, a.V = V, a.temperature = (float)temperature;
  a.row_kl = ptr<float>(row_kl), a.loss = ptr<float>(loss);
  a.grad = optr(grad), a.ldg = grad.has_value() ? ld(*grad) : 0;
  a.workspace = ptr(workspace), a.ws_bytes = (size_t)workspace.numel() * workspace.element_size();
  c10::DeviceGuard g(teacher.device());
  check(kw_kd_loss(&a, stream_of(teacher)), w);
}

// cfg = [B, num_beams, V, begin_index, max_length, eos_id, fill_id, early_stopping]; parent_log / fin_parent: both
// (kw_beam_select_parents) or neither (kw_beam_select)
void beam_select_impl(const char* w, const Tensor& cand_val, const Tensor& cand_idx, Tensor& ids, optional<Tensor> bp,
                      Tensor& run_scores, Tensor& fin_seq, Tensor& fin_score, Tensor& fin_len, Tensor& fin_flag,
                      Tensor& unsat, Tensor& cur_len, Tensor& counter, Tensor& go, Tensor& done, Tensor& item_flags,
                      std::vector<int64_t> cfg, double length_penalty, Tensor* parent_log, Tensor* fin_parent) {
  dev(cand_val, w), dev(cand_idx, w), dev(ids, w), dev(bp, w), dev(run_scores, w), dev(fin_seq, w), dev(fin_score, w);
  dev(fin_len, w), dev(fin_flag, w), dev(unsat, w), dev(cur_len, w), dev(counter, w), dev(go, w), dev(done, w);
  dev(item_flags, w);
  TORCH_CHECK_VALUE(cfg.size() == 8, w, ": cfg must hold 8 integers");
  kw_beam_select_args a{};
  a.B = cfg[0], a.num_beams = (int32_t)cfg[1], a.V = cfg[2];
  a.cand_val = ptr<const float>(cand_val);
  a.cand_idx = ptr<const int32_t>(cand_idx);
  a.ids = ptr<int64_t>(ids);
  a.ids_stride = ids.stride(0);
  a.bp = optr<int32_t>(bp);
  a.bp_stride = bp.has_value() ? bp->stride(0) : 0;
  a.run_scores = ptr<float>(run_scores);
  a.fin_seq = ptr<int64_t>(fin_seq);
  a.fin_stride = fin_seq.size(-1);
  a.fin_score = ptr<float>(fin_score);
  a.fin_len = ptr<int32_t>(fin_len);
  a.fin_flag = ptr<int32_t>(fin_flag);
  a.unsat = ptr<int32_t>(unsat);
  a.cur_len = ptr<int32_t>(cur_len);
  a.begin_index = (int32_t)cfg[3], a.max_length = (int32_t)cfg[4], a.eos_id = (int32_t)cfg[5];
  a.fill_id = (int32_t)cfg[6];
  a.length_penalty = (float)length_penalty;
  a.early_stopping = (int32_t)cfg[7];
  a.counter = ptr<int32_t>(counter);
  a.go = ptr<int32_t>(go);
  a.done = ptr<int32_t>(done);
  a.item_flags = ptr<int32_t>(item_flags);
  c10::DeviceGuard g(ids.device());
  if (parent_log) {
    dev(*parent_log, w), dev(*fin_parent, w);
    TORCH_CHECK_VALUE(parent_log->scalar_type() == at::kInt && parent_log->is_contiguous() &&
                          parent_log->numel() >= a.max_length * a.B * a.num_beams &&
                          fin_parent->scalar_type() == at::kInt && fin_parent->is_contiguous() &&
                          fin_parent->numel() >= a.B * a.num_beams,
                      w, ": parent_log int32 [max_length][B * num_beams], fin_parent int32 [B][num_beams]");
    check(kw_beam_select_parents(&a, ptr<int32_t>(*parent_log), ptr<int32_t>(*fin_parent), stream_of(ids)), w);
  } else {
    check(kw_beam_select(&a, stream_of(ids)), w);
  }
}

void beam_select(const Tensor& cand_val, const Tensor& cand_idx, Tensor& ids, optional<Tensor> bp, Tensor& run_scores,
                 Tensor& fin_seq, Tensor& fin_score, Tensor& fin_len, Tensor& fin_flag, Tensor& unsat, Tensor& cur_len,
                 Tensor& counter, Tensor& go, Tensor& done, Tensor& item_flags, std::vector<int64_t> cfg,
                 double length_penalty) {
  beam_select_impl("kw_beam_select", cand_val, cand_idx, ids, bp, run_scores, fin_seq, fin_score, fin_len, fin_flag, unsat,
                   cur_len, counter, go, done, item_flags, cfg, length_penalty, nullptr, nullptr);
}

void beam_select_parents(const Tensor& cand_val, const Tensor& cand_idx, Tensor& ids, optional<Tensor> bp,
                         Tensor& run_scores, Tensor& fin_seq, Tensor& fin_score, Tensor& fin_len, Tensor& fin_flag,
                         Tensor& unsat, Tensor& cur_len, Tensor& counter, Tensor& go, Tensor& done, Tensor& item_flags,
                         std::vector<int64_t> cfg, double length_penalty, Tensor& parent_log, Tensor& fin_parent) {
  beam_select_impl("kw_beam_select_parents", cand_val, cand_idx, ids, bp, run_scores, fin_seq, fin_score, fin_len,
                   fin_flag, unsat, cur_len, counter, go, done, item_flags, cfg, length_penalty, &parent_log, &fin_parent);
}

// ---- token-level timestamps ---------------------------------------------------------------------------
std::vector<int32_t> i32(const std::vector<int64_t>& v) { return std::vector<int32_t>(v.begin(), v.end()); }

void align_capture(const Tensor& q, std::vector<int64_t> heads, std::vector<int64_t> slots, const Tensor& cur_len,
                   int64_t begin_index, Tensor& log) {
  const char* w = "kw_align_capture";
  dev(q, w), dev(cur_len, w), dev(log, w);
  TORCH_CHECK_VALUE(q.dim() == 2 && q.is_contiguous() && log.dim() == 4 && log.is_contiguous() && log.size(3) == 64 &&
                        log.size(1) == q.size(0) && log.scalar_type() == q.scalar_type() && heads.size() == slots.size(),
                    "kw_align_capture: q [B][d], log [A][B][t_log][64] of q's dtype, one slot per head");
  const auto h = i32(heads), sl = i32(slots);
  c10::DeviceGuard g(q.device());
  check(kw_align_capture(dt_of(q), ptr(q), q.size(0), q.size(1), h.data(), sl.data(), (int64_t)h.size(), log.size(0),
                         ptr<const int32_t>(cur_len), begin_index, ptr(log), log.size(2), stream_of(q)),
        w);
}

// qlog [A_all][B][t_log][64] and k_cache [n_layers'][B][H][S][64] (layer l's keys at index l * layer_step); the call
// covers pairs a0 .. a0 + A - 1 of qlog (pairs: their (layer, head), flattened)
void align_weights(const Tensor& qlog, int64_t a0, const Tensor& k_cache, int64_t layer_step, std::vector<int64_t> pairs,
                   int64_t T, Tensor& out) {
  const char* w = "kw_align_weights";
  dev(qlog, w), dev(k_cache, w), dev(out, w);
  const int64_t A = (int64_t)pairs.size() / 2;
  TORCH_CHECK_VALUE(qlog.dim() == 4 && qlog.is_contiguous() && k_cache.dim() == 5 && k_cache.is_contiguous() &&
                        k_cache.size(4) == 64 && qlog.size(3) == 64 && k_cache.scalar_type() == qlog.scalar_type() &&
                        k_cache.size(1) == qlog.size(1) && pairs.size() % 2 == 0 && a0 >= 0 && a0 + A <= qlog.size(0) &&
                        layer_step >= 1,
                    "kw_align_weights: qlog [A][B][t_log][64], k_cache [n][B][H][S][64] of one dtype");
  const int64_t B = qlog.size(1), H = k_cache.size(2), S = k_cache.size(3);
  TORCH_CHECK_VALUE(out.scalar_type() == at::kFloat && out.is_contiguous() && out.numel() >= A * B * T * S,
                    "kw_align_weights: out must be a contiguous float32 tensor of A * B * T * S elements");
  const auto p = i32(pairs);
  c10::DeviceGuard g(qlog.device());
  check(kw_align_weights(dt_of(qlog), ptr(qlog, a0 * B * qlog.size(2) * 64), qlog.size(2), ptr(k_cache),
                         layer_step * k_cache.stride(0), (k_cache.size(0) + layer_step - 1) / layer_step, p.data(), A, B,
                         H, S, T, ptr<float>(out), stream_of(qlog)),
        w);
}

// align_weights with a device row table: qlog [A_all][R][t_log][64], rows int32 [B][T] (entries in [0, R)), k_cache
// [n_layers'][B][H][S][64]
void align_weights_rows(const Tensor& qlog, int64_t a0, const Tensor& rows, const Tensor& k_cache, int64_t layer_step,
                        std::vector<int64_t> pairs, int64_t T, Tensor& out) {
  const char* w = "kw_align_weights_rows";
  dev(qlog, w), dev(rows, w), dev(k_cache, w), dev(out, w);
  const int64_t A = (int64_t)pairs.size() / 2;
  TORCH_CHECK_VALUE(qlog.dim() == 4 && qlog.is_contiguous() && k_cache.dim() == 5 && k_cache.is_contiguous() &&
                        k_cache.size(4) == 64 && qlog.size(3) == 64 && k_cache.scalar_type() == qlog.scalar_type() &&
                        pairs.size() % 2 == 0 && a0 >= 0 && a0 + A <= qlog.size(0) && layer_step >= 1,
                    "kw_align_weights_rows: qlog [A][R][t_log][64], k_cache [n][B][H][S][64] of one dtype");
  const int64_t R = qlog.size(1), B = k_cache.size(1), H = k_cache.size(2), S = k_cache.size(3);
  TORCH_CHECK_VALUE(T > 0 && rows.scalar_type() == at::kInt && rows.is_contiguous() && rows.numel() == B * T,
                    "kw_align_weights_rows: rows must be a contiguous int32 [B][T] tensor");
  TORCH_CHECK_VALUE(out.scalar_type() == at::kFloat && out.is_contiguous() && out.numel() >= A * B * T * S,
                    "kw_align_weights_rows: out must be a contiguous float32 tensor of A * B * T * S elements");
  const auto p = i32(pairs);
  c10::DeviceGuard g(qlog.device());
  check(kw_align_weights_rows(dt_of(qlog), ptr(qlog, a0 * R * qlog.size(2) * 64), R, qlog.size(2),
                              ptr<const int32_t>(rows), ptr(k_cache), layer_step * k_cache.stride(0),
                              (k_cache.size(0) + layer_step - 1) / layer_step, p.data(), A, B, H, S, T, ptr<float>(out),
                              stream_of(qlog)),
        w);
}

void align_reduce(const Tensor& weights, int64_t A, int64_t B, int64_t T, int64_t S, const optional<Tensor>& frames,
                  int64_t filter_width, Tensor& out, int64_t a_total, int64_t first, int64_t last) {
  const char* w = "kw_align_reduce";
  dev(weights, w), dev(frames, w), dev(out, w);
  TORCH_CHECK_VALUE(weights.scalar_type() == at::kFloat && weights.is_contiguous() && out.scalar_type() == at::kFloat &&
                        out.is_contiguous() && A > 0 && B > 0 && T > 0 && S > 0 && weights.numel() >= A * B * T * S &&
                        out.numel() >= B * T * S &&
                        (!frames.has_value() || (frames->scalar_type() == at::kInt && frames->numel() >= B)),
                    "kw_align_reduce: weights [A][B][T][S] f32, out [B][T][S] f32, frames int32 [B]");
  c10::DeviceGuard g(weights.device());
  check(kw_align_reduce(ptr<const float>(weights), A, B, T, S, optr<const int32_t>(frames), filter_width, ptr<float>(out),
                        a_total, (int)first, (int)last, stream_of(weights)),
        w);
}

void dtw(const Tensor& matrix, const optional<Tensor>& frames, Tensor& out, Tensor& workspace) {
  const char* w = "kw_dtw";
  dev(matrix, w), dev(frames, w), dev(out, w), dev(workspace, w);
  TORCH_CHECK_VALUE(matrix.dim() == 3 && matrix.is_contiguous() && matrix.scalar_type() == at::kFloat &&
                        out.scalar_type() == at::kInt && out.is_contiguous() &&
                        out.numel() >= matrix.size(0) * matrix.size(1) &&
                        (!frames.has_value() || (frames->scalar_type() == at::kInt && frames->numel() >= matrix.size(0))),
                    "kw_dtw: matrix [B][T][S] f32, out int32 [B][T], frames int32 [B]");
  c10::DeviceGuard g(matrix.device());
  check(kw_dtw(ptr<const float>(matrix), matrix.size(0), matrix.size(1), matrix.size(2), optr<const int32_t>(frames),
               ptr<int32_t>(out), ptr(workspace), (size_t)workspace.numel() * workspace.element_size(), stream_of(matrix)),
        w);
}

// ---- workspace / packing sizes (host queries) ---------------------------------------------------------
int64_t workspace_bytes(std::string kind, std::vector<int64_t> d) {
  auto n = [&](size_t i) { return at_(d, i, "kw::workspace_bytes"); };
  if (kind == "dec_linear") return (int64_t)kw_dec_linear_workspace_bytes(n(0), n(1));
  if (kind == "packed_weight") return (int64_t)kw_packed_weight_bytes(n(0), n(1));
  if (kind == "self_attn") return (int64_t)kw_self_attn_workspace(n(0), n(1), n(2));
  if (kind == "cross_attn") return (int64_t)kw_cross_attn_workspace(n(0), n(1), n(2), n(3), n(4));
  if (kind == "greedy_step") return (int64_t)kw_greedy_step_workspace(n(0));
  if (kind == "sample_step") return (int64_t)kw_sample_step_workspace(n(0));
  if (kind == "spec_accept") return (int64_t)kw_spec_accept_workspace(n(0));
  if (kind == "lm_greedy") return (int64_t)kw_dec_lm_greedy_workspace(n(0), n(1));
  if (kind == "qkv_self") return (int64_t)kw_dec_qkv_self_workspace(n(0), n(1));
  if (kind == "xq_cross") return (int64_t)kw_dec_xq_cross_workspace(n(0), n(1), n(2), n(3));
  if (kind == "beam_logprobs") return (int64_t)kw_beam_logprobs_workspace(n(0));
  if (kind == "kd_loss") return (int64_t)kw_kd_loss_workspace(n(0));
  if (kind == "dtw") return (int64_t)kw_dtw_workspace(n(0), n(1), n(2));
  // byte offsets of the hand-off status words inside those workspaces (include/kwhisper.h)
  if (kind == "qkv_self_status") return (int64_t)kw_dec_qkv_self_status_offset(n(0), n(1));
  if (kind == "xq_cross_status") return (int64_t)kw_dec_xq_cross_status_offset(n(0), n(1), n(2), n(3));
  if (kind == "cross_attn_status") return (int64_t)kw_cross_attn_status_offset(n(0), n(1), n(2), n(3), n(4));
  TORCH_CHECK_VALUE(false, "kw::workspace_bytes: unknown kind ", kind);
}

int64_t version() { return kw_version(); }

}  // namespace

TORCH_LIBRARY(kw, m) {
  m.def("version() -> int", &version);
  m.def("workspace_bytes(str kind, int[] dims) -> int", &workspace_bytes);
  m.def("log_mel(Tensor audio, Tensor mel_filters, Tensor(a!) out, Tensor(b!) workspace) -> ()");
  m.def("mel_to_time_major(Tensor mel, int c_pad, Tensor(a!) out) -> ()");
  m.def("gemm(Tensor A, Tensor W, Tensor? bias, Tensor(a!) C, Tensor? row_add, int[] geo, float scale, int dtype) -> ()");
  m.def("dec_linear(Tensor x, Tensor W, Tensor? bias, Tensor? ln_colsum, Tensor(a!)? C, Tensor(b!)? h, "
        "Tensor(c!)? hb, Tensor(d!) workspace, int[] geo, float ln_eps, float scale) -> ()");
  m.def("pack_weight(Tensor W, Tensor(a!) out) -> ()");
  m.def("layernorm(Tensor(a!) x, Tensor gamma, Tensor beta, float eps, Tensor(b!) y, Tensor? delta) -> ()");
  m.def("attention(Tensor qkv, int B, int H, int T, int hd, Tensor(a!) out, int flags=0) -> ()");
  m.def("embed(Tensor ids, int B, int q_len, Tensor cur_len, Tensor tok_emb, Tensor pos_emb, Tensor(a!) h, "
        "Tensor(b!)? hb, int flags=0) -> ()");
  m.def("self_attn_step(Tensor qkv, int B, int q_len, int H, int hd, Tensor(a!) k_cache, Tensor(b!) v_cache, "
        "int t_max, Tensor cur_len, Tensor(c!) out, Tensor(d!)? workspace, Tensor? bp) -> ()");
  m.def("self_attn_step_masked(Tensor qkv, int B, int q_len, int H, int hd, Tensor(a!) k_cache, Tensor(b!) v_cache, "
        "int t_max, Tensor cur_len, Tensor key_start, Tensor(c!) out, Tensor(d!)? workspace, Tensor? bp, int flags=0) -> ()");
  m.def("dec_qkv_self(Tensor x, Tensor W, Tensor? bias, Tensor ln_colsum, Tensor(a!) k_cache, Tensor(b!) v_cache, "
        "Tensor cur_len, Tensor(c!) out, Tensor(d!) workspace, int[] dims, float ln_eps, float scale) -> ()");
  m.def("dec_xq_cross(Tensor x, Tensor W, Tensor? bias, Tensor ln_colsum, Tensor k, Tensor v, Tensor(a!) out, "
        "Tensor(b!) workspace, int[] dims, float ln_eps, float scale) -> ()");
  m.def("cross_kv_quant(Tensor x, int n, int S, int hd, Tensor(a!) codes, Tensor(b!) scales) -> ()");
  m.def("cross_attn_step_fp8(Tensor q, int B, int q_len, int H, int hd, Tensor k, Tensor v, Tensor k_scale, Tensor v_scale, "
        "int S, Tensor(a!) out) -> ()");
  m.def("dec_xq_cross_fp8(Tensor x, Tensor W, Tensor? bias, Tensor ln_colsum, Tensor k, Tensor v, Tensor k_scale, "
        "Tensor v_scale, Tensor(a!) out, Tensor(b!) workspace, int[] dims, float ln_eps, float scale) -> ()");
  m.def("cross_attn_step(Tensor q, int B, int q_len, int H, int hd, Tensor k, Tensor v, int S, Tensor(a!) out, "
        "Tensor(b!) workspace) -> ()");
  m.def("greedy_step(Tensor(a!) logits, Tensor suppress_mask, Tensor? begin_suppress, Tensor(b!) ids, "
        "Tensor(c!) cur_len, Tensor(d!) unfinished, Tensor(e!) counter, Tensor(f!) n_unfinished, "
        "Tensor(g!)? scores_out, Tensor(h!)? workspace, int[] cfg) -> ()");
  m.def("sample_step(Tensor logits, Tensor suppress_mask, Tensor? begin_suppress, Tensor(a!) ids, Tensor(b!) cur_len, "
        "Tensor(c!) unfinished, Tensor(d!) counter, Tensor(e!) n_unfinished, Tensor inv_temperature, Tensor seed, "
        "Tensor attempt, Tensor(f!) sum_logprob, Tensor(g!) n_tokens, Tensor? active, Tensor(h!)? noise_out, "
        "Tensor(i!) workspace, int[] cfg) -> ()");
  m.def("spec_accept(Tensor logits, Tensor suppress_mask, Tensor? begin_suppress, Tensor(a!) ids, Tensor(b!) cur_len, "
        "Tensor(c!) unfinished, Tensor(d!) n_unfinished, Tensor(e!)? asst_cur_len, Tensor(f!)? asst_unfinished, "
        "Tensor(g!)? verify_len, Tensor(h!)? stats, Tensor(i!) workspace, int[] cfg) -> ()");
  m.def("dec_lm_greedy(Tensor x, Tensor W, Tensor? bias, Tensor ln_colsum, Tensor(a!)? logits, Tensor suppress_mask, "
        "Tensor? begin_suppress, Tensor(b!) ids, Tensor(c!) cur_len, Tensor(d!) unfinished, Tensor(e!) n_unfinished, "
        "Tensor(f!) workspace, int[] lm_geo, float ln_eps, int[] cfg) -> ()");
  m.def("beam_logprobs(Tensor logits, Tensor suppress_mask, Tensor? begin_suppress, Tensor ids, Tensor cur_len, "
        "Tensor(a!) cand_val, Tensor(b!) cand_idx, Tensor done, Tensor(c!)? workspace, int[] cfg) -> ()");
  m.def("beam_logprobs_rep(Tensor logits, Tensor suppress_mask, Tensor? begin_suppress, Tensor ids, Tensor cur_len, "
        "Tensor(a!) cand_val, Tensor(b!) cand_idx, Tensor done, Tensor(c!)? workspace, int[] cfg, float penalty, "
        "int ngram) -> ()");
  m.def("repeat_process(Tensor(a!) scores, Tensor ids, Tensor cur_len, float penalty, int ngram) -> ()");
  m.def("beam_logprobs_proc(Tensor logits, Tensor suppress_mask, Tensor? begin_suppress, Tensor ids, Tensor cur_len, "
        "Tensor(a!) cand_val, Tensor(b!) cand_idx, Tensor done, Tensor(c!)? workspace, int[] cfg, float penalty, "
        "int ngram, Tensor[] bias, int bias_max_len, Tensor[] bad_words, int bad_max_len) -> ()");
  m.def("seq_bias_process(Tensor(a!) scores, Tensor ids, Tensor cur_len, Tensor[] table, int max_len) -> ()");
  m.def("beam_select(Tensor cand_val, Tensor cand_idx, Tensor(a!) ids, Tensor(b!)? bp, Tensor(c!) run_scores, "
        "Tensor(d!) fin_seq, Tensor(e!) fin_score, Tensor(f!) fin_len, Tensor(g!) fin_flag, Tensor(h!) unsat, "
        "Tensor(i!) cur_len, Tensor(j!) counter, Tensor(k!) go, Tensor(l!) done, Tensor(m!) item_flags, int[] cfg, "
        "float length_penalty) -> ()");
  m.def("beam_select_parents(Tensor cand_val, Tensor cand_idx, Tensor(a!) ids, Tensor(b!)? bp, Tensor(c!) run_scores, "
        "Tensor(d!) fin_seq, Tensor(e!) fin_score, Tensor(f!) fin_len, Tensor(g!) fin_flag, Tensor(h!) unsat, "
        "Tensor(i!) cur_len, Tensor(j!) counter, Tensor(k!) go, Tensor(l!) done, Tensor(m!) item_flags, int[] cfg, "
        "float length_penalty, Tensor(n!) parent_log, Tensor(o!) fin_parent) -> ()");
  m.def("align_weights_rows(Tensor qlog, int a0, Tensor rows, Tensor k_cache, int layer_step, int[] pairs, int T, "
        "Tensor(a!) out) -> ()");
  m.def("align_capture(Tensor q, int[] heads, int[] slots, Tensor cur_len, int begin_index, Tensor(a!) log) -> ()");
  m.def("align_weights(Tensor qlog, int a0, Tensor k_cache, int layer_step, int[] pairs, int T, Tensor(a!) out) -> ()");
  m.def("align_reduce(Tensor weights, int A, int B, int T, int S, Tensor? frames, int filter_width, Tensor(a!) out, "
        "int a_total, int first, int last) -> ()");
  m.def("dtw(Tensor matrix, Tensor? frames, Tensor(a!) out, Tensor(b!) workspace) -> ()");
  m.def("kd_loss(Tensor teacher, Tensor student, Tensor labels, float temperature, Tensor(a!) row_kl, Tensor(b!) loss, "
        "Tensor(c!)? grad, Tensor(d!) workspace) -> ()");
}

TORCH_LIBRARY_IMPL(kw, CUDA, m) {
  m.impl("log_mel", &log_mel);
  m.impl("mel_to_time_major", &mel_to_time_major);
  m.impl("gemm", &gemm);
  m.impl("dec_linear", &dec_linear);
  m.impl("pack_weight", &pack_weight);
  m.impl("layernorm", &layernorm);
  m.impl("attention", &attention);
  m.impl("embed", &embed);
  m.impl("self_attn_step", &self_attn_step);
  m.impl("self_attn_step_masked", &self_attn_step_masked);
  m.impl("cross_attn_step", &cross_attn_step);
  m.impl("dec_qkv_self", &dec_qkv_self);
  m.impl("dec_xq_cross", &dec_xq_cross);
  m.impl("cross_kv_quant", &cross_kv_quant);
  m.impl("cross_attn_step_fp8", &cross_attn_step_fp8);
  m.impl("dec_xq_cross_fp8", &dec_xq_cross_fp8);
  m.impl("greedy_step", &greedy_step);
  m.impl("sample_step", &sample_step);
  m.impl("spec_accept", &spec_accept);
  m.impl("dec_lm_greedy", &dec_lm_greedy);
  m.impl("beam_logprobs", &beam_logprobs);
  m.impl("beam_logprobs_rep", &beam_logprobs_rep);
  m.impl("repeat_process", &repeat_process);
  m.impl("beam_logprobs_proc", &beam_logprobs_proc);
  m.impl("seq_bias_process", &seq_bias_process);
  m.impl("beam_select", &beam_select);
  m.impl("beam_select_parents", &beam_select_parents);
  m.impl("align_weights_rows", &align_weights_rows);
  m.impl("align_capture", &align_capture);
  m.impl("align_weights", &align_weights);
  m.impl("align_reduce", &align_reduce);
  m.impl("dtw", &dtw);
  m.impl("kd_loss", &kd_loss);
}
