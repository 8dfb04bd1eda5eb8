/*
 * kwhisper -- C ABI of the MI355X (gfx950) Whisper teacher hot path.
 *
 * Drop-in boundary: the Python host (kotoba-whisper_amd/kwhisper) binds these entry points with
 * ctypes and exposes HF's WhisperForConditionalGeneration.generate() / WhisperFeatureExtractor API
 * (SURVEY.md §8b).  Every pointer below is a DEVICE pointer unless stated; the caller owns all
 * memory (kernels never allocate); every call is asynchronous on `stream` (a hipStream_t, 0 =
 * null stream) and is safe to capture in a hipGraph.  Return value: KW_OK or a KW_E* code;
 * kw_last_error() gives the message.  Nothing throws across the ABI.
 *
 * Element types: KW_DT_F32 = float32, KW_DT_BF16 = bfloat16 (raw uint16 storage).
 * Reference interfaces each entry point replaces are cited as TF/<file>:<line>, where
 * TF = transformers 5.15.0 (the arithmetic of kotoba-whisper's hot path, run_pseudo_labelling.py:338).
 */
#ifndef KWHISPER_H
#define KWHISPER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* kw_stream_t;

enum { KW_OK = 0, KW_EINVAL = 1, KW_EHIP = 2, KW_EUNSUPPORTED = 3 };
enum { KW_DT_F32 = 0, KW_DT_BF16 = 1 };
enum { KW_EPI_STORE = 0, KW_EPI_RESID = 1, KW_EPI_HEADSPLIT = 2 };

/* ABI version (major*100 + minor) and the last error message of this thread. */
int kw_version(void);  /* 112 */
const char* kw_last_error(void);

/* A new non-blocking stream of its own (hipStreamCreateWithFlags), for callers that must not share one: the streams a
 * hipGraph capture forks into (PyTorch hands out streams from a fixed pool, so two host threads can be given the same
 * one, and a thread's launches on a stream another thread's capture has forked into join that capture). */
int kw_stream_create(kw_stream_t* out);
int kw_stream_destroy(kw_stream_t stream);

/* a1 -- log-mel spectrogram.
 * Replaces WhisperFeatureExtractor._torch_extract_fbank_features (TF/models/whisper/
 * feature_extraction_whisper.py:135-168): stft(n_fft 400, hop 160, periodic hann, center, reflect)
 * -> |X|^2 -> drop last frame -> mel_filters.T @ P -> log10(clamp 1e-10) -> per-clip max(x, max-8)
 * -> (x+4)/4.   audio: [batch][audio_stride] f32 (first n_samples used, n_samples % 160 == 0,
 * already padded/truncated as in __call__ :300-307); mel_filters: [201][n_mels] f32;
 * out: [batch][n_mels][n_samples/160] f32; workspace: >= 4*batch bytes. */
int kw_log_mel(const float* audio, int64_t batch, int64_t n_samples, int64_t audio_stride,
               const float* mel_filters, int n_mels, float* out, void* workspace, kw_stream_t stream);

/* Conv stem input re-layout: mel [B][C][T] f32 -> time-major, zero-padded [B][T+2][c_pad] (dtype),
 * so that Conv1d(k=3, p=1) is a GEMM whose im2col row t is the contiguous 3*c_pad slice at row t
 * (TF/models/whisper/modeling_whisper.py:566-567,618-619). */
int kw_mel_to_time_major(const float* mel, int64_t B, int64_t C, int64_t T, int64_t c_pad,
                         void* out, int out_dtype, kw_stream_t stream);

/* Linear / conv-as-GEMM:  C = epilogue(A . W^T + bias)  (nn.Linear, TF modeling_whisper.py:279-282,
 * 375-376, 444-445, 499-503, 566-567, 1080).
 * Row maps: logical row r of A lives at A + (r / a_rows_per_batch)*a_batch_stride
 * + (r % a_rows_per_batch)*lda (elements); the same for C.  W: [N][K] (or packed, kw_gemv).
 * Epilogues: STORE  C = act(acc + bias) * (col < scale_cols ? scale : 1) (+ row_add[r % period][col])
 *            RESID  C(f32) += acc + bias           (residual add, TF modeling_whisper.py:398,407)
 *            HEADSPLIT  as STORE, written to C[part][b][h][t][d] with part = col / (heads*head_dim),
 *                       b = r / hs_seq, t = r % hs_seq  (q/k/v and cross-K/V cache layout). */
typedef struct {
  int dtype;                 /* A and W element type */
  int c_dtype;               /* C element type (RESID: must be KW_DT_F32) */
  const void* A;
  int64_t lda, a_rows_per_batch, a_batch_stride;
  const void* W;
  const float* bias;         /* [N] or NULL */
  void* C;
  int64_t ldc, c_rows_per_batch, c_batch_stride;
  int64_t M, N, K;
  int epilogue;              /* KW_EPI_* */
  int gelu;                  /* exact-erf GELU after bias */
  float scale;               /* applied to columns [0, scale_cols) after bias/GELU */
  int64_t scale_cols;
  const float* row_add;      /* [period][N] f32 added after the activation, or NULL */
  int64_t row_add_period;
  int64_t hs_seq, hs_heads, hs_head_dim;
} kw_gemm_args;

int kw_gemm(const kw_gemm_args* args, kw_stream_t stream);

/* ---- decode step (bf16 engine) --------------------------------------------------------------- */

/* Decode-step linear over packed weights, any M (launched in 32-row chunks):
 *   A = x (bf16 [M][ldx]) or, if ln != 0, the LayerNorm (x - mean) * rstd (eps ln_eps) of each row of it,
 *   with gamma/beta folded into W / bias by the caller (W' = W diag(gamma), b' = b + W beta) and
 *   ln_colsum[n] = sum_k W'[n][k] (f32, of the bf16 values packed); computed as
 *   rstd * (x W'^T - mean * ln_colsum) with each row's statistics taken from x itself
 *   (TF modeling_whisper.py:446,476,500 + 469-503, proj_out :1080);
 *   STORE: C[m][n] = act(acc + bias) * (n < scale_cols ? scale : 1), C f32 or bf16;
 *   RESID: h[m][n] += acc + bias (f32 residual, modeling_whisper.py:482,495,503) and hb = bf16(h), the
 *          bf16 mirror the next LayerNorm-fused linear reads.
 * W: packed by kw_pack_weight.  workspace: >= kw_dec_linear_workspace_bytes(N, K) bytes, zero-filled
 * before first use; one workspace may serve all calls on one stream.  What must be zero is its first 16 KB, the
 * K-split arrival counters, and every call leaves those zero again; the rest (used by K-split shapes only) is
 * scratch for partial sums, written before it is read and left holding the last call's.
 * Results are bitwise deterministic (fixed-order reductions, no float atomics).
 *
 * Fragment-major activations: ldx == KW_LD_TILED says x is stored in the order the matrix cores take it
 * (the A operand of v_mfma_f32_16x16x32_bf16), for M <= 32 rows in T = ceil(M / 16) row tiles: element (m, k)
 * is element k % 8 of 16-B piece ((k / 32) * T + m / 16) * 64 + m % 16 + 16 * ((k % 32) / 8), the buffer holding
 * (K / 32) * T * 1 KB.  Rows M .. 16 T - 1 may hold anything (they feed discarded outputs only).  Same results,
 * bit for bit; a wave's load of one (k-tile, row tile) is one contiguous 1-KB access.  Read by kw_dec_linear
 * (M <= 32; LM head shapes: those its persistent kernel covers, kw_dec_lm_greedy_supported), kw_dec_lm_greedy,
 * kw_dec_qkv_self and kw_dec_xq_cross (a block called with ldx == KW_LD_TILED also WRITES its out [M][d] in this
 * order, for the o / xo linear that follows); any other use returns KW_EINVAL.
 * Written by the producers of the bf16 residual mirror: kw_dec_linear's RESID epilogue with
 * epilogue = KW_EPI_RESID | KW_EPI_HB_TILED (hb fragment-major over ceil(M / 16) row tiles, M <= 32, N % 32 == 0;
 * h stays [M][ldh] f32) and kw_embed with dtype | KW_EMBED_HB_TILED (q_len 1, B <= 32, bf16 tables, d % 32 == 0).
 * Rows >= M of the buffer are never written. */
#define KW_LD_TILED ((int64_t)-1)
#define KW_EPI_HB_TILED 0x100
#define KW_EMBED_HB_TILED 0x100
typedef struct {
  const void* x;
  int64_t ldx;               /* row stride in elements, or KW_LD_TILED */
  int ln;                    /* fuse the LayerNorm of x (STORE only) */
  float ln_eps;
  const float* ln_colsum;    /* [N], required with ln */
  const void* W;
  const float* bias;         /* [N] f32 or NULL */
  int epilogue;              /* KW_EPI_STORE or KW_EPI_RESID (| KW_EPI_HB_TILED) */
  void* C;                   /* STORE output [M][ldc] */
  int64_t ldc;
  int c_dtype;
  int gelu;
  float scale;
  int64_t scale_cols;
  float* h;                  /* RESID: f32 residual [M][ldh] (in/out) */
  void* hb;                  /* RESID: bf16 mirror [M][ldh] (out) */
  int64_t ldh;
  int64_t M, N, K;
  void* workspace;
  size_t ws_bytes;
} kw_dec_linear_args;

int kw_dec_linear(const kw_dec_linear_args* args, kw_stream_t stream);
size_t kw_dec_linear_workspace_bytes(int64_t N, int64_t K);
/* W [N][K] bf16 -> packed [ceil(N/32)*2][K/32][64 lanes][8] bf16 (columns >= N zero); K % 32 == 0. */
int kw_pack_weight(const void* W, int64_t N, int64_t K, void* packed, kw_stream_t stream);
size_t kw_packed_weight_bytes(int64_t N, int64_t K);

/* LayerNorm (eps) over the last dim of x [rows][dim] f32 -> y [rows][dim] (y_dtype);
 * TF modeling_whisper.py:371,377,434,443,446,642,790. dim % 4 == 0, dim <= 2048.  delta (bf16
 * [rows][dim] or NULL): the producing linear's output, added to x in place first (the residual add
 * of :398,407 fused in front of the next LayerNorm).  gamma, beta: [dim] f32.  x, gamma, beta and an f32 y
 * must be 16-B aligned, delta and a bf16 y 8-B aligned (the widths of the kernel's accesses); anything else
 * returns KW_EINVAL.  rows == 0 returns KW_OK and launches nothing. */
int kw_layernorm(float* x, int64_t rows, int64_t dim, const float* gamma, const float* beta,
                 float eps, void* y, int y_dtype, const void* delta, kw_stream_t stream);
/* The same over a bf16 residual stream x [rows][dim] (the encoder's bf16 path): x += delta is rounded
 * to bf16, as the reference's residual add in a bf16 model is. dim % 8 == 0, dim <= 2048; x, y, delta,
 * gamma and beta 16-B aligned (KW_EINVAL otherwise). */
int kw_layernorm_bf16res(void* x, int64_t rows, int64_t dim, const float* gamma, const float* beta,
                         float eps, void* y, int y_dtype, const void* delta, kw_stream_t stream);

/* Encoder self-attention softmax(Q K^T) V (q pre-scaled; TF sdpa_attention.py:79-166, non-causal).
 * qkv: [3][B][H][T][hd] (dtype), out: [B][T][H*hd] (dtype). hd == 64.  dtype | KW_ATTN_Q_LOG2 (bf16 only):
 * q also carries log2(e) (scores in log2 units -- the producer folds it into its q scale), which saves the
 * softmax one multiply-add per score. */
#define KW_ATTN_Q_LOG2 0x100
int kw_attention(int dtype, const void* qkv, int64_t B, int64_t H, int64_t T, int64_t hd, void* out,
                 kw_stream_t stream);

/* Decoder input embedding: h[b*q_len+i] = tok_emb[ids[b][L-q_len+i]] + pos_emb[L-q_len+i]
 * with L = *cur_len read on device (TF modeling_whisper.py:737-762; no embed scale); hb (optional,
 * bf16, may be NULL) receives bf16(h) for the bf16 engine's LayerNorm-fused linears -- fragment-major with
 * dtype | KW_EMBED_HB_TILED (see kw_dec_linear). */
int kw_embed(int dtype, const int64_t* ids, int64_t ids_stride, int64_t B, int64_t q_len,
             const int32_t* cur_len, const void* tok_emb, const void* pos_emb, int64_t d, float* h,
             void* hb, kw_stream_t stream);

/* Decoder self-attention over a static cache (TF modeling_whisper.py:469-480, cache_utils.py:127-145):
 * appends k/v of the q_len newest positions [L-q_len, L) to k_cache/v_cache [B][H][t_max][hd],
 * then causal attention for those positions. qkv: [B*q_len][3*H*hd]; out [B*q_len][H*hd]; t_max <= 512.
 * q_len == 1 needs workspace >= kw_self_attn_workspace(B, H, t_max) bytes, zero-filled before first use
 * (arrival counters every call leaves at zero); q_len > 1 ignores it.  bp (q_len == 1 only, or NULL):
 * beam-search slot table [B][bp_stride] int32 -- key/value position k < L-1 of row b is read from
 * cache row bp[b][k] (beams share their prefix; the reorder of cache_utils.py:2035-2038 moves no K/V). */
int kw_self_attn_step(int dtype, const void* qkv, int64_t B, int64_t q_len, int64_t H, int64_t hd,
                      void* k_cache, void* v_cache, int64_t t_max, const int32_t* cur_len,
                      const int32_t* bp, int64_t bp_stride, void* out, void* workspace, size_t ws_bytes,
                      kw_stream_t stream);
size_t kw_self_attn_workspace(int64_t B, int64_t H, int64_t t_max);

/* kw_self_attn_step with a per-row first key, for left-padded prompts (TF generation_whisper.py:1908: the
 * decoder_attention_mask of a conditioned long-form pass; the pads sit in front of a row and keep their positions).
 * key_start: [B] int32 on the device.  Row b attends key positions k with key_start[b] <= k <= own position; keys
 * below key_start[b] are never read (the cache may hold anything there).  The new positions' K/V are appended for
 * every row as in kw_self_attn_step.  A query position below its row's key_start (a pad) has no key: its output
 * row is zeros.  bp, workspace and the dtypes as in kw_self_attn_step.  key_start all zero: q_len == 1 writes
 * kw_self_attn_step's bits in both dtypes.  q_len > 1, f32: one workgroup per (row, head, query position) with
 * kw_self_attn_step's summation order per query, the same bits again.  q_len > 1, bf16: a causal MFMA tile kernel
 * (one wave per 16 query positions, 32-key tiles), within bf16 rounding of kw_self_attn_step;
 * dtype | KW_SELF_ATTN_PER_QUERY selects the per-query form for bf16 too (bitwise kw_self_attn_step; measurements). */
#define KW_SELF_ATTN_PER_QUERY 0x100
int kw_self_attn_step_masked(int dtype, const void* qkv, int64_t B, int64_t q_len, int64_t H, int64_t hd,
                             void* k_cache, void* v_cache, int64_t t_max, const int32_t* cur_len,
                             const int32_t* key_start, const int32_t* bp, int64_t bp_stride, void* out,
                             void* workspace, size_t ws_bytes, kw_stream_t stream);

/* The self-attention block of one greedy decode step in ONE launch (bf16): the LayerNorm-fused QKV projection
 * (TF modeling_whisper.py:446,469-471; q * head_dim^-0.5 :309) and the self-attention step over the static
 * cache with the new key / value appended (:469-480, cache_utils.py:127-145) -- kw_dec_linear(qkv) followed by
 * kw_self_attn_step(q_len 1) without the kernel boundary (the projection and caches bitwise the same, the
 * attention output within bf16 rounding: its keys are summed in 16-slot passes): the projection's output is
 * handed to the attention in-launch as 8-byte {bf16 x 2, tag} granules while the cached K/V rows load.
 * cur_len outside [1, min(256, t_max)] sets the workspace status word (kw_dec_qkv_self_status_offset) and writes NaN.
 *   x: hb [M][ldx] bf16 (the residual mirror; LayerNorm applied as kw_dec_linear's ln); W: packed [3d][d] with
 *   gamma folded (kw_pack_weight); ln_colsum / bias: [3d] f32; scale multiplies the q columns (< d);
 *   k_cache / v_cache: one layer's [M][H][t_max][64] bf16; cur_len: L on device (positions [0, L-1) cached,
 *   L-1 new), L <= 256; out: [M][d] bf16.  M <= 32, d = 64 H, d <= 1280.
 * workspace >= kw_dec_qkv_self_workspace(M, d) bytes, ZERO-FILLED before first use (every call re-arms it).
 * Every in-launch wait is on work dispatched before it (no co-residency assumption: safe beside other work on
 * the GPU).  kw_dec_qkv_self_supported(): 1 when the shape is covered. */
typedef struct {
  const void* x;
  int64_t ldx;
  float ln_eps;
  const float* ln_colsum;
  const void* W;
  const float* bias;
  float scale;
  int64_t M, d, H;
  void* k_cache;
  void* v_cache;
  int64_t t_max;
  const int32_t* cur_len;
  void* out;
  void* workspace;
  size_t ws_bytes;
} kw_dec_qkv_self_args;

int kw_dec_qkv_self(const kw_dec_qkv_self_args* args, kw_stream_t stream);
size_t kw_dec_qkv_self_workspace(int64_t M, int64_t d);
int kw_dec_qkv_self_supported(int64_t M, int64_t d, int64_t H);

/* The cross-attention block's query projection and attention step of one greedy decode step in ONE launch
 * (bf16): the LayerNorm-fused q projection (TF modeling_whisper.py:483; q * head_dim^-0.5 :309) and the
 * attention over the item's encoder K / V (:323-356) -- kw_dec_linear(xq) followed by kw_cross_attn_step
 * (q_len 1) without the kernel boundary, bit for bit: the projection hands the query to the attention
 * in-launch as 8-byte {bf16 x 2, tag} granules while the chunks' K / V streams are already in flight.
 *   x: hb [M][ldx] bf16; W: packed [d][d] with gamma folded (kw_pack_weight); ln_colsum / bias: [d] f32; scale
 *   multiplies every column; k / v: one layer's [M][H][S][64] bf16 (item m's K / V); out: [M][d] bf16.
 *   M <= 32, d = 64 H <= 1280, S such that kw_cross_attn_step's chunks hold 225..256 keys (e.g. 1500).
 * workspace >= kw_dec_xq_cross_workspace(M, d, H, S) bytes, ZERO-FILLED before first use (every call re-arms
 * it).  Every in-launch wait is on work dispatched before it (no co-residency assumption: safe beside other
 * work on the GPU).  kw_dec_xq_cross_supported(): 1 when the shape is covered. */
typedef struct {
  const void* x;
  int64_t ldx;
  float ln_eps;
  const float* ln_colsum;
  const void* W;
  const float* bias;
  float scale;
  int64_t M, d, H;
  const void* k;
  const void* v;
  int64_t S;
  void* out;
  void* workspace;
  size_t ws_bytes;
} kw_dec_xq_cross_args;

int kw_dec_xq_cross(const kw_dec_xq_cross_args* args, kw_stream_t stream);
size_t kw_dec_xq_cross_workspace(int64_t M, int64_t d, int64_t H, int64_t S);
int kw_dec_xq_cross_supported(int64_t M, int64_t d, int64_t H, int64_t S);

/* Which grid a bf16 one-row cross-attention of `rows` = B * H (row, head) pairs over S keys launches (for
 * profilers naming kernels): 1 = one workgroup per pair streaming its chunks (cross_attn_row_kernel; used when
 * the pairs fill the CUs and fit at once and S = 1500), 0 = one workgroup per (pair, chunk).  fused: the
 * kw_dec_xq_cross variant.  Both give bitwise the same rows. */
int kw_cross_attn_pair_kernel(int64_t rows, int64_t S, int fused);

/* Decoder cross-attention against cached encoder K/V [B][H][S][hd] (TF modeling_whisper.py:323-326).
 * q: [B*q_len][H*hd]; out: [B*q_len][H*hd]; S <= 2048; workspace >= kw_cross_attn_workspace(...) bytes and
 * ZERO-FILLED before its first use (it holds arrival counters that every call leaves at zero). */
int kw_cross_attn_step(int dtype, const void* q, int64_t B, int64_t q_len, int64_t H, int64_t hd,
                       const void* k, const void* v, int64_t S, void* out, void* workspace,
                       size_t ws_bytes, kw_stream_t stream);
size_t kw_cross_attn_workspace(int64_t B, int64_t q_len, int64_t H, int64_t hd, int64_t S);

/* Hand-off status of kw_dec_qkv_self / kw_dec_xq_cross / kw_cross_attn_step: the byte offset, inside the
 * caller's workspace of that entry point (same dimensions), of an int32 STATUS word.  A launch whose in-launch
 * hand-off poll timed out (a protocol failure, never expected) -- or, for kw_dec_qkv_self, whose cur_len was
 * outside [1, min(256, t_max)] -- sets it nonzero and writes NaN into the rows concerned; no kernel clears it.
 * The caller reads it after synchronizing the stream and, when it is set, rejects that work's results and
 * zero-fills the whole workspace (a late producer may have left granules armed) before the next launch
 * (failures surface as errors, not as tokens; kwhisper.decode raises KWError).
 * The int32 after the status word of kw_dec_qkv_self / kw_dec_xq_cross is a FAULT-INJECTION word for tests:
 * while it is nonzero, the next launch's first projection workgroup skips its publish and clears it, so
 * that launch's consumers of the projection's columns [0, 16) time out and set the status word. */
size_t kw_dec_qkv_self_status_offset(int64_t M, int64_t d);
size_t kw_dec_xq_cross_status_offset(int64_t M, int64_t d, int64_t H, int64_t S);
size_t kw_cross_attn_status_offset(int64_t B, int64_t q_len, int64_t H, int64_t hd, int64_t S);

/* ---- fp8 cross K/V (additive, ABI 112 unchanged; opt-in: WhisperEngine(cross_kv_dtype="fp8_e4m3")) ----------
 * The cross-attention K / V cache at one byte per element.  Format:
 *   codes:  uint8 [2L][B][H][S][64], OCP e4m3fn (the gfx950 fp8; NOT the fnuz variant): the bf16 cache's layout.
 *   scales: float32 [2L][B][H][64]: one per (K or V of a layer, item, head, head dim), taken over the S frames.
 * From the bf16 values x that the cross-K/V GEMM wrote (kw_gemm, KW_EPI_HEADSPLIT), per channel:
 *   a     = max_s |x|
 *   scale = a / 448.0f
 *   inv   = 448.0f / a            (one correctly rounded f32 division per channel)
 *   a == 0:  scale = inv = 0 and every code 0
 *   code  = e4m3_rne(x * inv)     (one f32 multiply, round to nearest even; |x * inv| exceeds 448 by f32 rounding
 *                                  at most, and that rounds to 448)
 *   dequantised value = float(code) * scale
 * Non-finite K / V is out of scope.
 *
 * kw_cross_kv_quant: x bf16 [n][S][64] -> codes uint8 [n][S][64], scales f32 [n][64], n = the (K/V, layer, item, head)
 * tiles of the call, any S >= 1; x and codes 16-B aligned.  Replaces nothing in TF (the reference keeps bf16): it
 * follows the k_proj / v_proj of TF modeling_whisper.py:323-335 once per item. */
int kw_cross_kv_quant(const void* x, int64_t n, int64_t S, int64_t hd, void* codes, float* scales, kw_stream_t stream);

/* kw_cross_attn_step over the fp8 cache (TF modeling_whisper.py:323-356 on the dequantised K / V): q, out bf16
 * [B*q_len][H*hd]; k / v: one layer's codes [B][H][S][64]; k_scale / v_scale: its scales [B][H][64].  f32 arithmetic
 * on the decoded codes; K's scales multiply the query once (q'[i] = q[i] * log2(e) * s_k[i]), V's the output
 * (o[i] * s_v[i] / l).  Differences from the bf16 dispatch:
 *   - ONE grid at every batch size: one workgroup per (query row, head) pair streaming the pair's six chunks (the pair
 *     kernel of kw_cross_attn_pair_kernel); no chunk grid, no multi-row kernel, no workspace, no hand-off, no status
 *     word.  Small batches under-fill the device, large ones take several rounds; a row's output does not depend on
 *     its batch.
 *   - q_len > 1 (the prefill) runs as B * q_len * H pairs: query row r reads item r / q_len, so K / V is re-read once
 *     per position.
 *   - S must split into six chunks of 225..256 keys (1500: 6 x 250; 1399: 5 x 234 + 229; 1536: 6 x 256); anything
 *     else, and hd != 64, is KW_EUNSUPPORTED with a message.
 * q, k, v, k_scale 16-B aligned. */
int kw_cross_attn_step_fp8(const void* q, int64_t B, int64_t q_len, int64_t H, int64_t hd, const void* k, const void* v,
                           const float* k_scale, const float* v_scale, int64_t S, void* out, kw_stream_t stream);

/* kw_dec_xq_cross over the fp8 cache: the LayerNorm-fused q projection and kw_cross_attn_step_fp8 (q_len 1) in ONE
 * launch, bit for bit kw_dec_linear(xq) followed by kw_cross_attn_step_fp8.  Arguments as kw_dec_xq_cross_args with
 * k / v one layer's codes [M][H][S][64] and k_scale / v_scale its scales [M][H][64].  The projection workgroups lead
 * the grid; every wait is on work dispatched earlier in the same launch.  The workspace is kw_dec_xq_cross's:
 * kw_dec_xq_cross_workspace(M, d, H, S) bytes, zero-filled before first use, with the status word and the
 * fault-injection word at kw_dec_xq_cross_status_offset(M, d, H, S).  Shapes: M <= 32, d = 64 H <= 1280, S as
 * kw_cross_attn_step_fp8 (kw_dec_xq_cross_fp8_supported(): 1 when covered; the pair grid at every M). */
typedef struct {
  const void* x;
  int64_t ldx;
  float ln_eps;
  const float* ln_colsum;
  const void* W;
  const float* bias;
  float scale;
  int64_t M, d, H;
  const void* k;
  const void* v;
  const float* k_scale;
  const float* v_scale;
  int64_t S;
  void* out;
  void* workspace;
  size_t ws_bytes;
} kw_dec_xq_cross_fp8_args;

int kw_dec_xq_cross_fp8(const kw_dec_xq_cross_fp8_args* args, kw_stream_t stream);
int kw_dec_xq_cross_fp8_supported(int64_t M, int64_t d, int64_t H, int64_t S);

/* One greedy decoding step on f32 logits [B][V] (TF generation/utils.py:2894-2937):
 * SuppressTokens -> SuppressTokensAtBegin (when L == begin_index) -> WhisperTimeStamp (if
 * return_timestamps; TF generation/logits_process.py:1816-2047) -> argmax (first max) ->
 * finished rows emit pad -> ids[b][L] = token; unfinished[b] updated (EOS / L+1 >= max_length);
 * the last workgroup advances *cur_len and writes *n_unfinished.  suppress_mask: [V] uint8 (1 = suppressed).
 * scores_out: optional [B][V] f32 copy of the processed scores (NULL to skip). */
typedef struct {
  float* logits;
  int64_t B, V;
  const uint8_t* suppress_mask;
  const int32_t* begin_suppress;
  int32_t n_begin_suppress;
  int32_t return_timestamps;
  int32_t ts_begin, no_ts_id, eos_id, pad_id;
  int32_t max_initial_ts;     /* -1 = None */
  int64_t* ids;               /* [B][ids_stride] */
  int64_t ids_stride;
  int32_t* cur_len;
  int32_t max_length, begin_index;
  int32_t* unfinished;        /* [B] */
  int32_t* counter;           /* [1] scratch, zero before first use */
  int32_t* n_unfinished;      /* [1] rows still unfinished after this step (written by the last workgroup) */
  float* scores_out;
  void* workspace;            /* optional, zero-filled once, >= kw_greedy_step_workspace(B) bytes: without
                                 timestamps / scores_out each row is split over several workgroups whose
                                 partial argmaxes the row's last arriver combines (NULL: one workgroup per row) */
  size_t ws_bytes;
} kw_sampler_args;

int kw_greedy_step(const kw_sampler_args* args, kw_stream_t stream);
size_t kw_greedy_step_workspace(int64_t B);

/* The LM head and the greedy step of one decode step in ONE launch (no timestamps): kw_dec_linear(lm) -- the final
 * LayerNorm folded, proj_out (TF modeling_whisper.py:790,1080) -- followed by kw_greedy_step (TF generation/
 * utils.py:2894-2937: SuppressTokens, SuppressTokensAtBegin, argmax, finished rows emit pad, stopping) without the
 * kernel boundary: every workgroup of the LM head's weight stream publishes, per row, the processed arg-max of its
 * run of columns, and the last one to arrive merges them and finishes the step.  The token is kw_greedy_step's
 * (first index among equal maxima; a NaN logit never wins).
 *   lm: a kw_dec_linear LM head -- LayerNorm-fused (ln = 1) STORE, M = B <= 32 rows; lm->C: f32 logits [B][ldc], or
 *       NULL to skip storing them (the greedy step needs only the arg-max);
 *   g:  a kw_sampler_args of the same B x V with return_timestamps = 0 and scores_out = NULL; g->logits and
 *       g->counter are not used; g->workspace >= kw_dec_lm_greedy_workspace(B, V) bytes, ZERO-FILLED before first
 *       use (every launch re-arms it); g->max_length - g->begin_index <= 448: the launch looks for a row's earlier
 *       EOS in the 448 positions after begin_index only, so a longer generation is KW_EUNSUPPORTED (kw_greedy_step
 *       scans every position up to cur_len).
 * kw_dec_lm_greedy_supported(B, V, d): 1 when the shape is covered (else use kw_dec_linear + kw_greedy_step). */
int kw_dec_lm_greedy(const kw_dec_linear_args* lm, const kw_sampler_args* g, kw_stream_t stream);
size_t kw_dec_lm_greedy_workspace(int64_t B, int64_t V);
int kw_dec_lm_greedy_supported(int64_t B, int64_t V, int64_t d);

/* ---- sampling step with running log-probabilities (additive, ABI 112 unchanged) -------------------------
 * One decode step's token choice for all rows, for Whisper's temperature fallback (TF models/whisper/
 * generation_whisper.py:970-1116; sampling as TF generation/utils.py _sample: processors, temperature warp, softmax,
 * multinomial).  The processors, the finished-row handling (pad), the stopping rules, the *cur_len advance and
 * *n_unfinished are kw_greedy_step's, so the step replays from the same hipGraph loop; both return_timestamps modes.
 * Every row is split over several workgroups whose partials the row's last arriver merges (as kw_greedy_step with a
 * workspace), so workspace is REQUIRED: >= kw_sample_step_workspace(B) bytes, zero-filled once (launches leave it zeroed).
 *
 * Token.  s(v) = the processed scores (SuppressTokens, SuppressTokensAtBegin, WhisperTimeStamp with its probability-
 * mass rule evaluated on the un-warped scores).  *inv_temperature == 0: argmax_v s(v), first index on ties -- exactly
 * kw_greedy_step's token.  Otherwise argmax_v( s(v) * inv_temperature + g(v) ) over the v with s(v) > -inf (first index
 * on ties), g = Gumbel noise: in distribution softmax(s / T) followed by a multinomial draw.
 *
 * Noise.  Counter-based Philox4x32-10 (multipliers 0xD2511F53 on word 0, 0xCD9E8D57 on word 2; key increments
 * 0x9E3779B9, 0xBB67AE85; ten rounds), generated in the kernel:
 *   counter = (v >> 2, L, row, *attempt)   L = the position written (*cur_len at entry), row = the row's index b
 *   key     = (low, high) 32-bit halves of *seed
 *   x       = output word v & 3
 * so the noise of (seed, attempt, row, L, v) does not depend on B, on the split or on the grid.  The uniform takes the
 * TOP 20 BITS of x: u = ((x >> 12) + 0.5) * 2^-20, in [2^-21, 1 - 2^-21], and g = -logf(-logf(u)) (f32), finite for
 * every x: g in [-2.679, 14.557].  (20 bits: the draw stays recoverable from the stored f32 g, see noise_out.)
 *
 * Running statistics, for the rows not finished before this step (first EOS counted, pad positions after it not):
 *   sum_logprob[b] += s(tok) - logsumexp_v s(v)   and   n_tokens[b] += 1     (f32, in step order)
 * over the fully processed scores -- when the mass rule bans text the normaliser runs over the timestamps only -- and
 * without the temperature (TF generation_whisper.py:1958-1974: scores * rescale_temperature); sum / n is
 * _retrieve_avg_logprobs' value.  The caller zeroes both before the first step of a decode.
 *
 * active (optional, [B] uint8): a row with 0 is finished from the first step -- it emits pad, is not counted in
 * *n_unfinished and accumulates nothing (a fallback attempt re-decodes only the rows that need it).
 * noise_out (optional, [B][V] f32): receives g(v) for every v (0 when *inv_temperature == 0); validation only.
 * inv_temperature, seed and attempt are DEVICE pointers read by the launch: one captured graph serves a schedule. */
typedef struct {
  const float* logits;        /* [B][V] f32 raw logits */
  int64_t B, V;
  const uint8_t* suppress_mask;
  const int32_t* begin_suppress;
  int32_t n_begin_suppress;
  int32_t return_timestamps;
  int32_t ts_begin, no_ts_id, eos_id, pad_id;
  int32_t max_initial_ts;     /* -1 = None */
  int64_t* ids;               /* [B][ids_stride] */
  int64_t ids_stride;
  int32_t* cur_len;
  int32_t max_length, begin_index;
  int32_t* unfinished;        /* [B] */
  int32_t* counter;           /* [1] scratch, zero before first use */
  int32_t* n_unfinished;      /* [1] */
  const float* inv_temperature; /* [1] 1 / T, or 0 for the argmax */
  const uint64_t* seed;       /* [1] */
  const uint32_t* attempt;    /* [1] */
  float* sum_logprob;         /* [B] in/out */
  int32_t* n_tokens;          /* [B] in/out */
  const uint8_t* active;      /* [B] or NULL */
  float* noise_out;           /* [B][V] or NULL */
  void* workspace;
  size_t ws_bytes;
} kw_sample_args;

int kw_sample_step(const kw_sample_args* args, kw_stream_t stream);
size_t kw_sample_step_workspace(int64_t B);

/* ---- speculative decoding: the accept step (additive, ABI 112 unchanged) -------------------------------
 * One launch per round, for ONE row (generate(assistant_model=...), batch size 1).  An assistant decoder has drafted K
 * tokens into ids[L, L + K), L = *cur_len of the main decoder; the main decoder's forward over the K + 1 newest
 * positions left logits [K + 1][V] (f32), row j predicting position L + j.  For j = 0 .. K the launch computes t_j, the
 * token kw_greedy_step would choose at *cur_len = L + j with the history ids[0, L + j) -- the drafts before j in
 * place, so a draft that closes a timestamp pair or shifts the probability-mass rule acts on the positions behind it.
 * The processors are kw_greedy_step's (SuppressTokens, SuppressTokensAtBegin at L + j == begin_index,
 * WhisperTimeStamp), each position is split over workgroups as there, ties go to the first index: t_j equals
 * kw_greedy_step's token (with a workspace) bit for bit.  Then, q running from 0:
 *   L + q >= max_length: the row is finished, nothing is written at or beyond max_length;
 *   q < K and ids[L + q] == t_q: the draft is accepted (n += 1); an accepted EOS, or L + q + 1 >= max_length,
 *     finishes the row; otherwise go on with q + 1;
 *   else ids[L + q] = t_q -- the correction, or at q == K the bonus token -- which finishes the row if it is EOS or
 *     L + q + 1 >= max_length; stop.
 * new length = the position after the last token kept.  A finished row: ids[new length, min(L + K + 1, max_length))
 * = pad_id, *unfinished = 0, *n_unfinished = 0 (else 1).  Device state written (plain stores by one thread):
 *   *cur_len = new length; *asst_cur_len = new length and *asst_unfinished = 1 (the assistant may have drafted an
 *   EOS) where given; *verify_len = new length + K (the cur_len the next round's K + 1-position forward reads) where
 *   given; stats[0] += 1 (rounds), stats[1] += K (drafted), stats[2] += n (accepted) where given.
 * *unfinished == 0 at entry: the launch decides nothing and leaves ids, lengths, flags and stats as they are (replays
 * behind the host's poll are harmless); it only puts *asst_cur_len back to *cur_len, so an assistant that keeps
 * drafting behind a finished row never moves further than K + 1 positions past the final length.
 * workspace: REQUIRED, >= kw_spec_accept_workspace(K) bytes (0 for an unsupported K), zero-filled once; every launch
 * leaves it all zero.  1 <= K <= 31; max_length <= ids_stride. */
typedef struct {
  const float* logits;        /* [K + 1][V] f32 raw logits of positions L .. L + K */
  int64_t V;
  int32_t K;
  const uint8_t* suppress_mask;
  const int32_t* begin_suppress;
  int32_t n_begin_suppress;
  int32_t return_timestamps;
  int32_t ts_begin, no_ts_id, eos_id, pad_id;
  int32_t max_initial_ts;     /* -1 = None */
  int64_t* ids;               /* [ids_stride]: the row */
  int64_t ids_stride;
  int32_t* cur_len;           /* [1] the main decoder's */
  int32_t max_length, begin_index;
  int32_t* unfinished;        /* [1] */
  int32_t* n_unfinished;      /* [1] */
  int32_t* asst_cur_len;      /* [1] or NULL */
  int32_t* asst_unfinished;   /* [1] or NULL */
  int32_t* verify_len;        /* [1] or NULL */
  int32_t* stats;             /* [3] rounds, drafted, accepted; or NULL */
  void* workspace;
  size_t ws_bytes;
} kw_spec_accept_args;

int kw_spec_accept(const kw_spec_accept_args* args, kw_stream_t stream);
size_t kw_spec_accept_workspace(int64_t K);

/* ---- beam search step (a10: TF/generation/utils.py:3208-3527), num_return_sequences = 1 ----------
 * Running rows are R = B * num_beams, item-major (row = b * num_beams + beam).  One step is
 * kw_beam_logprobs then kw_beam_select; both read the device cur_len and do nothing once *done != 0,
 * so the step can be replayed from a hipGraph past the end of the search. */

/* log_softmax of each row's raw f32 logits (utils.py:3380), the Whisper processors on the log-probs
 * (as kw_greedy_step, with the row's own history ids[r][0..L) ), and the row's k best processed
 * log-probs, descending, ties to the lower token id: cand_val/cand_idx [R][k], k <= 16.  A row with
 * fewer than k finite scores goes on with -inf and its lowest -inf token ids, as a top-k over the row. */
typedef struct {
  const float* logits;
  int64_t R, V;
  const uint8_t* suppress_mask;
  const int32_t* begin_suppress;
  int32_t n_begin_suppress;
  int32_t return_timestamps;
  int32_t ts_begin, no_ts_id, eos_id;
  int32_t max_initial_ts;     /* -1 = None */
  const int64_t* ids;         /* [R][ids_stride] running histories */
  int64_t ids_stride;
  const int32_t* cur_len;
  int32_t begin_index;
  int32_t k;
  float* cand_val;
  int32_t* cand_idx;
  const int32_t* done;
  void* workspace;            /* optional, zero-filled once, >= kw_beam_logprobs_workspace(R) bytes: each row
                                 over several workgroups + a last-arriver merge (NULL: one workgroup per row) */
  size_t ws_bytes;
} kw_beam_logprobs_args;

int kw_beam_logprobs(const kw_beam_logprobs_args* args, kw_stream_t stream);
size_t kw_beam_logprobs_workspace(int64_t R);

/* Selection for one step (utils.py:3077-3205, 3008-3075): top 2*num_beams continuations over
 * beams x vocab of (log-prob + running score), MaxLength / EOS criteria, the next running beams
 * (ids rows rewritten in place: parent history + token; bp rows: parent slot table + own slot),
 * the finished set (fin_seq/fin_score/fin_len/fin_flag, length_penalty, early_stopping 0 = False,
 * 1 = True, 2 = "never"), the early-stop heuristic (unsat) and, from the last item, *go (1 = the
 * reference loop continues) / *done, and *cur_len += 1.  Initial state: ids rows = prompt, bp rows =
 * own row for p < P (or bp NULL when the K/V cache is not shared), run_scores = [0, -1e9, ...] per
 * item, fin_seq = fill_id, fin_score = -1e9, fin_len = fin_flag = 0, unsat = 1, counter = go = done = 0.
 * 2 <= num_beams <= 8, max_length <= 512, fin_stride / ids_stride / bp_stride >= max_length.
 * A step writes positions [0, cur_len] of the ids / bp rows and [0, max_length) of the fin_seq rows;
 * what a row holds beyond is left alone.
 * The continuations come from each row's 2*num_beams candidates, not from the whole vocabulary.  That
 * is the reference's flat top-k over beams x vocab except when a row's score absorbs log-prob
 * differences: a token outside the row's candidates whose f32 sum (log-prob + score) equals that of
 * a candidate, has the lower id and is among the item's 2*num_beams best sums.  The reference then
 * keeps the lower ids of the tie, this step the higher log-probs.  A row with a -1e9 score (ulp 64)
 * ties all its tokens above -32 this way; such a row is reached only when the other rows of its item
 * hold fewer than 2*num_beams finite candidates between them. */
typedef struct {
  int64_t B;
  int32_t num_beams;
  int64_t V;
  const float* cand_val;
  const int32_t* cand_idx;
  int64_t* ids;
  int64_t ids_stride;
  int32_t* bp;
  int64_t bp_stride;
  float* run_scores;          /* [R] */
  int64_t* fin_seq;           /* [B][num_beams][fin_stride] */
  int64_t fin_stride;
  float* fin_score;           /* [B][num_beams] */
  int32_t* fin_len;           /* generated tokens of each finished sequence */
  int32_t* fin_flag;
  int32_t* unsat;             /* [B] */
  int32_t* cur_len;
  int32_t begin_index;        /* prompt length */
  int32_t max_length;
  int32_t eos_id;
  int32_t fill_id;            /* pad_token_id (or eos when there is none) */
  float length_penalty;
  int32_t early_stopping;
  int32_t* counter;
  int32_t* go;
  int32_t* done;
  int32_t* item_flags;        /* [B][3] scratch */
} kw_beam_select_args;

int kw_beam_select(const kw_beam_select_args* args, kw_stream_t stream);

/* kw_beam_select that also records who produced what (additive, ABI 112 unchanged; token timestamps under beam
 * search need the reference's beam_indices).  Everything kw_beam_select writes is written bit for bit the same; two
 * more outputs, both int32 on the device:
 *   parent_log [max_length][B * num_beams]: the step at cur_len = L writes row L -- parent_log[L][r] is the running
 *     row (of the whole batch, b * num_beams + beam) that next running row r continues;
 *   fin_parent [B][num_beams]: for every slot of the finished set, the running row its hypothesis' last token was
 *     taken from; it moves with its slot exactly as fin_score / fin_len / fin_flag do (initial state: any value).
 * With fin_len, a backtrace from fin_parent through parent_log gives the running row that produced every token of a
 * finished hypothesis: row[n - 1] = fin_parent, row[k - 1] = parent_log[begin_index + k - 1][row[k]]. */
int kw_beam_select_parents(const kw_beam_select_args* args, int32_t* parent_log, int32_t* fin_parent,
                           kw_stream_t stream);

/* ---- token-level timestamps (additive, ABI 112 unchanged) --------------------------------------------
 * return_token_timestamps: WhisperGenerationMixin._extract_token_timestamps, _median_filter and
 * _dynamic_time_warping (TF/models/whisper/generation_whisper.py:241-381, 43-61, 64-115) on device.
 * Head dimension 64.  `heads`, `slots` and `pairs` below are HOST arrays, read (and range-checked) at the call. */

/* One decode step's log entry.  q: [B][d] (dtype), the scaled cross-attention queries of one layer for the step whose
 * position the device cur_len names; for i < n (<= 32) the 64-wide slice of head heads[i] of every row is copied to
 * log[slots[i]][b][t][0..63], log: [n_slots][B][t_log][64] (dtype), t = cur_len - 1 - begin_index (the index of the
 * step's input token among the generated ones); steps with t outside [0, t_log) write nothing. */
int kw_align_capture(int dtype, const void* q, int64_t B, int64_t d, const int32_t* heads, const int32_t* slots,
                     int64_t n, int64_t n_slots, const int32_t* cur_len, int64_t begin_index, void* log, int64_t t_log,
                     kw_stream_t stream);

/* out[a][b][t][s] = softmax_s(qlog[a][b][t] . k_cache[pairs[a][0]][b][pairs[a][1]][s]) for t < T, a < A (<= 32 per
 * call), f32 accumulation and output.  qlog: [A][B][t_log][64], k_cache: layer l's keys [B][H][S][64] at
 * k_cache + l * k_layer_stride elements (both dtype, 16-B aligned); pairs: [A][2] (layer < n_layers, head < H);
 * out: [A][B][T][S] f32 (TF modeling_whisper.py:323-356 with scaling 1.0, the queries being scaled already). */
int kw_align_weights(int dtype, const void* qlog, int64_t t_log, const void* k_cache, int64_t k_layer_stride,
                     int64_t n_layers, const int32_t* pairs, int64_t A, int64_t B, int64_t H, int64_t S, int64_t T,
                     float* out, kw_stream_t stream);

/* kw_align_weights through a row table (beam search): the log holds R = B * n running rows per pair (item-major),
 * qlog: [A][R][t_log][64], and step t of item b is the step of log row r = rows[b][t]: its query is qlog[a][r][t] and
 * its keys are those of r's item, k_cache[layer][r / n] -- item b itself for every step of b's own hypothesis; another
 * item only where the table names a row of another item (the reference's fall-back to running row 0, TF
 * generation_whisper.py:287-289).  rows: DEVICE int32 [B][T] with entries in [0, R); an entry outside is clamped into
 * the range (wrong weights for that step, never a read outside the log or the cache).  out: [A][B][T][S] f32 as above.
 * Every (step, key) value is computed by kw_align_weights' arithmetic: out[a][b][t] equals, bit for bit, row
 * [a][rows[b][t]][t] of kw_align_weights run over all R rows (each with its item's keys). */
int kw_align_weights_rows(int dtype, const void* qlog, int64_t R, int64_t t_log, const int32_t* rows,
                          const void* k_cache, int64_t k_layer_stride, int64_t n_layers, const int32_t* pairs, int64_t A,
                          int64_t B, int64_t H, int64_t S, int64_t T, float* out, kw_stream_t stream);

/* weights [A][B][T][S] f32 -> the DTW matrix out [B][T][S] f32: each (a, b, frame) column z-scored over the T steps
 * (population std; a zero std gives NaN as in torch), a median filter of odd filter_width (<= 15) along the frames with
 * reflect padding over the row's first frames[b] frames (device int32 [B], NULL = S; skipped when that count is
 * <= filter_width / 2), the mean over the pairs, negated.  Columns >= frames[b] are written as 0.  More than 32 pairs
 * go in chunks: each call adds its A pairs (first != 0 starts from zero), the call with last != 0 divides by a_total
 * and negates. */
int kw_align_reduce(const float* weights, int64_t A, int64_t B, int64_t T, int64_t S, const int32_t* frames,
                    int64_t filter_width, float* out, int64_t a_total, int first, int last, kw_stream_t stream);

/* _dynamic_time_warping + the text-index jumps of its path, one workgroup per row: matrix [B][T][S] f32 (row b uses
 * its first frames[b] columns; device int32 [B], NULL = S), T <= 1024.  out[b][t] (int32) = the frame index at which
 * the path first reaches step t (the reference's time_indices[jumps]; -1 where the path reaches the step before any
 * frame).  float32 cost, the reference's tie rule with plain IEEE `<`.  workspace: >= kw_dtw_workspace(B, T, S) bytes
 * (the trace, one byte per cell). */
int kw_dtw(const float* matrix, int64_t B, int64_t T, int64_t S, const int32_t* frames, int32_t* out, void* workspace,
           size_t ws_bytes, kw_stream_t stream);
size_t kw_dtw_workspace(int64_t B, int64_t T, int64_t S);

/* ---- repetition_penalty / no_repeat_ngram_size (additive, ABI 112 unchanged) -------------------------
 * GenerationMixin's RepetitionPenaltyLogitsProcessor followed by NoRepeatNGramLogitsProcessor (TF generation/
 * logits_process.py:406-413, 1121-1139), which run BEFORE the Whisper processors (TF generation/utils.py:1174-1183,
 * merge at :1293).  Both read a row's whole history ids[r][0 .. L), L = *cur_len (a DEVICE scalar read by the launch,
 * so a captured step replays): forced tokens, a conditioned pass's previous text and its left pads included.
 *   penalty: every token v that occurs in the history gets s[v] = s[v] < 0 ? s[v] * penalty : s[v] / penalty -- f32,
 *            a true IEEE division, computed once from the original s[v] however often v occurs (NaN, -0.0 and +-inf
 *            take what that expression gives).  1.0 = off.
 *   ngram:   n > 0: with L >= n, for every window ids[i .. i+n) with i + n <= L whose first n-1 tokens equal the
 *            history's last n-1 tokens, s[window's last token] = -inf (n = 1 bans every token of the history; a token
 *            both penalised and banned ends as -inf).  0 = off.
 * History ids outside [0, V) are skipped, never dereferenced.  penalty <= 0 or not finite, ngram < 0 or a NULL pointer:
 * KW_EINVAL, nothing is launched. */

/* In place on f32 scores [R][V], one workgroup per row: the greedy and sampled tails run it on the raw logits between
 * the LM head and kw_greedy_step / kw_sample_step.  No workspace.  ids: [R][ids_stride] int64, ids_stride <= 4096
 * (KW_EUNSUPPORTED beyond: a thread holds its history positions' original scores in registers until every thread of
 * the row has read its own).  penalty == 1.0 && ngram == 0 leaves the buffer untouched (nothing is launched). */
int kw_repeat_process(float* scores, int64_t R, int64_t V, const int64_t* ids, int64_t ids_stride,
                      const int32_t* cur_len, float penalty, int32_t ngram, kw_stream_t stream);

/* kw_beam_logprobs with the two processors applied to every element's log-prob -- computed exactly as
 * kw_beam_logprobs computes it, (x - max) - log(sum exp(x - max)), and not renormalised afterwards (TF generation/
 * utils.py:3380-3381) -- before the Whisper processors and the timestamp mass rule.  Arguments, workspace, done and k
 * as kw_beam_logprobs.  V <= 65536 (two vocabulary bitsets per workgroup; KW_EUNSUPPORTED beyond).  With
 * penalty == 1.0 && ngram == 0 the launch IS kw_beam_logprobs's: cand_val / cand_idx are bitwise its results.
 * With a workspace (each row over several workgroups) it is two launches on the stream: a slice cannot penalise a
 * log-prob before the row's normaliser is known, so one workgroup per row first leaves (max, log sum exp) in two spare
 * floats of the row's workspace record, and the split launch reads them -- kernel order, no in-launch hand-off. */
int kw_beam_logprobs_rep(const kw_beam_logprobs_args* args, float penalty, int32_t ngram, kw_stream_t stream);

/* ---- sequence_bias / bad_words_ids (additive, ABI 112 unchanged) ------------------------------------------
 * GenerationMixin's SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor (TF generation/logits_process.py:
 * 1288-1319, 1450-1467): the first runs immediately BEFORE the repetition pair, the second immediately AFTER it and
 * before the Whisper processors (TF generation/utils.py:1154-1155, 1174-1183, 1207-1213).  A processor is a set of
 * (token sequence, f32 value) entries; NoBadWords is SequenceBias with every value -inf.  For a row with history
 * ids[r][0 .. L), L = *cur_len (a DEVICE scalar, so a captured step replays; the forced tokens, a conditioned pass's
 * previous text and its left pads are all part of the history):
 *   an entry of n tokens is considered when n <= L; n == 1 always applies; n > 1 applies when the history's last n-1
 *   tokens equal the entry's first n-1.  The bias of a token starts at 0, takes its length-1 entry's value, and every
 *   applying longer entry that ends in the token adds its value, in the processor's own order, in f32; then
 *   score[token] = score[token] + bias.  Infinite values are ordinary floats: -inf bans, +inf + -inf is NaN.
 * The table is the processor flattened on the host (kwhisper/seq_bias.py builds it), all arrays in DEVICE memory:
 *   entries grouped by their last token with a stable sort, groups in strictly ascending token order; inside a group the
 *   length-1 entry first, the others in the processor's order -- so one reader walking a group forms the reference's
 *   sum.  Every token id of the table is in [0, V): the host checks it, the kernels never dereference one that is not.
 * Caps: n_seq <= KW_SEQ_BIAS_MAX_SEQS entries of at most KW_SEQ_BIAS_MAX_LEN tokens each (max_len states the table's
 * longest); beyond them KW_EUNSUPPORTED, nothing is launched. */
#define KW_SEQ_BIAS_MAX_SEQS 4096
#define KW_SEQ_BIAS_MAX_LEN 32
typedef struct {
  const int32_t* tokens;     /* [seq_off[n_seq]] the entries' tokens, back to back */
  const int32_t* seq_off;    /* [n_seq + 1] entry s is tokens[seq_off[s] .. seq_off[s + 1]) */
  const float* values;       /* [n_seq] */
  const int32_t* group_off;  /* [n_groups + 1] group g is entries group_off[g] .. group_off[g + 1) */
  const int32_t* group_tok;  /* [n_groups] the groups' last tokens, strictly ascending */
  int32_t n_seq, n_groups;
  int32_t max_len;           /* the longest entry's token count */
} kw_seq_bias_table;

/* In place on f32 scores [R][V], one workgroup per row, a thread per group: it tests the group's entries against the
 * tail of the row's history, sums the applying values in order and adds the sum to its token -- one writer per element,
 * no float atomics; an element of no group is not touched.  The greedy and sampled tails run it on the raw logits:
 * with a sequence_bias table before kw_repeat_process, with a bad_words_ids table after it.  ids / ids_stride /
 * cur_len as kw_repeat_process reads them (L = min(*cur_len, ids_stride)).  n_seq == 0 launches nothing. */
int kw_seq_bias_process(float* scores, int64_t R, int64_t V, const int64_t* ids, int64_t ids_stride,
                        const int32_t* cur_len, const kw_seq_bias_table* table, kw_stream_t stream);

/* kw_beam_logprobs_rep with the two processors around the repetition pair, on every element's log-prob: the
 * sequence_bias table's sum is added before the penalty, the bad_words_ids table's applying entries are OR-ed into the
 * n-gram ban bitset (a ban is -inf whatever came before).  Either table may be NULL or empty; with both empty the
 * launch IS kw_beam_logprobs_rep's.  Each workgroup builds its row's matches once in LDS (a vocabulary bitset and one
 * sum per group).  V <= 65536 (KW_EUNSUPPORTED beyond), workspace and launches as kw_beam_logprobs_rep. */
int kw_beam_logprobs_proc(const kw_beam_logprobs_args* args, float penalty, int32_t ngram,
                          const kw_seq_bias_table* bias, const kw_seq_bias_table* bad_words, kw_stream_t stream);

/* ---- distillation loss on the teacher's logits (additive, ABI 112 unchanged) --------------------------
 * The temperature KL of kotoba-whisper's train_step (run_distillation.py:614-622, 652-657): with
 * p = softmax(teacher / T) and q = softmax(student / T) over the V columns of a row,
 *   row_kl[r] = sum_v p_v (log p_v - log q_v)     (a term with p_v == 0 is 0, as KLDivLoss's xlogy makes it)
 *   loss      = T^2 * sum_r row_kl[r] / n_valid   (n_valid = rows with labels[r] >= 0, counted on the device: the
 *                                                  host never synchronises)
 *   grad[r][v] = T * (q_v - p_v) / n_valid        (d loss / d student, in the student's dtype; NULL: forward only)
 * A row with a negative label is ignored: exactly 0 in row_kl and in every element of its grad row.  n_valid == 0
 * gives loss = NaN (the reference's 0 / 0) and an all-zero grad.
 * teacher: f32 [N][ldt]; student: f32 or bf16 (s_dtype) [N][lds]; labels: int64 [N]; row_kl: f32 [N]; loss: f32 [1];
 * grad: s_dtype [N][ldg].  Row strides are in elements and >= V; rows need element alignment only (V = 51865 with
 * ld == V is fine, nothing is padded).  grad sharing a byte with student or teacher is KW_EINVAL (the reference's
 * cross-entropy term still reads the student's logits).  Each logit is read twice (an online max / sum pass, then the
 * terms), all accumulation is f32, and there are no float atomics: loss, row_kl and grad are bitwise the same from run
 * to run.  workspace: >= kw_kd_loss_workspace(N) bytes, zero-filled before first use (calls leave it zeroed); three
 * launches on `stream`.  Invalid arguments: KW_EINVAL with a message, nothing is launched. */
typedef struct {
  const float* teacher;
  int64_t ldt;
  const void* student;
  int64_t lds;
  int s_dtype;               /* KW_DT_F32 or KW_DT_BF16: student and grad */
  const int64_t* labels;
  int64_t N, V;
  float temperature;         /* finite, > 0 */
  float* row_kl;
  float* loss;
  void* grad;                /* or NULL */
  int64_t ldg;
  void* workspace;
  size_t ws_bytes;
} kw_kd_loss_args;

int kw_kd_loss(const kw_kd_loss_args* args, kw_stream_t stream);
size_t kw_kd_loss_workspace(int64_t N);

#ifdef __cplusplus
}
#endif
#endif /* KWHISPER_H */
