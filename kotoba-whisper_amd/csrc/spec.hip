// Speculative decoding, the accept step (kw_spec_accept; include/kwhisper.h has the contract): one launch per round,
// for one row.  The main model's logits of the K + 1 positions L .. L + K are each turned into the token kw_greedy_step
// would choose there -- position j over NSPLIT workgroups; the slice load, the row state, each slice's statistics, the
// arrival count and the slice-ordered merge are the very functions greedy_step_split_ts_kernel calls (processors.h),
// with the drafts ids[L, L + j) as part of the history -- and the last of all (K + 1) x NSPLIT workgroups to arrive
// merges every position, walks the drafts (longest agreeing prefix, then the correction or the bonus token) and
// advances the device state of both decoders.  What this file states for itself is that walk.
#include <math.h>

#include "processors.h"

namespace {

using namespace kwp;

constexpr int KMAX = 31;  // K + 1 <= 32 positions: one thread of the last arriver per position

__global__ __launch_bounds__(SPLIT_T) void spec_accept_kernel(kw_spec_accept_args a) {
  __shared__ float shf[SPLIT_T / 64];
  __shared__ int shi[SPLIT_T / 64];
  __shared__ RowState st_sh;
  __shared__ int last_sh;
  __shared__ int tok_sh[KMAX + 1];
  // a finished row: nothing to do (no workgroup arrives, so the count stays zero); the flag is written by this
  // launch's last arriver only, after every workgroup has read it
  const int j = blockIdx.x, sl = blockIdx.y;
  const int tid = threadIdx.x;
  if (*a.unfinished == 0) {
    // (the assistant has drafted on behind the finished row: its next replay starts from the final length again)
    if (j == 0 && sl == 0 && tid == 0 && a.asst_cur_len) *a.asst_cur_len = *a.cur_len;
    return;
  }
  const int K = a.K, nq = K + 1;
  const int L0 = *a.cur_len;
  const int L = L0 + j;  // the position this workgroup's token would be written to
  const int64_t* ids = a.ids;
  const int V = (int)a.V;
  float* part = reinterpret_cast<float*>(a.workspace) + ((int64_t)j * NSPLIT + sl) * PART;
  int* cnt = reinterpret_cast<int*>(a.workspace) + (int64_t)nq * NSPLIT * PART;
  // a position at or beyond max_length has no token: arrive without a partial
  if (L < a.max_length) {
    const float* x = a.logits + (int64_t)j * a.V;
    const int per = (V + NSPLIT - 1) / NSPLIT;
    const int v0 = sl * per, v1 = min(V, v0 + per);
    float xv[SUNR];
    bool mk[SUNR];
    split_load(x, a.suppress_mask, v0, v1, xv, mk);  // in flight while the history is scanned
    // the row state from the id history [begin_index, L), the drafts before this position in place (no EOS flag:
    // the accept walk below stops at an EOS itself)
    const RowState st = history_row_state<SPLIT_T>(a, ids, L, a.return_timestamps != 0, nullptr, shi, &st_sh);
    float vals[7];
    split_slice_stats(st, x, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, v0, v1, xv, mk, shf, shi, vals);
    if (tid == 0) split_publish(part, vals);
  }
  if (tid == 0) last_sh = arrive_last(cnt, nq * NSPLIT);
  __syncthreads();
  if (!last_sh) return;
  // ---- the last arriver: position q's token by thread q ----
  if (tid < nq && L0 + tid < a.max_length) {
    float* row = reinterpret_cast<float*>(a.workspace) + (int64_t)tid * NSPLIT * PART;
    const int ii = split_merge_token(row, a.return_timestamps != 0);
    tok_sh[tid] = ii == 0x7fffffff ? 0 : ii;
#pragma unroll
    for (int q = 0; q < NSPLIT; ++q)  // the workspace is left zeroed
#pragma unroll
      for (int i = 0; i < 7; ++i) __hip_atomic_store(row + PART * q + i, 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (tid != 0) return;
  __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // ---- the accept walk: drafts ids[L0 + q] against the tokens, then the correction (q < K) or the bonus (q == K) ----
  int64_t* w = a.ids;
  int n = 0, new_len = L0, done = 0;
  for (int q = 0; q <= K; ++q) {
    const int p = L0 + q;
    if (p >= a.max_length) { done = 1; break; }
    const int tok = tok_sh[q];
    const bool match = q < K && w[p] == (int64_t)tok;
    if (!match) w[p] = tok;
    new_len = p + 1;
    n += match ? 1 : 0;
    if (tok == a.eos_id || new_len >= a.max_length) { done = 1; break; }
    if (!match) break;
  }
  if (done) {
    const int end = min(L0 + K + 1, a.max_length);
    for (int p = new_len; p < end; ++p) w[p] = a.pad_id;
    *a.unfinished = 0;
  }
  *a.n_unfinished = done ? 0 : 1;
  *a.cur_len = new_len;
  if (a.asst_cur_len) *a.asst_cur_len = new_len;
  if (a.asst_unfinished) *a.asst_unfinished = 1;
  if (a.verify_len) *a.verify_len = new_len + K;
  if (a.stats) {
    a.stats[0] += 1;
    a.stats[1] += K;
    a.stats[2] += n;
  }
}

}  // namespace

extern "C" size_t kw_spec_accept_workspace(int64_t K) {
  if (K < 1 || K > KMAX) return 0;
  return (size_t)(K + 1) * NSPLIT * PART * sizeof(float) + sizeof(int);
}

extern "C" int kw_spec_accept(const kw_spec_accept_args* a, kw_stream_t stream) {
  if (!a || !a->logits || !a->suppress_mask || !a->ids || !a->cur_len || !a->unfinished || !a->n_unfinished ||
      a->V <= 0 || a->V > 0x7fffffff || (a->n_begin_suppress > 0 && !a->begin_suppress) || a->begin_index < 0 ||
      a->max_length < 0 || (int64_t)a->max_length > a->ids_stride)
    return kw_set_error_msg(KW_EINVAL, "kw_spec_accept: invalid arguments");
  if (a->K < 1 || a->K > KMAX) return kw_set_error_msg(KW_EINVAL, "kw_spec_accept: K must be in [1, 31]");
  if (!a->workspace || a->ws_bytes < kw_spec_accept_workspace(a->K))
    return kw_set_error_msg(KW_EINVAL, "kw_spec_accept: workspace missing or smaller than kw_spec_accept_workspace(K)");
  hipLaunchKernelGGL(spec_accept_kernel, dim3((unsigned)(a->K + 1), NSPLIT), dim3(SPLIT_T), 0, (hipStream_t)stream, *a);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
