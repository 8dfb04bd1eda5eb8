// Greedy decode step on device (K14 + K15): logits processors, argmax, finished-row handling and
// the cur_len advance -- no host sync per step, so a whole decode step can live in one hipGraph.
//
// Reference order (transformers 5.15.0): SuppressTokens (TF/generation/logits_process.py:1869-1906)
// -> SuppressTokensAtBegin (:1816-1866, when input_ids.shape[-1] == begin_index) -> WhisperTimeStamp
// (:1909-2047, only with return_timestamps) -> argmax (TF/generation/utils.py:2925, first max wins)
// -> finished rows emit pad (:2929) -> MaxLength / EOS stopping (stopping_criteria.py:75-77).
// The WhisperTimeStamp per-row state (last / penultimate token, last timestamp, finished flag) is
// derived from the row's own id history each step, exactly as the reference re-derives it from
// input_ids.  Without a workspace: one 1024-thread workgroup per row; the processed row is recomputed on
// the fly in each of the four L2-resident passes (max, sum, timestamp log-sum-exp, argmax) instead of
// materialised.  With one: a row over NSPLIT workgroups (greedy_step_split_kernel, greedy_step_split_ts_kernel).
// Every step these kernels share with each other, with kw_sample_step below and with kw_spec_accept (the row
// state, the slice load and walk, the reductions, the arrival count, the end of a step) is a function of processors.h.
#include <math.h>

#include "processors.h"

namespace {

using namespace kwp;

__global__ __launch_bounds__(ST) void greedy_step_kernel(kw_sampler_args a) {
  __shared__ float shf[ST / 64];
  __shared__ int shi[ST / 64];
  __shared__ RowState st_sh;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int L = *a.cur_len;
  const int64_t* ids = a.ids + (int64_t)b * a.ids_stride;
  const float* x = a.logits + (int64_t)b * a.V;
  const int V = (int)a.V;

  // ---- history: finished flag and the WhisperTimeStamp row state --------------------------------
  int fin = 0;
  RowState st = history_row_state<ST>(a, ids, L, a.return_timestamps, &fin, shi, &st_sh);
  // ---- timestamp probability-mass rule (logits_process.py:2040-2045) ---------------------------
  if (st.rt) timestamp_rule(st, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, V, [&](int v) { return x[v]; }, shf);

  // ---- argmax (first index on ties) -----------------------------------------------------------
  // 8 loads of the logits and the suppress mask in flight per thread before any compare (a one-load
  // loop pays an L2 round trip per 4 KB of the row)
  float best = -INFINITY;
  int bi = 0x7fffffff;
  constexpr int UNR = 8;
  for (int v0 = tid; v0 < V; v0 += ST * UNR) {
    float xv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int v = v0 + u * ST;
      xv[u] = v < V ? x[v] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int v = v0 + u * ST;
      if (v < V) {
        const float s = process(st, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, v, xv[u]);
        if (a.scores_out) a.scores_out[(int64_t)b * a.V + v] = s;
        if (s > best || (s == best && v < bi)) { best = s; bi = v; }
      }
    }
  }
  // (wg_argmax<ST>, spelled out with thread 0 alone merging the waves: with the call here hipcc's gfx950 code lost
  // the first unrolled element's logit on the timestamp path above, and test_greedy_step_vs_oracle caught it)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if ((tid & 63) == 0) { shf[tid >> 6] = best; shi[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    float bb = shf[0];
    int ii = shi[0];
    for (int i = 1; i < ST / 64; ++i) {
      if (shf[i] > bb || (shf[i] == bb && shi[i] < ii)) { bb = shf[i]; ii = shi[i]; }
    }
    finish_row(a, b, L, fin, ii);
  }
}

// Split-row variant (no timestamps, no scores_out): row b's V logits are cut into NSPLIT slices of one
// 512-thread workgroup each (16 loads in flight per thread: one memory round trip per slice instead of
// a serial walk over the row); each slice publishes its (max, first index, finished flag) write-through,
// and the last of all B x NSPLIT workgroups to arrive combines every row's slices in slice order (first
// index on ties, as torch.argmax) and finishes the step as finish_row does, for every row at once.
__global__ __launch_bounds__(SPLIT_T) void greedy_step_split_kernel(kw_sampler_args a) {
  __shared__ float shf[SPLIT_T / 64];
  __shared__ int shi[SPLIT_T / 64];
  const int b = blockIdx.x, sl = blockIdx.y;
  const int tid = threadIdx.x;
  const int L = *a.cur_len;
  const int64_t* ids = a.ids + (int64_t)b * a.ids_stride;
  const float* x = a.logits + (int64_t)b * a.V;
  const int V = (int)a.V;
  const int per = (V + NSPLIT - 1) / NSPLIT;
  const int v0 = sl * per, v1 = min(V, v0 + per);
  const bool first = L == a.begin_index;
  // the slice's logits and SuppressTokens bytes all in flight first (a mask load inside the compare chain
  // below cost one round trip per element; the history scan's loop waits on every load it has issued)
  float xv[SUNR];
  bool mk[SUNR];
  split_load(x, a.suppress_mask, v0, v1, xv, mk);
  // a row is finished once it emitted EOS (stopping_criteria.py:75-77): one id per thread, in parallel
  // (the row's last arriver needs it; a serial walk there would pay one load latency per position)
  int fin = 0;
  for (int p = a.begin_index + tid; p < L; p += SPLIT_T) fin |= ids[p] == a.eos_id;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int vb = v0; vb < v1;) {  // one round for V <= NSPLIT * 8192
#pragma unroll
    for (int u = 0; u < SUNR; ++u) {
      const int v = vb + tid + u * SPLIT_T;
      if (v < v1) {
        float s = mk[u] ? -INFINITY : xv[u];
        if (first)
          for (int i = 0; i < a.n_begin_suppress; ++i)
            if (a.begin_suppress[i] == v) s = -INFINITY;
        if (s > best || (s == best && v < bi)) { best = s; bi = v; }
      }
    }
    vb += SPLIT_T * SUNR;
    if (vb < v1) split_load(x, a.suppress_mask, vb, v1, xv, mk);  // beyond that the window is reloaded, not walked as a tail
  }
  // (wg_argmax<SPLIT_T>, spelled out: thread 0 alone merges the waves, behind the barrier the finished flag needs
  // anyway -- the call's two barriers more measured +0.18 us on 15.25 us at B = 32, V = 51866)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if ((tid & 63) == 0) { shf[tid >> 6] = best; shi[tid >> 6] = bi; }
  fin = __syncthreads_or(fin);
  // one arrival count over all B x NSPLIT workgroups: the last to arrive finishes every row (a thread per
  // row), so the step pays one atomic round trip instead of a per-row count, an ids store + fence and a
  // second count, and the unfinished flags are summed in LDS instead of re-read
  __shared__ int last_sh, nunf_sh;
  if (tid == 0) {
    nunf_sh = 0;
    for (int i = 1; i < SPLIT_T / 64; ++i)
      if (shf[i] > best || (shf[i] == best && shi[i] < bi)) { best = shf[i]; bi = shi[i]; }
    float* part = reinterpret_cast<float*>(a.workspace) + ((int64_t)b * NSPLIT + sl) * PART;
    __hip_atomic_store(part, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<int*>(part) + 1, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<int*>(part) + 2, fin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_sh = arrive_last(a.counter, (int)a.B * NSPLIT);
  }
  __syncthreads();
  if (!last_sh) return;
  int n_unf = 0;
  for (int r = tid; r < (int)a.B; r += SPLIT_T) {
    const float* row = reinterpret_cast<const float*>(a.workspace) + (int64_t)r * NSPLIT * PART;
    float pv[NSPLIT];
    int pi[NSPLIT], pf[NSPLIT];
#pragma unroll
    for (int q = 0; q < NSPLIT; ++q) {  // every partial load in flight before the first compare
      pv[q] = __hip_atomic_load(row + PART * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pi[q] = __hip_atomic_load(reinterpret_cast<const int*>(row) + PART * q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pf[q] = __hip_atomic_load(reinterpret_cast<const int*>(row) + PART * q + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float bb = -INFINITY;
    int ii = 0x7fffffff, rf = 0;
#pragma unroll
    for (int q = 0; q < NSPLIT; ++q) {  // slice order = index order: strict > keeps the first max
      if (pv[q] > bb || (pv[q] == bb && pi[q] < ii)) { bb = pv[q]; ii = pi[q]; }
      rf |= pf[q];  // (every slice scanned the same history: all equal)
    }
    if (ii == 0x7fffffff) ii = 0;
    const int64_t tok = rf ? (int64_t)a.pad_id : (int64_t)ii;
    a.ids[(int64_t)r * a.ids_stride + L] = tok;
    const int done = rf || tok == a.eos_id || (L + 1) >= a.max_length;
    a.unfinished[r] = done ? 0 : 1;
    n_unf += done ? 0 : 1;
  }
  if (n_unf) atomicAdd(&nunf_sh, n_unf);
  __syncthreads();
  if (tid == 0) {
    *a.n_unfinished = nunf_sh;
    *a.counter = 0;
    *a.cur_len = L + 1;
  }
}

// Split-row variant WITH timestamps.  WhisperTimeStamp's probability-mass rule (logits_process.py:
// 2040-2045: ban text when logsumexp(logprobs[ts:]) > max(logprobs[:ts])) needs whole-row statistics, so
// each slice publishes, over its processed scores, the text maximum (+ first index), the timestamp
// maximum (+ first index), its own maximum with the sum of exp(s - that maximum), and the timestamp
// sum of exp(s - timestamp maximum); the row's last arriver merges them (log-sum-exp rescaling), applies
// the rule and picks the token (first index on ties, text before timestamps).
__global__ __launch_bounds__(SPLIT_T) void greedy_step_split_ts_kernel(kw_sampler_args a) {
  __shared__ float shf[SPLIT_T / 64];
  __shared__ int shi[SPLIT_T / 64];
  __shared__ RowState st_sh;
  const int b = blockIdx.x, sl = blockIdx.y;
  const int tid = threadIdx.x;
  const int L = *a.cur_len;
  const int64_t* ids = a.ids + (int64_t)b * a.ids_stride;
  const float* x = a.logits + (int64_t)b * a.V;
  const int V = (int)a.V;
  const int per = (V + NSPLIT - 1) / NSPLIT;
  const int v0 = sl * per, v1 = min(V, v0 + per);
  float xv[SUNR];
  bool mk[SUNR];
  split_load(x, a.suppress_mask, v0, v1, xv, mk);  // in flight while the history is scanned
  int fin = 0;
  const RowState st = history_row_state<SPLIT_T>(a, ids, L, 1, &fin, shi, &st_sh);
  // ---- the slice's statistics over its processed scores, published; the row's last arriver merges ----
  float vals[7];
  split_slice_stats(st, x, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, v0, v1, xv, mk, shf, shi, vals);
  if (tid != 0) return;
  float* part = reinterpret_cast<float*>(a.workspace) + ((int64_t)b * NSPLIT + sl) * PART;
  int* rcnt = reinterpret_cast<int*>(a.workspace) + (int64_t)a.B * NSPLIT * PART + b;
  split_publish(part, vals);
  if (!arrive_last(rcnt, NSPLIT)) return;
  __hip_atomic_store(rcnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  finish_row(a, b, L, fin, split_merge_token(reinterpret_cast<const float*>(a.workspace) + (int64_t)b * NSPLIT * PART, 1));
}

// ---- sampling step with running log-probabilities (kw_sample_step; include/kwhisper.h has the contract) ----
// greedy_step_split_ts_kernel's split, publish and last-arriver merge, in both timestamp modes, with two additions,
// which are all this kernel states for itself: every slice also keeps the best PERTURBED score s * inv_T + g of its
// text and of its timestamp tokens (the mass rule needs the whole row before text may be chosen, so the merge decides
// between them), and the row's merge adds the chosen token's log-probability under the processed, un-warped scores
// to the row's running sum.

// Philox4x32-10 (Salmon et al., SC'11): word `w` of the block of counter c, key k
__device__ __forceinline__ uint32_t philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                  uint32_t k1, int w) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
}

// the top 20 bits of a draw -> u in [2^-21, 1 - 2^-21] -> Gumbel noise in [-2.679, 14.557] (finite for every draw)
__device__ __forceinline__ float gumbel_noise(uint32_t x) {
  const float u = ((float)(x >> 12) + 0.5f) * 0x1p-20f;
  return -logf(-logf(u));
}

struct SampleRng {
  uint32_t k0, k1, L, row, attempt;
  float inv_t;
  bool on;
  float* out;  // the row's noise_out or NULL
  __device__ __forceinline__ float perturb(int v, float s) const {
    float g = 0.f;
    if (on) g = gumbel_noise(philox4x32_10((uint32_t)v >> 2, L, row, attempt, k0, k1, v & 3));
    if (out) out[v] = g;
    return on ? s * inv_t + g : s;
  }
};

__global__ __launch_bounds__(SPLIT_T) void sample_step_kernel(kw_sample_args a) {
  __shared__ float shf[SPLIT_T / 64];
  __shared__ int shi[SPLIT_T / 64];
  __shared__ RowState st_sh;
  const int b = blockIdx.x, sl = blockIdx.y;
  const int tid = threadIdx.x;
  const int L = *a.cur_len;
  const int64_t* ids = a.ids + (int64_t)b * a.ids_stride;
  const float* x = a.logits + (int64_t)b * a.V;
  const int V = (int)a.V;
  const int per = (V + NSPLIT - 1) / NSPLIT;
  const int v0 = sl * per, v1 = min(V, v0 + per);
  float xv[SUNR];
  bool mk[SUNR];
  split_load(x, a.suppress_mask, v0, v1, xv, mk);  // in flight while the history is scanned
  SampleRng rng;
  {
    const uint64_t seed = *a.seed;
    rng.k0 = (uint32_t)seed, rng.k1 = (uint32_t)(seed >> 32);
    rng.L = (uint32_t)L, rng.row = (uint32_t)b, rng.attempt = *a.attempt;
    rng.inv_t = *a.inv_temperature;
    rng.on = rng.inv_t != 0.f;
    rng.out = a.noise_out ? a.noise_out + (int64_t)b * a.V : nullptr;
  }
  int fin = a.active ? a.active[b] == 0 : 0;  // an inactive row is finished
  const RowState st = history_row_state<SPLIT_T>(a, ids, L, a.return_timestamps != 0, &fin, shi, &st_sh);
  // ---- the slice's statistics: plain maxima and best perturbed scores of both classes, then the two sums ----
  float sv[SUNR];
  split_process(st, a.begin_suppress, a.n_begin_suppress, v0, v1, xv, mk, sv);
  struct Acc {
    float mt = -INFINITY, ms = -INFINITY;  // plain maxima
    SliceBest p;                           // best perturbed scores among the scores that are not -inf
  };
  Acc m = split_fold(st, x, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, v0, v1, sv, Acc(),
                     [&](Acc m, int v, float s) {
                       const float p = rng.perturb(v, s);
                       const bool text = v < st.ts_begin;
                       if (text) m.mt = fmaxf(m.mt, s); else m.ms = fmaxf(m.ms, s);
                       if (s > -INFINITY) m.p = slice_take(m.p, text, p, v);
                       return m;
                     });
  float pt = m.p.mt, ps = m.p.ms;
  int jt = m.p.it, js = m.p.is;
  wg_argmax<SPLIT_T>(pt, jt, shf, shi);
  wg_argmax<SPLIT_T>(ps, js, shf, shi);
  const float mt = wg_max<SPLIT_T>(m.mt, shf), ms = wg_max<SPLIT_T>(m.ms, shf);
  const float mall = fmaxf(mt, ms);
  struct Sums { float sa = 0.f, sts = 0.f; } z;
  if (mall > -INFINITY)
    z = split_fold(st, x, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, v0, v1, sv, z, [&](Sums z, int v, float s) {
      if (s > -INFINITY) {
        z.sa += expf(s - mall);
        if (v >= st.ts_begin) z.sts += expf(s - ms);
      }
      return z;
    });
  const float sa = wg_sum<SPLIT_T>(z.sa, shf), sts = wg_sum<SPLIT_T>(z.sts, shf);
  if (tid != 0) return;
  float* part = reinterpret_cast<float*>(a.workspace) + ((int64_t)b * NSPLIT + sl) * PART;
  int* rcnt = reinterpret_cast<int*>(a.workspace) + (int64_t)a.B * NSPLIT * PART + b;
  const float vals[8] = {mt, ms, sa, sts, pt, __int_as_float(jt), ps, __int_as_float(js)};
  split_publish(part, vals);
  if (!arrive_last(rcnt, NSPLIT)) return;
  __hip_atomic_store(rcnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // ---- the row's merge: the perturbed arg-max of the class the mass rule leaves, and its log-probability ----
  const float* row = reinterpret_cast<const float*>(a.workspace) + (int64_t)b * NSPLIT * PART;
  float P[NSPLIT][8];
#pragma unroll
  for (int q = 0; q < NSPLIT; ++q)  // every partial load in flight before the merge
#pragma unroll
    for (int i = 0; i < 8; ++i) P[q][i] = __hip_atomic_load(row + PART * q + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  float bt = -INFINITY, bs = -INFINITY, bpt = -INFINITY, bps = -INFINITY;
  int kt = 0x7fffffff, ks = 0x7fffffff;
  for (int q = 0; q < NSPLIT; ++q) {  // slice order = index order
    const int qt = __float_as_int(P[q][5]), qs = __float_as_int(P[q][7]);
    bt = fmaxf(bt, P[q][0]);
    bs = fmaxf(bs, P[q][1]);
    if (P[q][4] > bpt || (P[q][4] == bpt && qt < kt)) { bpt = P[q][4]; kt = qt; }
    if (P[q][6] > bps || (P[q][6] == bps && qs < ks)) { bps = P[q][6]; ks = qs; }
  }
  const float M = fmaxf(bt, bs), Mts = bs;
  float S = 0.f, Sts = 0.f;
  for (int q = 0; q < NSPLIT; ++q) {
    const float qm = fmaxf(P[q][0], P[q][1]);
    if (qm > -INFINITY) S += P[q][2] * expf(qm - M);
    if (P[q][1] > -INFINITY) Sts += P[q][3] * expf(P[q][1] - Mts);
  }
  int ban = 0;
  if (st.rt && M > -INFINITY) ban = mass_rule_ban(bt, Mts, M, S, Sts);  // on the un-warped scores
  int ii;
  if (ban) ii = ks;
  else ii = (bps > bpt) ? ks : kt;  // a tie keeps the text token (the lower index)
  if (!fin) {
    // log-probability of the token under the processed scores: with text banned they are the timestamps alone
    RowState sb = st;
    sb.ban_text = ban;
    const float s_tok = ii == 0x7fffffff ? -INFINITY
                                         : process(sb, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, ii, x[ii]);
    const float lp = ban ? (s_tok - Mts) - logf(Sts) : (s_tok - M) - logf(S);
    a.sum_logprob[b] += lp;
    a.n_tokens[b] += 1;
  }
  finish_row(a, b, L, fin, ii);
}

}  // namespace

extern "C" size_t kw_sample_step_workspace(int64_t B) {
  return (size_t)B * NSPLIT * PART * sizeof(float) + (size_t)B * sizeof(int);
}

extern "C" int kw_sample_step(const kw_sample_args* a, kw_stream_t stream) {
  if (!a || !a->logits || !a->suppress_mask || !a->ids || !a->cur_len || !a->unfinished || !a->counter || !a->n_unfinished ||
      !a->inv_temperature || !a->seed || !a->attempt || !a->sum_logprob || !a->n_tokens || a->B <= 0 || a->V <= 0 ||
      a->V > 0x7fffffff || (a->n_begin_suppress > 0 && !a->begin_suppress))
    return kw_set_error_msg(KW_EINVAL, "kw_sample_step: invalid arguments");
  if (!a->workspace || a->ws_bytes < kw_sample_step_workspace(a->B))
    return kw_set_error_msg(KW_EINVAL, "kw_sample_step: workspace missing or smaller than kw_sample_step_workspace(B)");
  hipLaunchKernelGGL(sample_step_kernel, dim3((unsigned)a->B, NSPLIT), dim3(SPLIT_T), 0, (hipStream_t)stream, *a);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" size_t kw_greedy_step_workspace(int64_t B) {
  return (size_t)B * NSPLIT * PART * sizeof(float) + (size_t)B * sizeof(int);
}

extern "C" int kw_greedy_step(const kw_sampler_args* a, kw_stream_t stream) {
  if (!a || !a->logits || !a->suppress_mask || !a->ids || !a->cur_len || !a->unfinished || !a->counter || !a->n_unfinished || a->B <= 0 ||
      a->V <= 0 || (a->n_begin_suppress > 0 && !a->begin_suppress))
    return kw_set_error_msg(KW_EINVAL, "kw_greedy_step: invalid arguments");
  const bool split = a->workspace && a->ws_bytes >= kw_greedy_step_workspace(a->B) && !a->scores_out;
  if (split && a->return_timestamps)
    hipLaunchKernelGGL(greedy_step_split_ts_kernel, dim3((unsigned)a->B, NSPLIT), dim3(SPLIT_T), 0, (hipStream_t)stream, *a);
  else if (split)
    hipLaunchKernelGGL(greedy_step_split_kernel, dim3((unsigned)a->B, NSPLIT), dim3(SPLIT_T), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(greedy_step_kernel, dim3((unsigned)a->B), dim3(ST), 0, (hipStream_t)stream, *a);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
