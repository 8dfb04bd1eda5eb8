// Whisper logits processors on device, and every piece the token-step kernels share: kw_greedy_step and
// kw_sample_step (sampling.hip), kw_spec_accept (spec.hip) and the processor half of kw_beam_logprobs (beam.hip).
// SuppressTokens (TF/generation/logits_process.py:1869-1906) -> SuppressTokensAtBegin (:1816-1866,
// when input_ids.shape[-1] == begin_index) -> WhisperTimeStamp (:1909-2047): the per-row state (last /
// penultimate token, last timestamp, first step) is re-derived from the row's own id history each step,
// exactly as the reference re-derives it from input_ids.
// The kernels are specified against each other bit for bit (accept = the greedy token, sample at 1 / T = 0 = greedy,
// split = one workgroup), so each step of theirs is written once, here: the workgroup reductions, the row state, the
// slice load and walk, the mass rule's decision, the arrival count and the end of a step.  The argument structs
// share their field names; the helpers that read them are templates over the struct type.  Four sites keep a step
// spelled out, each with the measurement or the fault that decided it in a comment: the arg-max tails of
// greedy_step_kernel and greedy_step_split_kernel, the two walks of split_slice_stats, and beam's slice load.
#pragma once
#include <math.h>

#include "kw_common.h"

namespace kwp {

constexpr int ST = 1024;  // threads of a one-workgroup row

struct RowState {
  int L, begin, ts_begin, no_ts, eos;
  int rt;          // return_timestamps
  int last_ts, pen_ts, has_stamp, stamp_lo;  // stamp_lo: first allowed timestamp id
  int first_step;
  int max_init;    // -1 = none
  int ban_text;
};

// process() with the SuppressTokens flag of v already loaded: the split kernels fetch the mask bytes of their
// slice together with the logits (a mask load inside the per-element compare chain cost one vmcnt(0) round
// trip per element)
__device__ __forceinline__ float process_m(const RowState& st, bool masked, const int32_t* __restrict__ bsup,
                                           int nbsup, int v, float x) {
  if (masked) return -INFINITY;
  if (st.first_step) {
    for (int i = 0; i < nbsup; ++i)
      if (bsup[i] == v) return -INFINITY;
  }
  if (st.rt) {
    if (v == st.no_ts) return -INFINITY;
    if (st.last_ts) {
      if (st.pen_ts) {
        if (v >= st.ts_begin) return -INFINITY;
      } else {
        if (v < st.eos) return -INFINITY;
      }
    }
    if (st.has_stamp && v >= st.ts_begin && v < st.stamp_lo) return -INFINITY;
    if (st.first_step) {
      if (v < st.ts_begin) return -INFINITY;
      if (st.max_init >= 0 && v > st.ts_begin + st.max_init) return -INFINITY;
    }
    if (st.ban_text && v < st.ts_begin) return -INFINITY;
  }
  return x;
}

__device__ __forceinline__ float process(const RowState& st, const uint8_t* __restrict__ mask,
                                         const int32_t* __restrict__ bsup, int nbsup, int v, float x) {
  return process_m(st, mask[v] != 0, bsup, nbsup, v, x);
}

// ---- workgroup reductions of NT threads: lane -> wave -> the NT / 64 LDS slots in index order.  Every thread
// returns the same value; the closing barrier frees the slots for the next reduction.
template <int NT>
__device__ __forceinline__ float wg_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < NT / 64; ++i) r = fmaxf(r, sh[i]);
  __syncthreads();
  return r;
}
template <int NT>
__device__ __forceinline__ float wg_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < NT / 64; ++i) r += sh[i];
  __syncthreads();
  return r;
}
// the maximum with its index, the first index among equal maxima (torch.argmax)
template <int NT>
__device__ __forceinline__ void wg_argmax(float& best, int& bi, float* shf, int* shi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { shf[threadIdx.x >> 6] = best; shi[threadIdx.x >> 6] = bi; }
  __syncthreads();
  best = shf[0];
  bi = shi[0];
  for (int i = 1; i < NT / 64; ++i)
    if (shf[i] > best || (shf[i] == best && shi[i] < bi)) { best = shf[i]; bi = shi[i]; }
  __syncthreads();
}

// ---- the row state ---------------------------------------------------------------------------------------------
// History facts -> RowState: the length L, the generation constants of the argument struct (rt apart: one kernel
// knows it), the last two tokens t1 = ids[L - 1], t2 = ids[L - 2] (looked at only where the history holds them) and
// the position and token of the history's last timestamp (lp = -1: none).
template <typename A>
__device__ __forceinline__ RowState make_row_state(const A& a, int L, int rt, int64_t t1, int64_t t2, int lp,
                                                   int lp_tok) {
  RowState st;
  st.L = L; st.begin = a.begin_index; st.ts_begin = a.ts_begin; st.no_ts = a.no_ts_id; st.eos = a.eos_id;
  st.rt = rt; st.max_init = a.max_initial_ts; st.ban_text = 0;
  const int n = L - a.begin_index;
  st.first_step = (L == a.begin_index);
  st.last_ts = n >= 1 && t1 >= a.ts_begin;
  st.pen_ts = n < 2 || t2 >= a.ts_begin;
  st.has_stamp = lp >= 0;
  st.stamp_lo = st.has_stamp ? ((st.last_ts && !st.pen_ts) ? lp_tok : lp_tok + 1) : 0;
  return st;
}

// The row state of a workgroup of NT threads, from the id history [begin_index, L): the position of the last
// timestamp (a parallel scan, then the reductions), with fin also the "emitted EOS" flag OR-ed into *fin (fin = NULL:
// the kernel has no use for it); one thread fills the state, every thread returns it past the closing barrier.
template <int NT, typename A>
__device__ __forceinline__ RowState history_row_state(const A& a, const int64_t* __restrict__ ids, int L, int rt,
                                                      int* fin, int* shi, RowState* st_sh) {
  const int tid = threadIdx.x;
  int f = fin ? *fin : 0, lsp = -1;
  for (int p = a.begin_index + tid; p < L; p += NT) {
    const int64_t t = ids[p];
    f |= t == a.eos_id;
    if (t >= a.ts_begin) lsp = max(lsp, p);
  }
  if (fin) *fin = __syncthreads_or(f);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lsp = max(lsp, __shfl_xor(lsp, o, 64));
  if ((tid & 63) == 0) shi[tid >> 6] = lsp;
  __syncthreads();
  if (tid == 0) {
    int lp = shi[0];
    for (int i = 1; i < NT / 64; ++i) lp = max(lp, shi[i]);
    const int n = L - a.begin_index;
    *st_sh = make_row_state(a, L, rt, n >= 1 ? ids[L - 1] : 0, n >= 2 ? ids[L - 2] : 0, lp, lp >= 0 ? (int)ids[lp] : 0);
  }
  __syncthreads();
  return *st_sh;
}

// WhisperTimeStamp's probability-mass rule (logits_process.py:2040-2045) on the processed scores
// s(v) = process(.., f(v)): ban text when logsumexp(logprobs[ts:]) > max(logprobs[:ts]).  Shift
// invariant, so f may be raw logits (greedy) or log-probs (beam).  (One ST-thread workgroup per row; it takes the
// timestamp sum from the log-probs, the split kernels' mass_rule_ban from the slices' rescaled sums.)
template <typename F>
__device__ __forceinline__ void timestamp_rule(RowState& st, const uint8_t* mask, const int32_t* bsup, int nbsup,
                                               int V, F f, float* shf) {
  const int tid = threadIdx.x;
  float m_all = -INFINITY, m_text = -INFINITY, m_ts = -INFINITY;
#pragma unroll 8
  for (int v = tid; v < V; v += ST) {
    const float s = process(st, mask, bsup, nbsup, v, f(v));
    m_all = fmaxf(m_all, s);
    if (v < st.ts_begin) m_text = fmaxf(m_text, s); else m_ts = fmaxf(m_ts, s);
  }
  m_all = wg_max<ST>(m_all, shf);
  m_text = wg_max<ST>(m_text, shf);
  m_ts = wg_max<ST>(m_ts, shf);
  float sum = 0.f;
#pragma unroll 8
  for (int v = tid; v < V; v += ST) {
    const float s = process(st, mask, bsup, nbsup, v, f(v));
    sum += expf(s - m_all);
  }
  sum = wg_sum<ST>(sum, shf);
  const float lse = logf(sum);
  const float lp_text_max = (m_text - m_all) - lse;
  const float lp_ts_max = (m_ts - m_all) - lse;
  float tsum = 0.f;
  if (lp_ts_max > -INFINITY) {
    for (int v = st.ts_begin + tid; v < V; v += ST) {
      const float s = process(st, mask, bsup, nbsup, v, f(v));
      const float lp = (s - m_all) - lse;
      tsum += expf(lp - lp_ts_max);
    }
  }
  tsum = wg_sum<ST>(tsum, shf);
  const float ts_lse = lp_ts_max > -INFINITY ? lp_ts_max + logf(tsum) : -INFINITY;
  if (ts_lse > lp_text_max) st.ban_text = 1;
}

// ---- a row split over workgroups (kw_greedy_step with a workspace, kw_sample_step, kw_spec_accept, and
// kw_beam_logprobs with one) ----------------------------------------------------------------------------------------
// Row b's V scores are cut into NSPLIT slices of one SPLIT_T-thread workgroup each (SUNR loads in flight per thread);
// every slice publishes its statistics, and the row's last arriver merges them in slice order.
constexpr int SPLIT_T = 512, NSPLIT = 8, SUNR = 16, PART = 8;  // PART: floats published per slice

// the slice's logits and SuppressTokens bytes from v0 on, all in flight before anything waits on them
__device__ __forceinline__ void split_load(const float* __restrict__ x, const uint8_t* __restrict__ mask, int v0, int v1,
                                           float (&xv)[SUNR], bool (&mk)[SUNR]) {
#pragma unroll
  for (int u = 0; u < SUNR; ++u) {
    const int v = v0 + threadIdx.x + u * SPLIT_T, vc = min(v, v1 - 1);  // unconditional (clamped) loads: no branches
    const float xr = x[vc];                                                  // and phis between them
    const uint8_t mr = mask[vc];
    xv[u] = v < v1 ? xr : -INFINITY;
    mk[u] = v < v1 ? mr != 0 : true;
  }
}

// the loaded window's processed scores, kept in registers
__device__ __forceinline__ void split_process(const RowState& st, const int32_t* __restrict__ bsup, int nbsup, int v0,
                                              int v1, const float (&xv)[SUNR], const bool (&mk)[SUNR],
                                              float (&sv)[SUNR]) {
#pragma unroll
  for (int u = 0; u < SUNR; ++u) {
    const int v = v0 + threadIdx.x + u * SPLIT_T;
    sv[u] = v < v1 ? process_m(st, mk[u], bsup, nbsup, v, xv[u]) : -INFINITY;
  }
}

// acc = f(acc, v, s) over this thread's processed scores of the slice [v0, v1), in index order: the register-held
// window, then -- V > NSPLIT * SPLIT_T * SUNR only -- the tail beyond it, processed from memory at every visit.  (The
// accumulator travels by value: a lambda that wrote captured locals from two branches kept them in scratch memory.)
template <typename T, typename F>
__device__ __forceinline__ T split_fold(const RowState& st, const float* __restrict__ x,
                                        const uint8_t* __restrict__ mask, const int32_t* __restrict__ bsup, int nbsup,
                                        int v0, int v1, const float (&sv)[SUNR], T acc, F f) {
#pragma unroll
  for (int u = 0; u < SUNR; ++u) {
    const int v = v0 + threadIdx.x + u * SPLIT_T;
    if (v < v1) acc = f(acc, v, sv[u]);
  }
  for (int vb = v0 + SPLIT_T * SUNR; vb < v1; vb += SPLIT_T) {
    const int v = vb + threadIdx.x;
    if (v < v1) acc = f(acc, v, process(st, mask, bsup, nbsup, v, x[v]));
  }
  return acc;
}

struct SliceBest {  // the best text and the best timestamp score, each with its first index
  float mt = -INFINITY, ms = -INFINITY;
  int it = 0x7fffffff, is = 0x7fffffff;
};
// (by value in and out: a function that reached the four members through a pointer is simplified on its own before
// it is inlined, its two branches' stores become one store through a selected pointer, and the accumulators then
// stay in scratch memory)
__device__ __forceinline__ SliceBest slice_take(SliceBest m, bool text, float s, int v) {
  if (text) {
    if (s > m.mt || (s == m.mt && v < m.it)) { m.mt = s; m.it = v; }
  } else if (s > m.ms || (s == m.ms && v < m.is)) { m.ms = s; m.is = v; }
  return m;
}

// Over the slice's processed scores: the text maximum (+ first index), the timestamp maximum (+ first index), the
// slice maximum with the sum of exp(s - that maximum), and the timestamp sum of exp(s - timestamp maximum) -- the two
// sums only with timestamps (they feed the mass rule alone).  Every thread returns the same seven values.
// (Its two walks stay spelled out: through split_fold, greedy_step_split_ts_kernel measured +0.5 us on 26.8 us and
// spec_accept_kernel with timestamps +0.6 us on 22.8 us, both outside the run-to-run spread of the spelled-out form.)
__device__ __forceinline__ void split_slice_stats(const RowState& st, const float* __restrict__ x,
                                                  const uint8_t* __restrict__ mask, const int32_t* __restrict__ bsup,
                                                  int nbsup, int v0, int v1, const float (&xv)[SUNR],
                                                  const bool (&mk)[SUNR], float* shf, int* shi, float (&vals)[7]) {
  const int tid = threadIdx.x;
  float sv[SUNR];
  float mt = -INFINITY, ms = -INFINITY;
  int it = 0x7fffffff, is = 0x7fffffff;
#pragma unroll
  for (int u = 0; u < SUNR; ++u) {
    const int v = v0 + tid + u * SPLIT_T;
    sv[u] = v < v1 ? process_m(st, mk[u], bsup, nbsup, v, xv[u]) : -INFINITY;
    if (v < v1) {
      if (v < st.ts_begin) {
        if (sv[u] > mt || (sv[u] == mt && v < it)) { mt = sv[u]; it = v; }
      } else {
        if (sv[u] > ms || (sv[u] == ms && v < is)) { ms = sv[u]; is = v; }
      }
    }
  }
  for (int vb = v0 + SPLIT_T * SUNR; vb < v1; vb += SPLIT_T) {  // V > NSPLIT * 8192 only
    const int v = vb + tid;
    if (v < v1) {
      const float s = process(st, mask, bsup, nbsup, v, x[v]);
      if (v < st.ts_begin) {
        if (s > mt || (s == mt && v < it)) { mt = s; it = v; }
      } else if (s > ms || (s == ms && v < is)) { ms = s; is = v; }
    }
  }
  wg_argmax<SPLIT_T>(mt, it, shf, shi);
  wg_argmax<SPLIT_T>(ms, is, shf, shi);
  const float mall = fmaxf(mt, ms);
  float sa = 0.f, sts = 0.f;
  if (st.rt && mall > -INFINITY) {
#pragma unroll
    for (int u = 0; u < SUNR; ++u) {
      const int v = v0 + tid + u * SPLIT_T;
      if (v < v1 && sv[u] > -INFINITY) {
        sa += expf(sv[u] - mall);
        if (v >= st.ts_begin) sts += expf(sv[u] - ms);
      }
    }
    for (int vb = v0 + SPLIT_T * SUNR; vb < v1; vb += SPLIT_T) {
      const int v = vb + tid;
      if (v < v1) {
        const float s = process(st, mask, bsup, nbsup, v, x[v]);
        if (s > -INFINITY) {
          sa += expf(s - mall);
          if (v >= st.ts_begin) sts += expf(s - ms);
        }
      }
    }
  }
  sa = wg_sum<SPLIT_T>(sa, shf);
  sts = wg_sum<SPLIT_T>(sts, shf);
  vals[0] = mt; vals[1] = __int_as_float(it); vals[2] = ms; vals[3] = __int_as_float(is);
  vals[4] = mall; vals[5] = sa; vals[6] = sts;
}

// One thread: publish the slice's N values write-through (ahead of the arrival count that follows)
template <int N>
__device__ __forceinline__ void split_publish(float* part, const float (&vals)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) __hip_atomic_store(part + i, vals[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One thread, its workgroup's values published: wait for those stores, count the workgroup in, and say whether it
// is the last of the n that count on cnt
__device__ __forceinline__ bool arrive_last(int* cnt, int n) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n - 1;
}

// The mass rule's decision (logits_process.py:2040-2045) from a row's merged statistics: bt / Mts the text / timestamp
// maximum, M the row's, S = sum exp(s - M) over the row and Sts = sum exp(s - Mts) over its timestamps (M > -inf)
__device__ __forceinline__ int mass_rule_ban(float bt, float Mts, float M, float S, float Sts) {
  const float lse = logf(S);
  const float lp_text_max = (bt - M) - lse;
  const float lp_ts_max = (Mts - M) - lse;
  const float ts_lse = lp_ts_max > -INFINITY ? lp_ts_max + logf(Sts) : -INFINITY;
  return ts_lse > lp_text_max;
}

// One thread of the row's last arriver: the row's token from its NSPLIT published slices (row = the row's first
// slice), in slice order = index order -- the mass rule with timestamps, then the first index among equal maxima,
// text before timestamps.  0x7fffffff when every score is -inf.
__device__ __forceinline__ int split_merge_token(const float* row, int rt) {
  float P[NSPLIT][7];
#pragma unroll
  for (int q = 0; q < NSPLIT; ++q)  // every partial load in flight before the merge
#pragma unroll
    for (int i = 0; i < 7; ++i) P[q][i] = __hip_atomic_load(row + PART * q + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  float bt = -INFINITY, bs = -INFINITY, M = -INFINITY;
  int jt = 0x7fffffff, js = 0x7fffffff;
  for (int q = 0; q < NSPLIT; ++q) {
    const int qt = __float_as_int(P[q][1]), qs = __float_as_int(P[q][3]);
    if (P[q][0] > bt || (P[q][0] == bt && qt < jt)) { bt = P[q][0]; jt = qt; }
    if (P[q][2] > bs || (P[q][2] == bs && qs < js)) { bs = P[q][2]; js = qs; }
    M = fmaxf(M, P[q][4]);
  }
  const float Mts = bs;
  int ban = 0;
  if (rt && M > -INFINITY) {
    float S = 0.f, Sts = 0.f;
    for (int q = 0; q < NSPLIT; ++q) {
      if (P[q][4] > -INFINITY) S += P[q][5] * expf(P[q][4] - M);
      if (P[q][2] > -INFINITY) Sts += P[q][6] * expf(P[q][2] - Mts);
    }
    ban = mass_rule_ban(bt, Mts, M, S, Sts);
  }
  if (ban) return js;
  return (bs > bt) ? js : jt;  // a tie keeps the text token (the lower index)
}

// One thread, row b's token ii known (0x7fffffff: every score -inf, torch.argmax -> 0): the token or, on a finished
// row, pad into ids[b][L]; the row's unfinished flag (EOS / MaxLength, stopping_criteria.py:75-77); and the last of
// the B rows to arrive closes the step -- n_unfinished, the counter back to zero, cur_len advanced.
template <typename A>
__device__ __forceinline__ void finish_row(const A& a, int b, int L, int fin, int ii) {
  if (ii == 0x7fffffff) ii = 0;
  const int64_t tok = fin ? (int64_t)a.pad_id : (int64_t)ii;
  a.ids[(int64_t)b * a.ids_stride + L] = tok;
  const int done = fin || tok == a.eos_id || (L + 1) >= a.max_length;
  a.unfinished[b] = done ? 0 : 1;
  __threadfence();
  const int prev = atomicAdd(a.counter, 1);
  if (prev == (int)a.B - 1) {
    __threadfence();
    int n = 0;
    for (int i = 0; i < (int)a.B; ++i) n += __hip_atomic_load(a.unfinished + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *a.n_unfinished = n;
    *a.counter = 0;
    *a.cur_len = L + 1;
    __threadfence();
  }
}

}  // namespace kwp
