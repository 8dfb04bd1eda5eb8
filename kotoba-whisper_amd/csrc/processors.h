// Whisper logits processors on device, shared by the greedy (sampling.hip) and beam (beam.hip) steps.
// SuppressTokens (TF/generation/logits_process.py:1869-1906) -> SuppressTokensAtBegin (:1816-1866,
// when input_ids.shape[-1] == begin_index) -> WhisperTimeStamp (:1909-2047): the per-row state (last /
// penultimate token, last timestamp, first step) is re-derived from the row's own id history each step,
// exactly as the reference re-derives it from input_ids.
#pragma once
#include <math.h>

#include "kw_common.h"

namespace kwp {

constexpr int ST = 1024;

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

__device__ float block_reduce_max(float v, float* sh) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < ST / 64; ++i) r = fmaxf(r, sh[i]);
  __syncthreads();
  return r;
}

__device__ float block_reduce_sum(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < ST / 64; ++i) r += sh[i];
  __syncthreads();
  return r;
}


// Per-row processor state from the id history [begin, L) (one 1024-thread workgroup per row).
__device__ __forceinline__ RowState row_state(const int64_t* __restrict__ ids, int L, int begin, int ts_begin,
                                              int no_ts, int eos, int rt, int max_init, int* fin_out,
                                              int (*shi)[2], RowState* st_sh) {
  const int tid = threadIdx.x;
  int fin = 0, last_stamp_pos = -1;
  for (int p = begin + tid; p < L; p += ST) {
    const int64_t t = ids[p];
    if (t == eos) fin = 1;
    if (t >= ts_begin && p > last_stamp_pos) last_stamp_pos = p;
  }
  fin = __syncthreads_or(fin);
  {
    int v = last_stamp_pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    if ((tid & 63) == 0) shi[tid >> 6][0] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int lp = shi[0][0];
    for (int i = 1; i < ST / 64; ++i) lp = max(lp, shi[i][0]);
    RowState st;
    st.L = L; st.begin = begin; st.ts_begin = ts_begin; st.no_ts = no_ts; st.eos = eos;
    st.rt = rt; st.max_init = max_init; st.ban_text = 0;
    const int n = L - begin;
    st.first_step = (L == begin);
    st.last_ts = n >= 1 && ids[L - 1] >= ts_begin;
    st.pen_ts = n < 2 || ids[L - 2] >= ts_begin;
    st.has_stamp = lp >= 0;
    if (st.has_stamp) {
      const int last_stamp = (int)ids[lp];
      st.stamp_lo = (st.last_ts && !st.pen_ts) ? last_stamp : last_stamp + 1;
    } else {
      st.stamp_lo = 0;
    }
    *st_sh = st;
  }
  __syncthreads();
  *fin_out = fin;
  return *st_sh;
}

// WhisperTimeStamp's probability-mass rule (logits_process.py:2040-2045) on the processed scores
// s(v) = process(.., f(v)): ban text when logsumexp(logprobs[ts:]) > max(logprobs[:ts]).  Shift
// invariant, so f may be raw logits (greedy) or log-probs (beam).
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
  m_all = block_reduce_max(m_all, shf);
  m_text = block_reduce_max(m_text, shf);
  m_ts = block_reduce_max(m_ts, shf);
  float sum = 0.f;
#pragma unroll 8
  for (int v = tid; v < V; v += ST) {
    const float s = process(st, mask, bsup, nbsup, v, f(v));
    sum += expf(s - m_all);
  }
  sum = block_reduce_sum(sum, shf);
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
  tsum = block_reduce_sum(tsum, shf);
  const float ts_lse = lp_ts_max > -INFINITY ? lp_ts_max + logf(tsum) : -INFINITY;
  if (ts_lse > lp_text_max) st.ban_text = 1;
}

// ---- a row split over workgroups (kw_greedy_step with a workspace, kw_sample_step, kw_spec_accept) ----------------
// Row b's V scores are cut into NSPLIT slices of one SPLIT_T-thread workgroup each (SUNR loads in flight per thread);
// every slice publishes PART floats, and the row's last arriver merges them in slice order.  kw_spec_accept's tokens
// are held equal to kw_greedy_step's bit for bit, so the timestamp-mode slice statistics and their merge exist once,
// here, for both.
constexpr int SPLIT_T = 512, NSPLIT = 8, SUNR = 16, PART = 8;  // PART: floats published per slice

__device__ __forceinline__ float blk_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < SPLIT_T / 64; ++i) r = fmaxf(r, sh[i]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float blk_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < SPLIT_T / 64; ++i) r += sh[i];
  __syncthreads();
  return r;
}
__device__ __forceinline__ void blk_argmax(float& best, int& bi, float* shf, int* shi) {
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
  for (int i = 1; i < SPLIT_T / 64; ++i)
    if (shf[i] > best || (shf[i] == best && shi[i] < bi)) { best = shf[i]; bi = shi[i]; }
  __syncthreads();
}

// the slice's logits and SuppressTokens bytes, all in flight before anything waits on them
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

// the row state at length L, given lp = the position of the history's last timestamp (-1: none); one thread
__device__ __forceinline__ RowState split_row_state(const int64_t* __restrict__ ids, int L, int lp, int begin,
                                                    int ts_begin, int no_ts, int eos, int rt, int max_init) {
  RowState st;
  st.L = L; st.begin = begin; st.ts_begin = ts_begin; st.no_ts = no_ts; st.eos = eos;
  st.rt = rt; st.max_init = max_init; st.ban_text = 0;
  const int n = L - begin;
  st.first_step = (L == begin);
  st.last_ts = n >= 1 && ids[L - 1] >= ts_begin;
  st.pen_ts = n < 2 || ids[L - 2] >= ts_begin;
  st.has_stamp = lp >= 0;
  st.stamp_lo = st.has_stamp ? ((st.last_ts && !st.pen_ts) ? (int)ids[lp] : (int)ids[lp] + 1) : 0;
  return st;
}

// Over the slice's processed scores: the text maximum (+ first index), the timestamp maximum (+ first index), the
// slice maximum with the sum of exp(s - that maximum), and the timestamp sum of exp(s - timestamp maximum) -- the two
// sums only with timestamps (they feed the mass rule alone).  Every thread returns the same seven values.
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
  blk_argmax(mt, it, shf, shi);
  blk_argmax(ms, is, shf, shi);
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
  sa = blk_sum(sa, shf);
  sts = blk_sum(sts, shf);
  vals[0] = mt; vals[1] = __int_as_float(it); vals[2] = ms; vals[3] = __int_as_float(is);
  vals[4] = mall; vals[5] = sa; vals[6] = sts;
}

// One thread: publish the slice's seven values write-through (ahead of the arrival count that follows)
__device__ __forceinline__ void split_publish(float* part, const float (&vals)[7]) {
#pragma unroll
  for (int i = 0; i < 7; ++i) __hip_atomic_store(part + i, vals[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One thread of the row's last arriver: the row's token from its NSPLIT published slices (row = the row's first
// slice), in slice order = index order -- the mass rule (logits_process.py:2040-2045) with timestamps, then the first
// index among equal maxima, text before timestamps.  0x7fffffff when every score is -inf.
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
    const float lse = logf(S);
    const float lp_text_max = (bt - M) - lse;
    const float lp_ts_max = (Mts - M) - lse;
    const float ts_lse = lp_ts_max > -INFINITY ? lp_ts_max + logf(Sts) : -INFINITY;
    ban = ts_lse > lp_text_max;
  }
  if (ban) return js;
  return (bs > bt) ? js : jt;  // a tie keeps the text token (the lower index)
}

}  // namespace kwp
