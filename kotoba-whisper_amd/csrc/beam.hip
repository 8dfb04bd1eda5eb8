// Beam search step on device (a10): GenerationMixin._beam_search (TF/generation/utils.py:3208-3527)
// for one decode step, captured in the same hipGraph as the decoder forward.
//
//  kw_beam_logprobs (one 1024-thread workgroup per running row = batch item x beam):
//    log_softmax of the raw f32 logits (:3380), the Whisper processors on the log-probs (Suppress ->
//    SuppressAtBegin -> WhisperTimeStamp, processors.h; :3381), and the row's K best processed
//    log-probs (K = 2 * num_beams: the global top-K over beams x vocab of log-prob + beam score is
//    inside the union of the rows' top-K, adding a per-row constant keeps a row's order -- up to the f32
//    ties a score makes of different log-probs, the one exception include/kwhisper.h states).
//  kw_beam_select (one workgroup per batch item):
//    _get_top_k_continuations (:3077), the MaxLength / EOS stopping criteria on the K continuations,
//    _get_running_beams_for_next_iteration (:3131), _update_finished_beams (:3153, length penalty,
//    early_stopping), the cache reorder (:3445-3456) and _check_early_stop_heuristic (:3008) /
//    _beam_search_has_unfinished_sequences (:3055).  The reorder moves no K/V: every running row
//    keeps a slot table bp[row][pos] = the cache row that holds its position pos (a beam's history
//    is its parent's table + its own new slot), so a reorder rewrites nb x L int32 per item
//    instead of gathering nb x layers x heads x L x 64 K/V values.
// All arithmetic is fp32 in the reference's order (log-prob + score, -1e9 masks, score /
// len**length_penalty); every top-k breaks ties by the lower flat index.
#include <math.h>
#include <stdio.h>

#include "processors.h"
#include "seqbias.h"

namespace {

using namespace kwp;

constexpr int KMAX = 16;  // candidates per row (2 * num_beams <= 16)
constexpr float NEG = -1.0e9f;

__device__ __forceinline__ bool better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// (score, token) as one 64-bit key ordered like better(): monotonic float bits above, ~token below.
// -0 is folded into +0 first (better() compares values).  Key 0 = no candidate.
__device__ __forceinline__ uint64_t bkey(float s, int v) {
  uint32_t b = __float_as_uint(s + 0.0f);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)b << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)v);
}
__device__ __forceinline__ float bkey_val(uint64_t k) {
  const uint32_t b = (uint32_t)(k >> 32);
  return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}
__device__ __forceinline__ int bkey_idx(uint64_t k) { return (int)(0xFFFFFFFFu - (uint32_t)k); }
// insert k into the descending triple (c0, c1, c2)
__device__ __forceinline__ void bins3(uint64_t k, uint64_t& c0, uint64_t& c1, uint64_t& c2) {
  const uint64_t h0 = k > c0 ? k : c0, l0 = k > c0 ? c0 : k;
  const uint64_t h1 = l0 > c1 ? l0 : c1, l1 = l0 > c1 ? c1 : l0;
  c0 = h0;
  c1 = h1;
  c2 = l1 > c2 ? l1 : c2;
}
// wave maximum of 64-bit keys on the VALU: DPP within 16-lane rows (quad_perm ^1 / ^2, then half-row and
// row mirrors once the quads / halves are uniform), v_permlane16/32_swap across rows -- no ds_bpermute round
// trips (a maximum is exact, so any reduction tree gives the butterfly's result)
template <int CTRL>
__device__ __forceinline__ uint64_t u64_max_dpp(uint64_t k) {
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(k >> 32), CTRL, 0xF, 0xF, false);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, 0xF, 0xF, false);
  const uint64_t o = ((uint64_t)hi << 32) | lo;
  return o > k ? o : k;
}
__device__ __forceinline__ uint64_t u64_max_swap16(uint64_t k) {
  const auto h = __builtin_amdgcn_permlane16_swap((uint32_t)(k >> 32), (uint32_t)(k >> 32), false, false);
  const auto l = __builtin_amdgcn_permlane16_swap((uint32_t)k, (uint32_t)k, false, false);
  const uint64_t a = ((uint64_t)h[0] << 32) | l[0], b = ((uint64_t)h[1] << 32) | l[1];
  return a > b ? a : b;
}
__device__ __forceinline__ uint64_t u64_max_swap32(uint64_t k) {
  const auto h = __builtin_amdgcn_permlane32_swap((uint32_t)(k >> 32), (uint32_t)(k >> 32), false, false);
  const auto l = __builtin_amdgcn_permlane32_swap((uint32_t)k, (uint32_t)k, false, false);
  const uint64_t a = ((uint64_t)h[0] << 32) | l[0], b = ((uint64_t)h[1] << 32) | l[1];
  return a > b ? a : b;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t k) {
  k = u64_max_dpp<0xB1>(k);   // quad_perm [1,0,3,2]
  k = u64_max_dpp<0x4E>(k);   // quad_perm [2,3,0,1]
  k = u64_max_dpp<0x141>(k);  // row_half_mirror
  k = u64_max_dpp<0x140>(k);  // row_mirror
  return u64_max_swap32(u64_max_swap16(k));
}

// The wave's best key, exactly wave_max_u64(k), at about a third of its VALU: a 32-bit maximum of the keys'
// value words (one v_max_u32 per DPP / swap step instead of a 64-bit compare and two selects), a ballot of the
// lanes that hold it, and the holder's key by readlane; only a tie on the value (several lanes, one value)
// falls back to the 64-bit maximum over those lanes (the lowest token among them).  Value words are never 0
// for a key (bkey's monotonic bits of any non-NaN score are >= 0x007FFFFF); key 0 = no candidate.
template <int CTRL>
__device__ __forceinline__ uint32_t u32_max_dpp(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
  return o > v ? o : v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = u32_max_dpp<0xB1>(v);
  v = u32_max_dpp<0x4E>(v);
  v = u32_max_dpp<0x141>(v);
  v = u32_max_dpp<0x140>(v);
  const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = a[0] > a[1] ? a[0] : a[1];
  const auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return b[0] > b[1] ? b[0] : b[1];
}
__device__ __forceinline__ uint64_t wave_best_key(uint64_t k) {
  const uint32_t hi = (uint32_t)(k >> 32);
  const uint32_t gh = wave_max_u32(hi);
  const uint64_t hit = __ballot(hi == gh && gh != 0);
  if (hit == 0) return 0;
  if (hit & (hit - 1)) return wave_max_u64(hi == gh ? k : 0);
  const int w = __builtin_ctzll(hit);
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, w) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, w);
}

// ---- repetition_penalty / no_repeat_ngram_size on the log-probs (kw_beam_logprobs_rep; the REP instantiations).
// RepetitionPenaltyLogitsProcessor then NoRepeatNGramLogitsProcessor (TF/generation/logits_process.py:406-413,
// 1121-1139) lead the processor list (TF/generation/utils.py:1174-1183) and see log_softmax(logits) in beam search
// (:3380-3381), with no renormalisation after them.  Each workgroup turns its row's history ids[0 .. L) into two
// vocabulary bitsets in LDS -- "occurs in the history" and "banned by an n-gram" -- and every log-prob the kernel
// forms goes through rep_apply before the Whisper processors and the timestamp mass rule see it.
constexpr int REP_VMAX = 65536, REP_WORDS = REP_VMAX / 32;

template <int NT>
__device__ __forceinline__ void rep_bitsets(uint32_t* hist, uint32_t* ban, const int64_t* __restrict__ ids, int L, int V,
                                            float penalty, int ngram) {
  const int tid = threadIdx.x;
  const int nw = (V + 31) >> 5;
  for (int i = tid; i < nw; i += NT) {
    hist[i] = 0;
    ban[i] = 0;
  }
  __syncthreads();
  if (penalty != 1.0f) {
    for (int p = tid; p < L; p += NT) {
      const int64_t t = ids[p];
      if (t >= 0 && t < V) atomicOr(&hist[t >> 5], 1u << (t & 31));
    }
  }
  if (ngram > 0 && L >= ngram) {
    const int64_t* tail = ids + (L - (ngram - 1));  // the history's last n-1 tokens
    for (int i = tid; i + ngram <= L; i += NT) {
      bool same = true;
      for (int j = 0; j < ngram - 1 && same; ++j) same = ids[i + j] == tail[j];
      if (!same) continue;
      const int64_t t = ids[i + ngram - 1];
      if (t >= 0 && t < V) atomicOr(&ban[t >> 5], 1u << (t & 31));
    }
  }
  __syncthreads();
}
// (f32, a true division, from the element's own log-prob; a banned token ends as -inf whatever the penalty gave)
__device__ __forceinline__ float rep_apply(const uint32_t* hist, const uint32_t* ban, float penalty, int v, float y) {
  if ((hist[v >> 5] >> (v & 31)) & 1u) y = y < 0.f ? y * penalty : y / penalty;
  if ((ban[v >> 5] >> (v & 31)) & 1u) y = -INFINITY;
  return y;
}

// ---- sequence_bias / bad_words_ids on the log-probs (kw_beam_logprobs_proc; the MODE 2 instantiations).
// SequenceBiasLogitsProcessor runs just ahead of the repetition pair, NoBadWordsLogitsProcessor just behind it
// (TF/generation/utils.py:1154-1155, 1207-1213).  Each workgroup walks both tables once against its row's history
// (seqbias.h): a sequence_bias group with an applying entry leaves its f32 sum in sb_sum[group] and its token's bit in
// sb_bits; a bad_words_ids group with an applying entry sets its token's bit in the n-gram ban bitset (-inf whatever
// came before).  Groups are in ascending token order, so an element whose bit is set finds its group by bisection --
// a handful of elements per row.
template <int NT>
__device__ __forceinline__ void seq_tables(uint32_t* sb_bits, float* sb_sum, uint32_t* ban, const kw_seq_bias_table& sb,
                                           const kw_seq_bias_table& bw, const int64_t* __restrict__ ids, int L, int V) {
  const int tid = threadIdx.x;
  const int nw = (V + 31) >> 5;
  for (int i = tid; i < nw; i += NT) sb_bits[i] = 0;
  __syncthreads();
  for (int g = tid; g < sb.n_groups; g += NT) {
    const int v = sb.group_tok[g];
    if (v < 0 || v >= V) continue;
    bool hit;
    const float b = kwsb::group_bias(sb, g, ids, L, &hit);
    if (!hit) continue;
    sb_sum[g] = b;
    atomicOr(&sb_bits[v >> 5], 1u << (v & 31));
  }
  for (int g = tid; g < bw.n_groups; g += NT) {
    const int v = bw.group_tok[g];
    if (v < 0 || v >= V) continue;
    bool hit;
    kwsb::group_bias(bw, g, ids, L, &hit);
    if (hit) atomicOr(&ban[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
}
// (y + bias, f32, ahead of rep_apply)
__device__ __forceinline__ float seq_bias_apply(const uint32_t* sb_bits, const float* sb_sum, const kw_seq_bias_table& sb,
                                                int v, float y) {
  if (!((sb_bits[v >> 5] >> (v & 31)) & 1u)) return y;
  int lo = 0, hi = sb.n_groups - 1;  // the bit says v is one of group_tok[0 .. n_groups)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sb.group_tok[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return y + sb_sum[lo];
}

// MODE 0: the plain kernels; 1: REP (kw_beam_logprobs_rep); 2: REP between the two sequence tables (.._proc)
template <int MODE>
__device__ __forceinline__ void beam_logprobs_body(const kw_beam_logprobs_args& a, float penalty, int ngram,
                                                   const kw_seq_bias_table* sb, const kw_seq_bias_table* bw) {
  constexpr bool REP = MODE >= 1, PROC = MODE == 2;
  __shared__ uint32_t rep_hist[REP ? REP_WORDS : 1], rep_ban[REP ? REP_WORDS : 1];
  __shared__ uint32_t sb_bits[PROC ? REP_WORDS : 1];
  __shared__ float sb_sum[PROC ? KW_SEQ_BIAS_MAX_SEQS : 1];
  __shared__ float shf[ST / 64];
  __shared__ int shi[ST / 64];
  __shared__ RowState st_sh;
  if (*a.done) return;
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int L = *a.cur_len;
  const int V = (int)a.V;
  const int K = a.k;
  const float* x = a.logits + (int64_t)r * a.V;
  const int64_t* ids = a.ids + (int64_t)r * a.ids_stride;

  // log_softmax normaliser of the raw row: lp = (x - max) - log(sum exp(x - max))
  float m = -INFINITY;
#pragma unroll 8
  for (int v = tid; v < V; v += ST) m = fmaxf(m, x[v]);
  m = wg_max<ST>(m, shf);
  float s = 0.f;
#pragma unroll 8
  for (int v = tid; v < V; v += ST) s += expf(x[v] - m);
  s = wg_sum<ST>(s, shf);
  const float ls = logf(s);
  if constexpr (REP) rep_bitsets<ST>(rep_hist, rep_ban, ids, L, V, penalty, ngram);
  if constexpr (PROC) seq_tables<ST>(sb_bits, sb_sum, rep_ban, *sb, *bw, ids, L, V);
  auto lp = [&](int v) {
    float y = (x[v] - m) - ls;
    if constexpr (PROC) y = seq_bias_apply(sb_bits, sb_sum, *sb, v, y);
    if constexpr (REP) return rep_apply(rep_hist, rep_ban, penalty, v, y);
    return y;
  };

  RowState st = history_row_state<ST>(a, ids, L, a.return_timestamps, nullptr, shi, &st_sh);
  if (st.rt) timestamp_rule(st, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, V, lp, shf);

  // per-thread sorted top-K of its strided slice as 64-bit (score, token) keys ordered like better() -- a -inf
  // score is a key too, so a row with fewer than K finite scores goes on with its lowest -inf tokens, as the
  // reference's top-k does -- then K rounds of a block maximum over the heads
  uint64_t tk[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) tk[i] = 0;
  for (int v = tid; v < V; v += ST) {
    uint64_t c = bkey(process(st, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, v, lp(v)), v);
    if (c <= tk[KMAX - 1]) continue;  // (keeps KMAX >= K per thread)
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
      if (c > tk[i]) {
        const uint64_t t1 = tk[i];
        tk[i] = c;
        c = t1;
      }
    }
  }
  __shared__ uint64_t wk[ST / 64];
  __shared__ uint64_t win_k;
  int head = 0;
  for (int k = 0; k < K; ++k) {
    uint64_t hk = 0;
#pragma unroll
    for (int i = 0; i < KMAX; ++i)
      if (i == head) hk = tk[i];
    const uint64_t wg = wave_max_u64(hk);
    if ((tid & 63) == 0) wk[tid >> 6] = wg;
    __syncthreads();
    if (tid == 0) {
      uint64_t g = wk[0];
      for (int w = 1; w < ST / 64; ++w) g = wk[w] > g ? wk[w] : g;
      win_k = g;
      if (g == 0) {  // fewer than K tokens in the row
        a.cand_val[(int64_t)r * K + k] = -INFINITY;
        a.cand_idx[(int64_t)r * K + k] = 0;
      }
    }
    __syncthreads();
    const uint64_t g = win_k;
    if (g != 0 && hk == g) {  // token ids are unique: one thread holds the winner; it writes its own f32 value
      const int v = bkey_idx(g);
      a.cand_val[(int64_t)r * K + k] = process(st, a.suppress_mask, a.begin_suppress, a.n_begin_suppress, v, lp(v));
      a.cand_idx[(int64_t)r * K + k] = v;
      ++head;
    }
    __syncthreads();
  }
}

// (the kernels keep one symbol each: REP is a flag of the shared body, the plain launch's code is as it was)
__global__ __launch_bounds__(ST) void beam_logprobs_kernel(kw_beam_logprobs_args a) {
  beam_logprobs_body<0>(a, 1.0f, 0, nullptr, nullptr);
}
__global__ __launch_bounds__(ST) void beam_lp_rep_kernel(kw_beam_logprobs_args a, float penalty, int ngram) {
  beam_logprobs_body<1>(a, penalty, ngram, nullptr, nullptr);
}
__global__ __launch_bounds__(ST) void beam_lp_proc_kernel(kw_beam_logprobs_args a, float penalty, int ngram,
                                                          kw_seq_bias_table sb, kw_seq_bias_table bw) {
  beam_logprobs_body<2>(a, penalty, ngram, &sb, &bw);
}

// ---- split-row variant: a row over NSPLIT workgroups (the one-workgroup kernel above walks a whole
// vocabulary row serially in several passes; at R = 160-320 running rows that is most of a step).
// Each slice keeps its logits in registers and publishes: the raw maximum and sum of exp (the
// log_softmax normaliser), WhisperTimeStamp's statistics of its processed scores (as the greedy
// split kernel), and its best KP processed scores overall and among timestamps (KP = k + 4 > k, so a
// log-prob tie that the raw order would split differently stays inside the candidates).  The row's
// last arriver merges the normaliser, applies the timestamp rule, turns candidates into log-probs
// lp = (x - m) - log(s) and keeps the k best by (lp desc, token asc).
constexpr int KP = KMAX + 4, BPART = 96;  // (NSPLIT, SPLIT_T, SUNR: processors.h)
constexpr int REP_NORM = BPART - 2;  // REP: the row's (max, log sum exp) in its first slice record
static_assert(9 + 4 * KP <= REP_NORM, "the slice record's published floats must leave the normaliser's two alone");

__device__ __forceinline__ void bl_argmax(float& best, int& bi, int& bt, float* shf, int* shi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64), ot = __shfl_xor(bt, o, 64);
    if (better(ob, oi, best, bi)) { best = ob; bi = oi; bt = ot; }
  }
  if ((threadIdx.x & 63) == 0) {
    shf[threadIdx.x >> 6] = best;
    shi[2 * (threadIdx.x >> 6)] = bi;
    shi[2 * (threadIdx.x >> 6) + 1] = bt;
  }
  __syncthreads();
  best = shf[0]; bi = shi[0]; bt = shi[1];
  for (int w = 1; w < SPLIT_T / 64; ++w)
    if (better(shf[w], shi[2 * w], best, bi)) { best = shf[w]; bi = shi[2 * w]; bt = shi[2 * w + 1]; }
  __syncthreads();
}

// REP: the processors act on log-probs and are not shift invariant, so a slice cannot stay in raw-logit space until
// the merge.  A launch of its own ahead of this one (beam_rep_norm_kernel, one workgroup per row) leaves the row's
// normaliser -- max and log(sum exp), the one-workgroup kernel's arithmetic -- in two spare floats of the row's first
// slice record (a record publishes at most 9 + 4 KP of its BPART floats, and the merge reads no more); every slice
// turns its logits into penalised / banned log-probs up front, and the merge takes the candidates' values as they
// are instead of normalising them.  (Each slice taking the normaliser itself, eight reads of every row, cost 77 us at
// R = 160, V = 51866 -- more than the whole plain launch.)
template <int MODE>
__device__ __forceinline__ void beam_logprobs_split_body(const kw_beam_logprobs_args& a, float penalty, int ngram,
                                                         const kw_seq_bias_table* sb, const kw_seq_bias_table* bw) {
  constexpr bool REP = MODE >= 1, PROC = MODE == 2;
  __shared__ uint32_t rep_hist[REP ? REP_WORDS : 1], rep_ban[REP ? REP_WORDS : 1];
  __shared__ uint32_t sb_bits[PROC ? REP_WORDS : 1];
  __shared__ float sb_sum[PROC ? KW_SEQ_BIAS_MAX_SEQS : 1];
  __shared__ RowState st_sh;
  __shared__ float pub[BPART];
  if (*a.done) return;
  const int r = blockIdx.x, sl = blockIdx.y;
  const int tid = threadIdx.x;
  const int L = *a.cur_len;
  const int V = (int)a.V;
  const int K = a.k;
  const float* x = a.logits + (int64_t)r * a.V;
  const int64_t* ids = a.ids + (int64_t)r * a.ids_stride;
  const int per = (V + NSPLIT - 1) / NSPLIT;
  const int v0 = sl * per, v1 = min(V, v0 + per);
  float xv[SUNR];
  bool mk[SUNR];
  // (kwp::split_load, spelled out: the call moved this kernel's schedule and measured +0.3 us on 31.6 us at R = 40)
#pragma unroll
  for (int u = 0; u < SUNR; ++u) {
    const int v = v0 + tid + u * SPLIT_T, vc = min(v, v1 - 1);  // unconditional (clamped) loads: no branches
    const float xr = x[vc];                                           // and phis between them
    const uint8_t mr = a.suppress_mask[vc];
    xv[u] = v < v1 ? xr : -INFINITY;
    mk[u] = v < v1 ? mr != 0 : true;
  }
  if constexpr (REP) {
    const float* nrm = reinterpret_cast<const float*>(a.workspace) + (int64_t)r * NSPLIT * BPART + REP_NORM;
    const float m = nrm[0], ls = nrm[1];  // (beam_rep_norm_kernel, the launch before this one)
    rep_bitsets<SPLIT_T>(rep_hist, rep_ban, ids, L, V, penalty, ngram);
    if constexpr (PROC) seq_tables<SPLIT_T>(sb_bits, sb_sum, rep_ban, *sb, *bw, ids, L, V);
#pragma unroll
    for (int u = 0; u < SUNR; ++u) {
      const int v = v0 + tid + u * SPLIT_T;
      if (v < v1) {
        float y = (xv[u] - m) - ls;
        if constexpr (PROC) y = seq_bias_apply(sb_bits, sb_sum, *sb, v, y);
        xv[u] = rep_apply(rep_hist, rep_ban, penalty, v, y);
      }
    }
  }
  // row state from the history (kwp::history_row_state's, with no dependent load): the last timestamp position
  // travels with its token in one 64-bit key, the last two tokens are read up front
  const int n_hist = L - a.begin_index;
  const int64_t tok_l1 = n_hist >= 1 ? ids[L - 1] : 0, tok_l2 = n_hist >= 2 ? ids[L - 2] : 0;
  uint64_t lkey = 0;  // ((position + 1) << 32) | token of the row's last timestamp
  for (int p = a.begin_index + tid; p < L; p += SPLIT_T) {
    const int64_t t = ids[p];
    if (t >= a.ts_begin) lkey = ((uint64_t)(uint32_t)(p + 1) << 32) | (uint32_t)t;
  }
  lkey = wave_max_u64(lkey);
  __shared__ uint64_t lkeys[SPLIT_T / 64];
  if ((tid & 63) == 0) lkeys[tid >> 6] = lkey;
  __syncthreads();
  if (tid == 0) {
    uint64_t lk = lkeys[0];
    for (int i = 1; i < SPLIT_T / 64; ++i) lk = lkeys[i] > lk ? lkeys[i] : lk;
    st_sh = make_row_state(a, L, a.return_timestamps, tok_l1, tok_l2, (int)(lk >> 32) - 1, (int)(uint32_t)lk);
  }
  __syncthreads();
  const RowState st = st_sh;
  // processed scores (raw-logit space; every processor is shift invariant) and their statistics
  float sv[SUNR];
  float mr = -INFINITY, mt = -INFINITY, ms = -INFINITY;
  int it = 0x7fffffff, is = 0x7fffffff;
#pragma unroll
  for (int u = 0; u < SUNR; ++u) {
    const int v = v0 + tid + u * SPLIT_T;
    mr = fmaxf(mr, xv[u]);
    sv[u] = v < v1 ? process_m(st, mk[u], a.begin_suppress, a.n_begin_suppress, v, xv[u]) : -INFINITY;
    if (v < v1) {
      if (v < st.ts_begin) {
        if (better(sv[u], v, mt, it)) { mt = sv[u]; it = v; }
      } else if (better(sv[u], v, ms, is)) { ms = sv[u]; is = v; }
    }
  }
  // one workgroup round for the three maxima (the raw maximum of the log_softmax normaliser; the best
  // text and timestamp scores as 64-bit keys), one for the three sums
  __shared__ float rmx[SPLIT_T / 64];
  __shared__ uint64_t rkt[SPLIT_T / 64], rks[SPLIT_T / 64];
  __shared__ float rsum[3][SPLIT_T / 64];
  {
    mr = wave_max(mr);
    uint64_t kt = 0, ks = 0;
    if (st.rt) {
      kt = wave_max_u64(bkey(mt, it));
      ks = wave_max_u64(bkey(ms, is));
    }
    if ((tid & 63) == 0) { rmx[tid >> 6] = mr; rkt[tid >> 6] = kt; rks[tid >> 6] = ks; }
    __syncthreads();
    mr = rmx[0];
    kt = rkt[0];
    ks = rks[0];
    for (int w = 1; w < SPLIT_T / 64; ++w) {
      mr = fmaxf(mr, rmx[w]);
      kt = rkt[w] > kt ? rkt[w] : kt;
      ks = rks[w] > ks ? rks[w] : ks;
    }
    if (st.rt) {
      mt = bkey_val(kt); it = bkey_idx(kt);
      ms = bkey_val(ks); is = bkey_idx(ks);
    }
  }
  float sr = 0.f, sa = 0.f, sts = 0.f, mall = -INFINITY;
  if (st.rt) mall = fmaxf(mt, ms);
#pragma unroll
  for (int u = 0; u < SUNR; ++u) {
    const int v = v0 + tid + u * SPLIT_T;
    if (v < v1) {
      sr += expf(xv[u] - mr);
      if (mall > -INFINITY && sv[u] > -INFINITY) {
        sa += expf(sv[u] - mall);
        if (v >= st.ts_begin) sts += expf(sv[u] - ms);
      }
    }
  }
  {
    sr = wave_sum(sr);
    sa = wave_sum(sa);
    sts = wave_sum(sts);
    if ((tid & 63) == 0) { rsum[0][tid >> 6] = sr; rsum[1][tid >> 6] = sa; rsum[2][tid >> 6] = sts; }
    __syncthreads();
    sr = sa = sts = 0.f;
    for (int w = 0; w < SPLIT_T / 64; ++w) {
      sr += rsum[0][w];
      sa += rsum[1][w];
      sts += rsum[2][w];
    }
  }
  // the slice's KP best processed scores (all tokens; and timestamps only, for the text-ban case):
  // each wave takes its own kp best by shuffle-only rounds (no workgroup barrier per round), then wave 0
  // takes the slice's kp best of the waves' 8 x kp
  const int kp = min(K + 4, KP);
  const int lane = tid & 63, wv = tid >> 6;
  __shared__ uint64_t wck[2][SPLIT_T / 64][KP];
  // timestamp tokens sit at the top of the vocabulary: only the slices holding some need the second list
  const int nlist = (st.rt && v1 > st.ts_begin) ? 2 : 1;
  for (int list = 0; list < nlist; ++list) {
    // each lane keeps its 3 best keys below ``floor`` (the last key it gave up), refilled from its 16
    // registers in the rare round that empties it; a round is one wave max of the lanes' heads
    uint64_t c0 = 0, c1 = 0, c2 = 0, floor = ~0ull;
    auto fill = [&]() {
      c0 = c1 = c2 = 0;
#pragma unroll
      for (int u = 0; u < SUNR; ++u) {
        const int v = v0 + tid + u * SPLIT_T;
        const uint64_t k = (v < v1 && (list == 0 || v >= st.ts_begin)) ? bkey(sv[u], v) : 0;
        if (k < floor) bins3(k, c0, c1, c2);
      }
    };
    fill();
    for (int j = 0; j < kp; ++j) {
      const uint64_t g = wave_best_key(c0);
      if (lane == 0) wck[list][wv][j] = g;
      bool need = false;
      if (g != 0 && c0 == g) {
        floor = g;
        c0 = c1; c1 = c2; c2 = 0;
        need = c0 == 0;
      }
      if (__ballot(need)) {
        if (need) fill();
      }
    }
  }
  __syncthreads();
  if (wv == 0) {
    for (int list = 0; list < 2; ++list) {
      if (list >= nlist) {  // (no timestamp tokens in this slice: an empty list)
        if (lane < kp) {
          pub[9 + list * 2 * KP + 2 * lane] = -INFINITY;
          pub[9 + list * 2 * KP + 2 * lane + 1] = __int_as_float(0x7fffffff);
        }
        continue;
      }
      // the waves' 8 x kp keys (kp <= KP: at most 3 per lane), then kp rounds of a wave max
      uint64_t c0 = 0, c1 = 0, c2 = 0;
      const int n = (SPLIT_T / 64) * kp;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int e = lane + 64 * t;
        if (e < n) bins3(wck[list][e / kp][e % kp], c0, c1, c2);
      }
      for (int j = 0; j < kp; ++j) {
        const uint64_t g = wave_best_key(c0);
        if (g != 0 && c0 == g) { c0 = c1; c1 = c2; c2 = 0; }
        if (lane == 0) {
          pub[9 + list * 2 * KP + 2 * j] = g ? bkey_val(g) : -INFINITY;
          pub[9 + list * 2 * KP + 2 * j + 1] = __int_as_float(g ? bkey_idx(g) : 0x7fffffff);
        }
      }
    }
  }
  if (tid == 0) {
    pub[0] = mr; pub[1] = sr; pub[2] = mt; pub[3] = __int_as_float(it); pub[4] = ms;
    pub[5] = __int_as_float(is); pub[6] = mall; pub[7] = sa; pub[8] = sts;
  }
  __syncthreads();
  float* part = reinterpret_cast<float*>(a.workspace) + ((int64_t)r * NSPLIT + sl) * BPART;
  int* rcnt = reinterpret_cast<int*>(a.workspace) + (int64_t)a.R * NSPLIT * BPART + r;
  const int npub = 9 + (st.rt ? 4 : 2) * KP;
  if (tid < npub) __hip_atomic_store(part + tid, pub[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  __shared__ int last;
  if (tid == 0) {
    const int prev = __hip_atomic_fetch_add(rcnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == NSPLIT - 1;
    if (last) __hip_atomic_store(rcnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last) return;
  // the row's partials into LDS by the whole workgroup (one round trip), then one thread merges
  __shared__ float allp[NSPLIT * BPART];
  const float* row = reinterpret_cast<const float*>(a.workspace) + (int64_t)r * NSPLIT * BPART;
  for (int i = tid; i < NSPLIT * BPART; i += SPLIT_T)
    allp[i] = (i % BPART) < npub ? __hip_atomic_load(row + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
  __syncthreads();
  if (wv != 0) return;
  // wave 0 merges: every lane derives the row's normaliser and the text-ban decision from the NSPLIT
  // slice records (identical on all lanes), then k rounds of a wave arg-max pick the candidates
  auto ld = [&](int q, int i) { return allp[q * BPART + i]; };
  float m = -INFINITY;
  for (int q = 0; q < NSPLIT; ++q) m = fmaxf(m, ld(q, 0));
  float ssum = 0.f;
  for (int q = 0; q < NSPLIT; ++q) {
    const float mq = ld(q, 0);
    if (mq > -INFINITY) ssum += ld(q, 1) * expf(mq - m);
  }
  const float ls = logf(ssum);
  int ban = 0;
  if (st.rt) {
    float bt_ = -INFINITY, bs_ = -INFINITY, M = -INFINITY;
    int jt = 0x7fffffff, js = 0x7fffffff;
    for (int q = 0; q < NSPLIT; ++q) {
      if (better(ld(q, 2), __float_as_int(ld(q, 3)), bt_, jt)) { bt_ = ld(q, 2); jt = __float_as_int(ld(q, 3)); }
      if (better(ld(q, 4), __float_as_int(ld(q, 5)), bs_, js)) { bs_ = ld(q, 4); js = __float_as_int(ld(q, 5)); }
      M = fmaxf(M, ld(q, 6));
    }
    float S = 0.f, Sts = 0.f;
    for (int q = 0; q < NSPLIT; ++q) {
      if (ld(q, 6) > -INFINITY) S += ld(q, 7) * expf(ld(q, 6) - M);
      if (ld(q, 4) > -INFINITY) Sts += ld(q, 8) * expf(ld(q, 4) - bs_);
    }
    if (M > -INFINITY) ban = mass_rule_ban(bt_, bs_, M, S, Sts);
  }
  // candidates of the chosen list as log-probs, three per lane (NSPLIT x kp <= 192)
  const int base = 9 + (ban ? 2 * KP : 0);
  const int n = NSPLIT * kp;
  float c[3];
  int ci3[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int e = lane + 64 * t;
    c[t] = -INFINITY;
    ci3[t] = 0x7fffffff;
    if (e < n) {
      const int q = e / kp, j = e - q * kp;
      const float sval = ld(q, base + 2 * j);
      const int idx = __float_as_int(ld(q, base + 2 * j + 1));
      if (idx != 0x7fffffff) {
        if constexpr (REP) c[t] = sval;  // (a log-prob already, not renormalised)
        else c[t] = sval > -INFINITY ? (sval - m) - ls : -INFINITY;
        ci3[t] = idx;
      }
    }
  }
  // k rounds of a wave maximum over 64-bit (log-prob, token) keys ordered like better() (token indices are
  // unique, so exactly one lane holds the winner; it writes its own f32 value and retires the key)
  uint64_t kk[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) kk[t] = ci3[t] != 0x7fffffff ? bkey(c[t], ci3[t]) : 0;
  int nf = -1;  // the row's finite candidates, once the places have run past them
  for (int j = 0; j < K; ++j) {
    uint64_t b = kk[0] > kk[1] ? kk[0] : kk[1];
    b = b > kk[2] ? b : kk[2];
    const uint64_t g = wave_best_key(b);
    if (nf < 0 && (g == 0 || !(bkey_val(g) > -INFINITY))) nf = j;
    // a -inf place names the lowest token that is -inf (the reference's top-k).  Under the text ban those are
    // the text tokens, which the timestamp list does not hold: ts_begin places of them, then the list's own
    if (ban && nf >= 0 && j - nf < st.ts_begin) {
      if (lane == 0) {
        a.cand_val[(int64_t)r * K + j] = -INFINITY;
        a.cand_idx[(int64_t)r * K + j] = j - nf;
      }
      continue;
    }
    if (g == 0) {  // no candidate left (cannot happen with a sane config): as the reference's -inf / 0
      if (lane == 0) {
        a.cand_val[(int64_t)r * K + j] = -INFINITY;
        a.cand_idx[(int64_t)r * K + j] = 0;
      }
      continue;
    }
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if (kk[t] == g) {
        a.cand_val[(int64_t)r * K + j] = c[t];
        a.cand_idx[(int64_t)r * K + j] = ci3[t];
        kk[t] = 0;
      }
  }
}

__global__ __launch_bounds__(SPLIT_T) void beam_logprobs_split_kernel(kw_beam_logprobs_args a) {
  beam_logprobs_split_body<0>(a, 1.0f, 0, nullptr, nullptr);
}
__global__ __launch_bounds__(SPLIT_T) void beam_lp_rep_split_kernel(kw_beam_logprobs_args a, float penalty, int ngram) {
  beam_logprobs_split_body<1>(a, penalty, ngram, nullptr, nullptr);
}
__global__ __launch_bounds__(SPLIT_T) void beam_lp_proc_split_kernel(kw_beam_logprobs_args a, float penalty, int ngram,
                                                                     kw_seq_bias_table sb, kw_seq_bias_table bw) {
  beam_logprobs_split_body<2>(a, penalty, ngram, &sb, &bw);
}
// the row's log_softmax normaliser, as beam_logprobs_body takes it, for the launch above
__global__ __launch_bounds__(ST) void beam_rep_norm_kernel(kw_beam_logprobs_args a) {
  __shared__ float shf[ST / 64];
  if (*a.done) return;
  const int r = blockIdx.x, tid = threadIdx.x, V = (int)a.V;
  const float* x = a.logits + (int64_t)r * a.V;
  float m = -INFINITY;
#pragma unroll 8
  for (int v = tid; v < V; v += ST) m = fmaxf(m, x[v]);
  m = wg_max<ST>(m, shf);
  float s = 0.f;
#pragma unroll 8
  for (int v = tid; v < V; v += ST) s += expf(x[v] - m);
  s = wg_sum<ST>(s, shf);
  if (tid == 0) {
    float* nrm = reinterpret_cast<float*>(a.workspace) + (int64_t)r * NSPLIT * BPART + REP_NORM;
    nrm[0] = m;
    nrm[1] = logf(s);
  }
}

// K rounds of a block arg-max over n (value, key) pairs in LDS; writes the winners' positions in order.
__device__ void block_topk(const float* val, const int* key, int n, int k, int* out_pos, float* shf, int* shi) {
  const int tid = threadIdx.x;
  __shared__ int taken[256];
  for (int i = tid; i < n; i += blockDim.x) taken[i] = 0;
  __syncthreads();
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bk = 0x7fffffff, bp = -1;
    for (int i = tid; i < n; i += blockDim.x)
      if (!taken[i] && (bp < 0 || better(val[i], key[i], bv, bk))) {
        bv = val[i];
        bk = key[i];
        bp = i;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int ok = __shfl_xor(bk, o, 64), op = __shfl_xor(bp, o, 64);
      if (op >= 0 && (bp < 0 || better(ov, ok, bv, bk))) {
        bv = ov;
        bk = ok;
        bp = op;
      }
    }
    if ((tid & 63) == 0) {
      shf[tid >> 6] = bv;
      shi[2 * (tid >> 6)] = bk;
      shi[2 * (tid >> 6) + 1] = bp;
    }
    __syncthreads();
    if (tid == 0) {
      float gv = shf[0];
      int gk = shi[0], gp = shi[1];
      for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
        const int wp = shi[2 * w + 1];
        if (wp >= 0 && (gp < 0 || better(shf[w], shi[2 * w], gv, gk))) {
          gv = shf[w];
          gk = shi[2 * w];
          gp = wp;
        }
      }
      out_pos[j] = gp;
      taken[gp] = 1;
    }
    __syncthreads();
  }
}

constexpr int BT = 256;  // beam_select threads
constexpr int NBMAX = 8;
constexpr int TMAX = 512;  // history length bound (max_target_positions 448)

// PAR (kw_beam_select_parents): the step also records who produced what -- plog[L][r] = the running row that next
// running row r continues, fin_par[b][slot] = the running row a finished hypothesis was taken from (it moves with its
// slot as fin_score / fin_len / fin_flag do).  Everything else is the plain step, write for write.
template <bool PAR>
__device__ __forceinline__ void beam_select_body(const kw_beam_select_args& a, int32_t* __restrict__ plog,
                                                 int32_t* __restrict__ fin_par) {
  __shared__ float cval[256];
  __shared__ int ckey[256];
  __shared__ float shf[BT / 64];
  __shared__ int shi[2 * (BT / 64)];
  __shared__ int top[KMAX], run_pos[NBMAX], fin_pos[NBMAX];
  __shared__ float t_lp[KMAX], t_run[KMAX], t_fin[KMAX];
  __shared__ int t_par[KMAX], t_tok[KMAX], t_hit[KMAX];
  __shared__ float m_val[NBMAX + KMAX];
  __shared__ int m_key[NBMAX + KMAX];
  __shared__ float old_fs[NBMAX];
  __shared__ int old_fl[NBMAX], old_ff[NBMAX];
  __shared__ int old_fp[PAR ? NBMAX : 1];
  __shared__ int hist[NBMAX][TMAX];  // parents' token histories (ids < 2^31)
  __shared__ int bph[NBMAX][TMAX];   // parents' slot tables
  __shared__ int fst[NBMAX][TMAX];   // the item's finished rows before this step
  __shared__ int last;
  if (*a.done) return;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nb = a.num_beams, K = 2 * nb;
  const int L = *a.cur_len, P = a.begin_index;
  const int V = (int)a.V;
  const int r0 = b * nb;

  // 1. candidates: row j's K processed log-probs + its running score; key = flat index j*V + v
  const int n = nb * K;
  for (int i = tid; i < n; i += BT) {
    const int j = i / K;
    cval[i] = a.cand_val[(int64_t)(r0 + j) * K + (i - j * K)] + a.run_scores[r0 + j];
    ckey[i] = j * V + a.cand_idx[(int64_t)(r0 + j) * K + (i - j * K)];
  }
  for (int i = tid; i < nb; i += BT) {
    old_fs[i] = a.fin_score[(int64_t)b * nb + i];
    old_fl[i] = a.fin_len[(int64_t)b * nb + i];
    old_ff[i] = a.fin_flag[(int64_t)b * nb + i];
    if constexpr (PAR) old_fp[i] = fin_par[(int64_t)b * nb + i];
  }
  // parents' histories (positions < L) and slot tables, before anything is rewritten
  for (int i = tid; i < nb * L; i += BT) {
    const int j = i / L, p = i - j * L;
    hist[j][p] = (int)a.ids[(int64_t)(r0 + j) * a.ids_stride + p];
    if (a.bp) bph[j][p] = a.bp[(int64_t)(r0 + j) * a.bp_stride + p];
  }
  __syncthreads();
  // 2. top-K continuations (:3077-3129)
  block_topk(cval, ckey, n, K, top, shf, shi);
  const bool at_max = L + 1 >= a.max_length;
  if (tid < K) {
    const int i = top[tid];
    t_lp[tid] = cval[i];
    t_par[tid] = ckey[i] / V;
    t_tok[tid] = ckey[i] - (ckey[i] / V) * V;
    const int hit = at_max || t_tok[tid] == a.eos_id;  // MaxLength / EOS criteria on the new sequence
    t_hit[tid] = hit;
    t_run[tid] = t_lp[tid] + (hit ? 1.f : 0.f) * NEG;  // :3144
  }
  __syncthreads();
  // 3. running beams for the next step (:3131-3151): top nb of t_run, key = candidate rank
  if (tid < K) {
    cval[tid] = t_run[tid];
    ckey[tid] = tid;
  }
  __syncthreads();
  block_topk(cval, ckey, K, nb, run_pos, shf, shi);
  // 4. finished beams (:3153-3205)
  if (tid == 0) {
    int all_fin = 1;
    for (int j = 0; j < nb; ++j) all_fin &= old_ff[j] != 0;
    const float full = (all_fin && a.early_stopping == 1) ? 1.f : 0.f;
    const float unsat0 = a.unsat[b] ? 0.f : 1.f;  // (~unsat) as f32
    const float den = (float)pow((double)(L + 1 - P), (double)a.length_penalty);
    for (int c = 0; c < K; ++c) {
      const int did = t_hit[c] && c < nb;
      float tl = t_lp[c] / den;
      tl = tl + full * NEG;
      tl = tl + unsat0 * NEG;
      tl = tl + (did ? 0.f : 1.f) * NEG;
      t_fin[c] = tl;
    }
    for (int j = 0; j < nb; ++j) {
      m_val[j] = old_fs[j];
      m_key[j] = j;
    }
    for (int c = 0; c < K; ++c) {
      m_val[nb + c] = t_fin[c];
      m_key[nb + c] = nb + c;
    }
  }
  __syncthreads();
  block_topk(m_val, m_key, nb + K, nb, fin_pos, shf, shi);
  // 5. the new finished set: old entries come from the LDS copy, new ones are a candidate's parent
  //    history + its token, fill (pad) beyond -- as the reference's static-shape sequences
  //    (positions < max_length only: what a row holds beyond, up to fin_stride, is the caller's)
  const int Tf = (int)a.fin_stride, Tm = a.max_length;
  for (int i = tid; i < nb * Tm; i += BT) {
    const int j = i / Tm, p = i - j * Tm;
    fst[j][p] = (int)a.fin_seq[((int64_t)b * nb + j) * Tf + p];
  }
  __shared__ int fin_src[NBMAX];
  if (tid < nb) fin_src[tid] = fin_pos[tid];
  __syncthreads();
  for (int i = tid; i < nb * Tm; i += BT) {
    const int s = i / Tm, p = i - s * Tm;
    const int src = fin_src[s];
    int v;
    if (src < nb) {
      v = fst[src][p];
    } else {
      const int c = src - nb;
      v = p < L ? hist[t_par[c]][p] : (p == L ? t_tok[c] : a.fill_id);
    }
    a.fin_seq[((int64_t)b * nb + s) * Tf + p] = v;
  }
  if (tid < nb) {
    const int src = fin_src[tid];
    float fs;
    int fl, ff;
    if (src < nb) {
      fs = old_fs[src];
      fl = old_fl[src];
      ff = old_ff[src];
    } else {
      fs = t_fin[src - nb];
      fl = L + 1 - P;
      ff = t_hit[src - nb] && (src - nb) < nb;
    }
    a.fin_score[(int64_t)b * nb + tid] = fs;
    a.fin_len[(int64_t)b * nb + tid] = fl;
    a.fin_flag[(int64_t)b * nb + tid] = ff;
    if constexpr (PAR) fin_par[(int64_t)b * nb + tid] = src < nb ? old_fp[src] : r0 + t_par[src - nb];
  }
  // 6. running rows: parent history + new token, slot table of the parent + own slot at L
  for (int i = tid; i < nb * (L + 1); i += BT) {
    const int j = i / (L + 1), p = i - j * (L + 1);
    const int c = run_pos[j];
    a.ids[(int64_t)(r0 + j) * a.ids_stride + p] = p < L ? hist[t_par[c]][p] : (int64_t)t_tok[c];
    if (a.bp) a.bp[(int64_t)(r0 + j) * a.bp_stride + p] = p < L ? bph[t_par[c]][p] : r0 + j;
  }
  if (tid < nb) a.run_scores[r0 + tid] = t_run[run_pos[tid]];
  if constexpr (PAR) {
    if (tid < nb) plog[(int64_t)L * ((int64_t)a.B * nb) + r0 + tid] = r0 + t_par[run_pos[tid]];
  }
  __syncthreads();
  // 7. early-stop heuristic (:3008-3053) at cur_len + 1, and this item's loop-condition inputs
  if (tid == 0) {
    const int Ln = L + 1;
    const int bhl = (a.early_stopping == 2 && a.length_penalty > 0.f) ? (a.max_length - P) : (Ln - P);
    const float best_run = t_run[run_pos[0]] / (float)pow((double)bhl, (double)a.length_penalty);
    float worst = INFINITY;
    int all_fin = 1;
    for (int j = 0; j < nb; ++j) {
      worst = fminf(worst, a.fin_score[(int64_t)b * nb + j]);
      all_fin &= a.fin_flag[(int64_t)b * nb + j] != 0;
    }
    int any_better = 0;
    for (int j = 0; j < nb; ++j) {
      const float wf = a.fin_flag[(int64_t)b * nb + j] ? worst : NEG;
      any_better |= best_run > wf;
    }
    const int uns = a.unsat[b] && any_better;
    a.unsat[b] = uns;
    int all_hit = 1;
    for (int c = 0; c < K; ++c) all_hit &= t_hit[c];
    a.item_flags[3 * b] = uns;
    a.item_flags[3 * b + 1] = all_fin;
    a.item_flags[3 * b + 2] = all_hit;
    __threadfence();
    const int prev = atomicAdd(a.counter, 1);
    last = prev == (int)a.B - 1;
  }
  __syncthreads();
  // 8. the last item: _beam_search_has_unfinished_sequences over the batch, advance cur_len
  if (last && tid == 0) {
    __threadfence();
    int improve = 0, all_fin = 1, all_hit = 1;
    for (int i = 0; i < (int)a.B; ++i) {
      improve |= __hip_atomic_load(a.item_flags + 3 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      all_fin &= __hip_atomic_load(a.item_flags + 3 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      all_hit &= __hip_atomic_load(a.item_flags + 3 * i + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int open = !(all_fin && a.early_stopping == 1);
    const int go = improve && open && !all_hit;
    *a.go = go;
    if (!go) *a.done = 1;
    *a.counter = 0;
    *a.cur_len = L + 1;
    __threadfence();
  }
}

// (one symbol each, PAR a flag of the shared body: the plain launch's code is as it was)
__global__ __launch_bounds__(BT) void beam_select_kernel(kw_beam_select_args a) {
  beam_select_body<false>(a, nullptr, nullptr);
}
__global__ __launch_bounds__(BT) void beam_select_par_kernel(kw_beam_select_args a, int32_t* plog, int32_t* fin_par) {
  beam_select_body<true>(a, plog, fin_par);
}

bool beam_select_args_ok(const kw_beam_select_args* a) {
  return a && a->B > 0 && a->num_beams >= 2 && a->num_beams <= NBMAX && a->V > 0 && a->cand_val && a->cand_idx &&
         a->ids && a->run_scores && a->fin_seq && a->fin_score && a->fin_len && a->fin_flag && a->unsat && a->cur_len &&
         a->counter && a->go && a->done && a->item_flags && a->ids_stride >= a->max_length &&
         a->fin_stride >= a->max_length && a->max_length <= TMAX && (!a->bp || a->bp_stride >= a->max_length);
}

}  // namespace

extern "C" size_t kw_beam_logprobs_workspace(int64_t R) {
  return (size_t)R * NSPLIT * BPART * sizeof(float) + (size_t)R * sizeof(int);
}

extern "C" int kw_beam_logprobs(const kw_beam_logprobs_args* a, kw_stream_t stream) {
  if (!a || !a->logits || !a->suppress_mask || !a->ids || !a->cur_len || !a->cand_val || !a->cand_idx || !a->done ||
      a->R <= 0 || a->V <= 0 || a->k < 1 || a->k > KMAX || (a->n_begin_suppress > 0 && !a->begin_suppress))
    return kw_set_error_msg(KW_EINVAL, "kw_beam_logprobs: invalid arguments (k <= 16)");
  if (a->workspace && a->ws_bytes >= kw_beam_logprobs_workspace(a->R) && a->V <= (int64_t)NSPLIT * SPLIT_T * SUNR)
    hipLaunchKernelGGL(beam_logprobs_split_kernel, dim3((unsigned)a->R, NSPLIT), dim3(SPLIT_T), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(beam_logprobs_kernel, dim3((unsigned)a->R), dim3(ST), 0, (hipStream_t)stream, *a);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" int kw_beam_logprobs_rep(const kw_beam_logprobs_args* a, float penalty, int32_t ngram, kw_stream_t stream) {
  if (!a || !a->logits || !a->suppress_mask || !a->ids || !a->cur_len || !a->cand_val || !a->cand_idx || !a->done ||
      a->R <= 0 || a->V <= 0 || a->k < 1 || a->k > KMAX || (a->n_begin_suppress > 0 && !a->begin_suppress) ||
      !(penalty > 0.f) || !isfinite(penalty) || ngram < 0)
    return kw_set_error_msg(KW_EINVAL,
                            "kw_beam_logprobs_rep: invalid arguments (k <= 16, penalty > 0 and finite, ngram >= 0)");
  if (a->V > REP_VMAX) return kw_set_error_msg(KW_EUNSUPPORTED, "kw_beam_logprobs_rep: V > 65536");
  if (penalty == 1.0f && ngram == 0) return kw_beam_logprobs(a, stream);  // both off: that very launch
  if (a->workspace && a->ws_bytes >= kw_beam_logprobs_workspace(a->R) && a->V <= (int64_t)NSPLIT * SPLIT_T * SUNR) {
    hipLaunchKernelGGL(beam_rep_norm_kernel, dim3((unsigned)a->R), dim3(ST), 0, (hipStream_t)stream, *a);
    hipLaunchKernelGGL(beam_lp_rep_split_kernel, dim3((unsigned)a->R, NSPLIT), dim3(SPLIT_T), 0, (hipStream_t)stream, *a,
                       penalty, (int)ngram);
  } else {
    hipLaunchKernelGGL(beam_lp_rep_kernel, dim3((unsigned)a->R), dim3(ST), 0, (hipStream_t)stream, *a, penalty,
                       (int)ngram);
  }
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" int kw_beam_logprobs_proc(const kw_beam_logprobs_args* a, float penalty, int32_t ngram,
                                     const kw_seq_bias_table* bias, const kw_seq_bias_table* bad_words,
                                     kw_stream_t stream) {
  const char* why = "";
  int rc = kwsb::table_check(bias, &why);
  if (!rc) rc = kwsb::table_check(bad_words, &why);
  if (rc) {
    char msg[160];
    snprintf(msg, sizeof(msg), "kw_beam_logprobs_proc: %s", why);
    return kw_set_error_msg(rc, msg);
  }
  if (kwsb::table_empty(bias) && kwsb::table_empty(bad_words))
    return kw_beam_logprobs_rep(a, penalty, ngram, stream);  // no table: that very launch
  if (!a || !a->logits || !a->suppress_mask || !a->ids || !a->cur_len || !a->cand_val || !a->cand_idx || !a->done ||
      a->R <= 0 || a->V <= 0 || a->k < 1 || a->k > KMAX || (a->n_begin_suppress > 0 && !a->begin_suppress) ||
      !(penalty > 0.f) || !isfinite(penalty) || ngram < 0)
    return kw_set_error_msg(KW_EINVAL,
                            "kw_beam_logprobs_proc: invalid arguments (k <= 16, penalty > 0 and finite, ngram >= 0)");
  if (a->V > REP_VMAX) return kw_set_error_msg(KW_EUNSUPPORTED, "kw_beam_logprobs_proc: V > 65536");
  const kw_seq_bias_table none{};  // (n_groups 0: its arrays are never read)
  const kw_seq_bias_table sb = kwsb::table_empty(bias) ? none : *bias;
  const kw_seq_bias_table bw = kwsb::table_empty(bad_words) ? none : *bad_words;
  if (a->workspace && a->ws_bytes >= kw_beam_logprobs_workspace(a->R) && a->V <= (int64_t)NSPLIT * SPLIT_T * SUNR) {
    hipLaunchKernelGGL(beam_rep_norm_kernel, dim3((unsigned)a->R), dim3(ST), 0, (hipStream_t)stream, *a);
    hipLaunchKernelGGL(beam_lp_proc_split_kernel, dim3((unsigned)a->R, NSPLIT), dim3(SPLIT_T), 0, (hipStream_t)stream,
                       *a, penalty, (int)ngram, sb, bw);
  } else {
    hipLaunchKernelGGL(beam_lp_proc_kernel, dim3((unsigned)a->R), dim3(ST), 0, (hipStream_t)stream, *a, penalty,
                       (int)ngram, sb, bw);
  }
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" int kw_beam_select(const kw_beam_select_args* a, kw_stream_t stream) {
  if (!beam_select_args_ok(a))
    return kw_set_error_msg(KW_EINVAL, "kw_beam_select: invalid arguments (2 <= num_beams <= 8, max_length <= 512)");
  hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)a->B), dim3(BT), 0, (hipStream_t)stream, *a);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" int kw_beam_select_parents(const kw_beam_select_args* a, int32_t* parent_log, int32_t* fin_parent,
                                      kw_stream_t stream) {
  if (!beam_select_args_ok(a) || !parent_log || !fin_parent)
    return kw_set_error_msg(KW_EINVAL, "kw_beam_select_parents: invalid arguments (kw_beam_select's, and both "
                                       "parent outputs)");
  hipLaunchKernelGGL(beam_select_par_kernel, dim3((unsigned)a->B), dim3(BT), 0, (hipStream_t)stream, *a, parent_log,
                     fin_parent);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
