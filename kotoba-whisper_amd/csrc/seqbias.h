// One group of a kw_seq_bias_table against a row's history: the walk kw_seq_bias_process (seqbias.hip) and
// kw_beam_logprobs_proc (beam.hip) share.  SequenceBiasLogitsProcessor.__call__ (TF/generation/logits_process.py:
// 1288-1319): bias = 0; bias += length_1_bias (:1297); for every longer entry in the processor's order that fits the
// history (:1303) and whose first n-1 tokens equal the history's last n-1 (:1307-1310), bias[last token] += value
// (:1311-1315); scores + bias (:1318).  The table keeps a group's length-1 entry first and the others in that order,
// so the sum below is the reference's f32 sum (an entry that does not apply adds the reference's 0.0).
#pragma once
#include <stdint.h>

#include "kw_common.h"

namespace kwsb {

// The bias of group g's token for the history ids[0 .. L).  *hit: some entry applied (the sum is not the empty 0).
__device__ __forceinline__ float group_bias(const kw_seq_bias_table& t, int g, const int64_t* __restrict__ ids, int L,
                                            bool* hit) {
  float sum = 0.f;
  bool any = false;
  const int s0 = t.group_off[g], s1 = t.group_off[g + 1];
  for (int s = s0; s < s1; ++s) {
    const int o = t.seq_off[s], n = t.seq_off[s + 1] - o;
    if (n < 1 || n > L) continue;  // longer than the context: ignored (:1303)
    bool same = true;
    const int64_t* tail = ids + (L - (n - 1));  // the history's last n-1 tokens
    for (int j = 0; j < n - 1 && same; ++j) same = tail[j] == (int64_t)t.tokens[o + j];
    if (!same) continue;
    sum += t.values[s];
    any = true;
  }
  *hit = any;
  return sum;
}

inline bool table_empty(const kw_seq_bias_table* t) { return !t || t->n_seq == 0; }

// KW_OK, or the error a table's host-side fields earn (the arrays are device memory: their content is the caller's)
inline int table_check(const kw_seq_bias_table* t, const char** why) {
  if (!t || t->n_seq == 0) return KW_OK;
  if (t->n_seq < 0 || t->n_groups < 1 || t->n_groups > t->n_seq || t->max_len < 1 || !t->tokens || !t->seq_off ||
      !t->values || !t->group_off || !t->group_tok) {
    *why = "invalid sequence table (counts, NULL array)";
    return KW_EINVAL;
  }
  if (t->n_seq > KW_SEQ_BIAS_MAX_SEQS || t->max_len > KW_SEQ_BIAS_MAX_LEN) {
    *why = "sequence table beyond KW_SEQ_BIAS_MAX_SEQS entries / KW_SEQ_BIAS_MAX_LEN tokens";
    return KW_EUNSUPPORTED;
  }
  return KW_OK;
}

}  // namespace kwsb
