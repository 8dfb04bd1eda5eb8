// GenerationMixin's SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor on device, for the greedy and sampled step
// tails (TF/generation/logits_process.py:1288-1319, 1450-1467): in place on the raw f32 logits [R][V].  sequence_bias
// runs ahead of kw_repeat_process, bad_words_ids (the same processor, every value -inf) behind it and ahead of the
// Whisper processors of kw_greedy_step / kw_sample_step (TF/generation/utils.py:1154-1155, 1174-1183, 1207-1213).
// The beam tail applies the same two to log-probs inside kw_beam_logprobs_proc (beam.hip).
//
// One workgroup per row, a thread per group of the table (the entries that end in one token; seqbias.h walks it): the
// thread sums its group's applying values in the reference's order and adds the sum to its token.  Groups have distinct
// tokens, so an element has one writer: no atomics, no barrier, and nothing but the groups' tokens is read or written.
#include <stdio.h>

#include "kw_common.h"
#include "seqbias.h"

namespace {

constexpr int SBT = 256;  // threads per row

__global__ __launch_bounds__(SBT) void seq_bias_process_kernel(float* __restrict__ scores, int V,
                                                               const int64_t* __restrict__ ids_all, int64_t ids_stride,
                                                               const int32_t* __restrict__ cur_len,
                                                               kw_seq_bias_table t) {
  float* s = scores + (int64_t)blockIdx.x * V;
  const int64_t* ids = ids_all + (int64_t)blockIdx.x * ids_stride;
  const int L = min(*cur_len, (int)ids_stride);
  for (int g = threadIdx.x; g < t.n_groups; g += SBT) {
    const int v = t.group_tok[g];
    if (v < 0 || v >= V) continue;  // (the host refuses such a table; never dereferenced)
    bool hit;
    const float b = kwsb::group_bias(t, g, ids, L, &hit);
    s[v] = s[v] + b;  // (scores + bias, :1318: a group none of whose entries applies adds the reference's 0.0)
  }
}

}  // namespace

extern "C" int kw_seq_bias_process(float* scores, int64_t R, int64_t V, const int64_t* ids, int64_t ids_stride,
                                   const int32_t* cur_len, const kw_seq_bias_table* table, kw_stream_t stream) {
  if (!scores || !ids || !cur_len || !table || R <= 0 || V <= 0 || V > 0x7fffffff || ids_stride <= 0 ||
      ids_stride > 0x7fffffff)
    return kw_set_error_msg(KW_EINVAL, "kw_seq_bias_process: invalid arguments");
  const char* why = "";
  if (const int rc = kwsb::table_check(table, &why)) {
    char msg[160];
    snprintf(msg, sizeof(msg), "kw_seq_bias_process: %s", why);
    return kw_set_error_msg(rc, msg);
  }
  if (table->n_seq == 0) return KW_OK;  // an empty processor: the buffer stays bit-identical
  hipLaunchKernelGGL(seq_bias_process_kernel, dim3((unsigned)R), dim3(SBT), 0, (hipStream_t)stream, scores, (int)V, ids,
                     ids_stride, cur_len, *table);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
