// GenerationMixin's two anti-repetition processors on device, for the greedy and sampled step tails:
// RepetitionPenaltyLogitsProcessor (TF/generation/logits_process.py:406-413) then NoRepeatNGramLogitsProcessor
// (:1121-1139), in place on the raw f32 logits [R][V], before the Whisper processors of kw_greedy_step /
// kw_sample_step (TF/generation/utils.py:1174-1183: they lead the processor list).  The beam tail applies the same two
// to log-probs inside kw_beam_logprobs_rep (beam.hip).
//
// One workgroup per row, threads striding over the row's history ids[0 .. L), L read from the device cur_len:
//   1. gather: every history position's token and its ORIGINAL score into registers;
//   2. barrier; scatter the penalised values.  The reference gathers before it scatters, so a token that occurs k
//      times is penalised once: its k writers all store the same value, computed from the same original.  Without the
//      barrier a late gather would read an early scatter's result and penalise it again;
//   3. barrier; the n-gram bans (-inf) last, so a token both penalised and banned ends as -inf.
// A row touches at most 2 L floats; nothing else of the buffer is read or written.
#include <math.h>

#include "kw_common.h"

namespace {

constexpr int RT = 512;   // threads per row
constexpr int RPER = 8;   // history positions per thread held in registers: ids_stride <= RT * RPER

__global__ __launch_bounds__(RT) void repeat_process_kernel(float* __restrict__ scores, int V,
                                                            const int64_t* __restrict__ ids_all, int64_t ids_stride,
                                                            const int32_t* __restrict__ cur_len, float penalty,
                                                            int ngram) {
  const int tid = threadIdx.x;
  float* s = scores + (int64_t)blockIdx.x * V;
  const int64_t* ids = ids_all + (int64_t)blockIdx.x * ids_stride;
  const int L = min(*cur_len, (int)ids_stride);
  if (penalty != 1.0f) {
    int tok[RPER];
    float org[RPER];
#pragma unroll
    for (int i = 0; i < RPER; ++i) {
      const int p = tid + i * RT;
      tok[i] = -1;
      org[i] = 0.f;
      if (p < L) {
        const int64_t t = ids[p];
        if (t >= 0 && t < V) {
          tok[i] = (int)t;
          org[i] = s[t];
        }
      }
    }
    __syncthreads();  // every original score is in a register before any is overwritten
#pragma unroll
    for (int i = 0; i < RPER; ++i)
      if (tok[i] >= 0) s[tok[i]] = org[i] < 0.f ? org[i] * penalty : org[i] / penalty;
  }
  if (ngram <= 0 || L < ngram) return;  // (uniform over the workgroup)
  __syncthreads();  // the bans land after the penalised values
  const int64_t* tail = ids + (L - (ngram - 1));  // the history's last n-1 tokens
  for (int i = tid; i + ngram <= L; i += RT) {
    bool same = true;
    for (int j = 0; j < ngram - 1 && same; ++j) same = ids[i + j] == tail[j];
    if (!same) continue;
    const int64_t t = ids[i + ngram - 1];
    if (t >= 0 && t < V) s[t] = -INFINITY;
  }
}

}  // namespace

extern "C" int kw_repeat_process(float* scores, int64_t R, int64_t V, const int64_t* ids, int64_t ids_stride,
                                 const int32_t* cur_len, float penalty, int32_t ngram, kw_stream_t stream) {
  if (!scores || !ids || !cur_len || R <= 0 || V <= 0 || V > 0x7fffffff || ids_stride <= 0 || !(penalty > 0.f) ||
      !isfinite(penalty) || ngram < 0)
    return kw_set_error_msg(KW_EINVAL, "kw_repeat_process: invalid arguments (penalty > 0 and finite, ngram >= 0)");
  if (ids_stride > (int64_t)RT * RPER)
    return kw_set_error_msg(KW_EUNSUPPORTED, "kw_repeat_process: ids_stride > 4096");
  if (penalty == 1.0f && ngram == 0) return KW_OK;  // both processors off: the buffer stays bit-identical
  hipLaunchKernelGGL(repeat_process_kernel, dim3((unsigned)R), dim3(RT), 0, (hipStream_t)stream, scores, (int)V, ids,
                     ids_stride, cur_len, penalty, (int)ngram);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
