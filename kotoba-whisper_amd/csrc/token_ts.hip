// Token-level timestamps (TF/models/whisper/generation_whisper.py:43-115, 241-381) on device:
//   kw_align_capture   per decode step: the alignment heads' cross-attention queries -> a log [A][B][t_log][64]
//   kw_align_weights   after decoding: softmax_s(q_t . K[b,h,s,:]) of every logged step, K from the cross cache
//   kw_align_weights_rows   the same with step t of item b read from log row rows[b][t] (beam search: the running row
//                      that produced the returned hypothesis' token)
//   kw_align_reduce    z-score over steps, median filter over frames, mean over heads, negate -> DTW matrix
//   kw_dtw             dynamic time warping (anti-diagonal wavefront) + backtrace -> frame index of every step
// The host only turns frame indices into seconds and lays the results out.
#include "kw_common.h"

namespace {

constexpr int HD = 64;
constexpr int CAP_MAX = 32;   // alignment heads of one layer per capture launch
constexpr int WT = 16;        // steps per kw_align_weights workgroup
constexpr int WTHREADS = 256;
constexpr int RF = 64;        // output frames per kw_align_reduce workgroup
constexpr int MEDW_MAX = 15;  // widest median filter
constexpr int RHALO = 8;      // >= MEDW_MAX / 2
constexpr int R_AMAX = 32;    // alignment pairs per kw_align_weights / kw_align_reduce launch

struct CapArgs {
  int32_t head[CAP_MAX];
  int32_t slot[CAP_MAX];
};
struct PairArgs {
  int32_t layer[R_AMAX];
  int32_t head[R_AMAX];
};

// one wave per (pair, row): 64 elements of the query row
template <typename T>
__global__ __launch_bounds__(64) void align_capture_kernel(const T* __restrict__ q, int d, CapArgs a, int B,
                                                           const int32_t* __restrict__ cur_len, int begin_index,
                                                           T* __restrict__ log, int t_log) {
  const int t = cur_len[0] - 1 - begin_index;  // index of the step's input token among the generated ones
  if (t < 0 || t >= t_log) return;
  const int p = blockIdx.x, b = blockIdx.y, l = threadIdx.x;
  log[(((int64_t)a.slot[p] * B + b) * t_log + t) * HD + l] = q[(int64_t)b * d + (int64_t)a.head[p] * HD + l];
}

// Where a block's WT queries lie: consecutive steps of one log row (kw_align_weights), or every step in a log row of
// its own, named by a device table (kw_align_weights_rows).  operator()(r): the 64 elements of the block's step r.
// align_scores takes the steps it computes and writes as a bit set (`steps`): all nt of them for kw_align_weights;
// kw_align_weights_rows goes once per item whose keys some of the block's steps attend.
template <typename T>
struct StepsOfRow {
  const T* q;  // step t0 of the row
  __device__ __forceinline__ const T* operator()(int r) const { return q + r * HD; }
};
template <typename T>
struct StepsByTable {
  const T* log;         // [R][t_log][64] of one pair
  const int32_t* rows;  // the item's table entries from step t0 on
  int R, t_log, t0;
  // (an entry outside [0, R) is clamped: a bad table gives wrong weights, never a read outside the log)
  __device__ __forceinline__ int row(int r) const { return min(max(rows[r], 0), R - 1); }
  __device__ __forceinline__ const T* operator()(int r) const { return log + ((int64_t)row(r) * t_log + t0 + r) * HD; }
};

// K[s][0..63] (f32) into registers
__device__ __forceinline__ void load_row64(const float* p, float* k) {
#pragma unroll
  for (int i = 0; i < HD / 4; ++i) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * i);
    k[4 * i] = v[0], k[4 * i + 1] = v[1], k[4 * i + 2] = v[2], k[4 * i + 3] = v[3];
  }
}

// Raw scores o[t][s] = q_t . K[s] of one (pair, row, block of WT steps), bf16: on the matrix cores.  A wave takes
// 16 key positions at a time: D = Q K^T by two v_mfma_f32_16x16x32_bf16 over the 64-wide head, both operands straight
// from global memory (lane l: 8 consecutive elements of row l & 15 at k = 8 (l >> 4), of Q for A and of K for B);
// D's lane holds column l & 15 (the key position) of rows 4 (l >> 4) .. + 3 (the steps).
template <typename Q>
__device__ __forceinline__ void align_scores(const Q& ql, const bf16_t* __restrict__ K, int S, uint32_t steps,
                                             float* __restrict__ o) {
  static_assert(WT == 16, "one MFMA row tile per block");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const bf16x8 zero = {};
  bf16x8 qa[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    qa[kk] = ((steps >> r) & 1) ? *reinterpret_cast<const bf16x8*>(ql(r) + kk * 32 + 8 * g) : zero;
  for (int st = wave; st * 16 < S; st += WTHREADS / 64) {
    const int s = st * 16 + r;
    bf16x8 kb[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      kb[kk] = s < S ? *reinterpret_cast<const bf16x8*>(K + (int64_t)s * HD + kk * 32 + 8 * g) : zero;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[0], kb[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[1], kb[1], acc, 0, 0, 0);
    if (s < S) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((steps >> (4 * g + i)) & 1) o[(int64_t)(4 * g + i) * S + s] = acc[i];
    }
  }
}

// f32 (the parity engine): exact f32 FMAs.  A thread owns key positions s = tid, tid + 256, ...: it takes K[s][0..63]
// into registers once and dots it with the block's queries (LDS, broadcast reads).
template <typename Q>
__device__ __forceinline__ void align_scores(const Q& ql, const float* __restrict__ K, int S, uint32_t steps,
                                             float* __restrict__ o) {
  __shared__ float qs[WT][HD];
  for (int i = threadIdx.x; i < WT * HD; i += WTHREADS)
    qs[i / HD][i % HD] = ((steps >> (i / HD)) & 1) ? ql(i / HD)[i % HD] : 0.f;
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += WTHREADS) {
    float k[HD];
    load_row64(K + (int64_t)s * HD, k);
#pragma unroll 1  // (rolled: unrolled, the queries' LDS reads are hoisted out of the s loop into > 256 registers)
    for (int t = 0; t < WT; ++t) {
      if (!((steps >> t) & 1)) continue;
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < HD; ++c) acc = fmaf(qs[t][c], k[c], acc);
      o[(int64_t)t * S + s] = acc;
    }
  }
}

// The raw scores of a block's nt steps lie in `o`: a wave per step normalises its row in place (max, exp and sum,
// divide -- torch's softmax).
__device__ __forceinline__ void align_softmax(float* __restrict__ o, int S, int nt) {
  __syncthreads();  // the scores other waves wrote
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wave; t < nt; t += WTHREADS / 64) {
    float* row = o + (int64_t)t * S;
    float m = -INFINITY;
    for (int s = lane; s < S; s += 64) m = fmaxf(m, row[s]);
    m = wave_max(m);
    float sum = 0.f;
    for (int s = lane; s < S; s += 64) {
      const float e = expf(row[s] - m);
      row[s] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    for (int s = lane; s < S; s += 64) row[s] = row[s] / sum;
  }
}

// grid (ceil(T / WT), B, A)
template <typename T>
__global__ __launch_bounds__(WTHREADS) void align_weights_kernel(const T* __restrict__ qlog, const T* __restrict__ kcache,
                                                                 int64_t k_layer_stride, PairArgs pairs, int B, int H,
                                                                 int S, int Tn, int t_log, float* __restrict__ out) {
  const int t0 = blockIdx.x * WT, b = blockIdx.y, a = blockIdx.z;
  const int nt = min(WT, Tn - t0);  // steps of this block
  const StepsOfRow<T> ql{qlog + (((int64_t)a * B + b) * t_log + t0) * HD};
  const T* K = kcache + (int64_t)pairs.layer[a] * k_layer_stride + ((int64_t)b * H + pairs.head[a]) * (int64_t)S * HD;
  float* o = out + (((int64_t)a * B + b) * Tn + t0) * (int64_t)S;
  align_scores(ql, K, S, (1u << nt) - 1u, o);
  align_softmax(o, S, nt);
}

// The same grid; the log has R = B * per rows per pair, item b's step t lies in row rows[b][t] (rows: [B][Tn]) and
// attends the keys of that row's item, rows[b][t] / per -- item b for the steps of b's own hypothesis, another item
// only where the reference falls back to running row 0.  The block's steps go item by item (one pass almost always).
template <typename T>
__global__ __launch_bounds__(WTHREADS) void align_weights_rows_kernel(const T* __restrict__ qlog,
                                                                      const int32_t* __restrict__ rows, int R,
                                                                      const T* __restrict__ kcache, int64_t k_layer_stride,
                                                                      PairArgs pairs, int B, int H, int S, int Tn,
                                                                      int t_log, float* __restrict__ out) {
  const int t0 = blockIdx.x * WT, b = blockIdx.y, a = blockIdx.z;
  const int nt = min(WT, Tn - t0);
  const StepsByTable<T> ql{qlog + (int64_t)a * R * t_log * HD, rows + (int64_t)b * Tn + t0, R, t_log, t0};
  float* o = out + (((int64_t)a * B + b) * Tn + t0) * (int64_t)S;
  const int per = R / B;
  uint32_t todo = (1u << nt) - 1u;  // (the table is the same for every thread: the loop is uniform)
  while (todo) {
    const int item = ql.row(__builtin_ctz(todo)) / per;
    uint32_t steps = 0;
    for (int r = 0; r < nt; ++r)
      if (((todo >> r) & 1) && ql.row(r) / per == item) steps |= 1u << r;
    const T* K =
        kcache + (int64_t)pairs.layer[a] * k_layer_stride + ((int64_t)item * H + pairs.head[a]) * (int64_t)S * HD;
    align_scores(ql, K, S, steps, o);
    todo &= ~steps;
    if (todo) __syncthreads();  // (the f32 path's query tile in LDS is rewritten by the next pass)
  }
  align_softmax(o, S, nt);
}

// torch.sort's order: ascending, NaN last
__device__ __forceinline__ void cswap(float& a, float& b) {
  const bool sw = (a > b) || (a != a);
  const float lo = sw ? b : a, hi = sw ? a : b;
  a = lo, b = hi;
}

// grid (ceil(S / RF), B), 256 threads.  Phase 1: mean and standard deviation over the steps of every (pair, column)
// of the tile and its halo (reflect-mapped); phase 2: a wave per step, a lane per frame: z-score the window, take its
// median, sum over the pairs.
template <int width>
__global__ __launch_bounds__(256) void align_reduce_kernel(const float* __restrict__ w, int A, int B, int Tn, int S,
                                                           const int32_t* __restrict__ frames, float* __restrict__ out,
                                                           int a_total, int first, int last) {
  __shared__ float s_mean[R_AMAX][RF + 2 * RHALO];
  __shared__ float s_std[R_AMAX][RF + 2 * RHALO];
  const int f0 = blockIdx.x * RF, b = blockIdx.y, tid = threadIdx.x;
  int F = frames ? frames[b] : S;
  F = F < 0 ? 0 : (F > S ? S : F);
  constexpr int pad = width / 2;
  const bool filt = F > pad;  // _median_filter returns its input when the frame count is <= pad
  const int ncol = RF + 2 * pad;
  // column c of the tile <-> frame f0 - pad + c, reflected into [0, F)
  auto frame_of = [&](int c) {
    int f = f0 - pad + c;
    if (!filt) return f;
    if (f < 0) f = -f;
    if (f >= F) f = 2 * (F - 1) - f;
    return f;
  };
  if (f0 < F) {
    for (int i = tid; i < A * ncol; i += 256) {
      const int a = i / ncol, c = i % ncol, f = frame_of(c);
      float mean = 0.f, sd = 0.f;
      if (f >= 0 && f < F) {
        const float* col = w + ((int64_t)a * B + b) * Tn * (int64_t)S + f;
        float sum = 0.f;
        for (int t = 0; t < Tn; ++t) sum += col[(int64_t)t * S];
        mean = sum / (float)Tn;
        float ss = 0.f;
        for (int t = 0; t < Tn; ++t) {
          const float dlt = col[(int64_t)t * S] - mean;
          ss = fmaf(dlt, dlt, ss);
        }
        sd = sqrtf(ss / (float)Tn);
      }
      s_mean[a][c] = mean, s_std[a][c] = sd;
    }
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63, f = f0 + lane;
  if (f >= S) return;
  for (int t = wave; t < Tn; t += 4) {
    float* dst = out + ((int64_t)b * Tn + t) * S + f;
    if (f >= F) {  // columns past the row's frame count are not part of the matrix
      if (last) *dst = 0.f;
      continue;
    }
    float acc = first ? 0.f : *dst;
    for (int a = 0; a < A; ++a) {
      const float* row = w + (((int64_t)a * B + b) * Tn + t) * (int64_t)S;
      float v;
      if (!filt) {
        const int c = lane + pad;
        v = (row[f] - s_mean[a][c]) / s_std[a][c];
      } else {
        float z[width];
#pragma unroll
        for (int j = 0; j < width; ++j) {
          const int c = lane + j;
          z[j] = (row[frame_of(c)] - s_mean[a][c]) / s_std[a][c];
        }
        // selection sort up to the median
#pragma unroll
        for (int i = 0; i <= pad; ++i)
#pragma unroll
          for (int j = i + 1; j < width; ++j) cswap(z[i], z[j]);
        v = z[pad];
      }
      acc += v;
    }
    *dst = last ? -(acc / (float)a_total) : acc;
  }
}

// One workgroup per row, thread i <-> text index i (1-based), marching over anti-diagonals d = i + j.
// cost[i-1][j-1] is what the thread read as cost[i-1][j] one diagonal earlier, cost[i][j-1] its own last value, so only
// cost[i-1][j] crosses threads (LDS, double-buffered: one barrier per diagonal).  The trace is one byte per cell.
__global__ void dtw_kernel(const float* __restrict__ m, int Tn, int S, const int32_t* __restrict__ frames,
                           uint8_t* __restrict__ trace, int32_t* __restrict__ out) {
  extern __shared__ float buf[];  // [2][Tn + 1]
  const int b = blockIdx.x, i = threadIdx.x + 1;
  int F = frames ? frames[b] : S;
  F = F < 0 ? 0 : (F > S ? S : F);
  const float* row = m + ((int64_t)b * Tn + (i - 1)) * (int64_t)S;
  uint8_t* trow = trace + ((int64_t)b * Tn + (i - 1)) * (int64_t)S;
  const bool live = i <= Tn;
  float c0 = i == 1 ? 0.f : INFINITY;  // cost[i-1][0]
  float own = INFINITY;                // cost[i][0]
  if (live) buf[i] = INFINITY, buf[Tn + 1 + i] = INFINITY;
  if (threadIdx.x == 0) buf[0] = INFINITY, buf[Tn + 1] = INFINITY;  // cost[0][j >= 1]
  __syncthreads();
  float nxt = (live && F >= 1) ? row[0] : 0.f;
  for (int d = 2; d <= Tn + F; ++d) {
    const int j = d - i;
    const bool act = live && j >= 1 && j <= F;
    if (act) {
      const float mv = nxt;
      if (j + 1 <= F) nxt = row[j];  // next diagonal's value, in flight across the barrier
      const float c1 = buf[((d - 1) & 1) * (Tn + 1) + i - 1];
      const float c2 = own;
      float c;
      uint8_t tr;
      if (c0 < c1 && c0 < c2) c = c0, tr = 0;
      else if (c1 < c0 && c1 < c2) c = c1, tr = 1;
      else c = c2, tr = 2;
      own = mv + c;
      c0 = c1;
      trow[j - 1] = tr;
      buf[(d & 1) * (Tn + 1) + i] = own;
    }
    __syncthreads();
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // backtrace (trace[0][:] = 2, trace[:][0] = 1): walking back, the last visit of a text index is its first frame
  const uint8_t* tb = trace + (int64_t)b * Tn * (int64_t)S;
  int ii = Tn, jj = F;
  while (ii > 0 || jj > 0) {
    if (ii >= 1) out[(int64_t)b * Tn + ii - 1] = jj - 1;
    const int tr = ii == 0 ? 2 : (jj == 0 ? 1 : tb[(int64_t)(ii - 1) * S + (jj - 1)]);
    if (tr == 0) --ii, --jj;
    else if (tr == 1) --ii;
    else --jj;
  }
}

}  // namespace

extern "C" int kw_align_capture(int dtype, const void* q, int64_t B, int64_t d, const int32_t* heads,
                                const int32_t* slots, int64_t n, int64_t n_slots, const int32_t* cur_len,
                                int64_t begin_index, void* log, int64_t t_log, kw_stream_t stream) {
  if (!q || !heads || !slots || !cur_len || !log || B <= 0 || d <= 0 || d % HD != 0 || n <= 0 || n > CAP_MAX ||
      n_slots <= 0 || t_log <= 0 || begin_index < 0 || (dtype != KW_DT_F32 && dtype != KW_DT_BF16))
    return kw_set_error_msg(KW_EINVAL, "kw_align_capture: invalid arguments (d % 64 == 0, 1 <= n <= 32)");
  CapArgs a;
  for (int64_t i = 0; i < n; ++i) {
    if (heads[i] < 0 || heads[i] >= d / HD || slots[i] < 0 || slots[i] >= n_slots)
      return kw_set_error_msg(KW_EINVAL, "kw_align_capture: head or log slot out of range");
    a.head[i] = heads[i], a.slot[i] = slots[i];
  }
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)n, (unsigned)B);
  if (dtype == KW_DT_F32)
    hipLaunchKernelGGL(align_capture_kernel<float>, grid, dim3(64), 0, s, (const float*)q, (int)d, a, (int)B, cur_len,
                       (int)begin_index, (float*)log, (int)t_log);
  else
    hipLaunchKernelGGL(align_capture_kernel<bf16_t>, grid, dim3(64), 0, s, (const bf16_t*)q, (int)d, a, (int)B, cur_len,
                       (int)begin_index, (bf16_t*)log, (int)t_log);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" int kw_align_weights(int dtype, const void* qlog, int64_t t_log, const void* k_cache, int64_t k_layer_stride,
                                int64_t n_layers, const int32_t* pairs, int64_t A, int64_t B, int64_t H, int64_t S,
                                int64_t T, float* out, kw_stream_t stream) {
  if (!qlog || !k_cache || !pairs || !out || A <= 0 || A > R_AMAX || B <= 0 || H <= 0 || S <= 0 || T <= 0 || T > t_log ||
      k_layer_stride < 0 || n_layers <= 0 || B > 65535 || (dtype != KW_DT_F32 && dtype != KW_DT_BF16) ||
      (uintptr_t)k_cache % 16 != 0 || (uintptr_t)qlog % 16 != 0 || (k_layer_stride * (dtype == KW_DT_F32 ? 4 : 2)) % 16 != 0)
    return kw_set_error_msg(KW_EINVAL, "kw_align_weights: invalid arguments (A <= 32 per launch, 1 <= T <= t_log, "
                                       "16-B aligned cache)");
  PairArgs pa;
  for (int64_t i = 0; i < A; ++i) {
    if (pairs[2 * i] < 0 || pairs[2 * i] >= n_layers || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= H)
      return kw_set_error_msg(KW_EINVAL, "kw_align_weights: (layer, head) out of range");
    pa.layer[i] = pairs[2 * i], pa.head[i] = pairs[2 * i + 1];
  }
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((T + WT - 1) / WT), (unsigned)B, (unsigned)A);
  if (dtype == KW_DT_F32)
    hipLaunchKernelGGL(align_weights_kernel<float>, grid, dim3(WTHREADS), 0, s, (const float*)qlog, (const float*)k_cache,
                       k_layer_stride, pa, (int)B, (int)H, (int)S, (int)T, (int)t_log, out);
  else
    hipLaunchKernelGGL(align_weights_kernel<bf16_t>, grid, dim3(WTHREADS), 0, s, (const bf16_t*)qlog,
                       (const bf16_t*)k_cache, k_layer_stride, pa, (int)B, (int)H, (int)S, (int)T, (int)t_log, out);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" int kw_align_weights_rows(int dtype, const void* qlog, int64_t R, int64_t t_log, const int32_t* rows,
                                     const void* k_cache, int64_t k_layer_stride, int64_t n_layers, const int32_t* pairs,
                                     int64_t A, int64_t B, int64_t H, int64_t S, int64_t T, float* out,
                                     kw_stream_t stream) {
  if (!qlog || !rows || !k_cache || !pairs || !out || A <= 0 || A > R_AMAX || B <= 0 || R <= 0 || R > (1 << 20) ||
      R % (B > 0 ? B : 1) != 0 ||
      H <= 0 || S <= 0 || T <= 0 || T > t_log || k_layer_stride < 0 || n_layers <= 0 || B > 65535 ||
      (dtype != KW_DT_F32 && dtype != KW_DT_BF16) || (uintptr_t)k_cache % 16 != 0 || (uintptr_t)qlog % 16 != 0 ||
      (uintptr_t)rows % 4 != 0 || (k_layer_stride * (dtype == KW_DT_F32 ? 4 : 2)) % 16 != 0)
    return kw_set_error_msg(KW_EINVAL, "kw_align_weights_rows: invalid arguments (A <= 32 per launch, 1 <= T <= t_log, "
                                       "R a multiple of B, 16-B aligned cache)");
  PairArgs pa;
  for (int64_t i = 0; i < A; ++i) {
    if (pairs[2 * i] < 0 || pairs[2 * i] >= n_layers || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= H)
      return kw_set_error_msg(KW_EINVAL, "kw_align_weights_rows: (layer, head) out of range");
    pa.layer[i] = pairs[2 * i], pa.head[i] = pairs[2 * i + 1];
  }
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((T + WT - 1) / WT), (unsigned)B, (unsigned)A);
  if (dtype == KW_DT_F32)
    hipLaunchKernelGGL(align_weights_rows_kernel<float>, grid, dim3(WTHREADS), 0, s, (const float*)qlog, rows, (int)R,
                       (const float*)k_cache, k_layer_stride, pa, (int)B, (int)H, (int)S, (int)T, (int)t_log, out);
  else
    hipLaunchKernelGGL(align_weights_rows_kernel<bf16_t>, grid, dim3(WTHREADS), 0, s, (const bf16_t*)qlog, rows, (int)R,
                       (const bf16_t*)k_cache, k_layer_stride, pa, (int)B, (int)H, (int)S, (int)T, (int)t_log, out);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" int kw_align_reduce(const float* weights, int64_t A, int64_t B, int64_t T, int64_t S, const int32_t* frames,
                               int64_t filter_width, float* out, int64_t a_total, int first, int last,
                               kw_stream_t stream) {
  if (!weights || !out || A <= 0 || A > R_AMAX || B <= 0 || B > 65535 || T <= 0 || S <= 0 || a_total < A ||
      filter_width <= 0 || filter_width % 2 != 1 || filter_width > MEDW_MAX)
    return kw_set_error_msg(KW_EINVAL, "kw_align_reduce: invalid arguments (A <= 32 per launch, odd filter width <= 15)");
  const dim3 grid((unsigned)((S + RF - 1) / RF), (unsigned)B);
#define KW_REDUCE_W(W)                                                                                              \
  case W:                                                                                                           \
    hipLaunchKernelGGL(align_reduce_kernel<W>, grid, dim3(256), 0, (hipStream_t)stream, weights, (int)A, (int)B,   \
                       (int)T, (int)S, frames, out, (int)a_total, first, last);                                     \
    break;
  switch ((int)filter_width) {
    KW_REDUCE_W(1) KW_REDUCE_W(3) KW_REDUCE_W(5) KW_REDUCE_W(7) KW_REDUCE_W(9) KW_REDUCE_W(11) KW_REDUCE_W(13)
    KW_REDUCE_W(15)
  }
#undef KW_REDUCE_W
  KW_CHECK_LAUNCH();
  return KW_OK;
}

extern "C" size_t kw_dtw_workspace(int64_t B, int64_t T, int64_t S) {
  if (B <= 0 || T <= 0 || S <= 0) return 0;
  return (size_t)B * (size_t)T * (size_t)S;
}

extern "C" int kw_dtw(const float* matrix, int64_t B, int64_t T, int64_t S, const int32_t* frames, int32_t* out,
                      void* workspace, size_t ws_bytes, kw_stream_t stream) {
  if (!matrix || !out || !workspace || B <= 0 || T <= 0 || T > 1024 || S <= 0 || S > (1 << 20))
    return kw_set_error_msg(KW_EINVAL, "kw_dtw: invalid arguments (1 <= T <= 1024)");
  if (ws_bytes < kw_dtw_workspace(B, T, S)) return kw_set_error_msg(KW_EINVAL, "kw_dtw: workspace too small");
  const unsigned threads = (unsigned)((T + 63) / 64 * 64);
  hipLaunchKernelGGL(dtw_kernel, dim3((unsigned)B), dim3(threads), 2 * (size_t)(T + 1) * sizeof(float),
                     (hipStream_t)stream, matrix, (int)T, (int)S, frames, (uint8_t*)workspace, out);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
