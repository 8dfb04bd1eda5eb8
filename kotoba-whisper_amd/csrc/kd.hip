// Knowledge-distillation loss on the teacher's logits (kw_kd_loss; include/kwhisper.h has the contract): the
// temperature KL of run_distillation.py:614-622,652-657, forward and the student's gradient.
//
// Three launches on the stream, ordered by the stream alone (no in-launch hand-off, no float atomics):
//   kd_count_kernel  one workgroup: n_valid = #{labels >= 0} into the workspace;
//   kd_row_kernel    one workgroup per row.  Pass 1 reads the teacher and the student row once each, every thread
//                    keeping a running (max, sum of exp) pair per tensor (online softmax), merged over the workgroup
//                    in a fixed order.  Pass 2 reads both rows again (from cache: a row is 2-4 x 104 KB) and writes
//                    the row's divergence and its gradient row;
//   kd_final_kernel  one workgroup: loss = T^2 * sum(row_kl) / n_valid in a fixed order, n_valid back to zero.
// Every sum has a fixed association (thread-strided loops, xor butterflies, wave partials combined in wave order), so
// loss, row_kl and grad are bitwise the same from run to run.
//
// Row starts are only element-aligned (V = 51865 with ld == V).  Pass 1 walks each tensor on its own 16-byte grid:
// the elements before the row's first 16-byte boundary and after its last one go to the first threads one by one.
// Pass 2 walks the teacher's grid and takes the student and the gradient at the same element positions with
// element-aligned vector accesses (the hardware's unaligned mode; aligned whenever the rows happen to be).
#include <float.h>
#include <math.h>

#include "kw_common.h"

namespace {

constexpr int KD_T = 512;  // threads of a row's workgroup
constexpr int KD_W = KD_T / KW_WAVE;
constexpr int KD_R = 1024;  // threads of the two one-workgroup reductions

struct MS {
  float m, s;  // running maximum, sum of exp(x - m)
};

__device__ __forceinline__ MS ms_merge(MS a, MS b) {
  // (symmetric in a and b, bit for bit: every lane of a butterfly ends with the same pair)
  const float m = fmaxf(a.m, b.m);
  return {m, a.s * __expf(a.m - m) + b.s * __expf(b.m - m)};
}

__device__ __forceinline__ void ms_add(MS& a, float x) {
  if (x > a.m) {
    a.s = a.s * __expf(a.m - x) + 1.f;
    a.m = x;
  } else {
    a.s += __expf(x - a.m);
  }
}

template <typename T> struct Piece;  // a 16-byte piece of a row
template <> struct Piece<float> {
  static constexpr int E = 4;
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = x[e];
  }
};
template <> struct Piece<bf16_t> {
  static constexpr int E = 8;
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const u32x4 x = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = __uint_as_float(x[e] << 16);
      v[2 * e + 1] = __uint_as_float(x[e] & 0xffff0000u);
    }
  }
};

// elements of a row before its first 16-byte boundary (at most V)
template <typename T>
__device__ __forceinline__ int row_head(const T* x, int V) {
  const int h = (int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) / sizeof(T));
  return min(h, V);
}

// one thread's share of a row's (max, sum exp) of x * inv_t
template <typename T>
__device__ __forceinline__ MS row_stats(const T* __restrict__ x, int V, float inv_t, int tid) {
  constexpr int E = Piece<T>::E;
  MS a{-FLT_MAX, 0.f};
  const int head = row_head(x, V);
  const int nvec = (V - head) / E;
  const int tail0 = head + nvec * E;
  if (tid < head) ms_add(a, TypeIO<T>::ld(x + tid) * inv_t);
  if (tid < V - tail0) ms_add(a, TypeIO<T>::ld(x + tail0 + tid) * inv_t);
  const T* xb = x + head;
  for (int i = tid; i < nvec; i += KD_T) {
    float v[E];
    Piece<T>::ld(xb + (int64_t)i * E, v);
    float mx = v[0] * inv_t;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      v[e] *= inv_t;
      mx = fmaxf(mx, v[e]);
    }
    if (mx > a.m) {
      a.s *= __expf(a.m - mx);
      a.m = mx;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) a.s += __expf(v[e] - a.m);
  }
  return a;
}

// the workgroup's pair: xor butterfly inside each wave, then the KD_W wave pairs in wave order (every thread alike)
__device__ __forceinline__ MS block_ms(MS a, MS* sh, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MS b;
    b.m = __shfl_xor(a.m, o, 64);
    b.s = __shfl_xor(a.s, o, 64);
    a = ms_merge(a, b);
  }
  if ((tid & 63) == 0) sh[tid >> 6] = a;
  __syncthreads();
  MS r = sh[0];
#pragma unroll
  for (int w = 1; w < KD_W; ++w) r = ms_merge(r, sh[w]);
  return r;
}

// four consecutive elements at an element-aligned address
__device__ __forceinline__ void ld4(const float* p, float* v) {
  f32x4 x;
  __builtin_memcpy(&x, p, 16);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = x[e];
}
__device__ __forceinline__ void ld4(const bf16_t* p, float* v) {
  u32x2 x;
  __builtin_memcpy(&x, p, 8);
  v[0] = __uint_as_float(x[0] << 16);
  v[1] = __uint_as_float(x[0] & 0xffff0000u);
  v[2] = __uint_as_float(x[1] << 16);
  v[3] = __uint_as_float(x[1] & 0xffff0000u);
}
__device__ __forceinline__ void st4(float* p, const float* v) {
  const f32x4 x = {v[0], v[1], v[2], v[3]};
  __builtin_memcpy(p, &x, 16);
}
__device__ __forceinline__ void st4(bf16_t* p, const float* v) {
  const u32x2 x = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
  __builtin_memcpy(p, &x, 8);
}

struct KdRow {
  float mt, ms, rst, rss, dl, gsc;  // maxima, 1 / sums, log St - log Ss, T / n_valid
};

// one element: its divergence term (returned) and its gradient
__device__ __forceinline__ float kd_elem(const KdRow& k, float a, float b, float& g) {
  const float da = a - k.mt, db = b - k.ms;
  const float p = __expf(da) * k.rst, q = __expf(db) * k.rss;
  g = (q - p) * k.gsc;
  // log p - log q = (da - log St) - (db - log Ss); a term with p == 0 is 0 whatever the logarithms are (xlogy)
  return p > 0.f ? p * ((da - db) - k.dl) : 0.f;
}

template <typename ST>
__global__ __launch_bounds__(KD_T) void kd_row_kernel(const float* __restrict__ teacher, int64_t ldt,
                                                      const ST* __restrict__ student, int64_t lds,
                                                      const int64_t* __restrict__ labels, int V, float temperature,
                                                      const int* __restrict__ n_valid, float* __restrict__ row_kl,
                                                      ST* __restrict__ grad, int64_t ldg) {
  __shared__ MS sh_t[KD_W], sh_s[KD_W];
  __shared__ float sh_kl[KD_W];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  ST* g = grad ? grad + r * ldg : nullptr;
  if (labels[r] < 0) {  // an ignored row: exactly zero in row_kl and in every gradient element
    if (tid == 0) row_kl[r] = 0.f;
    if (g) {
      const float z[4] = {0.f, 0.f, 0.f, 0.f};
      const int nvec = V / 4;
      for (int i = tid; i < nvec; i += KD_T) st4(g + (int64_t)i * 4, z);
      if (tid < V - nvec * 4) TypeIO<ST>::st(g + nvec * 4 + tid, 0.f);
    }
    return;
  }
  const float* t = teacher + r * ldt;
  const ST* s = student + r * lds;
  const float inv_t = 1.0f / temperature;
  // ---- pass 1: online (max, sum exp) of both rows ----
  const MS at = block_ms(row_stats(t, V, inv_t, tid), sh_t, tid);
  const MS as = block_ms(row_stats(s, V, inv_t, tid), sh_s, tid);
  KdRow k;
  k.mt = at.m, k.ms = as.m;
  k.rst = 1.0f / at.s, k.rss = 1.0f / as.s;
  k.dl = logf(at.s) - logf(as.s);
  k.gsc = temperature / (float)*n_valid;  // (a valid row exists: this one)
  // ---- pass 2: the divergence terms and the gradient, on the teacher's 16-byte grid ----
  const int head = row_head(t, V);
  const int nvec = (V - head) / 4;
  const int tail0 = head + nvec * 4;
  float kl = 0.f;
  {
    int e = -1;  // this thread's element of the head / tail, if any
    if (tid < head) e = tid;
    else if (tid >= 64 && tid - 64 < V - tail0) e = tail0 + tid - 64;
    if (e >= 0) {
      float gv;
      kl += kd_elem(k, t[e] * inv_t, TypeIO<ST>::ld(s + e) * inv_t, gv);
      if (g) TypeIO<ST>::st(g + e, gv);
    }
  }
  for (int i = tid; i < nvec; i += KD_T) {
    const int64_t o = head + (int64_t)i * 4;
    float a[4], b[4], gv[4];
    Piece<float>::ld(t + o, a);
    ld4(s + o, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) kl += kd_elem(k, a[e] * inv_t, b[e] * inv_t, gv[e]);
    if (g) st4(g + o, gv);
  }
  kl = wave_sum(kl);
  if ((tid & 63) == 0) sh_kl[tid >> 6] = kl;
  __syncthreads();
  if (tid == 0) {
    float tot = sh_kl[0];
#pragma unroll
    for (int w = 1; w < KD_W; ++w) tot += sh_kl[w];
    row_kl[r] = tot;
  }
}

__global__ __launch_bounds__(KD_R) void kd_count_kernel(const int64_t* __restrict__ labels, int64_t N,
                                                        int* __restrict__ n_valid) {
  __shared__ int sh[KD_R / KW_WAVE];
  const int tid = threadIdx.x;
  int c = 0;
  for (int64_t i = tid; i < N; i += KD_R) c += labels[i] >= 0 ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((tid & 63) == 0) sh[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < KD_R / KW_WAVE; ++w) tot += sh[w];
    *n_valid = tot;
  }
}

__global__ __launch_bounds__(KD_R) void kd_final_kernel(const float* __restrict__ row_kl, int64_t N, float temperature,
                                                        int* __restrict__ n_valid, float* __restrict__ loss) {
  __shared__ float sh[KD_R / KW_WAVE];
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int64_t i = tid; i < N; i += KD_R) s += row_kl[i];
  s = wave_sum(s);
  if ((tid & 63) == 0) sh[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    float tot = sh[0];
    for (int w = 1; w < KD_R / KW_WAVE; ++w) tot += sh[w];
    const int n = *n_valid;
    *loss = tot / (float)n * (temperature * temperature);  // n == 0: 0 / 0 = NaN, as the reference's mean over nothing
    *n_valid = 0;  // the workspace is left zeroed
  }
}

// whether [a, a + an) and [b, b + bn) share a byte
bool overlaps(const void* a, size_t an, const void* b, size_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bn && y < x + an;
}

}  // namespace

extern "C" size_t kw_kd_loss_workspace(int64_t N) {
  if (N < 1) return 0;
  return 64;
}

extern "C" int kw_kd_loss(const kw_kd_loss_args* a, kw_stream_t stream) {
  if (!a || !a->teacher || !a->student || !a->labels || !a->row_kl || !a->loss)
    return kw_set_error_msg(KW_EINVAL, "kw_kd_loss: teacher, student, labels, row_kl and loss must not be NULL");
  if (a->s_dtype != KW_DT_F32 && a->s_dtype != KW_DT_BF16)
    return kw_set_error_msg(KW_EINVAL, "kw_kd_loss: the student's dtype must be KW_DT_F32 or KW_DT_BF16");
  if (a->N < 1 || a->N > 0x7fffffff || a->V < 1 || a->V > 0x7fffffff || a->ldt < a->V || a->lds < a->V ||
      (a->grad && a->ldg < a->V))
    return kw_set_error_msg(KW_EINVAL, "kw_kd_loss: 1 <= N, V < 2^31 and every row stride >= V");
  if (!(a->temperature > 0.f) || !isfinite(a->temperature))
    return kw_set_error_msg(KW_EINVAL, "kw_kd_loss: temperature must be a finite float > 0");
  const size_t es = a->s_dtype == KW_DT_F32 ? 4 : 2;
  if (((uintptr_t)a->teacher & 3) || ((uintptr_t)a->student & (es - 1)) || ((uintptr_t)a->grad & (es - 1)) ||
      ((uintptr_t)a->labels & 7) || ((uintptr_t)a->row_kl & 3) || ((uintptr_t)a->loss & 3))
    return kw_set_error_msg(KW_EINVAL, "kw_kd_loss: a pointer is not aligned to its element type");
  if (!a->workspace || a->ws_bytes < kw_kd_loss_workspace(a->N) || ((uintptr_t)a->workspace & 3))
    return kw_set_error_msg(KW_EINVAL, "kw_kd_loss: workspace missing or smaller than kw_kd_loss_workspace(N)");
  if (a->grad) {
    const size_t gn = (size_t)((a->N - 1) * a->ldg + a->V) * es;
    if (overlaps(a->grad, gn, a->student, (size_t)((a->N - 1) * a->lds + a->V) * es) ||
        overlaps(a->grad, gn, a->teacher, (size_t)((a->N - 1) * a->ldt + a->V) * 4))
      return kw_set_error_msg(KW_EINVAL, "kw_kd_loss: grad must not alias student or teacher (the cross-entropy "
                                         "loss still reads the student's logits)");
  }
  hipStream_t st = (hipStream_t)stream;
  int* n_valid = reinterpret_cast<int*>(a->workspace);
  hipLaunchKernelGGL(kd_count_kernel, dim3(1), dim3(KD_R), 0, st, a->labels, a->N, n_valid);
  KW_CHECK_LAUNCH();
  if (a->s_dtype == KW_DT_F32)
    hipLaunchKernelGGL(kd_row_kernel<float>, dim3((unsigned)a->N), dim3(KD_T), 0, st, a->teacher, a->ldt,
                       reinterpret_cast<const float*>(a->student), a->lds, a->labels, (int)a->V, a->temperature,
                       n_valid, a->row_kl, reinterpret_cast<float*>(a->grad), a->ldg);
  else
    hipLaunchKernelGGL(kd_row_kernel<bf16_t>, dim3((unsigned)a->N), dim3(KD_T), 0, st, a->teacher, a->ldt,
                       reinterpret_cast<const bf16_t*>(a->student), a->lds, a->labels, (int)a->V, a->temperature,
                       n_valid, a->row_kl, reinterpret_cast<bf16_t*>(a->grad), a->ldg);
  KW_CHECK_LAUNCH();
  hipLaunchKernelGGL(kd_final_kernel, dim3(1), dim3(KD_R), 0, st, a->row_kl, a->N, a->temperature, n_valid, a->loss);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
