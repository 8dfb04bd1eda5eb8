// kw_cross_kv_quant: the cross-attention K / V cache from bf16 to OCP e4m3fn codes with one f32 scale per
// (tile, head dim), the format of include/kwhisper.h "fp8 cross K/V".  Run once per batch item on what the
// cross-K/V GEMM (kw_gemm, KW_EPI_HEADSPLIT; TF modeling_whisper.py:323-335) wrote; the decode steps then read the
// codes (kw_cross_attn_step_fp8, kw_dec_xq_cross_fp8) 128 x 32 times.
#include "attn_common.h"
#include "kw_common.h"

namespace {

constexpr float E4M3_MAX = 448.0f;

// One workgroup per [S][64] tile.  Thread (slot = tid / 4, part = tid % 4) holds dims 16 part .. 16 part + 15 of rows
// slot, slot + 64, ...: two 16-B loads per row, one 16-B store of its 16 codes.  Pass 1 is the column absmax (a
// maximum of bf16 magnitudes, taken on their bit patterns: exact and order-independent), pass 2 re-reads the tile
// (192 KB at S = 1500: L2 / Infinity Cache) and converts.
__global__ __launch_bounds__(256) void cross_kv_quant_kernel(const bf16_t* __restrict__ x, int S, uint8_t* __restrict__ codes,
                                                             float* __restrict__ scales) {
  __shared__ unsigned amax[HD];
  const int tid = threadIdx.x, part = tid & 3, slot = tid >> 2;
  const int64_t tile = blockIdx.x;
  const u32x4* src = reinterpret_cast<const u32x4*>(x + tile * S * HD) + part * 2;  // row r: src + r * 8
  if (tid < HD) amax[tid] = 0u;
  __syncthreads();
  unsigned m[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = 0u;
  for (int r = slot; r < S; r += 64) {
    const u32x4 a = src[r * 8], b = src[r * 8 + 1];
    const uint32_t w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      m[2 * i] = max(m[2 * i], w[i] & 0x7fffu);
      m[2 * i + 1] = max(m[2 * i + 1], (w[i] >> 16) & 0x7fffu);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) m[i] = max(m[i], (unsigned)__shfl_xor((int)m[i], o, 64));
    if ((tid & 63) < 4) atomicMax(&amax[part * 16 + i], m[i]);
  }
  __syncthreads();
  float inv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float a = bf2f((bf16_t)amax[part * 16 + i]);
    inv[i] = a > 0.f ? E4M3_MAX / a : 0.f;  // one correctly rounded division per channel
  }
  if (tid < HD) scales[tile * HD + tid] = bf2f((bf16_t)amax[tid]) / E4M3_MAX;
  u32x4* dst = reinterpret_cast<u32x4*>(codes + tile * S * HD) + part;  // row r: dst + r * 4
  for (int r = slot; r < S; r += 64) {
    const u32x4 a = src[r * 8], b = src[r * 8 + 1];
    const uint32_t w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    u32x4 c;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t ww = w[2 * i + (e >> 1)];
        const float v = __uint_as_float((e & 1) ? (ww & 0xffff0000u) : (ww << 16)) * inv[4 * i + e];
        // |x inv| passes 448 by f32 rounding at most, which rounds to 448 anyway: clamped, because the conversion
        // does not saturate (e4m3fn has no infinity: an overflow would be NaN)
        f[e] = __builtin_amdgcn_fmed3f(v, -E4M3_MAX, E4M3_MAX);
      }
      int p = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
      p = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], p, true);
      // a zero channel's codes are 0, whatever the sign of its zeros
      const uint32_t keep = (inv[4 * i] != 0.f ? 0xffu : 0u) | (inv[4 * i + 1] != 0.f ? 0xff00u : 0u) |
                            (inv[4 * i + 2] != 0.f ? 0xff0000u : 0u) | (inv[4 * i + 3] != 0.f ? 0xff000000u : 0u);
      c[i] = (uint32_t)p & keep;
    }
    dst[r * 4] = c;
  }
}

}  // namespace

extern "C" int kw_cross_kv_quant(const void* x, int64_t n, int64_t S, int64_t hd, void* codes, float* scales,
                                 kw_stream_t stream) {
  if (!x || !codes || !scales || n <= 0 || S <= 0 || n > 0x7fffffff || S > (1 << 24))
    return kw_set_error_msg(KW_EINVAL, "kw_cross_kv_quant: invalid arguments");
  if (hd != HD) return kw_set_error_msg(KW_EUNSUPPORTED, "kw_cross_kv_quant: head_dim must be 64");
  if ((uintptr_t)x % 16 || (uintptr_t)codes % 16)
    return kw_set_error_msg(KW_EINVAL, "kw_cross_kv_quant: x and codes must be 16-B aligned");
  hipLaunchKernelGGL(cross_kv_quant_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (int)S,
                     (uint8_t*)codes, scales);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
