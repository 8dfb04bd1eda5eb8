// The tile steps of the decode linears (declin.hip) and of the projection fused into another kernel's launch
// (decproj.h), each written once: fragment loads, the MFMA loop, the LayerNorm row statistics on the matrix cores and
// their fold into the epilogue.  The bitwise guarantees the tests hold (rows kernel == chunked launch, fused qkv / xq
// projection == kw_dec_linear, fragment-major == row-major) rest on every kernel doing these steps operation for
// operation alike: a kernel composes the helpers, it does not copy them.  A wave owns k-tiles [kt0, kt1), at most KTM;
// ktl = max(kt1 - 1, kt0) clamps the loads of the slots past kt1 (loaded, never multiplied).
#pragma once
#include "kw_common.h"

namespace {

// column groups of ncb 16-column blocks covering N columns (a workgroup's share of the output)
template <typename T>
__host__ __device__ constexpr T col_groups(T N, int ncb) {
  return (N + 16 * ncb - 1) / (16 * ncb);
}

// the wave's weight fragments of column group cg: packed [N/16][K/32][64 lanes][8], one coalesced 16 B per lane each.
// NT: non-temporal (a weight slice streamed once)
template <int KTM, int NCB, bool NT>
__device__ __forceinline__ void load_w_frags(const bf16x8* W, int cg, int nkt, int kt0, int ktl, int lane,
                                             bf16x8 (&w)[NCB][KTM]) {
#pragma unroll
  for (int c = 0; c < NCB; ++c)
#pragma unroll
    for (int u = 0; u < KTM; ++u) {
      const bf16x8* src = W + ((int64_t)(cg * NCB + c) * nkt + min(kt0 + u, ktl)) * 64 + lane;
      w[c][u] = NT ? __builtin_nontemporal_load(src) : *src;
    }
}

// the wave's activation fragments from row-major x: rows lane & 15 (a0) and 16 + (lane & 15) (a1, H2), clamped to
// M - 1 (rows past M are copies, never stored)
template <int KTM, bool H2>
__device__ __forceinline__ void load_x_frags_rows(const bf16_t* x, int64_t ldx, int M, int kt0, int ktl, int lane,
                                                  bf16x8 (&a0)[KTM], bf16x8 (&a1)[KTM]) {
  const int r0 = min(lane & 15, M - 1), r1 = min(16 + (lane & 15), M - 1), akoff = 8 * (lane >> 4);
#pragma unroll
  for (int u = 0; u < KTM; ++u) {
    const int k = min(kt0 + u, ktl) * 32 + akoff;
    a0[u] = *reinterpret_cast<const bf16x8*>(x + (int64_t)r0 * ldx + k);
    if constexpr (H2) a1[u] = *reinterpret_cast<const bf16x8*>(x + (int64_t)r1 * ldx + k);
  }
}

// ... from fragment-major x (KW_LD_TILED, xt row tiles): a (k-tile, row half) fragment is one contiguous 1-KB piece --
// no row clamp (a missing second tile re-reads the first: its output rows are >= M)
template <int KTM, bool H2>
__device__ __forceinline__ void load_x_frags_tiled(const bf16_t* x, int xt, int kt0, int ktl, int lane,
                                                   bf16x8 (&a0)[KTM], bf16x8 (&a1)[KTM]) {
  const bf16x8* xf = reinterpret_cast<const bf16x8*>(x) + lane;
  const int t1 = xt > 1 ? 64 : 0;
#pragma unroll
  for (int u = 0; u < KTM; ++u) {
    const bf16x8* f = xf + (int64_t)(min(kt0 + u, ktl) * xt) * 64;
    a0[u] = *f;
    if constexpr (H2) a1[u] = f[t1];
  }
}

// MFMA over the wave's k-tiles (raw operand: the LayerNorm is applied in the epilogue); c0 / c1: the two row halves
template <int KTM, int NCB, bool H2>
__device__ __forceinline__ void mfma_tile(const bf16x8 (&a0)[KTM], const bf16x8 (&a1)[KTM], const bf16x8 (&w)[NCB][KTM],
                                          int kt0, int kt1, f32x4 (&c0)[NCB], f32x4 (&c1)[NCB]) {
#pragma unroll
  for (int c = 0; c < NCB; ++c) {
    c0[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    c1[c] = c0[c];
  }
#pragma unroll
  for (int u = 0; u < KTM; ++u) {
    if (kt0 + u < kt1) {
#pragma unroll
      for (int c = 0; c < NCB; ++c) {
        c0[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[u], w[c][u], c0[c], 0, 0, 0);
        if constexpr (H2) c1[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[u], w[c][u], c1[c], 0, 0, 0);
      }
    }
  }
}

// LayerNorm statistics of the tile's rows over the wave's k-tiles, on the matrix cores: X.1 gives the row sums, X.X^T's
// diagonal the row sums of squares (the A fragment of X is also the B fragment of X^T); fixed-order fp32 accumulation.
// Written to the (virtual) wave's slot rp[32][2] = (sum, sum of squares) per row; the waves are summed in order by
// ln_finish_row.
template <int KTM, bool H2>
__device__ __forceinline__ void ln_row_partials(const bf16x8 (&a0)[KTM], const bf16x8 (&a1)[KTM], int kt0, int kt1,
                                                int lane, float (*rp)[2]) {
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0, q0 = s0, q1 = s0;
#pragma unroll
  for (int u = 0; u < KTM; ++u)
    if (kt0 + u < kt1) {
      s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[u], ones, s0, 0, 0, 0);
      if constexpr (H2) s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[u], ones, s1, 0, 0, 0);
      q0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[u], a0[u], q0, 0, 0, 0);
      if constexpr (H2) q1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[u], a1[u], q1, 0, 0, 0);
    }
  // C layout: lane holds rows 4*(lane>>4)+i, column lane&15 (every column of X.1 holds the row sums)
  if ((lane & 15) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rp[4 * (lane >> 4) + i][0] = s0[i];
      if constexpr (H2) rp[16 + 4 * (lane >> 4) + i][0] = s1[i];
    }
  }
  const int di = (lane & 15) - 4 * (lane >> 4);  // diagonal element of this lane, if any
  if (di >= 0 && di < 4) {
    rp[lane & 15][1] = q0[di];
    if constexpr (H2) rp[16 + (lane & 15)][1] = q1[di];
  }
}

// rstd of a row from its sum of squares (inv = 1 / K)
__device__ __forceinline__ float ln_rstd(float sq, float inv, float mean, float eps) {
  return rsqrtf(fmaxf(sq * inv - mean * mean, 0.f) + eps);
}

// row m's (mean, rstd) into rstat[m]: its nw (virtual) waves' partials summed in wave order.  One row per calling
// lane; the caller keeps its own lane predicate
__device__ __forceinline__ void ln_finish_row(const float (*rpart)[32][2], int nw, int m, int K, float eps,
                                              float (*rstat)[2]) {
  float sx = 0.f, sq = 0.f;
  for (int w2 = 0; w2 < nw; ++w2) {
    sx += rpart[w2][m][0];
    sq += rpart[w2][m][1];
  }
  const float inv = 1.f / (float)K;
  const float mean = sx * inv;
  rstat[m][0] = mean;
  rstat[m][1] = ln_rstd(sq, inv, mean, eps);
}

// LN(x) W'^T = rstd * (x W'^T - mean * colsum(W')): the LayerNorm folded into an accumulator value
__device__ __forceinline__ float ln_fold(float v, float mean, float rstd, float cs) { return rstd * (v - mean * cs); }

}  // namespace
