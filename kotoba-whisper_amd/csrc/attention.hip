// Attention kernels for the Whisper hot path on gfx950.
//
// Encoder (K6): flash-style bf16 attention, non-causal, T = 1500, head_dim 64
// (TF/models/whisper/modeling_whisper.py:284-356 + TF/integrations/sdpa_attention.py:79-166;
// q arrives pre-scaled by head_dim^-0.5 from the QKV epilogue, modeling_whisper.py:309).
//   Per workgroup: one (batch, head, 128-query tile); 4 waves x 32 queries.  Scores are computed
//   TRANSPOSED, S^T = K Q^T (v_mfma_f32_32x32x16_bf16), so each lane owns one query's scores and the
//   row softmax needs only in-lane math plus one lane^32 exchange.  O^T = V^T P^T takes P^T straight
//   from the S^T accumulators (no LDS round trip) and V^T from a row-major V tile through
//   ds_read_b64_tr_b16.  K/V tiles (64 keys) are staged global->LDS by global_load_lds_dwordx4 into a
//   2-deep ring with XOR-swizzled images (K: chunk ^ ((row>>1)&7) for ds_read_b128; V: chunk ^
//   (((row>>1)&1)<<2) for the transposed reads) -- both conflict-free.  O is normalised and staged
//   through LDS for 16-B coalesced stores.
// Encoder f32 path: exact-fp32 reference-order kernel for the parity mode.
// Decoder self-attention (K10): static KV cache append + attention; one new position per row splits
//   the keys into <= 256-key chunks like the cross-attention (prefill, q_len > 1: one workgroup per
//   (b, h) walking the queries).  kw_self_attn_step_masked: the same with a per-row first key (left-padded
//   prompts of a conditioned long-form pass).  Its kernels are thin entries over the unmasked kernels' code:
//   self_attn_step1_masked is self_step1_body with the chunks starting at the row's first key,
//   self_attn_prefill_masked (f32) is self_attn_step's per-query work (self_attend_query) with one workgroup
//   per (b, h, query position), so a prompt of ~228 positions runs side by side.  Only
//   self_attn_prefill_masked_mfma is code of its own (bf16: one wave per 16 query positions, S^T = K Q^T and
//   O^T = V^T P^T on v_mfma_f32_16x16x32_bf16 over 32-key tiles).
// Decoder cross-attention (K11): split-S partial softmax over cached encoder K/V in <= 256-key chunks,
//   8 lanes per key row so every K and V load is a coalesced 1-KB wave access, and every load of the
//   chunk (64 KB) issued before the first score; the last-arriving chunk combines the partials in the
//   same launch (write-through partials + arrival counter, MI355X_MICROARCH "Valid forms" row 1).
#include <math.h>
#include <stdio.h>

#include <type_traits>

#include "attn_common.h"
#include "decproj.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(2))) unsigned int v2u32;
typedef __attribute__((ext_vector_type(4))) unsigned int v4u32;

namespace {

// lane ^ 32 reductions by v_permlane32_swap (a VALU half-exchange; no LDS round trip like ds_bpermute):
// with both operands = v, one result holds the lane's own value and the other its partner's
__device__ __forceinline__ float xor32_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xor32_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ------------------------------------------------------------------------------------------------
// encoder flash attention, bf16
// ------------------------------------------------------------------------------------------------
constexpr int AQ = 128;        // queries per workgroup
constexpr int AK = 64;         // keys per tile
constexpr int TILE_BYTES = AK * HD * 2;  // 8 KB
constexpr int ATT_LDS = 2 * 2 * TILE_BYTES;  // K,V x 2 stages = 32 KB (O staging reuses it)

__global__ __launch_bounds__(256, 2) void attn_fwd_bf16(const bf16_t* __restrict__ qkv, int B, int H, int T,
                                                       bf16_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) char smem[ATT_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_qt = (T + AQ - 1) / AQ;
  const int bh = blockIdx.x / n_qt;
  const int qt = blockIdx.x - bh * n_qt;
  const int b = bh / H, h = bh - (bh / H) * H;
  const int64_t head_elems = (int64_t)T * HD;
  const bf16_t* Q = qkv + ((int64_t)(0 * B + b) * H + h) * head_elems;
  const bf16_t* K = qkv + ((int64_t)(1 * B + b) * H + h) * head_elems;
  const bf16_t* V = qkv + ((int64_t)(2 * B + b) * H + h) * head_elems;

  const int q_lane = qt * AQ + wave * 32 + (lane & 31);
  const int hh = lane >> 5;
  // Q fragments (B operand of S^T = K Q^T): lane holds Q[q][16s + 8h .. +7]
  bf16x8 qf[4];
  {
    const int qr = min(q_lane, T - 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(Q + (int64_t)qr * HD + 16 * s + 8 * hh);
  }

  // staging: each tile (64 rows x 128 B) = 8 glds instructions; wave w issues rows [16w, 16w+16)
  const int n_kt = (T + AK - 1) / AK;
  auto stage = [&](int s, int kt) {
    char* kb = smem + s * 2 * TILE_BYTES;
    char* vb = kb + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int g = wave * 2 + i;  // 8-row group
      const int row = 8 * g + (lane >> 3);
      const int key = min(kt * AK + row, T - 1);
      const int slot = lane & 7;
      const int ck = slot ^ ((row >> 1) & 7);
      const int cv = slot ^ (((row >> 1) & 1) << 2);
      glds16(K + (int64_t)key * HD + ck * 8, kb + g * 1024);
      glds16(V + (int64_t)key * HD + cv * 8, vb + g * 1024);
    }
  };

  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  stage(0, 0);
  for (int kt = 0; kt < n_kt; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < n_kt) stage((kt + 1) & 1, kt + 1);
    const char* kb = smem + (kt & 1) * 2 * TILE_BYTES;
    const char* vb = kb + TILE_BYTES;

    // S^T for 2 key blocks of 32
    f32x16 st[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[i][r] = 0.f;
      const int row = i * 32 + (lane & 31);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int c = 2 * s + hh;
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kb + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
        st[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st[i], 0, 0, 0);
      }
    }
    // mask keys >= T (last tile only), row max
    const int key0 = kt * AK;
    if (key0 + AK > T) {  // ragged last tile only
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          if (key >= T) st[i][r] = -INFINITY;
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[i][r]);
    mx = xor32_max(mx);
    float rs = 0.f;
    bf16x8 pf[2][2];
    {
      // deferred rescale: the exponent reference m_run only moves when a score exceeds it by more than
      // 8 (p <= e^8, exact in f32 and in bf16's range); most tiles skip the O / l rescale entirely
      const bool bump = mx > m_run + 8.0f;
      if (__builtin_amdgcn_ballot_w64(bump)) {
        const float m_new = bump ? mx : m_run;
        const float alpha = bump ? __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E) : 1.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
        l_run *= alpha;
        m_run = m_new;
      }
      const float mneg = -m_run * LOG2E;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            // raw v_exp_f32: arguments are <= 8 * log2(e) and very negative ones may flush to 0
            const float p = __builtin_amdgcn_exp2f(fmaf(st[i][8 * s + e], LOG2E, mneg));
            rs += p;
            pf[i][s][e] = (__bf16)p;
          }
    }
    l_run += xor32_sum(rs);

    // O^T += V^T P^T ; A operand via ds_read_b64_tr_b16 from the row-major V tile.  The transposed
    // reads are inline asm: as builtins the compiler cannot tell the V image from the next tile's
    // in-flight LDS-DMA and puts an s_waitcnt vmcnt(0) (wait for the prefetch) in front of them.
    // Step n = (key block i, 16-key step s) reads 4 pieces; step n+1's reads are issued before step
    // n's MFMAs (counted lgkmcnt).
    const int li = lane & 15, qq = li >> 2, pp = li & 3, grp = (lane >> 4) & 1;
    auto vread = [&](int n, v2u32 (&t)[2][2]) {
      const int i = n >> 1, s = n & 1;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int row = i * 32 + 16 * s + 8 * half + 4 * hh + qq;
          const int chunk = db * 4 + 2 * grp + (pp >> 1);
          const int off = row * 128 + ((chunk ^ (((row >> 1) & 1) << 2)) << 4) + (pp & 1) * 8;
          asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(t[db][half]) : "v"(lds_u32(vb + off)));
        }
    };
    v2u32 vt[2][2][2];
    vread(0, vt[0]);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      if (n + 1 < 4) {
        vread(n + 1, vt[(n + 1) & 1]);
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(vt[n & 1][0][0]), "+v"(vt[n & 1][0][1]), "+v"(vt[n & 1][1][0]),
                     "+v"(vt[n & 1][1][1]));
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vt[n & 1][0][0]), "+v"(vt[n & 1][0][1]), "+v"(vt[n & 1][1][0]),
                     "+v"(vt[n & 1][1][1]));
      }
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const v4u32 w = {vt[n & 1][db][0][0], vt[n & 1][db][0][1], vt[n & 1][db][1][0], vt[n & 1][db][1][1]};
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), pf[n >> 1][n & 1], o[db], 0, 0, 0);
      }
    }
  }

  // normalise and stage O (q rows x 64 hd, bf16) through LDS for coalesced stores
  __syncthreads();
  bf16_t* os = reinterpret_cast<bf16_t*>(smem) + wave * 32 * HD;  // 4 KB per wave
  const float inv_l = 1.0f / l_run;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      os[(lane & 31) * HD + d] = f2bf(o[db][r] * inv_l);
    }
  __syncthreads();
  // each wave writes its 32 rows x 128 B: 256 16-B chunks, 4 per lane
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int chunk = i * 64 + lane;
    const int qr = chunk >> 3, cc = chunk & 7;
    const int q = qt * AQ + wave * 32 + qr;
    if (q < T) {
      const uint4 v = *reinterpret_cast<const uint4*>(os + qr * HD + cc * 8);
      *reinterpret_cast<uint4*>(out + ((int64_t)b * T + q) * (H * HD) + h * HD + cc * 8) = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Encoder attention with log2-unit q (the bf16 engine, kw_attention's KW_ATTN_Q_LOG2).  q carries log2(e) too
// (folded into the QKV GEMM epilogue's q scale: one bf16 rounding as before) and the matrix cores subtract the
// running reference: a fifth k-step per 32-key block multiplies K~ = (1, 1, 0, ...) by Q~ = (hi, lo, 0, ...) with
// hi + lo = -m_run (two bf16 terms: exact to 2^-16 of m_run), so the MFMA output is already the exponent and
// p = exp2(s) is ONE v_exp per score.  The reference moves only when a score exceeds it by more than 8 / ln 2
// (p <= e^8), then that tile is shifted once more and O / l rescaled.  The kernel is vector-issue-bound (18 MFMAs
// per 64-key tile beside 32 v_exp, the row sums and the bf16 packing), so the tile does nothing else:
//  * no row maximum on the common path: the tile's p = exp2(s) and row sums are computed straight away; only a
//    wave in which some lane's sum exceeds 2980 (< e^8 = 2^11.5415602: a lane whose maximum would move the
//    reference has a p, hence a sum, above it; NaN takes the branch too) computes the maxima, moves the
//    reference and recomputes the tile (its scores again from the same LDS image: bitwise) -- every lane ends
//    with the p of the always-compute-the-maximum order (r03x: bitwise equal to that kernel on every shape
//    tested, 405 vs 460 us per launch at large-v3 B = 32, tools/lab/enc_attn_l2_ab.py);
//  * the two ring stages as static parities (the loop unrolled by two): every LDS fragment read is a lane base
//    plus an immediate offset;
//  * K / V tiles by buffer_load ... lds from per-head buffer descriptors (base and size in SGPRs, advanced per
//    tile on the scalar unit): no per-tile address arithmetic, and rows past T read as zeros (the ragged last
//    tile's scores there are masked to -inf; their V rows enter as 0 * 0).
// (Row sums as P.1 on the matrix cores: 143 registers, 3 waves per SIMD, slower -- profiles/r03_lab_notes.md)
template <int N_, int PAR>  // one 16-key step of the P.V product: V^T fragments by transposed reads at immediates
__device__ __forceinline__ void attn_vread(uint32_t b0, uint32_t b1, v2u32 (&t)[2][2]) {
  constexpr int i = N_ >> 1, s = N_ & 1;
  constexpr int o0 = PAR * 2 * TILE_BYTES + TILE_BYTES + (i * 32 + 16 * s) * 128;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t[0][0]) : "v"(b0), "i"(o0));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t[0][1]) : "v"(b0), "i"(o0 + 8 * 128));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t[1][0]) : "v"(b1), "i"(o0));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t[1][1]) : "v"(b1), "i"(o0 + 8 * 128));
}

__global__ __launch_bounds__(256, 4) void attn_fwd_l2(const bf16_t* __restrict__ qkv, int B, int H, int T,
                                                      bf16_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) char smem[ATT_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_qt = (T + AQ - 1) / AQ;
  const int bh = blockIdx.x / n_qt;
  const int qt = blockIdx.x - bh * n_qt;
  const int b = bh / H, h = bh - (bh / H) * H;
  const int64_t head_elems = (int64_t)T * HD;
  const bf16_t* Q = qkv + ((int64_t)(0 * B + b) * H + h) * head_elems;
  const bf16_t* K = qkv + ((int64_t)(1 * B + b) * H + h) * head_elems;
  const bf16_t* V = qkv + ((int64_t)(2 * B + b) * H + h) * head_elems;

  const int q_lane = qt * AQ + wave * 32 + (lane & 31);
  const int hh = lane >> 5;
  bf16x8 qf[4];
  {
    const int qr = min(q_lane, T - 1);
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(Q + (int64_t)qr * HD + 16 * s + 8 * hh);
  }

  // staging (attn_fwd_bf16's image): wave w moves rows [16w, 16w + 16) of each tile, lane = (row, 16-B slot)
  uint32_t voff_k[2], voff_v[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = 8 * (wave * 2 + i) + (lane >> 3);
    const int slot = lane & 7;
    voff_k[i] = (uint32_t)(row * HD + (slot ^ ((row >> 1) & 7)) * 8) * 2;
    voff_v[i] = (uint32_t)(row * HD + (slot ^ (((row >> 1) & 1) << 2)) * 8) * 2;
  }
  const int n_kt = (T + AK - 1) / AK;
  if (T % AK) {  // rows past T: whatever the DMA leaves there must be finite (their P is 0; 0 * NaN is not)
#pragma unroll
    for (int i = 0; i < ATT_LDS / (256 * 16); ++i)
      *reinterpret_cast<uint4*>(smem + (i * 256 + tid) * 16) = make_uint4(0, 0, 0, 0);
    __syncthreads();
  }
  auto stage = [&](auto par_c, int kt) __attribute__((always_inline)) {
    constexpr int par = decltype(par_c)::value;
    const int nrec = (T - kt * AK) * HD * 2;  // this tile's rows to the head's end: later rows read as 0
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)(K + (int64_t)kt * AK * HD), (short)0, nrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)(V + (int64_t)kt * AK * HD), (short)0, nrec, 0x00020000);
    char* kb = smem + par * 2 * TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int g = wave * 2 + i;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (__attribute__((address_space(3))) void*)(kb + g * 1024), 16, voff_k[i], 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void*)(kb + TILE_BYTES + g * 1024), 16,
                                               voff_v[i], 0, 0, 0);
    }
  };

  // fragment-read lane bases: K rows (lane & 31) + 32 i, 16-B chunk (2 s + hh) ^ ((row >> 1) & 7) per k-step s;
  // V^T by transposed reads, 16-B chunk (db ^ ((qq >> 1) & 1)) * 4 + 2 grp + (pp >> 1) (attn_fwd_bf16's vread)
  const uint32_t sbase = lds_u32(smem);
  uint32_t kofs[4];
  {
    const int r = lane & 31, r7 = (r >> 1) & 7;
#pragma unroll
    for (int s = 0; s < 4; ++s) kofs[s] = (uint32_t)(r * 128 + (((2 * s + hh) ^ r7) << 4));
  }
  uint32_t vb0, vb1;
  {
    const int li = lane & 15, qq = li >> 2, pp = li & 3, grp = (lane >> 4) & 1, x = (qq >> 1) & 1;
    const uint32_t lanepart = (uint32_t)((4 * hh + qq) * 128 + (2 * grp + (pp >> 1)) * 16 + (pp & 1) * 8);
    vb0 = sbase + lanepart + (uint32_t)((0 ^ x) * 64);
    vb1 = sbase + lanepart + (uint32_t)((1 ^ x) * 64);
  }

  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = 0.f, l_run = 0.f;
  bf16x8 kone, qref;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    kone[e] = (__bf16)((hh == 0 && e < 2) ? 1.0f : 0.0f);
    qref[e] = (__bf16)0.0f;
  }

  auto tile = [&](auto par_c, auto first_c, int kt) __attribute__((always_inline)) {
    constexpr int par = decltype(par_c)::value;
    constexpr bool first = decltype(first_c)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < n_kt) stage(std::integral_constant<int, 1 - par>{}, kt + 1);
    const char* kb = smem + par * 2 * TILE_BYTES;

    // S^T for 2 key blocks of 32 (log2 units, minus the reference), keys >= T masked in the ragged last tile
    f32x16 st[2];
    auto scores = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[i][r] = 0.f;
        st[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kone, qref, st[i], 0, 0, 0);  // -m_run
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kb + i * 32 * 128 + kofs[s]);
          st[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st[i], 0, 0, 0);
        }
      }
      const int key0 = kt * AK;
      if (key0 + AK > T) {  // ragged last tile only
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = key0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (key >= T) st[i][r] = -INFINITY;
          }
      }
    };
    scores();
    float rs;
    bf16x8 pf[2][2];
    auto expsum = [&]() __attribute__((always_inline)) {
      rs = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float p = __builtin_amdgcn_exp2f(st[i][8 * s + e]);
            rs += p;
            pf[i][s][e] = (__bf16)p;
          }
    };
    // the reference move: only where a score exceeds the reference by more than 8 / ln 2
    auto rebase = [&]() __attribute__((always_inline)) {
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[i][r]);
      mx = xor32_max(mx);
      const bool bump = first || mx > 11.5415602f;
      if (__builtin_amdgcn_ballot_w64(bump)) {
        const float d = bump ? mx : 0.f;
        const float alpha = (bump && !first) ? __builtin_amdgcn_exp2f(-d) : 1.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            o[i][r] *= alpha;
            st[i][r] -= d;
          }
        l_run *= alpha;
        m_run += d;
        const float nm = -m_run;
        const __bf16 hi = (__bf16)nm;
        const __bf16 lo = (__bf16)(nm - (float)hi);
        qref[0] = hh == 0 ? hi : (__bf16)0.0f;
        qref[1] = hh == 0 ? lo : (__bf16)0.0f;
      }
    };
    if constexpr (first) {
      rebase();
      expsum();
    } else {
      expsum();
      if (__builtin_amdgcn_ballot_w64(!(rs <= 2980.0f))) {  // rare: some lane may move its reference
        // the scores again (the same MFMAs on the same LDS image: bitwise), so st need not stay live through the
        // common path (opaque operands: the compiler would otherwise keep the first st instead)
        asm volatile("" : "+v"(qref), "+v"(kone)::"memory");
        scores();
        rebase();
        expsum();
      }
    }
    l_run += xor32_sum(rs);

    // O^T += V^T P^T (attn_fwd_bf16's order): step n + 1's transposed reads issued before step n's MFMAs
    v2u32 vt[2][2][2];
    attn_vread<0, par>(vb0, vb1, vt[0]);
    auto pv = [&](auto n_c) __attribute__((always_inline)) {
      constexpr int n = decltype(n_c)::value;
      if constexpr (n + 1 < 4) {
        attn_vread<n + 1, par>(vb0, vb1, vt[(n + 1) & 1]);
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(vt[n & 1][0][0]), "+v"(vt[n & 1][0][1]), "+v"(vt[n & 1][1][0]),
                     "+v"(vt[n & 1][1][1]));
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vt[n & 1][0][0]), "+v"(vt[n & 1][0][1]), "+v"(vt[n & 1][1][0]),
                     "+v"(vt[n & 1][1][1]));
      }
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const v4u32 w = {vt[n & 1][db][0][0], vt[n & 1][db][0][1], vt[n & 1][db][1][0], vt[n & 1][db][1][1]};
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), pf[n >> 1][n & 1], o[db], 0, 0, 0);
      }
    };
    pv(std::integral_constant<int, 0>{});
    pv(std::integral_constant<int, 1>{});
    pv(std::integral_constant<int, 2>{});
    pv(std::integral_constant<int, 3>{});
  };

  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using F = std::integral_constant<bool, false>;
  stage(P0{}, 0);
  tile(P0{}, std::integral_constant<bool, true>{}, 0);
  int kt = 1;
  for (; kt + 1 < n_kt; kt += 2) {
    tile(P1{}, F{}, kt);
    tile(P0{}, F{}, kt + 1);
  }
  if (kt < n_kt) tile(P1{}, F{}, kt);

  // normalise and stage O (q rows x 64 hd, bf16) through LDS for coalesced stores
  __syncthreads();
  bf16_t* os = reinterpret_cast<bf16_t*>(smem) + wave * 32 * HD;  // 4 KB per wave
  const float inv_l = 1.0f / l_run;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      os[(lane & 31) * HD + d] = f2bf(o[db][r] * inv_l);
    }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int chunk = i * 64 + lane;
    const int qr = chunk >> 3, cc = chunk & 7;
    const int q = qt * AQ + wave * 32 + qr;
    if (q < T) {
      const uint4 v = *reinterpret_cast<const uint4*>(os + qr * HD + cc * 8);
      *reinterpret_cast<uint4*>(out + ((int64_t)b * T + q) * (H * HD) + h * HD + cc * 8) = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// encoder attention, f32 (parity mode): 4 waves = 4 queries share K/V tiles in LDS
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_fwd_f32(const float* __restrict__ qkv, int B, int H, int T,
                                                   float* __restrict__ out) {
  __shared__ float ks[64][HD + 1];
  __shared__ float vs[64][HD + 1];
  __shared__ float qs[4][HD];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_qb = (T + 3) / 4;
  const int bh = blockIdx.x / n_qb, qb = blockIdx.x - bh * n_qb;
  const int b = bh / H, h = bh - (bh / H) * H;
  const int64_t head_elems = (int64_t)T * HD;
  const float* Q = qkv + ((int64_t)(0 * B + b) * H + h) * head_elems;
  const float* K = qkv + ((int64_t)(1 * B + b) * H + h) * head_elems;
  const float* V = qkv + ((int64_t)(2 * B + b) * H + h) * head_elems;
  const int q = qb * 4 + wave;
  qs[wave][lane] = Q[(int64_t)min(q, T - 1) * HD + lane];
  float m = -INFINITY, l = 0.f, acc = 0.f;
  for (int k0 = 0; k0 < T; k0 += 64) {
    __syncthreads();
    for (int i = tid; i < 64 * HD; i += 256) {
      const int r = i >> 6, c = i & 63;
      const int key = min(k0 + r, T - 1);
      ks[r][c] = K[(int64_t)key * HD + c];
      vs[r][c] = V[(int64_t)key * HD + c];
    }
    __syncthreads();
    float s = 0.f;
#pragma unroll 16
    for (int c = 0; c < HD; ++c) s = fmaf(qs[wave][c], ks[lane][c], s);
    if (k0 + lane >= T) s = -INFINITY;
    const float mt = wave_max(s);
    const float mn = fmaxf(m, mt);
    const float alpha = expf(m - mn);
    const float p = expf(s - mn);
    l = l * alpha + wave_sum(p);
    acc *= alpha;
    for (int j = 0; j < 64; ++j) acc = fmaf(__shfl(p, j, 64), vs[j][lane], acc);
    m = mn;
  }
  if (q < T) out[((int64_t)b * T + q) * (H * HD) + h * HD + lane] = acc / l;
}

// ------------------------------------------------------------------------------------------------
// decoder attention helpers: 8 lanes per 64-wide key/value row (16-B loads, 1-KB wave accesses)
// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void load8(const T* p, float v[8]);
template <>
__device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float v[8]) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
template <>
__device__ __forceinline__ void load8<float>(const float* p, float v[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <typename T>
__device__ __forceinline__ void copy8(T* dst, const T* src) {
  if constexpr (sizeof(T) == 2) {
    *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
  } else {
    reinterpret_cast<float4*>(dst)[0] = reinterpret_cast<const float4*>(src)[0];
    reinterpret_cast<float4*>(dst)[1] = reinterpret_cast<const float4*>(src)[1];
  }
}

// Softmax-weighted sum over keys [k0, k1) for one query (block of 256 threads = 32 key slots x 8 lanes).
// kp(k)/vp(k) give the row pointers.  Returns (via LDS) m, l and o[64] (unnormalised) to thread 0..63.
template <typename T, typename KP, typename VP>
__device__ __forceinline__ void attend_rows(const float qv[8], int k0, int k1, KP kp, VP vp, float* sc,
                                            float (*red)[65], float* stat, float& m_out, float& l_out,
                                            float& o_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = lane & 7, kslot = wave * 8 + (lane >> 3);
  float mx = -INFINITY;
  // 4 rows per lane group in flight (addresses clamped, results masked: loads stay unconditional)
  for (int kb = k0 + kslot; kb < k1; kb += 128) {
    float kv[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j) load8<T>(kp(min(kb + 32 * j, k1 - 1)) + sub * 8, kv[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = fmaf(qv[i], kv[j][i], s);
      s = kw_sum8(s);
      const int k = kb + 32 * j;
      if (k < k1) {
        if (sub == 0) sc[k - k0] = s;
        mx = fmaxf(mx, s);
      }
    }
  }
  mx = wave_max(mx);
  if (lane == 0) stat[wave] = mx;
  __syncthreads();
  const float m = fmaxf(fmaxf(stat[0], stat[1]), fmaxf(stat[2], stat[3]));
  float sum = 0.f;
  for (int k = tid; k < k1 - k0; k += 256) {
    const float e = expf(sc[k] - m);
    sc[k] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) stat[4 + wave] = sum;
  __syncthreads();
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int kb = k0 + kslot; kb < k1; kb += 128) {
    float vv[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j) load8<T>(vp(min(kb + 32 * j, k1 - 1)) + sub * 8, vv[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kb + 32 * j;
      const float pk = k < k1 ? sc[k - k0] : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(pk, k < k1 ? vv[j][i] : 0.f, acc[i]);  // (stale masked rows)
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[kslot][sub * 8 + i] = acc[i];
  __syncthreads();
  m_out = m;
  l_out = (stat[4] + stat[5]) + (stat[6] + stat[7]);
  float o = 0.f;
  if (tid < HD)
    for (int s2 = 0; s2 < 32; ++s2) o += red[s2][tid];
  o_out = o;
}

// ------------------------------------------------------------------------------------------------
// Single-query attention over one chunk of <= 256 keys, every K and V load in flight at once
// (256 threads = 32 key slots x 8 lanes; lane (slot, sub) holds 16 B of rows slot, slot+32, ...).
// Returns the chunk's (m, l) to every thread and the unnormalised o[tid] to threads 0..63.
// ------------------------------------------------------------------------------------------------
template <typename T, typename KP, typename VP>
__device__ __forceinline__ void attend_chunk(const float qv[8], int k0, int k1, KP kp, VP vp, float (*red)[64],
                                             float* stat, float& m_out, float& l_out, float& o_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = lane & 7, slot = wave * 8 + (lane >> 3);
  Row8<T> kr[8], vr[8];
  // key groups j past the chunk (k0 + 32j >= k1: workgroup-uniform, e.g. the short self-attention chunks of
  // early decode steps) load nothing, and every use of their registers sits behind the same uniform test
  // (no zero fill: a phi of loaded and zeroed registers made the compiler copy a pending load register and
  // wait vmcnt(0) after the second row load).  kp(k, j) / vp(k, j) must not load either: an address that
  // waits on a load costs a vmcnt(0) per row.  Skipped groups contributed p = 0 before: same results.
  auto act = [&](int j) { return k0 + 32 * j < k1; };
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (act(j)) kr[j] = ld_row8<T>(kp(min(k0 + slot + 32 * j, k1 - 1), j) + sub * 8);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (act(j)) vr[j] = ld_row8<T>(vp(min(k0 + slot + 32 * j, k1 - 1), j) + sub * 8);
  if constexpr (sizeof(T) == 2) {
    float ql[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ql[i] = qv[i] * LOG2E;
    u32x4 k4[8], v4[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      k4[j] = kr[j].u[0];
      v4[j] = vr[j].u[0];
    }
    int nj = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) nj += act(j) ? 1 : 0;
    float mw, lw, acc[8];
    wave_row_bf16(ql, k4, v4, k0, k1, slot, nj, mw, lw, acc);
    if (lane < 8) {
#pragma unroll
      for (int i = 0; i < 8; ++i) red[wave][lane * 8 + i] = acc[i];
    }
    if (lane == 0) {
      stat[wave] = mw;
      stat[4 + wave] = lw;
    }
    __syncthreads();
    merge_waves_bf16(stat, red, tid, m_out, l_out, o_out);
    return;
  }
  float sc[8];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = -INFINITY;
    if (act(j)) {
      float kv[8];
      unpack8<T>(kr[j], kv);
      float sj = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) sj = fmaf(qv[i], kv[i], sj);
      sj = kw_sum8(sj);
      sc[j] = (k0 + slot + 32 * j < k1) ? sj : -INFINITY;
      mx = fmaxf(mx, sc[j]);
    }
  }
  mx = wave_max(mx);
  if (lane == 0) stat[wave] = mx;
  __syncthreads();
  const float m = fmaxf(fmaxf(stat[0], stat[1]), fmaxf(stat[2], stat[3]));
  float lsum = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (act(j)) {
      const bool valid = k0 + slot + 32 * j < k1;
      const float pj = valid ? expf(sc[j] - m) : 0.f;
      lsum += pj;
      float vv[8];
      unpack8<T>(vr[j], vv);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(pj, valid ? vv[i] : 0.f, acc[i]);  // (stale masked rows: see wave_values_bf16)
    }
  }
  // lanes of one wave with equal sub hold the same dims: reduce over lane bits 3..5
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    acc[i] = kw_sum_hi(acc[i]);
  }
  lsum = wave_sum(lsum) * 0.125f;  // every row's p was counted by its 8 lanes (exact: power of two)
  if (lane < 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) red[wave][lane * 8 + i] = acc[i];
  }
  if (lane == 0) stat[4 + wave] = lsum;
  __syncthreads();
  m_out = m;
  l_out = (stat[4] + stat[5]) + (stat[6] + stat[7]);
  o_out = tid < HD ? (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]) : 0.f;
}

// Combine of per-chunk partials (m, l, o[64]) published write-through by each chunk's workgroup; the
// last arriver (arrival counter) merges them in chunk order and writes the normalised output row.
template <typename T>
__device__ __forceinline__ void publish_and_combine(float* part, int* cnt, int ns, int split, float m, float l, float o,
                                                    T* out_row, int* last_flag) {
  const int tid = threadIdx.x;
  float* w = part + (int64_t)split * (HD + 2);
  if (tid < HD) __hip_atomic_store(w + 2 + tid, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) {
    __hip_atomic_store(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(w + 1, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int prev = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *last_flag = prev == ns - 1;
    if (prev == ns - 1) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!*last_flag || tid >= HD) return;
  constexpr int NSMAX = 8;
  float ms[NSMAX], ls[NSMAX], os[NSMAX];
#pragma unroll
  for (int q = 0; q < NSMAX; ++q) {
    if (q < ns) {
      ms[q] = __hip_atomic_load(part + q * (HD + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ls[q] = __hip_atomic_load(part + q * (HD + 2) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      os[q] = __hip_atomic_load(part + q * (HD + 2) + 2 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  float M = -INFINITY;
#pragma unroll
  for (int q = 0; q < NSMAX; ++q)
    if (q < ns) M = fmaxf(M, ms[q]);
  float lt = 0.f, ot = 0.f;
#pragma unroll
  for (int q = 0; q < NSMAX; ++q)
    if (q < ns) {
      const float f = chunk_scale<T>(ms[q] - M);
      lt = fmaf(ls[q], f, lt);
      ot = fmaf(os[q], f, ot);
    }
  TypeIO<T>::st(out_row + tid, ot / lt);
}
// Chunk-partial hand-off of the bf16 one-row cross-attention (cross_attn_dma_kernel, xq_cross_kernel) through
// 8-byte {data, tag} granules (MI355X_MICROARCH price list, handoff-1to1: one sc1 store each, sc1 polls, untorn),
// per WAVE: a non-final chunk's waves each publish their own (m_w, l_w, acc_w[64]) -- no barrier, no store
// drain, no counter -- and leave.  The final chunk (dispatched after the others) folds, wave by wave and in
// chunk order, every chunk's partial of that wave with fold_begin / fold_value, then merges the four waves with
// merge_waves_bf16: exactly what cross_attn_row_kernel's waves compute as they stream, so a row's output is
// bitwise the same whichever kernel the batch size selects.  Granules [ns - 1][4 waves][66]; each is re-armed
// (tag 0) by its single consumer.  A poll that outlasts XG_SPIN_LIMIT rounds (a protocol failure, never
// expected) raises the error word and writes NaN, so the failure is loud.
__device__ __forceinline__ void wave_partials_combine(unsigned long long* gr, int ns, int split, float mw, float lw,
                                                      const float (&acc)[8], float (*red)[64], float* stat,
                                                      bf16_t* out_el, int* err) {  // out_el: lane's element (dim tid & 63)
  constexpr int G = HD + 2, NSMAX = 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (lane < 8) {  // the wave's partial of dim d = lane*8 + i, read back by lane d of the same wave (in order)
#pragma unroll
    for (int i = 0; i < 8; ++i) red[wave][lane * 8 + i] = acc[i];
  }
  if (split != ns - 1) {  // one contiguous 512-B granule store per wave (whole lines: no partial write-through)
    unsigned long long* w = gr + ((int64_t)split * 4 + wave) * G;
    put_granule(w + 2 + lane, red[wave][lane]);
    if (lane == 0) {
      put_granule(w, mw);
      put_granule(w + 1, lw);
    }
    return;
  }
  // lane d of wave w: every earlier chunk's (m, l, acc[d]) of wave w in flight at once (indices clamped: the
  // loads are unconditional, one round trip), then one check
  float ms[NSMAX - 1], ls[NSMAX - 1], as[NSMAX - 1];
  bool bad = false;
  for (int it = 0; ns > 1; ++it) {
    unsigned long long x[3 * (NSMAX - 1)];
#pragma unroll
    for (int q = 0; q < NSMAX - 1; ++q) {
      const unsigned long long* gq = gr + ((int64_t)min(q, ns - 2) * 4 + wave) * G;
      x[3 * q] = peek_granule(gq);
      x[3 * q + 1] = peek_granule(gq + 1);
      x[3 * q + 2] = peek_granule(gq + 2 + lane);
    }
    bool ready = true;
#pragma unroll
    for (int i = 0; i < 3 * (NSMAX - 1); ++i) ready = ready && (x[i] >> 32) == 1ull;
    if (ready || it >= XG_SPIN_LIMIT) {
      bad = !ready;
#pragma unroll
      for (int q = 0; q < NSMAX - 1; ++q) {
        ms[q] = ready ? __uint_as_float((uint32_t)x[3 * q]) : __uint_as_float(0x7fc00000u);
        ls[q] = __uint_as_float((uint32_t)x[3 * q + 1]);
        as[q] = __uint_as_float((uint32_t)x[3 * q + 2]);
      }
      break;
    }
    __builtin_amdgcn_s_sleep(KW_POLL_SLEEP);
  }
  float M = -INFINITY, Lr = 0.f, A = 0.f;
#pragma unroll
  for (int q = 0; q < NSMAX; ++q) {
    if (q >= ns) break;
    float f0 = 0.f, f1 = 0.f;
    const bool own = q == ns - 1;
    const float a = own ? red[wave][lane] : as[q < NSMAX - 1 ? q : 0];
    const int mode = own ? fold_begin(mw, lw, M, Lr, f0, f1) : fold_begin(ms[q < NSMAX - 1 ? q : 0],
                                                                          ls[q < NSMAX - 1 ? q : 0], M, Lr, f0, f1);
    A = fold_value(mode, A, a, f0, f1);
  }
  if (bad) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // re-arm for the next launch: every value above was consumed by this lane (data dependence)
#pragma unroll
  for (int q = 0; q < NSMAX - 1; ++q)
    if (q < ns - 1) {
      unsigned long long* gq = gr + ((int64_t)q * 4 + wave) * G;
      __hip_atomic_store(gq + 2 + lane, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 0) {
        __hip_atomic_store(gq, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(gq + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  __syncthreads();  // every wave has read its own red[] row: reuse red / stat for the folded partials
  red[wave][lane] = A;
  if (lane == 0) {
    stat[wave] = M;
    stat[4 + wave] = Lr;
  }
  __syncthreads();
  if (tid < HD) {
    float m, l, o;
    merge_waves_bf16(stat, red, tid, m, l, o);
    TypeIO<bf16_t>::st(out_el, o / l);
  }
}

// ------------------------------------------------------------------------------------------------
// decoder self-attention: append to the static cache, then causal attention (q_len >= 1).
// New keys/values are read from the qkv rows themselves (never read back from the cache in the
// same launch).
// ------------------------------------------------------------------------------------------------
// the append of one new position of (b, h), qkv row qrow (its q; k at + d, v at + 2 d), cache row pos: thread
// c8 < 8 copies 16 B of its k and of its v
template <typename T>
__device__ __forceinline__ void self_append_row(const T* qrow, int d, int c8, T* kb, T* vb, int pos) {
  const T* row = qrow + c8 * 8;
  copy8<T>(kb + (int64_t)pos * HD + c8 * 8, row + d);
  copy8<T>(vb + (int64_t)pos * HD + c8 * 8, row + 2 * d);
}

// One query position of (b, h) by the whole workgroup, when the launch's q_len new positions start at p0: the
// query in qkv row qrow attends the keys [k_begin, k_end) -- cache rows (kb, vb) below p0, the launch's own qkv
// rows from p0 -- in attend_rows' order, and the normalised row goes to orow() (formed at the store).
template <typename T, typename OutRow>
__device__ __forceinline__ void self_attend_query(const T* qkv, int q_len, int d, int b, int h, const T* qrow, OutRow orow,
                                                  const T* kb, const T* vb, int p0, int k_begin, int k_end, float* sc,
                                                  float (*red)[65], float* stat) {
  const int tid = threadIdx.x, sub = tid & 7;
  auto kp = [&](int k) -> const T* {
    return k < p0 ? kb + (int64_t)k * HD : qkv + ((int64_t)b * q_len + (k - p0)) * 3 * d + d + h * HD;
  };
  auto vp = [&](int k) -> const T* {
    return k < p0 ? vb + (int64_t)k * HD : qkv + ((int64_t)b * q_len + (k - p0)) * 3 * d + 2 * d + h * HD;
  };
  float qv[8];
  load8<T>(qrow + sub * 8, qv);
  float m, l, o;
  attend_rows<T>(qv, k_begin, k_end, kp, vp, sc, red, stat, m, l, o);
  if (tid < HD) TypeIO<T>::st(orow() + tid, o / l);
}

template <typename T>
__global__ __launch_bounds__(256) void self_attn_step(const T* __restrict__ qkv, int q_len, int H, T* __restrict__ kc,
                                                      T* __restrict__ vc, int t_max, const int32_t* __restrict__ cur_len,
                                                      T* __restrict__ out) {
  __shared__ float sc[512];
  __shared__ float red[32][65];
  __shared__ float stat[8];
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh - (bh / H) * H;
  const int tid = threadIdx.x;
  const int L = *cur_len;
  const int d = H * HD;
  const int p0 = L - q_len;
  T* kb = kc + ((int64_t)b * H + h) * t_max * HD;
  T* vb = vc + ((int64_t)b * H + h) * t_max * HD;
  auto qrow = [&](int qi) -> const T* { return qkv + ((int64_t)b * q_len + qi) * 3 * d + h * HD; };
  for (int i = tid; i < q_len * 8; i += 256) self_append_row<T>(qrow(i >> 3), d, i & 7, kb, vb, p0 + (i >> 3));
  for (int qi = 0; qi < q_len; ++qi) {
    self_attend_query<T>(
        qkv, q_len, d, b, h, qrow(qi), [&] { return out + ((int64_t)b * q_len + qi) * d + h * HD; }, kb, vb, p0, 0,
        p0 + qi + 1, sc, red, stat);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------
// decoder cross-attention: split-S partial softmax; the last-arriving split of a (row, head) combines
// (arrival counter, agent-scope release/acquire -- placement independent).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void cross_attn_kernel(const T* __restrict__ q, int q_len, int H,
                                                         const T* __restrict__ kc, const T* __restrict__ vc, int S,
                                                         int chunk, float* __restrict__ ws, int* __restrict__ cnt,
                                                         T* __restrict__ out) {
  __shared__ float red[4][64];
  __shared__ float stat[8];
  __shared__ int last;
  const int row = blockIdx.x;  // (b*q_len + qi)*H + h
  const int split = blockIdx.y;
  const int ns = gridDim.y;
  const int h = row % H;
  const int bq = row / H;
  const int b = bq / q_len;
  const int sub = threadIdx.x & 7;
  const int k0 = split * chunk;
  const int k1 = min(S, k0 + chunk);
  const T* kb = kc + ((int64_t)b * H + h) * S * HD;
  const T* vb = vc + ((int64_t)b * H + h) * S * HD;
  float qv[8];
  load8<T>(q + (int64_t)bq * H * HD + h * HD + sub * 8, qv);
  float m, l, o;
  attend_chunk<T>(qv, k0, k1, [&](int k, int) { return kb + (int64_t)k * HD; },
                  [&](int k, int) { return vb + (int64_t)k * HD; }, red, stat, m, l, o);
  T* orow = out + (int64_t)bq * H * HD + h * HD;
  if (ns == 1) {
    if (threadIdx.x < HD) TypeIO<T>::st(orow + threadIdx.x, o / l);
    return;
  }
  publish_and_combine<T>(ws + (int64_t)row * ns * (HD + 2), cnt + row, ns, split, m, l, o, orow, &last);
}

// Cross-attention, bf16, one query row per (row, chunk) workgroup: the chunk grid.  One body, cross_chunk<QG>,
// is the (row, chunk) work of both cross_attn_dma_kernel (the query is a row in memory) and xq_cross_kernel (the
// query is handed over in-launch by projection workgroups); the two kernels only map blockIdx to (row, chunk),
// name the query and the output element, and xq_cross_kernel re-arms its query granules.  So the two compute the
// same bits by construction, and a change to the chunk schedule or the hand-off is made once.
//
// As cross_attn_kernel, but the chunk's K rows arrive by LDS-DMA (global_load_lds_dwordx4, non-temporal) and V by
// register loads (r02: 44.4-44.6 us vs 45.4-45.6 for register loads only, 50.3 with V by LDS-DMA too at 2
// workgroups per CU).  Wave w's DMA instruction j moves keys k0 + 32 j + 8 w + (0..7) (1 KB, lane = (key, 16-B
// piece)) to LDS piece 4 j + w and each lane reads back exactly its own 16 B, so the arithmetic is
// wave_row_bf16's (bitwise the rows of cross_attn_kernel / cross_attn_multi_kernel).  r03 (tools/lab/xa_lab.hip,
// large-v3 B = 32 over 32 distinct layers): the same grid only STREAMING its bytes reaches 38-40 us (6.1-6.5
// TB/s); the softmax work after the loads land costs the rest -- log2-unit scores with per-wave references (no
// mid-chunk barrier) and DPP sums take ~2 us of it, the granule combine (no store drain / counter round trips)
// another ~1 us.
#ifndef KW_XA_DMA
#define KW_XA_DMA 1  // 0: register loads only (cross_attn_kernel)
#endif
constexpr int XA_DMA = KW_XA_DMA;

__device__ __forceinline__ u32x4 lds_rd16(const char* p) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(lds_u32(p)) : "memory");
  return v;
}

// Keys [k0, k1) of one (row, head) pair -- chunk `split` of its ns -- against the pair's query, then the chunk-partial
// hand-off / combine (wave_partials_combine over the pair's granules gr; the last chunk writes out_el(), this lane's
// output element -- a callable, so its address arithmetic stays behind the loads).  kb / vb: the pair's K / V rows;
// kv: 32 KB of LDS for the K pieces.
// The query is `query`: 64 bf16 (!QG), or with QG the pair's 32 {bf16 x 2, tag} granules, which the projection
// workgroups of the same launch publish.  Its loads go out FIRST, then every K piece and V row of the chunk, and
// it is checked once the K pieces have landed: by then the projection (a few us; the first wave of chunks needs
// ~10 us to stream its 64 MB) has published, so the K / V stream never waits on it.
template <bool QG, typename OutEl>
__device__ __forceinline__ void cross_chunk(const void* query, const bf16_t* kb, const bf16_t* vb, int k0, int k1,
                                            unsigned long long* gr, int ns, int split, char* kv, float (*red)[64],
                                            float* stat, OutEl out_el, int* err) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane & 7, slot = wave * 8 + (lane >> 3);
  // inline asm for the query loads: hipcc would otherwise drain every LDS-DMA in flight before their use
  unsigned long long g[4];
  u32x4 qraw;
  const unsigned long long* q4 = reinterpret_cast<const unsigned long long*>(query) + sub * 4;
  if constexpr (QG) {
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("global_load_dwordx2 %0, %1, off sc1" : "=v"(g[i]) : "v"(q4 + i) : "memory");
  } else {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(qraw) : "v"(reinterpret_cast<const bf16_t*>(query) + sub * 8) : "memory");
  }
  // every group j is issued (clamped keys: the host guarantees k1 - k0 > 224, so group 7 has valid keys)
#pragma unroll
  for (int j = 0; j < 8; ++j) glds16_nt(kb + (int64_t)min(k0 + slot + 32 * j, k1 - 1) * HD + sub * 8, kv + (4 * j + wave) * 1024);
  u32x4 vr[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) vr[j] = ld_row8<bf16_t>(vb + (int64_t)min(k0 + slot + 32 * j, k1 - 1) * HD + sub * 8).u[0];
  // q and this wave's K pieces landed (V may fly)
  if constexpr (QG) {
    asm volatile("s_waitcnt vmcnt(8)" : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]) :: "memory");
    qraw = wait_query_granules(q4, g, err);
  } else {
    asm volatile("s_waitcnt vmcnt(8)" : "+v"(qraw) :: "memory");
  }
  float ql[8];
  query_log2(qraw, ql);
  // no barrier: each lane reads back only the 16 B its own DMA wrote, complete at the wave's vmcnt
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  u32x4 kr[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) kr[j] = lds_rd16(kv + (4 * j + wave) * 1024 + lane * 16);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kr[0]), "+v"(kr[1]), "+v"(kr[2]), "+v"(kr[3]), "+v"(kr[4]), "+v"(kr[5]),
               "+v"(kr[6]), "+v"(kr[7]));
  float mw, lw, acc[8];
  wave_row_bf16(ql, kr, vr, k0, k1, slot, 8, mw, lw, acc);
  wave_partials_combine(gr, ns, split, mw, lw, acc, red, stat, out_el(), err);
}

__global__ __launch_bounds__(256) void cross_attn_dma_kernel(const bf16_t* __restrict__ q, int q_len, int H,
                                                             const bf16_t* __restrict__ kc,
                                                             const bf16_t* __restrict__ vc, int S, int chunk,
                                                             unsigned long long* __restrict__ gran, int* __restrict__ err,
                                                             bf16_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) char kv[32 * 1024];
  __shared__ float red[4][64];
  __shared__ float stat[8];
  const int row = blockIdx.x, split = blockIdx.y, ns = gridDim.y;
  const int h = row % H, bq = row / H, b = bq / q_len;
  const int k0 = split * chunk, k1 = min(S, k0 + chunk);
  const int64_t pair = ((int64_t)b * H + h) * S * HD, el = (int64_t)bq * H * HD + h * HD;
  cross_chunk<false>(q + el, kc + pair, vc + pair, k0, k1, gran + (int64_t)row * ns * 4 * (HD + 2), ns, split, kv, red,
                     stat, [&] { return out + el + (threadIdx.x & 63); }, err);
}

// The launch descriptor of the bf16 one-row (q_len 1) cross-attention kernels that take their query either way:
// xq_cross_kernel and cross_attn_row_kernel<QG>.
struct CRP {
  const bf16_t* q;           // [rows][64] (row stride d) when the query is in memory (cross_attn_row_kernel<false>)
  unsigned long long* qg;    // [M][d/2] query granules when the projection runs in the launch
  unsigned long long* gran;  // the chunk grid's chunk-partial granules (xq_cross_kernel)
  const bf16_t* kc;
  const bf16_t* vc;
  int H, d, S, chunk, ns, n_lin;
  int* err;
  bf16_t* out;
  int out_t;  // out fragment-major over out_t row tiles (kw_dec_xq_cross with KW_LD_TILED); 0: row stride d
  ProjArgs proj;  // the query projection (rows M = proj.M), when it runs in the launch
};

// ... over the fp8 cache (cross_attn_row_fp8_kernel): kc / vc hold e4m3 codes, ks / vs one layer's scales
// [items][H][64]; query row r reads item r / q_len
struct CRP8 : CRP {
  const float* ks;
  const float* vs;
  int q_len;
};

// ------------------------------------------------------------------------------------------------
// The cross-attention block's query projection and attention step in ONE launch (bf16 engine, q_len 1):
// the LayerNorm-fused q projection (TF/models/whisper/modeling_whisper.py:483 encoder_attn_layer_norm,
// :309 q * head_dim^-0.5) and the chunk grid's attention over the item's encoder K/V (:323-356) --
// what kw_dec_linear(xq) followed by kw_cross_attn_step computes in two launches, bit for bit (the attention IS
// cross_attn_dma_kernel's code, cross_chunk).
//
//  * workgroups [0, n_lin): the query projection, 16 columns each -- dec_linear's arithmetic on 4 waves
//    (decproj.h: its 8 waves as virtual waves, reduced in the same order), published as 8-byte
//    {bf16 x 2, tag} granules [M][d/2];
//  * workgroups [n_lin, n_lin + M H ns): cross_chunk<true> per (row, chunk) in cross_attn_dma_kernel's dispatch
//    order (every row's chunk 0 first, the combining last chunk last).  The row's last chunk re-arms the row's
//    query granules after its combine (every other chunk of the row has read them: their partials, polled by the
//    combine, depend on them).
// The projection workgroups wait for nothing and lead the dispatch order; a chunk waits only for them and for
// earlier chunks of its row (the combine), so every wait is on work dispatched before it -- resident or
// finished, whatever else shares the GPU (no co-residency assumption).
// Polls are bounded: a timeout raises the error word and the row's output is NaN.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void xq_cross_kernel(CRP p) {
  __shared__ __attribute__((aligned(16))) char kv[32 * 1024];  // K pieces (chunks) / reduction scratch (projection)
  __shared__ float red[4][64];
  __shared__ float stat[8];
  if ((int)blockIdx.x < p.n_lin) {
    proj_publish_granules<false>(p.proj, blockIdx.x, kv, p.qg);
    return;
  }
  const int rows = p.proj.M * p.H;
  const int r = blockIdx.x - p.n_lin;
  const int row = r % rows, split = r / rows, ns = p.ns;
  const int h = row % p.H, b = row / p.H;
  const int tid = threadIdx.x;
  const int k0 = split * p.chunk, k1 = min(p.S, k0 + p.chunk);
  const int64_t pair = ((int64_t)b * p.H + h) * p.S * HD;
  unsigned long long* qg = p.qg + (int64_t)b * (p.d / 2) + h * 32;
  cross_chunk<true>(
      qg, p.kc + pair, p.vc + pair, k0, k1, p.gran + (int64_t)row * ns * 4 * (HD + 2), ns, split, kv, red, stat,
      [&] { return p.out + (p.out_t ? kw_tiled_off(b, h * HD + (tid & 63), p.out_t) : (int64_t)b * p.d + h * HD + (tid & 63)); },
      p.err);
  if (split == ns - 1 && tid < 32)  // re-arm the row's query for the next launch (every chunk has read it)
    __hip_atomic_store(qg + tid, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------
// Cross-attention, bf16, q_len 1, ONE workgroup per (row, head) pair looping over the pair's chunks with the
// next chunk's K / V in flight while the current one is computed -- used when every pair fits on the device
// at once (large-v3 B = 32: 640 workgroups, 3 per CU).  The chunk grid (cross_chunk) streams in rounds: every
// workgroup of a round lands its last byte at about the same time, then computes while the memory system idles
// (tools/lab/xa_lab.hip: the same grid only streaming is 38-40 us, with the softmax 44-46).  Here each wave
// keeps its own running softmax over the pair's chunks (log2-unit scores, wave_row_bf16, merged online with exp2
// rescales); the four waves merge once at the end -- no chunk partials, no combine, no workspace.  With QG the
// query comes from the projection workgroups [0, n_lin) of the launch through the same hand-off as
// xq_cross_kernel's (wait_query_granules) and the pair re-arms the granules after use.

// a chunk's 16-B pieces of the pair's K or V rows (lane: row k0 + slot + 32 j, bytes voff = (slot * 64 + sub * 8) * 2
// of it) through a buffer resource over the pair's S rows: rows past S read as 0 (masked like every row past the
// chunk end), so no per-piece clamp or 64-bit address arithmetic -- one add per piece
template <typename P>  // P: a lane's piece of a row, 16 B of bf16 (u32x4) or 8 B of e4m3 codes (u32x2, voff / k0 in those rows' bytes)
__device__ __forceinline__ void row_issue(__amdgpu_buffer_rsrc_t rs, int k0, uint32_t voff, P (&r)[8]) {
  constexpr int RB = HD * (int)sizeof(P) / 8;  // bytes of a row
  __builtin_amdgcn_sched_barrier(0);  // issue exactly here: the schedule is the point (the compiler would sink these
#pragma unroll                        // loads below the next chunk's arithmetic and wait on them there)
  for (int j = 0; j < 8; ++j) {
    if constexpr (sizeof(P) == 16)
      r[j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + (uint32_t)((k0 + 32 * j) * RB), 0, 2));
    else
      r[j] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, voff + (uint32_t)((k0 + 32 * j) * RB), 0, 2));
  }
  __builtin_amdgcn_sched_barrier(0);
}

// one chunk of the pair: its scores from K (then the caller's next V load goes out, the K registers being dead),
// its values from V, merged into the wave's running (M, Lr, A).  Every chunk holds more than 224 keys (the host's
// row_kernel_fits), so only key group j = 7 can fall past the chunk end.
constexpr int ROW_JV = 7;
template <typename P>
__device__ __forceinline__ void row_fold(float mw, const float (&sc)[8], const P (&vr)[8], int k0, int k1, int slot,
                                         float& M, float& Lr, float (&A)[8]) {
  float lw, acc[8], f0 = 0.f, f1 = 0.f;
  wave_values_bf16<32, ROW_JV>(sc, mw, vr, k0, k1, slot, 8, lw, acc);
  // m_w and l_w come out of full-wave butterflies (commutative adds / maxima: every lane holds the same bits), so
  // lane 0's copy IS the value: read as scalars, (M, Lr) and the fold mode are scalar and the fold is a scalar
  // branch, not eight exec-masked ones per chunk
  const float mu = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, mw)));
  const float lu = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, lw)));
  const int mode = fold_begin(mu, lu, M, Lr, f0, f1);
#pragma unroll
  for (int i = 0; i < 8; ++i) A[i] = fold_value(mode, A[i], acc[i], f0, f1);
}

// The pair kernel's body, for both caches: P = u32x4 pieces over the bf16 cache (CRP, cross_attn_row_kernel), P =
// u32x2 pieces of e4m3 codes over the fp8 cache (CRP8, cross_attn_row_fp8_kernel; what only that cache needs sits
// under `if constexpr (F8)`).  NS chunks per pair (6 for Whisper's 1500 frames): a static schedule, static load counts.
template <bool QG, int NS, typename P, typename Params>
__device__ __forceinline__ void cross_row_pair(const Params p, char* scratch, float (*red)[64], float* stat) {
  constexpr bool F8 = sizeof(P) == 8;
  using El = std::conditional_t<F8, uint8_t, bf16_t>;  // a cache element
  constexpr int EB = sizeof(El);
  if constexpr (QG) {
    if ((int)blockIdx.x < p.n_lin) {
      proj_publish_granules<true>(p.proj, blockIdx.x, scratch, p.qg);
      return;
    }
  }
  const int row = blockIdx.x - (QG ? p.n_lin : 0);
  const int h = row % p.H, b = row / p.H;
  int item = b;  // the K / V (and scales) of query row b: with q_len rows per item, item b / q_len's
  if constexpr (F8) item = b / p.q_len;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = lane & 7, slot = wave * 8 + (lane >> 3);
  const int64_t pair = (int64_t)item * p.H + h;
  const El* kb = reinterpret_cast<const El*>(p.kc) + pair * p.S * HD;
  const El* vb = reinterpret_cast<const El*>(p.vc) + pair * p.S * HD;
  unsigned long long* qg = QG ? p.qg + (int64_t)b * (p.d / 2) + h * 32 : nullptr;
  // the query's loads first (fp8: and the lane's 8 K scales), then the first two chunks' K / V
  unsigned long long g[4];
  u32x4 qraw;
  if constexpr (QG) {
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = peek_granule(qg + sub * 4 + i);
  } else {
    qraw = *reinterpret_cast<const u32x4*>(p.q + (int64_t)b * p.d + h * HD + sub * 8);
  }
  [[maybe_unused]] f32x4 ksc[2];
  if constexpr (F8) {
    const f32x4* ks4 = reinterpret_cast<const f32x4*>(p.ks + pair * HD + sub * 8);
    ksc[0] = ks4[0], ksc[1] = ks4[1];
  }
  constexpr int ns = NS;
  const int chunk = p.chunk, S = p.S;
  const __amdgpu_buffer_rsrc_t rsk = __builtin_amdgcn_make_buffer_rsrc((void*)kb, (short)0, S * HD * EB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsv = __builtin_amdgcn_make_buffer_rsrc((void*)vb, (short)0, S * HD * EB, 0x00020000);
  const uint32_t voff = (uint32_t)((slot * HD + sub * 8) * EB);
  // three sets of 8 pieces (32 registers each for bf16, 16 for fp8) in rotation: chunk c + 1's K goes out before
  // chunk c's scores, its V right after them (into chunk c's dead K registers), chunk c + 2's K after chunk c's
  // values (into its dead V registers) -- one chunk in flight while one is computed, 96 K / V registers live (bf16).
  // Five sets with two chunks in flight (fp8: the registers are there) measured no faster -- 29.2 against 28.9 us per
  // launch, profiles/fp8_cross_kbench.txt -- so the bytes in flight do not bound this kernel.
  P r0[8], r1[8], r2[8];
  row_issue(rsk, 0, voff, r0);
  row_issue(rsv, 0, voff, r1);
  if (ns > 1) row_issue(rsk, chunk, voff, r2);
  if constexpr (QG) qraw = wait_query_granules(qg + sub * 4, g, p.err);
  float ql[8];
  query_log2(qraw, ql);
  if constexpr (F8) {  // the pair's K scales multiply the query once, before the first score
#pragma unroll
    for (int i = 0; i < 8; ++i) ql[i] *= ksc[i >> 2][i & 3];
  }
  float M = -INFINITY, Lr = 0.f, A[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) A[i] = 0.f;
  // chunk c: K in rk, V in rv (the next chunk's K already in the third set); after the step V(c + 1) is in rk
  // and K(c + 2) in rv
  auto step = [&](const int c, P (&rk)[8], P (&rv)[8]) __attribute__((always_inline)) {
    float sc[8];
    const int k0 = c * chunk, k1 = min(S, k0 + chunk);
    const float mw = wave_scores_bf16<32, ROW_JV>(ql, rk, k0, k1, slot, 8, sc);
    if (c + 1 < ns) row_issue(rsv, k1, voff, rk);
    row_fold(mw, sc, rv, k0, k1, slot, M, Lr, A);
    if (c + 2 < ns) row_issue(rsk, k0 + 2 * chunk, voff, rv);
  };
#pragma unroll
  for (int c = 0; c < ns; c += 3) {
    step(c, r0, r1);                      // K(c) r0, V(c) r1 -> V(c+1) r0, K(c+2) r1
    if (c + 1 < ns) step(c + 1, r2, r0);  // K(c+1) r2, V(c+1) r0 -> V(c+2) r2, K(c+3) r0
    if (c + 2 < ns) step(c + 2, r1, r2);  // K(c+2) r1, V(c+2) r2 -> V(c+3) r1, K(c+4) r2
  }
  if (lane < 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) red[wave][lane * 8 + i] = A[i];
  }
  if (lane == 0) {
    stat[wave] = M;
    stat[4 + wave] = Lr;
  }
  __syncthreads();
  float m, l, o;
  merge_waves_bf16(stat, red, tid, m, l, o);
  if (tid < HD) {
    if constexpr (F8) o *= p.vs[pair * HD + tid];  // the pair's V scales, once, at the store
    TypeIO<bf16_t>::st(p.out + (p.out_t ? kw_tiled_off(b, h * HD + tid, p.out_t) : (int64_t)b * p.d + h * HD + tid), o / l);
  }
  if constexpr (QG) {
    if (tid < 32)  // re-arm the row's query for the next launch (every wave of this, its only reader, has read it)
      __hip_atomic_store(qg + tid, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool QG, int NS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void cross_attn_row_kernel(CRP p) {
  __shared__ __attribute__((aligned(16))) char scratch[QG ? PROJ_SCRATCH : 16];
  __shared__ float red[4][64];
  __shared__ float stat[8];
  cross_row_pair<QG, NS, u32x4>(p, scratch, red, stat);
}

// ------------------------------------------------------------------------------------------------
// The same pair kernel over the fp8 (e4m3) cross cache (include/kwhisper.h "fp8 cross K/V"): the only grid of
// kw_cross_attn_step_fp8 / kw_dec_xq_cross_fp8, at every batch size (a row's output then cannot depend on its batch)
// and for q_len > 1 (one pair per query row and head, each reading its own item's K / V).  The body is
// cross_row_pair on 8-byte pieces of codes (row_dims decodes them).  The pair's 64 K scales multiply the query
// once (8 per lane, loaded with the query), its V scales the output at the final store: no scale is loaded per key.
template <bool QG, int NS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void cross_attn_row_fp8_kernel(CRP8 p) {
  __shared__ __attribute__((aligned(16))) char scratch[QG ? PROJ_SCRATCH : 16];
  __shared__ float red[4][64];
  __shared__ float stat[8];
  cross_row_pair<QG, NS, u32x2>(p, scratch, red, stat);
}

// Cross-attention for several query rows of one item (the prefill's P prompt positions, and the beams of
// an item, which all read the same encoder K/V): QN rows per workgroup share ONE pass over the chunk's
// K/V (the one-row kernel above reads it once per row).  Per row the arithmetic is attend_chunk's,
// operation for operation, and the chunk combine is publish_and_combine's, so results are bitwise those
// of cross_attn_kernel.  Rows: r = b*q_len + qi, grouped QN at a time within an item.
template <typename T, int QN>
__global__ __launch_bounds__(256) void cross_attn_multi_kernel(const T* __restrict__ q, int q_len, int H,
                                                               const T* __restrict__ kc, const T* __restrict__ vc,
                                                               int S, int chunk, float* __restrict__ ws,
                                                               int* __restrict__ cnt, T* __restrict__ out) {
  static_assert(QN % 4 == 0 && QN <= 8, "rows in blocks of 4, at most 8 (the beam limit)");
  static_assert(sizeof(T) == 2, "bf16 rows (wave_row_bf16)");
  __shared__ float red[4][4][64];
  __shared__ float stat[4][8];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ngrp = (q_len + QN - 1) / QN;
  const int h = blockIdx.x % H;
  const int bg = blockIdx.x / H;
  const int b = bg / ngrp, qi0 = (bg - b * ngrp) * QN;
  const int nq = min(QN, q_len - qi0);
  const int split = blockIdx.y, ns = gridDim.y;
  const int sub = lane & 7, slot = wave * 8 + (lane >> 3);
  const int k0 = split * chunk, k1 = min(S, k0 + chunk);
  const T* kb = kc + ((int64_t)b * H + h) * S * HD;
  const T* vb = vc + ((int64_t)b * H + h) * S * HD;
  // every load in flight before any arithmetic: the group's query rows (clamped to its last row: no branch),
  // then the chunk's K and V rows; the scheduling barrier keeps the compiler from sinking the V loads below
  // the first row's scores (which put a vmcnt(0) between the K and V streams and another before each later
  // row's query load)
  Row8<T> qr[QN];
#pragma unroll
  for (int r = 0; r < QN; ++r) {
    const T* qp = q + ((int64_t)(b * q_len + qi0 + min(r, nq - 1))) * H * HD + h * HD + sub * 8;
    qr[r].u[0] = *reinterpret_cast<const u32x4*>(qp);
    if constexpr (sizeof(T) == 4) qr[r].u[1] = *(reinterpret_cast<const u32x4*>(qp) + 1);
  }
  Row8<T> kr[8], vr[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) kr[j] = ld_row8<T>(kb + (int64_t)min(k0 + slot + 32 * j, k1 - 1) * HD + sub * 8);
#pragma unroll
  for (int j = 0; j < 8; ++j) vr[j] = ld_row8<T>(vb + (int64_t)min(k0 + slot + 32 * j, k1 - 1) * HD + sub * 8);
  __builtin_amdgcn_sched_barrier(0);
  // rows in blocks of 4 (one combine thread per (row, dim) per block): the K/V registers stay live
  // across the blocks, so an item's QN rows cost ONE K/V pass
  constexpr int NB = QN / 4;
  float mrow[NB], lrow[NB], orow_acc[NB];  // this thread's row (block bk, row tid / 64): m, l, o[lane]
  u32x4 k4[8], v4[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k4[j] = kr[j].u[0];
    v4[j] = vr[j].u[0];
  }
#pragma unroll
  for (int r0 = 0; r0 < QN; r0 += 4) {
    if (r0 >= nq) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r0 + r >= nq) break;  // (uniform: rows past the group's last are neither computed nor read)
      float ql[8];
      unpack8<T>(qr[r0 + r], ql);
#pragma unroll
      for (int i = 0; i < 8; ++i) ql[i] *= LOG2E;
      float mw, lw, acc[8];
      wave_row_bf16(ql, k4, v4, k0, k1, slot, 8, mw, lw, acc);
      if (lane < 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[r][wave][lane * 8 + i] = acc[i];
      }
      if (lane == 0) {
        stat[r][wave] = mw;
        stat[r][4 + wave] = lw;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r == (tid >> 6)) merge_waves_bf16(stat[r], red[r], lane, mrow[r0 / 4], lrow[r0 / 4], orow_acc[r0 / 4]);
    __syncthreads();  // stat / red are rewritten by the next block
  }
  const int dd = lane;
  bool last_any = false;
  if (ns > 1) {
    // publish every owned (row, dim) partial, then one arrival per row group
#pragma unroll
    for (int bk = 0; bk < NB; ++bk) {
      const int rr = bk * 4 + (tid >> 6);
      if (rr < nq) {
        const int row = (b * q_len + qi0 + rr) * H + h;
        float* w = ws + (int64_t)row * ns * (HD + 2) + (int64_t)split * (HD + 2);
        __hip_atomic_store(w + 2 + dd, orow_acc[bk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (dd == 0) {
          __hip_atomic_store(w, mrow[bk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(w + 1, lrow[bk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* c = cnt + (b * q_len + qi0) * H + h;  // one counter per row group
    if (tid == 0) {
      const int prev = __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = prev == ns - 1;
      if (prev == ns - 1) __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    last_any = last;
    if (!last_any) return;
  }
#pragma unroll
  for (int bk = 0; bk < NB; ++bk) {
    const int rr = bk * 4 + (tid >> 6);
    if (rr >= nq) continue;
    T* orow = out + (int64_t)(b * q_len + qi0 + rr) * H * HD + h * HD;
    if (ns == 1) {
      TypeIO<T>::st(orow + dd, orow_acc[bk] / lrow[bk]);
      continue;
    }
    const int row = (b * q_len + qi0 + rr) * H + h;
    const float* part = ws + (int64_t)row * ns * (HD + 2);
    constexpr int NSMAX = 8;
    float ms[NSMAX], ls[NSMAX], os[NSMAX];
#pragma unroll
    for (int qq = 0; qq < NSMAX; ++qq) {
      if (qq < ns) {
        ms[qq] = __hip_atomic_load(part + qq * (HD + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ls[qq] = __hip_atomic_load(part + qq * (HD + 2) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        os[qq] = __hip_atomic_load(part + qq * (HD + 2) + 2 + dd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    float M = -INFINITY;
#pragma unroll
    for (int qq = 0; qq < NSMAX; ++qq)
      if (qq < ns) M = fmaxf(M, ms[qq]);
    float lt = 0.f, ot = 0.f;
#pragma unroll
    for (int qq = 0; qq < NSMAX; ++qq)
      if (qq < ns) {
        const float f = chunk_scale<T>(ms[qq] - M);
        lt = fmaf(ls[qq], f, lt);
        ot = fmaf(os[qq], f, ot);
      }
    TypeIO<T>::st(orow + dd, ot / lt);
  }
}

// Cross-attention for up to 32 query rows of one item on the matrix cores (beam rows, the beam
// prefill's P x beams positions): the encoder kernel's scheme -- S^T = K Q^T on v_mfma_f32_32x32x16_bf16,
// O^T = V^T P^T with P^T straight from the accumulators and V^T by ds_read_b64_tr_b16 -- on one 64-key
// tile per wave.  The 4 waves of a workgroup cover one <= 256-key chunk with a common row maximum
// (exchanged through LDS) and sum their (l, O) in wave order; the chunks combine as cross_attn_kernel's
// (write-through partials, the last arriver merges in chunk order).  P enters the matrix cores in bf16
// (the one-row kernel keeps it f32): rows agree with it to bf16 rounding, not bitwise.
#ifndef KW_CROSS_MFMA_MIN_Q
#define KW_CROSS_MFMA_MIN_Q 5  // (lab knob: rows per item from which the MFMA kernel takes over)
#endif
constexpr int XM_LDS = 4 * TILE_BYTES;  // per wave: its K, then V, image (32 KB); reused for the (l, O) merge

__global__ __launch_bounds__(256) void cross_attn_mfma_kernel(const bf16_t* __restrict__ q, int q_len, int H,
                                                              const bf16_t* __restrict__ kc,
                                                              const bf16_t* __restrict__ vc, int S, int chunk,
                                                              float* __restrict__ ws, int* __restrict__ cnt,
                                                              bf16_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char xsm[];
  __shared__ float wmax[4][32], wsum[4][32];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5, ql = lane & 31;
  const int ngrp = (q_len + 31) / 32;
  const int h = blockIdx.x % H;
  const int bg = blockIdx.x / H;
  const int b = bg / ngrp, qi0 = (bg - b * ngrp) * 32;
  const int nq = min(32, q_len - qi0);
  const int split = blockIdx.y, ns = gridDim.y;
  const int k0 = split * chunk, k1 = min(S, k0 + chunk);
  const int kt0 = k0 + 64 * wave;  // this wave's tile (keys past k1 are masked)
  const bf16_t* K = kc + ((int64_t)b * H + h) * S * HD;
  const bf16_t* V = vc + ((int64_t)b * H + h) * S * HD;
  // one 8-KB LDS image per wave: K lands there by LDS-DMA; V (loaded at the same time, into registers,
  // 16 B per lane per 8-row group) is written over it once the scores are computed
  char* kb = xsm + wave * TILE_BYTES;
  u32x4 vreg[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) {  // 64 rows x 128 B, XOR-swizzled as the encoder's K / V images
    const int row = 8 * g + (lane >> 3);
    const int key = min(kt0 + row, k1 - 1);
    const int slot = lane & 7;
    glds16(K + (int64_t)key * HD + (slot ^ ((row >> 1) & 7)) * 8, kb + g * 1024);
    vreg[g] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(V + (int64_t)key * HD + slot * 8));
  }
  // Q fragments (B operand of S^T = K Q^T): lane holds Q[row ql][16s + 8hh .. +7]
  bf16x8 qf[4];
  {
    const bf16_t* qr = q + (int64_t)(b * q_len + qi0 + min(ql, nq - 1)) * H * HD + h * HD;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qr + 16 * s + 8 * hh);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  f32x16 st[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) st[i][r] = 0.f;
    const int row = i * 32 + ql;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = 2 * s + hh;
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kb + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
      st[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], st[i], 0, 0, 0);
    }
  }
  // the wave's K image is consumed (its fragment reads completed before the MFMAs): V over it, in the
  // transposed-read swizzle (LDS ops of one wave complete in order)
  char* vb = kb;
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const int row = 8 * g + (lane >> 3), slot = lane & 7;
    *reinterpret_cast<u32x4*>(vb + row * 128 + ((slot ^ (((row >> 1) & 1) << 2)) << 4)) = vreg[g];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // S^T layout: lane holds query ql, keys i*32 + (r&3) + 8*(r>>2) + 4*hh
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (key >= k1) st[i][r] = -INFINITY;
      mx = fmaxf(mx, st[i][r]);
    }
  mx = xor32_max(mx);
  if (hh == 0) wmax[wave][ql] = mx;
  __syncthreads();
  const float m = fmaxf(fmaxf(wmax[0][ql], wmax[1][ql]), fmaxf(wmax[2][ql], wmax[3][ql]));
  const float mneg = -m * LOG2E;
  float rs = 0.f;
  bf16x8 pf[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float p = __builtin_amdgcn_exp2f(fmaf(st[i][8 * s + e], LOG2E, mneg));
        rs += p;
        pf[i][s][e] = (__bf16)p;
      }
  rs = xor32_sum(rs);
  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  {
    const int li = lane & 15, qq = li >> 2, pp = li & 3, grp = (lane >> 4) & 1;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int i = n >> 1, s = n & 1;
      v2u32 t[2][2];
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int row = i * 32 + 16 * s + 8 * half + 4 * hh + qq;
          const int ch = db * 4 + 2 * grp + (pp >> 1);
          const int off = row * 128 + ((ch ^ (((row >> 1) & 1) << 2)) << 4) + (pp & 1) * 8;
          asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(t[db][half]) : "v"(lds_u32(vb + off)));
        }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0][0]), "+v"(t[0][1]), "+v"(t[1][0]), "+v"(t[1][1]));
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const v4u32 w = {t[db][0][0], t[db][0][1], t[db][1][0], t[db][1][1]};
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), pf[i][s], o[db], 0, 0, 0);
      }
    }
  }
  // merge the waves: l and O^T (dims db*32 + (r&3) + 8*(r>>2) + 4*hh of query ql) summed in wave order
  if (hh == 0) wsum[wave][ql] = rs;
  __syncthreads();  // every wave is past its tile reads: the K/V images become the merge buffer
  float* mo = reinterpret_cast<float*>(xsm);  // [wave][query 32][dim 64]
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) mo[(wave * 32 + ql) * HD + db * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh] = o[db][r];
  __syncthreads();
  // thread (query tq, 8 dims from td): the chunk's (m, l, o) of its row
  const int tq = tid >> 3, td = (tid & 7) * 8;
  const bool mine = tq < nq;
  const float mq = fmaxf(fmaxf(wmax[0][tq], wmax[1][tq]), fmaxf(wmax[2][tq], wmax[3][tq]));
  const float lq = ((wsum[0][tq] + wsum[1][tq]) + wsum[2][tq]) + wsum[3][tq];
  float ov[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
    ov[e] = ((mo[(0 * 32 + tq) * HD + td + e] + mo[(1 * 32 + tq) * HD + td + e]) + mo[(2 * 32 + tq) * HD + td + e]) +
            mo[(3 * 32 + tq) * HD + td + e];
  const int row = (b * q_len + qi0 + min(tq, nq - 1)) * H + h;
  bf16_t* orow = out + (int64_t)(b * q_len + qi0 + min(tq, nq - 1)) * H * HD + h * HD + td;
  if (ns == 1) {
    if (mine) {
      const float inv = 1.f / lq;
#pragma unroll
      for (int e = 0; e < 8; ++e) orow[e] = f2bf(ov[e] * inv);
    }
    return;
  }
  float* part = ws + (int64_t)row * ns * (HD + 2);
  if (mine) {
    float* w = part + (int64_t)split * (HD + 2);
#pragma unroll
    for (int e = 0; e < 8; ++e) __hip_atomic_store(w + 2 + td + e, ov[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (td == 0) {
      __hip_atomic_store(w, mq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(w + 1, lq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* c = cnt + (b * q_len + qi0) * H + h;  // one counter per row group
  if (tid == 0) {
    const int prev = __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == ns - 1;
    if (prev == ns - 1) __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last || !mine) return;
  constexpr int NSMAX = 8;
  // every partial in flight before the first use: unconditional loads at a clamped chunk index (a load under
  // `qq2 < ns` feeding the fma chain waited vmcnt(0) per load), the chunks past ns masked in the arithmetic
  float ms[NSMAX], ls[NSMAX], op[NSMAX][8];
#pragma unroll
  for (int qq2 = 0; qq2 < NSMAX; ++qq2) {
    const float* pq = part + min(qq2, ns - 1) * (HD + 2);
    ms[qq2] = __hip_atomic_load(pq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ls[qq2] = __hip_atomic_load(pq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int e = 0; e < 8; ++e) op[qq2][e] = __hip_atomic_load(pq + 2 + td + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  float M = -INFINITY;
#pragma unroll
  for (int qq2 = 0; qq2 < NSMAX; ++qq2)
    if (qq2 < ns) M = fmaxf(M, ms[qq2]);
  float f[NSMAX], lt = 0.f;
#pragma unroll
  for (int qq2 = 0; qq2 < NSMAX; ++qq2) {
    f[qq2] = qq2 < ns ? expf(ms[qq2] - M) : 0.f;
    if (qq2 < ns) lt = fmaf(ls[qq2], f[qq2], lt);
  }
  const float inv = 1.f / lt;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float ot = 0.f;
#pragma unroll
    for (int qq2 = 0; qq2 < NSMAX; ++qq2)
      if (qq2 < ns) ot = fmaf(op[qq2][e], f[qq2], ot);
    orow[e] = f2bf(ot * inv);
  }
}

// decoder self-attention for one new position (q_len == 1): split 0 appends k/v at L-1; each split
// attends over its <= 256-key chunk of [ks, L) (the new row read from qkv, never from the cache in the
// same launch); splits beyond L exit; the last arriving split combines.  ks = 0 (self_attn_step1), or with
// MASKED the row's first key, key_start[b] (self_attn_step1_masked: left-padded prompts) -- the chunks start at
// ks, the keys below are never read, and ks == 0 gives the unmasked chunks and bits.  L - ks <= t_max <= 512: at
// most two chunks, the workspace of kw_self_attn_workspace.  MASKED and ks >= L (a pad position, no key): the
// position is appended all the same and the output row is zero.
template <typename T, bool BP, bool MASKED>
__device__ __forceinline__ void self_step1_body(const T* qkv, int H, T* kc, T* vc, int t_max, const int32_t* cur_len,
                                                const int32_t* key_start, const int32_t* bp, int bp_stride, float* ws,
                                                int* cnt, T* out, float (*red)[64], float* stat, int* last) {
  const int bh = blockIdx.x, split = blockIdx.y;
  const int b = bh / H, h = bh - (bh / H) * H;
  const int tid = threadIdx.x, sub = tid & 7;
  const int L = *cur_len;
  const int d = H * HD;
  const int p0 = L - 1;
  int ks = 0;
  if constexpr (MASKED) ks = max(key_start[b], 0);
  const int k0 = ks + split * 256;
  if constexpr (!MASKED) {
    if (k0 >= L) return;
  }
  const int ns = (L - ks + 255) / 256;
  T* kb = kc + ((int64_t)b * H + h) * t_max * HD;
  T* vb = vc + ((int64_t)b * H + h) * t_max * HD;
  const T* row = qkv + (int64_t)b * 3 * d + h * HD;
  T* orow = out + (int64_t)b * d + h * HD;
  if (split == 0 && tid < 8) {
    copy8<T>(kb + (int64_t)p0 * HD + tid * 8, row + d + tid * 8);
    copy8<T>(vb + (int64_t)p0 * HD + tid * 8, row + 2 * d + tid * 8);
  }
  if constexpr (MASKED) {
    if (k0 >= L) {
      if (split == 0 && tid < HD) TypeIO<T>::st(orow + tid, 0.f);
      return;
    }
  }
  float qv[8];
  load8<T>(row + sub * 8, qv);
  float m, l, o;
  // beam search: position k of this row lives in cache row bp[b][k] (a shared prefix), else in row b.  The
  // cache rows of this thread's 8 key slots (attend_chunk's k = min(k0 + slot + 32 j, k1 - 1)) are resolved
  // before any K/V load, so the 16 row loads issue back to back (a slot-table load inside the address of
  // each row put a vmcnt(0) before every row load, on the greedy path too)
  const int k1 = min(L, k0 + 256);
  const int kslot = (tid >> 6) * 8 + ((tid & 63) >> 3);
  int32_t crow[8];
  if constexpr (BP) {  // (a separate instantiation: a runtime branch joins with a vmcnt(0) before the K loads)
    const int32_t* bpr = bp + (int64_t)b * bp_stride;
#pragma unroll
    for (int j = 0; j < 8; ++j) crow[j] = bpr[min(k0 + kslot + 32 * j, k1 - 1)];  // < L <= t_max <= bp_stride
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) crow[j] = b;
  }
  auto slot = [&](int k, int j) -> int64_t { return ((int64_t)crow[j] * H + h) * t_max * HD + (int64_t)k * HD; };
  attend_chunk<T>(qv, k0, k1,
                  [&](int k, int j) -> const T* { return k < p0 ? kc + slot(k, j) : row + d; },
                  [&](int k, int j) -> const T* { return k < p0 ? vc + slot(k, j) : row + 2 * d; }, red, stat, m, l, o);
  if (ns == 1) {
    if (tid < HD) TypeIO<T>::st(orow + tid, o / l);
    return;
  }
  publish_and_combine<T>(ws + (int64_t)bh * 2 * (HD + 2), cnt + bh, ns, split, m, l, o, orow, last);
}

template <typename T, bool BP>
__global__ __launch_bounds__(256) void self_attn_step1(const T* __restrict__ qkv, int H, T* __restrict__ kc,
                                                       T* __restrict__ vc, int t_max, const int32_t* __restrict__ cur_len,
                                                       const int32_t* __restrict__ bp, int bp_stride,
                                                       float* __restrict__ ws, int* __restrict__ cnt, T* __restrict__ out) {
  __shared__ float red[4][64];
  __shared__ float stat[8];
  __shared__ int last;
  self_step1_body<T, BP, false>(qkv, H, kc, vc, t_max, cur_len, nullptr, bp, bp_stride, ws, cnt, out, red, stat, &last);
}

// The chunk schedule of the cross-attention over S keys for `rows` (row, head) pairs: ns = ceil(S / 256) chunks of
// chunk = ceil(S / ns) keys (<= 256: attend_chunk; S <= 2048 gives <= 8 chunks: the combines), the last one of `last`.
struct CrossGeo {
  int64_t rows, S;
  int ns, chunk, last;
  CrossGeo(int64_t rows_, int64_t S_) : rows(rows_), S(S_) {
    ns = (int)((S + 255) / 256);
    if (ns < 1) ns = 1;
    chunk = (int)((S + ns - 1) / ns);
    last = (int)(S - (int64_t)(ns - 1) * chunk);
  }
  // the chunk grid (cross_chunk: cross_attn_dma_kernel, xq_cross_kernel) issues all 8 key groups of a chunk: the
  // last group of every chunk must hold a valid key
  bool dma_ok() const { return chunk > 224 && chunk <= 256 && last > 224; }
  // the pair kernel (cross_attn_row_kernel) checks only key group ROW_JV against the chunk end
  bool row_groups_ok() const { return chunk > 32 * ROW_JV && last > 32 * ROW_JV; }
};

// ------------------------------------------------------------------------------------------------
// kw_self_attn_step_masked's kernels (emitted last in the code object: launch_self_attn_masked, which
// instantiates them, ends the file).
// ------------------------------------------------------------------------------------------------
// The same append and causal attention with a per-row first key (left-padded prompts: row b attends keys
// [key_start[b], own position], the keys below are never read), one workgroup per (row, head, query position):
// the query positions of a long prompt run side by side instead of one after the other.  A query is
// self_attn_step's (self_attend_query), so key_start == 0 gives that kernel's bits.  A query position below
// its row's key_start (a pad) has no key: its output is zero.  Each workgroup appends its own position's K/V.
template <typename T>
__global__ __launch_bounds__(256) void self_attn_prefill_masked(const T* __restrict__ qkv, int q_len, int H,
                                                                T* __restrict__ kc, T* __restrict__ vc, int t_max,
                                                                const int32_t* __restrict__ cur_len,
                                                                const int32_t* __restrict__ key_start,
                                                                T* __restrict__ out) {
  __shared__ float sc[512];
  __shared__ float red[32][65];
  __shared__ float stat[8];
  const int bh = blockIdx.x, qi = blockIdx.y;
  const int b = bh / H, h = bh - (bh / H) * H;
  const int tid = threadIdx.x;
  const int L = *cur_len;
  const int d = H * HD;
  const int p0 = L - q_len;
  const int ks = max(key_start[b], 0);
  T* kb = kc + ((int64_t)b * H + h) * t_max * HD;
  T* vb = vc + ((int64_t)b * H + h) * t_max * HD;
  const T* qrow = qkv + ((int64_t)b * q_len + qi) * 3 * d + h * HD;
  if (tid < 8) self_append_row<T>(qrow, d, tid, kb, vb, p0 + qi);
  T* orow = out + ((int64_t)b * q_len + qi) * d + h * HD;
  if (ks > p0 + qi) {  // workgroup-uniform
    if (tid < HD) TypeIO<T>::st(orow + tid, 0.f);
    return;
  }
  self_attend_query<T>(qkv, q_len, d, b, h, qrow, [&] { return orow; }, kb, vb, p0, ks, p0 + qi + 1, sc, red, stat);
}

// self_attn_step1 with a per-row first key: self_step1_body<T, BP, true>
template <typename T, bool BP>
__global__ __launch_bounds__(256) void self_attn_step1_masked(const T* __restrict__ qkv, int H, T* __restrict__ kc,
                                                              T* __restrict__ vc, int t_max,
                                                              const int32_t* __restrict__ cur_len,
                                                              const int32_t* __restrict__ key_start,
                                                              const int32_t* __restrict__ bp, int bp_stride,
                                                              float* __restrict__ ws, int* __restrict__ cnt,
                                                              T* __restrict__ out) {
  __shared__ float red[4][64];
  __shared__ float stat[8];
  __shared__ int last;
  self_step1_body<T, BP, true>(qkv, H, kc, vc, t_max, cur_len, key_start, bp, bp_stride, ws, cnt, out, red, stat, &last);
}

// The bf16 prefill as a causal tile kernel: one wave per (row, head, 16 query positions), keys in tiles of 32 from the
// row's first key.  Scores are computed transposed, S^T = K Q^T (v_mfma_f32_16x16x32_bf16: A = 16 keys x 32 dims, B =
// 32 dims x 16 queries, both 16-B row loads), so a lane owns one query (column lane & 15) and the keys 4g + r of each
// 16-key half (g = lane >> 4): the online softmax is in-lane plus two lane exchanges.  O^T = V^T P^T takes P^T straight
// from those accumulators as the B operand -- its k slots (g, j) stand for keys 4g + j (j < 4) and 16 + 4g + j - 4 of
// the tile, and V^T (A operand, through a row-major LDS image of the 32 V rows) is read in the same key order.  Keys
// below key_start are never addressed (tiles start there); addresses past the tile's last key are clamped to it and
// masked.  A pad query (no key) writes zeros.  The wave appends its own 16 positions' K/V.
__global__ __launch_bounds__(64) void self_attn_prefill_masked_mfma(const bf16_t* __restrict__ qkv, int q_len, int H,
                                                                    bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                                                                    int t_max, const int32_t* __restrict__ cur_len,
                                                                    const int32_t* __restrict__ key_start,
                                                                    bf16_t* __restrict__ out) {
  constexpr int VLD = HD + 8;  // LDS row of 144 B: the 16-B row writes and the 2-B column reads spread over the banks
  __shared__ __attribute__((aligned(16))) bf16_t vs[32 * VLD];
  const int bh = blockIdx.x, q0 = blockIdx.y * 16;
  const int b = bh / H, h = bh - (bh / H) * H;
  const int lane = threadIdx.x, qn = lane & 15, g = lane >> 4;
  const int L = *cur_len;
  const int d = H * HD;
  const int p0 = L - q_len;
  const int ks = max(key_start[b], 0);
  bf16_t* kb = kc + ((int64_t)b * H + h) * t_max * HD;
  bf16_t* vb = vc + ((int64_t)b * H + h) * t_max * HD;
  const bf16_t* rows = qkv + (int64_t)b * q_len * 3 * d + h * HD;  // row qi: rows + qi * 3d (+ d: k, + 2d: v)
  for (int i = lane; i < 16 * 8; i += 64) {
    const int qi = q0 + (i >> 3), c8 = (i & 7) * 8;
    if (qi < q_len) {
      copy8<bf16_t>(kb + (int64_t)(p0 + qi) * HD + c8, rows + (int64_t)qi * 3 * d + d + c8);
      copy8<bf16_t>(vb + (int64_t)(p0 + qi) * HD + c8, rows + (int64_t)qi * 3 * d + 2 * d + c8);
    }
  }
  const bool qok = q0 + qn < q_len;
  const int qi = min(q0 + qn, q_len - 1);
  const int pos = p0 + qi;
  const int kend = p0 + min(q0 + 16, q_len);  // one past the tile's last key
  bf16_t* orow = out + ((int64_t)b * q_len + qi) * d + h * HD;
  if (ks >= kend) {  // wave-uniform: every query of the tile is a pad
    if (qok) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) orow[16 * dt + 4 * g + r] = 0;
    }
    return;
  }
  auto kp = [&](int k) -> const bf16_t* { return k < p0 ? kb + (int64_t)k * HD : rows + (int64_t)(k - p0) * 3 * d + d; };
  auto vp = [&](int k) -> const bf16_t* { return k < p0 ? vb + (int64_t)k * HD : rows + (int64_t)(k - p0) * 3 * d + 2 * d; };
  bf16x8 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(rows + (int64_t)qi * 3 * d + 32 * kk + 8 * g);
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = ks; k0 < kend; k0 += 32) {
    // the tile's V rows to LDS (4 x 16 B per lane), K fragments straight from memory
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i, kr = c >> 3, c8 = (c & 7) * 8;
      *reinterpret_cast<uint4*>(vs + kr * VLD + c8) = *reinterpret_cast<const uint4*>(vp(min(k0 + kr, kend - 1)) + c8);
    }
    f32x4 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16_t* kr = kp(min(k0 + 16 * t + qn, kend - 1));
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kr + 32 * kk + 8 * g);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], st[t], 0, 0, 0);
      }
    }
    bool ok[2][4];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok[t][r] = qok && k0 + 16 * t + 4 * g + r <= pos;
        mx = fmaxf(mx, ok[t][r] ? st[t][r] : -INFINITY);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    const float sc = m == -INFINITY ? 0.f : expf(m - mn);
    float p[2][4], sum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[t][r] = ok[t][r] ? expf(st[t][r] - mn) : 0.f;
        sum += p[t][r];
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    l = l * sc + sum;
    m = mn;
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[j] = (__bf16)p[j >> 2][j & 3];
    __syncthreads();  // the V image is written
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x8 vf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bf16_t x = vs[(16 * (j >> 2) + 4 * g + (j & 3)) * VLD + 16 * dt + qn];
        vf[j] = *reinterpret_cast<const __bf16*>(&x);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) o[dt][r] *= sc;
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
    }
    __syncthreads();  // the V image is consumed
  }
  if (qok) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) orow[16 * dt + 4 * g + r] = l > 0.f ? f2bf(o[dt][r] * inv) : (bf16_t)0;
  }
}

}  // namespace

extern "C" int kw_attention(int dtype, const void* qkv, int64_t B, int64_t H, int64_t T, int64_t hd, void* out,
                            kw_stream_t stream) {
  if (!qkv || !out || B <= 0 || H <= 0 || T <= 0) return kw_set_error_msg(KW_EINVAL, "kw_attention: invalid arguments");
  if (hd != HD) return kw_set_error_msg(KW_EUNSUPPORTED, "kw_attention: head_dim must be 64");
  hipStream_t s = (hipStream_t)stream;
  const bool ql2 = (dtype & KW_ATTN_Q_LOG2) != 0;
  dtype &= ~KW_ATTN_Q_LOG2;
  if (ql2 && dtype != KW_DT_BF16) return kw_set_error_msg(KW_EUNSUPPORTED, "kw_attention: KW_ATTN_Q_LOG2 is bf16 only");
  if (dtype == KW_DT_BF16) {
    const int64_t grid = B * H * ((T + AQ - 1) / AQ);
    if (ql2)
      hipLaunchKernelGGL(attn_fwd_l2, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)qkv, (int)B, (int)H, (int)T,
                         (bf16_t*)out);
    else
      hipLaunchKernelGGL(attn_fwd_bf16, dim3((unsigned)grid), dim3(256), 0, s, (const bf16_t*)qkv, (int)B, (int)H, (int)T,
                         (bf16_t*)out);
  } else if (dtype == KW_DT_F32) {
    const int64_t grid = B * H * ((T + 3) / 4);
    hipLaunchKernelGGL(attn_fwd_f32, dim3((unsigned)grid), dim3(256), 0, s, (const float*)qkv, (int)B, (int)H, (int)T,
                       (float*)out);
  } else {
    return kw_set_error_msg(KW_EUNSUPPORTED, "kw_attention: dtype");
  }
  KW_CHECK_LAUNCH();
  return KW_OK;
}

// The self-attention workspace of the one-position step, byte offsets: f32 chunk partials [B H][2][HD+2] (t_max <= 512:
// at most two 256-key chunks per (b, h)) | arrival counters [B H].  Zero before first use.
struct SelfLayout {
  size_t counters, end;
  SelfLayout(int64_t B, int64_t H)
      : counters((size_t)(B * H) * 2 * (HD + 2) * sizeof(float)), end(counters + (size_t)(B * H) * sizeof(int)) {}
  float* part(void* ws) const { return reinterpret_cast<float*>(ws); }
  int* cnt(void* ws) const { return reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + counters); }
};

extern "C" size_t kw_self_attn_workspace(int64_t B, int64_t H, int64_t t_max) {
  (void)t_max;
  return SelfLayout(B, H).end;
}

// the argument checks of kw_self_attn_step and (masked: a key_start, q_len <= t_max, a dtype that is checked)
// kw_self_attn_step_masked, reported under the entry's name `fn`
static int self_attn_check(const char* fn, bool masked, int dtype, const void* qkv, int64_t B, int64_t q_len, int64_t H,
                           int64_t hd, const void* k_cache, const void* v_cache, int64_t t_max, const int32_t* cur_len,
                           const int32_t* key_start, const int32_t* bp, int64_t bp_stride, const void* out,
                           const void* workspace, size_t ws_bytes) {
  auto fail = [fn](int code, const char* what) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return kw_set_error_msg(code, msg);
  };
  if (!qkv || !k_cache || !v_cache || !cur_len || !out || B <= 0 || q_len <= 0 || H <= 0 || t_max <= 0 || t_max > 512 ||
      (masked && (!key_start || q_len > t_max)))
    return fail(KW_EINVAL, masked ? "invalid arguments (q_len <= t_max <= 512)" : "invalid arguments (t_max <= 512)");
  if (hd != HD) return fail(KW_EUNSUPPORTED, "head_dim must be 64");
  if (masked && dtype != KW_DT_BF16 && dtype != KW_DT_F32) return fail(KW_EUNSUPPORTED, "dtype");
  if (bp && (q_len != 1 || bp_stride < t_max))
    return fail(KW_EINVAL, "a slot table needs q_len == 1 and bp_stride >= t_max");
  if (q_len == 1 && (!workspace || ws_bytes < SelfLayout(B, H).end))
    return fail(KW_EINVAL, "needs a zero-filled workspace of kw_self_attn_workspace()");
  return KW_OK;
}

extern "C" int kw_self_attn_step(int dtype, const void* qkv, int64_t B, int64_t q_len, int64_t H, int64_t hd,
                                 void* k_cache, void* v_cache, int64_t t_max, const int32_t* cur_len,
                                 const int32_t* bp, int64_t bp_stride, void* out, void* workspace, size_t ws_bytes,
                                 kw_stream_t stream) {
  if (const int rc = self_attn_check("kw_self_attn_step", false, dtype, qkv, B, q_len, H, hd, k_cache, v_cache, t_max,
                                     cur_len, nullptr, bp, bp_stride, out, workspace, ws_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  if (q_len == 1) {
    const SelfLayout W(B, H);
    dim3 grid((unsigned)(B * H), (unsigned)((t_max + 255) / 256));
    if (dtype == KW_DT_BF16)
      hipLaunchKernelGGL((bp ? self_attn_step1<bf16_t, true> : self_attn_step1<bf16_t, false>), grid, dim3(256), 0, s,
                         (const bf16_t*)qkv, (int)H, (bf16_t*)k_cache, (bf16_t*)v_cache, (int)t_max, cur_len, bp,
                         (int)bp_stride, W.part(workspace), W.cnt(workspace), (bf16_t*)out);
    else
      hipLaunchKernelGGL((bp ? self_attn_step1<float, true> : self_attn_step1<float, false>), grid, dim3(256), 0, s,
                         (const float*)qkv, (int)H, (float*)k_cache, (float*)v_cache, (int)t_max, cur_len, bp,
                         (int)bp_stride, W.part(workspace), W.cnt(workspace), (float*)out);
  } else if (dtype == KW_DT_BF16) {
    hipLaunchKernelGGL(self_attn_step<bf16_t>, dim3((unsigned)(B * H)), dim3(256), 0, s, (const bf16_t*)qkv, (int)q_len,
                       (int)H, (bf16_t*)k_cache, (bf16_t*)v_cache, (int)t_max, cur_len, (bf16_t*)out);
  } else {
    hipLaunchKernelGGL(self_attn_step<float>, dim3((unsigned)(B * H)), dim3(256), 0, s, (const float*)qkv, (int)q_len,
                       (int)H, (float*)k_cache, (float*)v_cache, (int)t_max, cur_len, (float*)out);
  }
  KW_CHECK_LAUNCH();
  return KW_OK;
}

static size_t align64(size_t n) { return (n + 63) & ~(size_t)63; }

// The cross-attention workspace of `rows` (row, head) pairs, byte offsets: f32 partials [rows][ns][HD+2] | arrival
// counters [rows] (publish_and_combine kernels) | status word | fault-injection word (kw_dec_xq_cross's projection) |
// pad to 64 B | 8-byte wave granules [rows][ns][4 waves][HD+2] (the chunk grid: cross_chunk) -- kw_cross_attn_step's
// workspace ends here -- | pad to 64 B | query granules [M][d/2] (n_qg of them: kw_dec_xq_cross).  Every region is
// zero before first use.
struct CrossLayout {
  size_t partials = 0, counters, status, fault, wave_gran, step_end, query_gran, fused_end;
  explicit CrossLayout(const CrossGeo& g, int64_t n_qg = 0) {
    const size_t part_bytes = (size_t)g.rows * g.ns * (HD + 2) * sizeof(float);
    counters = part_bytes;
    status = counters + (size_t)g.rows * sizeof(int);
    fault = status + sizeof(int);
    wave_gran = align64(fault + sizeof(int));
    step_end = wave_gran + 8 * part_bytes;  // an 8-byte granule per f32 of a partial, per wave: 2 x 4
    query_gran = align64(step_end);
    fused_end = query_gran + (size_t)n_qg * sizeof(unsigned long long);
  }
  template <typename T>
  T* at(void* ws, size_t off) const {
    return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off);
  }
};

extern "C" size_t kw_cross_attn_workspace(int64_t B, int64_t q_len, int64_t H, int64_t hd, int64_t S) {
  (void)hd;
  return CrossLayout(CrossGeo(B * q_len * H, S)).step_end;
}

extern "C" size_t kw_cross_attn_status_offset(int64_t B, int64_t q_len, int64_t H, int64_t hd, int64_t S) {
  (void)hd;
  return CrossLayout(CrossGeo(B * q_len * H, S)).status;
}

// cross_attn_row_kernel when one round of pair workgroups covers the device -- at least one per CU, all resident
// at once (the occupancy query) -- and the A/B switch KW_CROSS_ROW=0 is not set (read once).
constexpr int ROW_NS = 6;  // cross_attn_row_kernel's chunk count (S = 1500)

template <bool QG>
static bool row_kernel_fits(const CrossGeo& g) {
  if (!g.row_groups_ok()) return false;
  static int per_cu = 0, off = -1;
  if (off < 0) {
    const char* e = getenv("KW_CROSS_ROW");
    off = (e && e[0] == '0') ? 1 : 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&cross_attn_row_kernel<QG, ROW_NS>), 256,
                                                     0) != hipSuccess)
      per_cu = 0;
  }
  const int ncu = kw_device_cus();  // 0 (unknown): the pair kernel is off
  return !off && g.ns == ROW_NS && ncu > 0 && g.rows >= ncu && g.rows <= (int64_t)ncu * per_cu;
}

// the launch descriptor's fields that kw_cross_attn_step and kw_dec_xq_cross fill alike (the query -- a row pointer, or
// the granules and the projection that publishes them -- is the caller's)
// (ws null: a launch without hand-offs, kw_cross_attn_step_fp8)
static CRP cross_crp(const CrossGeo& g, const CrossLayout& L, void* ws, int64_t H, const void* k, const void* v, void* out) {
  CRP p{};
  if (ws) {
    p.gran = L.at<unsigned long long>(ws, L.wave_gran);
    p.err = L.at<int>(ws, L.status);
  }
  p.kc = (const bf16_t*)k;
  p.vc = (const bf16_t*)v;
  p.H = (int)H, p.d = (int)(H * HD), p.S = (int)g.S, p.chunk = g.chunk, p.ns = g.ns;
  p.out = (bf16_t*)out;
  return p;
}

// ... and those of a launch that runs the query projection too (kw_dec_xq_cross, kw_dec_xq_cross_fp8; A: either
// entry's argument block): the query granules, the projection workgroups and their arguments, the output layout
template <typename A>
static void crp_fuse_projection(CRP& p, const CrossLayout& L, const A& a) {
  const int M = (int)a.M, d = (int)a.d;
  p.qg = L.at<unsigned long long>(a.workspace, L.query_gran);
  p.n_lin = d / 16;
  p.out_t = a.ldx == KW_LD_TILED ? (M + 15) / 16 : 0;
  p.proj = ProjArgs{reinterpret_cast<const bf16_t*>(a.x), a.ldx, M, d, d, a.ln_eps, a.ln_colsum,
                    reinterpret_cast<const bf16x8*>(a.W), a.bias, a.scale, d, p.err + 1};
}

extern "C" int kw_cross_attn_pair_kernel(int64_t rows, int64_t S, int fused) {
  const CrossGeo g(rows, S);
  return (fused ? row_kernel_fits<true>(g) : row_kernel_fits<false>(g)) ? 1 : 0;
}

extern "C" int kw_cross_attn_step(int dtype, const void* q, int64_t B, int64_t q_len, int64_t H, int64_t hd,
                                  const void* k, const void* v, int64_t S, void* out, void* workspace, size_t ws_bytes,
                                  kw_stream_t stream) {
  if (!q || !k || !v || !out || !workspace || B <= 0 || q_len <= 0 || H <= 0 || S <= 0)
    return kw_set_error_msg(KW_EINVAL, "kw_cross_attn_step: invalid arguments");
  if (hd != HD) return kw_set_error_msg(KW_EUNSUPPORTED, "kw_cross_attn_step: head_dim must be 64");
  const CrossGeo g(B * q_len * H, S);
  const CrossLayout L(g);
  if (ws_bytes < L.step_end) return kw_set_error_msg(KW_EINVAL, "kw_cross_attn_step: workspace too small");
  if (S > 2048) return kw_set_error_msg(KW_EUNSUPPORTED, "kw_cross_attn_step: S <= 2048 (8 chunks of 256)");
  const int ns = g.ns, chunk = g.chunk;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)g.rows, (unsigned)ns);
  float* part = L.at<float>(workspace, L.partials);
  int* cnt = L.at<int>(workspace, L.counters);
  if (dtype == KW_DT_BF16 && q_len > 1 && q_len <= 4) {  // several rows per item (prefill, beams): one K/V pass
    const dim3 gm((unsigned)(B * H), (unsigned)ns);
    hipLaunchKernelGGL((cross_attn_multi_kernel<bf16_t, 4>), gm, dim3(256), 0, s, (const bf16_t*)q, (int)q_len, (int)H,
                       (const bf16_t*)k, (const bf16_t*)v, (int)S, chunk, part, cnt, (bf16_t*)out);
  } else if (dtype == KW_DT_BF16 && q_len >= KW_CROSS_MFMA_MIN_Q) {  // beams: up to 32 rows per pass, MFMA
    static bool attr = false;
    if (!attr) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cross_attn_mfma_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, XM_LDS);
      if (e != hipSuccess) return kw_set_error(e);
      attr = true;
    }
    const dim3 gm((unsigned)(B * ((q_len + 31) / 32) * H), (unsigned)ns);
    hipLaunchKernelGGL(cross_attn_mfma_kernel, gm, dim3(256), XM_LDS, s, (const bf16_t*)q, (int)q_len, (int)H,
                       (const bf16_t*)k, (const bf16_t*)v, (int)S, chunk, part, cnt, (bf16_t*)out);
  } else if (dtype == KW_DT_BF16 && q_len > 4) {  // up to 8 rows per K/V pass, groups of 8 beyond
    const dim3 gm((unsigned)(B * ((q_len + 7) / 8) * H), (unsigned)ns);
    hipLaunchKernelGGL((cross_attn_multi_kernel<bf16_t, 8>), gm, dim3(256), 0, s, (const bf16_t*)q, (int)q_len, (int)H,
                       (const bf16_t*)k, (const bf16_t*)v, (int)S, chunk, part, cnt, (bf16_t*)out);
  } else if (dtype == KW_DT_BF16 && q_len == 1 && row_kernel_fits<false>(g)) {
    CRP p = cross_crp(g, L, workspace, H, k, v, out);
    p.q = (const bf16_t*)q;
    hipLaunchKernelGGL((cross_attn_row_kernel<false, ROW_NS>), dim3((unsigned)g.rows), dim3(256), 0, s, p);
  } else if (dtype == KW_DT_BF16 && XA_DMA && g.dma_ok())
    hipLaunchKernelGGL(cross_attn_dma_kernel, grid, dim3(256), 0, s, (const bf16_t*)q, (int)q_len, (int)H,
                       (const bf16_t*)k, (const bf16_t*)v, (int)S, chunk, L.at<unsigned long long>(workspace, L.wave_gran),
                       L.at<int>(workspace, L.status), (bf16_t*)out);
  else if (dtype == KW_DT_BF16)
    hipLaunchKernelGGL(cross_attn_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)q, (int)q_len, (int)H,
                       (const bf16_t*)k, (const bf16_t*)v, (int)S, chunk, part, cnt, (bf16_t*)out);
  else
    hipLaunchKernelGGL(cross_attn_kernel<float>, grid, dim3(256), 0, s, (const float*)q, (int)q_len, (int)H,
                       (const float*)k, (const float*)v, (int)S, chunk, part, cnt, (float*)out);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

// the shapes kw_dec_xq_cross covers: the projection's rows and width, and chunks the chunk grid's key groups fit
static bool xq_shape_ok(int64_t M, int64_t d, int64_t H, int64_t S) {
  return proj_shape_ok(M, d) && H >= 1 && d == HD * H && S >= 1 && S <= 2048 && CrossGeo(M * H, S).dma_ok();
}

extern "C" size_t kw_dec_xq_cross_workspace(int64_t M, int64_t d, int64_t H, int64_t S) {
  if (M < 1 || d < 2 || H < 1 || S < 1) return 0;
  return CrossLayout(CrossGeo(M * H, S), M * (d / 2)).fused_end;
}

extern "C" size_t kw_dec_xq_cross_status_offset(int64_t M, int64_t d, int64_t H, int64_t S) {
  (void)d;
  return CrossLayout(CrossGeo(M * H, S)).status;  // status word, then the fault-injection word
}

extern "C" int kw_dec_xq_cross_supported(int64_t M, int64_t d, int64_t H, int64_t S) {
  return xq_shape_ok(M, d, H, S) ? 1 : 0;  // (every wait is on earlier-dispatched work: no residency condition)
}

extern "C" int kw_dec_xq_cross(const kw_dec_xq_cross_args* a, kw_stream_t stream) {
  if (!a || !a->x || !a->W || !a->ln_colsum || !a->k || !a->v || !a->out || !a->workspace)
    return kw_set_error_msg(KW_EINVAL, "kw_dec_xq_cross: null pointer");
  if (!xq_shape_ok(a->M, a->d, a->H, a->S) || (a->ldx != KW_LD_TILED && (a->ldx < a->d || a->ldx % 8)) || (uintptr_t)a->x % 16)
    return kw_set_error_msg(KW_EINVAL, "kw_dec_xq_cross: M <= 32 rows, d = 64 H <= 1280, 224 < S / chunks <= 256, "
                                       "ldx % 8 == 0, 16-B aligned x");
  const CrossGeo g(a->M * a->H, a->S);
  const CrossLayout L(g, a->M * (a->d / 2));
  if (a->ws_bytes < L.fused_end)
    return kw_set_error_msg(KW_EINVAL, "kw_dec_xq_cross: needs a zero-filled workspace of kw_dec_xq_cross_workspace()");
  CRP p = cross_crp(g, L, a->workspace, a->H, a->k, a->v, a->out);
  crp_fuse_projection(p, L, *a);
  if (row_kernel_fits<true>(g))  // one pair workgroup per (row, head), chunks pipelined
    hipLaunchKernelGGL((cross_attn_row_kernel<true, ROW_NS>), dim3((unsigned)(p.n_lin + g.rows)), dim3(256), 0,
                       (hipStream_t)stream, p);
  else  // the chunk grid
    hipLaunchKernelGGL(xq_cross_kernel, dim3((unsigned)(p.n_lin + g.rows * g.ns)), dim3(256), 0, (hipStream_t)stream, p);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

// ---- the fp8 (e4m3) cross cache ------------------------------------------------------------------------------

// the one grid of the fp8 path: S must give the pair kernel its six chunks, each reaching key group ROW_JV
// the fp8 kernels' descriptor: cross_crp's fields over the codes, the layer's scales, q_len query rows per item
static CRP8 cross_crp8(const CRP& base, const float* ks, const float* vs, int64_t q_len) {
  CRP8 p{};
  static_cast<CRP&>(p) = base;
  p.ks = ks, p.vs = vs, p.q_len = (int)q_len;
  return p;
}

static bool fp8_geo_ok(const CrossGeo& g) { return g.S <= 2048 && g.ns == ROW_NS && g.row_groups_ok(); }
#define FP8_GEO_MSG ": S must split into 6 chunks of 225..256 keys (e.g. 1500, 1399, 1536)"

extern "C" int kw_cross_attn_step_fp8(const void* q, int64_t B, int64_t q_len, int64_t H, int64_t hd, const void* k,
                                      const void* v, const float* k_scale, const float* v_scale, int64_t S, void* out,
                                      kw_stream_t stream) {
  if (!q || !k || !v || !k_scale || !v_scale || !out || B <= 0 || q_len <= 0 || H <= 0 || S <= 0)
    return kw_set_error_msg(KW_EINVAL, "kw_cross_attn_step_fp8: invalid arguments");
  if (hd != HD) return kw_set_error_msg(KW_EUNSUPPORTED, "kw_cross_attn_step_fp8: head_dim must be 64");
  const CrossGeo g(B * q_len * H, S);
  if (!fp8_geo_ok(g))
    return kw_set_error_msg(KW_EUNSUPPORTED, "kw_cross_attn_step_fp8" FP8_GEO_MSG);
  if (g.rows > 0x7fffffff || (uintptr_t)q % 16 || (uintptr_t)k % 16 || (uintptr_t)v % 16 || (uintptr_t)k_scale % 16)
    return kw_set_error_msg(KW_EINVAL, "kw_cross_attn_step_fp8: q, k, v and k_scale must be 16-B aligned");
  CRP8 p = cross_crp8(cross_crp(g, CrossLayout(g), nullptr, H, k, v, out), k_scale, v_scale, q_len);
  p.q = (const bf16_t*)q;
  hipLaunchKernelGGL((cross_attn_row_fp8_kernel<false, ROW_NS>), dim3((unsigned)g.rows), dim3(256), 0, (hipStream_t)stream, p);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

static bool xq_fp8_shape_ok(int64_t M, int64_t d, int64_t H, int64_t S) {
  return proj_shape_ok(M, d) && H >= 1 && d == HD * H && S >= 1 && fp8_geo_ok(CrossGeo(M * H, S));
}

extern "C" int kw_dec_xq_cross_fp8_supported(int64_t M, int64_t d, int64_t H, int64_t S) {
  return xq_fp8_shape_ok(M, d, H, S) ? 1 : 0;  // (every wait is on earlier-dispatched work: no residency condition)
}

extern "C" int kw_dec_xq_cross_fp8(const kw_dec_xq_cross_fp8_args* a, kw_stream_t stream) {
  if (!a || !a->x || !a->W || !a->ln_colsum || !a->k || !a->v || !a->k_scale || !a->v_scale || !a->out || !a->workspace)
    return kw_set_error_msg(KW_EINVAL, "kw_dec_xq_cross_fp8: null pointer");
  if (a->M >= 1 && a->H >= 1 && a->S >= 1 && proj_shape_ok(a->M, a->d) && a->d == HD * a->H && !fp8_geo_ok(CrossGeo(a->M * a->H, a->S)))
    return kw_set_error_msg(KW_EUNSUPPORTED, "kw_dec_xq_cross_fp8" FP8_GEO_MSG);
  if (!xq_fp8_shape_ok(a->M, a->d, a->H, a->S) || (a->ldx != KW_LD_TILED && (a->ldx < a->d || a->ldx % 8)) ||
      (uintptr_t)a->x % 16 || (uintptr_t)a->k % 16 || (uintptr_t)a->v % 16 || (uintptr_t)a->k_scale % 16)
    return kw_set_error_msg(KW_EINVAL, "kw_dec_xq_cross_fp8: M <= 32 rows, d = 64 H <= 1280, ldx % 8 == 0, 16-B aligned x, "
                                       "k, v and k_scale");
  const CrossGeo g(a->M * a->H, a->S);
  const CrossLayout L(g, a->M * (a->d / 2));
  if (a->ws_bytes < L.fused_end)
    return kw_set_error_msg(KW_EINVAL, "kw_dec_xq_cross_fp8: needs a zero-filled workspace of kw_dec_xq_cross_workspace()");
  CRP8 p = cross_crp8(cross_crp(g, L, a->workspace, a->H, a->k, a->v, a->out), a->k_scale, a->v_scale, 1);
  crp_fuse_projection(p, L, *a);
  hipLaunchKernelGGL((cross_attn_row_fp8_kernel<true, ROW_NS>), dim3((unsigned)(p.n_lin + g.rows)), dim3(256), 0,
                     (hipStream_t)stream, p);
  KW_CHECK_LAUNCH();
  return KW_OK;
}

// (last in the file: kernel templates are emitted where they are first launched from)
template <typename T>
static void launch_self_attn_masked(const void* qkv, int64_t B, int64_t q_len, int64_t H, void* k_cache, void* v_cache,
                                    int64_t t_max, const int32_t* cur_len, const int32_t* key_start, const int32_t* bp,
                                    int64_t bp_stride, void* out, void* workspace, bool per_query, hipStream_t s) {
  if (q_len == 1) {
    const SelfLayout W(B, H);
    dim3 grid((unsigned)(B * H), (unsigned)((t_max + 255) / 256));
    hipLaunchKernelGGL((bp ? self_attn_step1_masked<T, true> : self_attn_step1_masked<T, false>), grid, dim3(256), 0, s,
                       (const T*)qkv, (int)H, (T*)k_cache, (T*)v_cache, (int)t_max, cur_len, key_start, bp,
                       (int)bp_stride, W.part(workspace), W.cnt(workspace), (T*)out);
  } else if (sizeof(T) == 2 && !per_query) {
    hipLaunchKernelGGL(self_attn_prefill_masked_mfma, dim3((unsigned)(B * H), (unsigned)((q_len + 15) / 16)), dim3(64), 0, s,
                       (const bf16_t*)qkv, (int)q_len, (int)H, (bf16_t*)k_cache, (bf16_t*)v_cache, (int)t_max, cur_len,
                       key_start, (bf16_t*)out);
  } else {
    hipLaunchKernelGGL(self_attn_prefill_masked<T>, dim3((unsigned)(B * H), (unsigned)q_len), dim3(256), 0, s,
                       (const T*)qkv, (int)q_len, (int)H, (T*)k_cache, (T*)v_cache, (int)t_max, cur_len, key_start,
                       (T*)out);
  }
}

extern "C" int kw_self_attn_step_masked(int dtype, const void* qkv, int64_t B, int64_t q_len, int64_t H, int64_t hd,
                                        void* k_cache, void* v_cache, int64_t t_max, const int32_t* cur_len,
                                        const int32_t* key_start, const int32_t* bp, int64_t bp_stride, void* out,
                                        void* workspace, size_t ws_bytes, kw_stream_t stream) {
  const bool per_query = (dtype & KW_SELF_ATTN_PER_QUERY) != 0;
  dtype &= ~KW_SELF_ATTN_PER_QUERY;
  if (const int rc = self_attn_check("kw_self_attn_step_masked", true, dtype, qkv, B, q_len, H, hd, k_cache, v_cache, t_max,
                                     cur_len, key_start, bp, bp_stride, out, workspace, ws_bytes))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == KW_DT_BF16)
    launch_self_attn_masked<bf16_t>(qkv, B, q_len, H, k_cache, v_cache, t_max, cur_len, key_start, bp, bp_stride, out,
                                    workspace, per_query, s);
  else
    launch_self_attn_masked<float>(qkv, B, q_len, H, k_cache, v_cache, t_max, cur_len, key_start, bp, bp_stride, out,
                                   workspace, per_query, s);
  KW_CHECK_LAUNCH();
  return KW_OK;
}
