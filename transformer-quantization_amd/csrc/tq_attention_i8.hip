// (f3) Fixed-range quantized self-attention core on the i8 matrix cores.
//
// Reference chain (models/quantized_bert.py:135-213), all on dequantised fp32 tensors with one ATen
// launch per step:   Q, K, V = quantized Linear outputs, split into heads (3 permute copies)
//     S = Q K^T                      batched fp32 GEMM            [B, H, T, T]
//     S = Q_scores(S) / sqrt(d) + mask ;  P = Q_probs(softmax(S))  5 element-wise sweeps
//     C = P V                        batched fp32 GEMM, permute copy back to [B, T, H d]
//     C = Q_ctx(C)
// With fixed per-tensor asymmetric ranges Q, K, V and P live on <= 8-bit grids, so both GEMMs are exact
// integer contractions of the grid indices (a - z) that the producing kernels already emit as
// int8(index - 128):
//     S[q,k] = s_q s_k ( sum_d a'_q a'_k + c_k sum_d a'_q + c_q sum_d a'_k + d c_q c_k ),   c = 128 - z
//     C[q,d] = s_p s_v ( sum_k a'_p a'_v + c_v sum_k a'_p + c_p sum_k a'_v + T c_p c_v )
// One workgroup (2 waves, 8 on grids that are not key-split: round 6) owns 32 (128) query rows of one (batch, head); each
// wave computes S^T = K Q^T for
// its 16 queries with T/16 v_mfma_i32_16x16x64_i8 (d = 64 = one MFMA K step), keeps the 16 x T scores
// in registers (lane = one query column, keys 16t + 4g + r), does the quantizers / mask / softmax
// there, packs the probability indices straight into the B operand of the second MFMA (the MFMA K
// dimension may be permuted freely as long as both operands agree, so the accumulator layout IS the
// operand layout once V^T is stored with the matching key permutation in LDS) and computes
// C^T = V^T P^T.  Row / column sums for the zero-point corrections are MFMAs against an all-ones
// operand.  Nothing but Q, K, V indices (3 x 64 B per token and head) is read and only C is written:
// the [B, H, T, T] score and probability tensors never exist in memory.
#include <algorithm>
#include <type_traits>

#include "tq_device.h"
#include "tq_host.h"

namespace tq {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kAttnWaves = 2;
constexpr int kAttnThreads = kAttnWaves * kWave;

struct AttnArgs {
  const int8_t *q, *k, *v;    // [B, T, H * 64] int8(index - 128)
  float* ctx;                 // [B, T, H * 64]
  int8_t* ctx_idx;            // optional int8(index - 128) of ctx (needs q_ctx)
  const float* mask;          // additive [B, T] or null
  uint32_t B, T, H;
  uint32_t in_stride;         // elements between consecutive tokens of q / k (H * 64, or 3 * H * 64 inside a stacked QKV buffer)
  uint32_t v_stride;          // the same for v (MobileBERT: Q | K stacked, V on its own)
  float denom;
  tq_quantizer qq, qk, qv;    // asymmetric, n_bits <= 8; per-tensor, or one grid per head (see wide_*)
  tq_quantizer q_scores, q_probs, q_ctx;
  int has_scores, has_ctx;
  // one grid per head: nonzero where qq / qk / qv / q_ctx carry per-column buffers [H * head_dim] (constant over each head's
  // columns: the caller's promise) that head h reads at column h * head_dim; 0: per-tensor, element 0
  uint32_t wide_q, wide_k, wide_v, wide_c;
#ifdef TQ_ATTN_PROF
  unsigned long long* prof;   // tools/tuning/attn_prof.py: 8 s_memtime stamps per workgroup
#endif
  int fast_ok;                // 0: keep the guarded-reciprocal element math (TQ_ATTN_FAST=0, parity tests)
};

// position of key (64 s + 16 tt + 4 g + r) inside a V^T row: 64 s + 16 g + 4 tt + r
__device__ __forceinline__ uint32_t key_slot(uint32_t key) {
  return (key & ~63u) | (((key >> 2) & 3u) << 4) | (((key >> 4) & 3u) << 2) | (key & 3u);
}

// RN(x / b) for N pairs given r = RN(1 / b), nb = -b (Markstein: exact fma residual, see tq_device.h); chunks of 8 pairs
// keep the live stage arrays small
template <int N>
__device__ __forceinline__ void quot2_n(f32x2* x, f32x2 r, f32x2 nb) {
  constexpr int C = N < 4 ? N : 4;
  static_assert(N % C == 0, "pairs");
#pragma unroll
  for (int c = 0; c < N; c += C) {
    f32x2 q0[C], e[C];
#pragma unroll
    for (int i = 0; i < C; ++i) q0[i] = x[c + i] * r;
#pragma unroll
    for (int i = 0; i < C; ++i) e[i] = __builtin_elementwise_fma(q0[i], nb, x[c + i]);
#pragma unroll
    for (int i = 0; i < C; ++i) x[c + i] = __builtin_elementwise_fma(e[i], r, q0[i]);
  }
}

// exp_neg_ieee (tq_device.h) for N register pairs: the same single IEEE operations per element -- v_pk_mul / v_pk_fma /
// v_pk_add ARE the scalar operations on two lanes -- so every result is bit-identical to the scalar function and to
// tq_exp_neg of oracle/tq_int_oracle.c; 10.5 instead of 16 issue slots per element (round 6: the exponential was 30 % of the
// VALU instructions of a launch, profiles/r06/attention_pmc_*.json).  Stage by stage over chunks of 8 pairs.
template <int N>
__device__ __forceinline__ void exp_neg_ieee2_n(f32x2* x) {
  constexpr int C = N < 4 ? N : 4;
  static_assert(N % C == 0, "pairs");
  auto k2 = [](float c) { return f32x2{c, c}; };
#pragma unroll
  for (int c = 0; c < N; c += C) {
    f32x2 k[C], r[C], y[C];
#pragma unroll
    for (int i = 0; i < C; ++i) k[i] = x[c + i] * k2(1.44269504088896341f);
#pragma unroll
    for (int i = 0; i < C; ++i) k[i] = f32x2{rintf(k[i].x), rintf(k[i].y)};
#pragma unroll
    for (int i = 0; i < C; ++i) r[i] = __builtin_elementwise_fma(k[i], k2(-0.693359375f), x[c + i]);
#pragma unroll
    for (int i = 0; i < C; ++i) r[i] = __builtin_elementwise_fma(k[i], k2(2.12194440e-4f), r[i]);
#pragma unroll
    for (int i = 0; i < C; ++i) y[i] = __builtin_elementwise_fma(k2(1.9875691500e-4f), r[i], k2(1.3981999507e-3f));
#pragma unroll
    for (int i = 0; i < C; ++i) y[i] = __builtin_elementwise_fma(y[i], r[i], k2(8.3334519073e-3f));
#pragma unroll
    for (int i = 0; i < C; ++i) y[i] = __builtin_elementwise_fma(y[i], r[i], k2(4.1665795894e-2f));
#pragma unroll
    for (int i = 0; i < C; ++i) y[i] = __builtin_elementwise_fma(y[i], r[i], k2(1.6666665459e-1f));
#pragma unroll
    for (int i = 0; i < C; ++i) y[i] = __builtin_elementwise_fma(y[i], r[i], k2(5.0000001201e-1f));
#pragma unroll
    for (int i = 0; i < C; ++i) y[i] = __builtin_elementwise_fma(y[i], r[i] * r[i], r[i]);
#pragma unroll
    for (int i = 0; i < C; ++i) y[i] = y[i] + k2(1.0f);
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const float ex = ldexpf(y[i].x, (int)k[i].x), ey = ldexpf(y[i].y, (int)k[i].y);
      x[c + i].x = x[c + i].x < -86.0f ? 0.0f : ex;       // (NaN: see exp_neg_ieee)
      x[c + i].y = x[c + i].y < -86.0f ? 0.0f : ey;
    }
  }
}

// 4 x 4 byte transpose of four dwords: o[e] = bytes e of (r0, r1, r2, r3), r0 in the low byte.  v_perm_b32 selects
// bytes 0..3 from its SECOND source and 4..7 from its first: 8 instructions (shifts / masks / ors: ~24).
__device__ __forceinline__ void transpose4x4_b8(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t (&o)[4]) {
  const uint32_t t0 = __builtin_amdgcn_perm(r1, r0, 0x05010400u);      // r0.b0 r1.b0 r0.b1 r1.b1
  const uint32_t t1 = __builtin_amdgcn_perm(r1, r0, 0x07030602u);      // r0.b2 r1.b2 r0.b3 r1.b3
  const uint32_t t2 = __builtin_amdgcn_perm(r3, r2, 0x05010400u);
  const uint32_t t3 = __builtin_amdgcn_perm(r3, r2, 0x07030602u);
  o[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
  o[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
  o[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
  o[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

#ifdef TQ_ATTN_PROF
#define TQ_STAMP(k)                                                                                   \
  do {                                                                                                \
    unsigned long long t_;                                                                            \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
    if (threadIdx.x == 0 && p.prof) p.prof[blockIdx.x * 8 + (k)] = t_;                                \
  } while (0)
#else
#define TQ_STAMP(k)
#endif

// value of the other key-half wave (same queries) through LDS; one barrier
__device__ __forceinline__ float pair_exchange(float (*slot)[16], float v, int wave, int kh, int r16, int g) {
  if (g == 0) slot[kh * 2 + wave][r16] = v;
  __syncthreads();
  return slot[(kh ^ 1) * 2 + wave][r16];
}

// SPLIT: four waves per 32 queries -- wave (qh, kh) owns 16 queries x one half of the keys.  One wave issues one VALU
// instruction per 4 cycles, and a 16 x T score tile is ~45 T instructions per lane: with B * H * T / 32 workgroups below
// ~2 waves per SIMD (BERT-base at batch 8: 0.75) the kernel is the latency of that one chain, so halving it pays for
// the three exchanges through LDS (row max, row sum, the integer partial sums of the second GEMM -- all exact, the
// float sum a + b is the same value in both waves).
// (Round 6, measured and not kept -- profiles/r06/attn_qt_ab.txt: a wave taking TWO 16-query tiles one after the other, V^T
// staging and parameter derivation paid once per 32 queries: 1561 -> 1415 instructions per tile but 165 registers, 3 waves
// per SIMD instead of 4: -4 % at B = 64, +11 % at B = 128 and at T = 256.)
// QW = query waves per workgroup of the one-wave-per-row form (2, or 8 on large grids: round 6).  With 8 waves a workgroup
// owns 128 queries of its (batch, head): the V tile is fetched and transposed into LDS once per 128 queries instead of
// once per 32, and the K tiles of the eight waves come from the same CU's L1.  Same per-wave code and data: bit-identical.
template <int NT_ALL, int DH, bool SPLIT, int QW = kAttnWaves>   // NT_ALL = T / 16 key tiles, DH = head dim (32 or 64)
__global__ __launch_bounds__(SPLIT ? 2 * kAttnThreads : QW * kWave) void attention_i8_k(AttnArgs p) {
#define TQ_ATTN_RAGGED 0
#define TQ_ATTN_HEADS true
#include "tq_attention_i8_body.h"
#undef TQ_ATTN_HEADS
#undef TQ_ATTN_RAGGED
}

// The one instantiation that the run-time head offset of a per-head grid costs registers (116 instead of 114 VGPRs; every
// other kernel of the three families compiles to the allocation it had without the offset): the plain two-wave ragged
// form at T_pad = 128, head_dim 64.  It keeps the per-tensor fetch at element 0, and launches with a per-head grid at that
// form go to attention_i8_ragged_heads_k.
template <int NT_ALL, int DH, bool SPLIT, int QW>
constexpr bool kRaggedPerTensorOnly = NT_ALL == 8 && DH == 64 && !SPLIT && QW == kAttnWaves;

// the same body over sequences of p.T <= 16 NT_ALL rows (tq_attention_i8_ragged_fwd)
template <int NT_ALL, int DH, bool SPLIT, int QW = kAttnWaves>
__global__ __launch_bounds__(SPLIT ? 2 * kAttnThreads : QW * kWave) void attention_i8_ragged_k(AttnArgs p) {
#define TQ_ATTN_RAGGED 1
#define TQ_ATTN_HEADS (!kRaggedPerTensorOnly<NT_ALL, DH, SPLIT, QW>)
#include "tq_attention_i8_body.h"
#undef TQ_ATTN_HEADS
#undef TQ_ATTN_RAGGED
}

// attention_i8_ragged_k with the per-head fetch, instantiated where kRaggedPerTensorOnly holds (launch_ragged)
template <int NT_ALL, int DH, bool SPLIT, int QW = kAttnWaves>
__global__ __launch_bounds__(SPLIT ? 2 * kAttnThreads : QW * kWave) void attention_i8_ragged_heads_k(AttnArgs p) {
#define TQ_ATTN_RAGGED 1
#define TQ_ATTN_HEADS true
#include "tq_attention_i8_body.h"
#undef TQ_ATTN_HEADS
#undef TQ_ATTN_RAGGED
}

// the ragged body over PACKED sequences (tq_attention_i8_varlen_fwd): sequence b owns rows seq_start[b] .. seq_start[b + 1] - 1
// of buffers of total_rows rows, p.T is the host's bound on every length (T_cap <= 16 NT_ALL)
template <int NT_ALL, int DH, bool SPLIT, int QW = kAttnWaves>
__global__ __launch_bounds__(SPLIT ? 2 * kAttnThreads : QW * kWave) void attention_i8_varlen_k(
    AttnArgs p, const int32_t* __restrict__ seq_start, uint32_t total_rows) {
#define TQ_ATTN_RAGGED 2
#define TQ_ATTN_HEADS true
#include "tq_attention_i8_body.h"
#undef TQ_ATTN_HEADS
#undef TQ_ATTN_RAGGED
}

}  // namespace tq

using namespace tq;

// per_head: Q, K, V (and the context, checked in the launcher) may also carry per-column buffers of wide = H * head_dim
// elements in natural column order (inner == 1), read once per head at its first column
static int check_i8_grid(const tq_quantizer* q, const char* what, uint64_t wide = 0) {
  TQ_REQUIRE(q != nullptr && q->delta != nullptr && q->zero_float != nullptr, "tq_attention_i8_fwd: %s quantizer missing", what);
  if (wide != 0 && q->n_params != 1) {
    TQ_REQUIRE(q->n_params == wide && q->inner == 1,
               "tq_attention_i8_fwd: %s grid has n_params %llu, inner %llu (1, or H * head_dim = %llu per-column parameters with inner 1)",
               what, (unsigned long long)q->n_params, (unsigned long long)q->inner, (unsigned long long)wide);
    TQ_REQUIRE(!q->symmetric && !q->log_domain && q->n_bits >= 1 && q->n_bits <= 8,
               "tq_attention_i8_fwd: a per-head %s grid must be asymmetric, linear-domain, n_bits <= 8", what);
    return TQ_OK;
  }
  TQ_REQUIRE(!q->symmetric && !q->log_domain && q->n_params == 1 && q->n_bits >= 1 && q->n_bits <= 8,
             "tq_attention_i8_fwd: %s must be a per-tensor asymmetric linear-domain quantizer with n_bits <= 8", what);
  return TQ_OK;
}

extern "C" int tq_attention_i8_fwd(const int8_t* q_idx, const int8_t* k_idx, const int8_t* v_idx, float* ctx,
                                   int8_t* ctx_idx, uint64_t B, uint64_t T, uint64_t H, uint64_t head_dim,
                                   uint64_t qkv_row_stride, const float* mask, float denom, const tq_quantizer* q_q,
                                   const tq_quantizer* q_k, const tq_quantizer* q_v, const tq_quantizer* q_scores,
                                   const tq_quantizer* q_probs, const tq_quantizer* q_ctx, tq_stream_t stream) {
  return tq_attention_i8_strided_fwd(q_idx, k_idx, v_idx, ctx, ctx_idx, B, T, H, head_dim, qkv_row_stride, qkv_row_stride, mask,
                                     denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx, stream);
}

// The two-wave ragged launch: the per-tensor-only instantiation hands launches with a per-head grid to its twin
template <int NT_ALL, int DH, bool SPLIT>
static void launch_ragged(const AttnArgs& a, dim3 grid, dim3 block, hipStream_t st) {
  if constexpr (kRaggedPerTensorOnly<NT_ALL, DH, SPLIT, kAttnWaves>) {
    if (a.wide_q | a.wide_k | a.wide_v | a.wide_c) {
      hipLaunchKernelGGL((attention_i8_ragged_heads_k<NT_ALL, DH, SPLIT>), grid, block, 0, st, a);
      return;
    }
  }
  hipLaunchKernelGGL((attention_i8_ragged_k<NT_ALL, DH, SPLIT>), grid, block, 0, st, a);
}

// All entry points: the argument checks and the launch.  ragged: T is any length in 1..512 and the kernels are the ragged
// forms instantiated on T_pad = 64 ceil(T / 64) (mask rows start at b * T floats: 4-byte alignment is all they have).
// seq_start != NULL (with ragged): the packed forms -- T is the bound T_cap on every length, the buffers hold total_rows rows.
static int attention_i8_launch(const int8_t* q_idx, const int8_t* k_idx, const int8_t* v_idx, float* ctx, int8_t* ctx_idx,
                               uint64_t B, uint64_t T, uint64_t H, uint64_t head_dim, uint64_t qkv_row_stride,
                               uint64_t v_row_stride, const float* mask, float denom, const tq_quantizer* q_q,
                               const tq_quantizer* q_k, const tq_quantizer* q_v, const tq_quantizer* q_scores,
                               const tq_quantizer* q_probs, const tq_quantizer* q_ctx, tq_stream_t stream, bool ragged, const char* who,
                               const int32_t* seq_start = nullptr, uint64_t total_rows = 0) {
  if (B == 0 || T == 0 || H == 0) return TQ_OK;
  TQ_REQUIRE(q_idx && k_idx && v_idx && ctx, "%s: NULL pointer", who);
  TQ_REQUIRE(head_dim == 64 || head_dim == 32, "%s: head_dim %llu unsupported (32, 64)", who, (unsigned long long)head_dim);
  if (ragged) {
    TQ_REQUIRE(T <= 512, "%s: sequence length %llu unsupported (1 to 512)", who, (unsigned long long)T);
  } else {
    TQ_REQUIRE(T % 64 == 0 && T <= 512, "%s: sequence length %llu unsupported (multiples of 64 up to 512)", who,
               (unsigned long long)T);
  }
  const uint64_t T_pad = (T + 63) / 64 * 64;         // the key tiles of the launch (== T unless ragged)
  TQ_REQUIRE(aligned16(q_idx) && aligned16(k_idx) && aligned16(v_idx) && aligned16(ctx) &&
             (mask == nullptr || (ragged ? reinterpret_cast<uintptr_t>(mask) % 4 == 0 : aligned16(mask))) &&
             (ctx_idx == nullptr || (reinterpret_cast<uintptr_t>(ctx_idx) % 4) == 0),
             "%s: 16-byte alignment required", who);
  TQ_REQUIRE(denom != 0.0f, "%s: denom == 0", who);
  if (qkv_row_stride == 0) qkv_row_stride = H * head_dim;
  if (v_row_stride == 0) v_row_stride = H * head_dim;
  TQ_REQUIRE(qkv_row_stride >= H * head_dim && qkv_row_stride % 16 == 0 && qkv_row_stride < (1ull << 31),
             "%s: bad qkv_row_stride %llu", who, (unsigned long long)qkv_row_stride);
  TQ_REQUIRE(v_row_stride >= H * head_dim && v_row_stride % 16 == 0 && v_row_stride < (1ull << 31),
             "%s: bad v_row_stride %llu", who, (unsigned long long)v_row_stride);
  TQ_REQUIRE(B * H * (T_pad / (16 * kAttnWaves)) < (1ull << 31), "%s: too many tiles", who);
  const uint64_t wide_n = H * head_dim;               // parameters of a per-head grid: one per column, natural order
  if (int e = check_i8_grid(q_q, "query", wide_n)) return e;
  if (int e = check_i8_grid(q_k, "key", wide_n)) return e;
  if (int e = check_i8_grid(q_v, "value", wide_n)) return e;
  if (int e = check_i8_grid(q_probs, "probabilities")) return e;
  const uint64_t rows = seq_start ? total_rows : B * T;   // rows of q / k / v / ctx
  if (q_scores) {
    if (int e = check_quantizer(q_scores, B * H * T * T, who)) return e;
    TQ_REQUIRE(q_scores->n_params == 1, "%s: per-tensor score quantizer only", who);
  }
  if (q_ctx) {
    if (int e = check_quantizer(q_ctx, rows * H * head_dim, who)) return e;
    TQ_REQUIRE(q_ctx->n_params == 1 || (q_ctx->n_params == wide_n && q_ctx->inner == 1),
               "%s: context quantizer has n_params %llu, inner %llu (1, or H * head_dim = %llu per-column parameters with inner 1)",
               who, (unsigned long long)q_ctx->n_params, (unsigned long long)q_ctx->inner, (unsigned long long)wide_n);
    TQ_REQUIRE(q_ctx->n_params == 1 || (!q_ctx->symmetric && !q_ctx->log_domain),
               "%s: a per-head context grid must be asymmetric and linear-domain", who);
    TQ_REQUIRE(ctx_idx == nullptr || (!q_ctx->symmetric && q_ctx->n_bits <= 8),
               "%s: ctx_idx needs an asymmetric <= 8-bit context quantizer", who);
  } else {
    TQ_REQUIRE(ctx_idx == nullptr, "%s: ctx_idx needs q_ctx", who);
  }
  AttnArgs a{};
  a.q = q_idx; a.k = k_idx; a.v = v_idx; a.ctx = ctx; a.ctx_idx = ctx_idx; a.mask = mask;
  a.B = (uint32_t)B; a.T = (uint32_t)T; a.H = (uint32_t)H; a.in_stride = (uint32_t)qkv_row_stride; a.v_stride = (uint32_t)v_row_stride; a.denom = denom;
  a.qq = *q_q; a.qk = *q_k; a.qv = *q_v; a.q_probs = *q_probs;
  a.has_scores = q_scores != nullptr; a.has_ctx = q_ctx != nullptr;
  a.fast_ok = tuning("TQ_ATTN_FAST", 1);
#ifdef TQ_ATTN_PROF
  { const char* e = getenv("TQ_ATTN_PROF_PTR"); a.prof = e ? reinterpret_cast<unsigned long long*>(strtoull(e, nullptr, 0)) : nullptr; }
#endif
  if (q_scores) a.q_scores = *q_scores;
  if (q_ctx) a.q_ctx = *q_ctx;
  const auto is_wide = [](const tq_quantizer* q) { return q != nullptr && q->n_params != 1 ? 1u : 0u; };
  a.wide_q = is_wide(q_q); a.wide_k = is_wide(q_k); a.wide_v = is_wide(q_v); a.wide_c = is_wide(q_ctx);
  const unsigned grid = (unsigned)(B * H * (T_pad / (16 * kAttnWaves)));
  const uint32_t rows32 = (uint32_t)rows;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // key split (4 waves per 32 queries) while the plain grid leaves the SIMDs under ~2 waves each: T % 128 == 0 only
  const int split_env = tuning("TQ_ATTN_SPLIT", -1);     // read per call: the tests flip it
  const bool split = T_pad % 128 == 0 && (split_env >= 0 ? split_env != 0 : grid <= 1024);
  // eight query waves per workgroup (one V^T staging per 128 queries) whenever the keys are not split: T % 128 == 0 only
  // (profiles/r06/attn_qw_ab.txt: -3 % at B = 32, -7 % at B = 64, -9 % at B = 128, -10 % at T = 256, -20 % at T = 512)
  const int qw_env = tuning("TQ_ATTN_QW", -1);           // read per call: the tests flip it
  const bool wide = !split && T_pad % 128 == 0 && (qw_env >= 0 ? qw_env == 8 : true);
#define TQ_ATTN_LAUNCH(NTV, DHV, SP)                                                                             \
  do {                                                                                                           \
    const dim3 block((SP) ? 2 * kAttnThreads : kAttnThreads);                                                    \
    if (seq_start) hipLaunchKernelGGL((attention_i8_varlen_k<NTV, DHV, SP>), dim3(grid), block, 0, st, a, seq_start, rows32); \
    else if (ragged) launch_ragged<NTV, DHV, SP>(a, dim3(grid), block, st);                                      \
    else hipLaunchKernelGGL((attention_i8_k<NTV, DHV, SP>), dim3(grid), block, 0, st, a);                        \
  } while (0)
#define TQ_ATTN_LAUNCH8(NTV, DHV)                                                                                \
  do {                                                                                                           \
    if (seq_start) hipLaunchKernelGGL((attention_i8_varlen_k<NTV, DHV, false, 8>), dim3(grid / 4), dim3(8 * kWave), 0, st, a, seq_start, rows32); \
    else if (ragged) hipLaunchKernelGGL((attention_i8_ragged_k<NTV, DHV, false, 8>), dim3(grid / 4), dim3(8 * kWave), 0, st, a); \
    else hipLaunchKernelGGL((attention_i8_k<NTV, DHV, false, 8>), dim3(grid / 4), dim3(8 * kWave), 0, st, a);    \
  } while (0)
#define TQ_ATTN(NTV)                                                                                             \
  case NTV * 16:                                                                                                 \
    if constexpr ((NTV) % 8 == 0) {                                                                              \
      if (split) {                                                                                               \
        if (head_dim == 64) TQ_ATTN_LAUNCH(NTV, 64, true);                                                       \
        else TQ_ATTN_LAUNCH(NTV, 32, true);                                                                      \
        break;                                                                                                   \
      }                                                                                                          \
    }                                                                                                            \
    if constexpr ((NTV) % 8 == 0) {                                                                              \
      if (wide) {                                                                                                \
        if (head_dim == 64) TQ_ATTN_LAUNCH8(NTV, 64);                                                            \
        else TQ_ATTN_LAUNCH8(NTV, 32);                                                                           \
        break;                                                                                                   \
      }                                                                                                          \
    }                                                                                                            \
    if (head_dim == 64) TQ_ATTN_LAUNCH(NTV, 64, false);                                                          \
    else TQ_ATTN_LAUNCH(NTV, 32, false);                                                                         \
    break
  switch (T_pad) {
    TQ_ATTN(4); TQ_ATTN(8); TQ_ATTN(12); TQ_ATTN(16); TQ_ATTN(20); TQ_ATTN(24); TQ_ATTN(28); TQ_ATTN(32);
    default: return set_error(TQ_EUNSUPPORTED, "%s: sequence length %llu", who, (unsigned long long)T);
  }
#undef TQ_ATTN_LAUNCH
#undef TQ_ATTN_LAUNCH8
#undef TQ_ATTN
  return check_launch(seq_start ? "attention_i8_varlen_k" : ragged ? "attention_i8_ragged_k" : "attention_i8_k");
}

extern "C" int tq_attention_i8_strided_fwd(const int8_t* q_idx, const int8_t* k_idx, const int8_t* v_idx, float* ctx,
                                           int8_t* ctx_idx, uint64_t B, uint64_t T, uint64_t H, uint64_t head_dim,
                                           uint64_t qkv_row_stride, uint64_t v_row_stride, const float* mask, float denom,
                                           const tq_quantizer* q_q, const tq_quantizer* q_k, const tq_quantizer* q_v,
                                           const tq_quantizer* q_scores, const tq_quantizer* q_probs,
                                           const tq_quantizer* q_ctx, tq_stream_t stream) {
  return attention_i8_launch(q_idx, k_idx, v_idx, ctx, ctx_idx, B, T, H, head_dim, qkv_row_stride, v_row_stride, mask, denom, q_q,
                             q_k, q_v, q_scores, q_probs, q_ctx, stream, false, "tq_attention_i8_fwd");
}

// Any sequence length in 1..512 (include/tq_hip.h): whole multiples of 64 are the launch above -- unless the mask is not
// 16-byte aligned (the whole-tile kernels read it four keys at a time): then the ragged form runs with p.T == T_pad, where
// every clamp and pad test is a no-op and the result is the same bits.
extern "C" int tq_attention_i8_ragged_fwd(const int8_t* q_idx, const int8_t* k_idx, const int8_t* v_idx, float* ctx,
                                          int8_t* ctx_idx, uint64_t B, uint64_t T, uint64_t H, uint64_t head_dim,
                                          uint64_t qkv_row_stride, uint64_t v_row_stride, const float* mask, float denom,
                                          const tq_quantizer* q_q, const tq_quantizer* q_k, const tq_quantizer* q_v,
                                          const tq_quantizer* q_scores, const tq_quantizer* q_probs,
                                          const tq_quantizer* q_ctx, tq_stream_t stream) {
  return attention_i8_launch(q_idx, k_idx, v_idx, ctx, ctx_idx, B, T, H, head_dim, qkv_row_stride, v_row_stride, mask, denom, q_q,
                             q_k, q_v, q_scores, q_probs, q_ctx, stream,
                             T % 64 != 0 || (mask != nullptr && !aligned16(mask)), "tq_attention_i8_ragged_fwd");
}

// Packed sequences of any lengths <= T_cap <= 512 (include/tq_hip.h): the ragged kernels' body with the sequence's rows taken
// from seq_start, in the launch form the ragged entry picks for [B, T_cap] -- the same instructions as that launch on the
// batch padded to T_cap rows per sequence, hence the same bits.  Always the ragged form (also at T_cap % 64 == 0: the
// lengths differ from sequence to sequence).
extern "C" int tq_attention_i8_varlen_fwd(const int8_t* q_idx, const int8_t* k_idx, const int8_t* v_idx, float* ctx,
                                          int8_t* ctx_idx, const int32_t* seq_start, uint64_t B, uint64_t total_rows,
                                          uint64_t T_cap, uint64_t H, uint64_t head_dim, uint64_t qkv_row_stride,
                                          uint64_t v_row_stride, const float* mask, float denom, const tq_quantizer* q_q,
                                          const tq_quantizer* q_k, const tq_quantizer* q_v, const tq_quantizer* q_scores,
                                          const tq_quantizer* q_probs, const tq_quantizer* q_ctx, tq_stream_t stream) {
  const char* who = "tq_attention_i8_varlen_fwd";
  if (B == 0 || H == 0 || T_cap == 0 || total_rows == 0) return TQ_OK;
  TQ_REQUIRE(seq_start != nullptr && reinterpret_cast<uintptr_t>(seq_start) % 4 == 0, "%s: seq_start NULL or not 4-byte aligned", who);
  TQ_REQUIRE(total_rows < (1ull << 31), "%s: total_rows %llu unsupported (below 2^31)", who, (unsigned long long)total_rows);
  return attention_i8_launch(q_idx, k_idx, v_idx, ctx, ctx_idx, B, T_cap, H, head_dim, qkv_row_stride, v_row_stride, mask, denom,
                             q_q, q_k, q_v, q_scores, q_probs, q_ctx, stream, true, who, seq_start, total_rows);
}
