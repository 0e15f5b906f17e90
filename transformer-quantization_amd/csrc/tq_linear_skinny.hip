// Integer Linear for SKINNY shapes (tq_linear_i8_skinny_fwd, tq_linear_i16x8_skinny_fwd): few rows (1 <= M <= 256), any number of
// output features, K a multiple of 16 -- BERT's pooler (M = batch, 768 -> 768, Tanh) and classifier (M = batch, N = num_labels),
// which no tile of csrc/tq_linear_i8.hip covers and which would otherwise run as fp32 GEMMs whose bits depend on the BLAS
// build.  The input may be two byte planes of a <= 16-bit grid (the mixed-precision recipes: 'P': 16 puts the classifier's input
// on a 16-bit grid) and its rows may come from a device row table (packed batches: the first token of sequence b is row
// seq_start[b] of the [M, d] hidden state).  The 8-bit entry is the 16-bit entry without planes and without a row table: one
// check-and-launch function and one kernel template serve both.  The contraction is the same exact int32 sum as
// tq_linear_i8_fwd's, so its order is free and the matrix cores are not needed:
//
//   * one wave per (output column n, group of 8 rows); the groups of a column are neighbouring waves (W row from L2);
//   * lanes stride over K in 16-byte chunks; a lane loads its W chunk ONCE and multiplies it into the 8 rows' chunks -- 4 v_dot4
//     per row and chunk into one int32 accumulator (8-bit form, HI = false), 8 into two (A_hi, A_lo) with the hi plane; rows
//     past M re-read row M - 1 (in bounds, result dropped);
//   * a butterfly over the wave leaves all 8 sums in every lane; lanes 0..7 run the epilogue for one row each and store with
//     element-sized vector stores, byte stores for the index planes (y and the planes need element alignment only: N = 2 has
//     unaligned rows).
// The up-to-8 row numbers of a wave are wave-uniform: they are requested with the parameter loads (one memory round trip for
// the lot) and pinned to scalar registers, since every x address depends on them.  A row number is
// clamped to [0, x_n_rows - 1] (to [0, M - 1] without a table, which no row reaches): an inconsistent table gives wrong
// results, never an access outside the x_n_rows rows.
//
//   HI:   tot = 256 A_hi + A_lo + (32896 - z_x) rowsum    exact in double (integers below 2^53), ONE rounding to fp32 -- the
//         arithmetic of linear_i16x8_k (csrc/tq_linear_i8.hip, X16), so that both give the same bits where both take the shape
//   else: tot = A_lo + (128 - z_x) rowsum                 int32
// Epilogue behind `pre` = oracle/tq_int_oracle.c (lin_pre, act_fn codes 0 / 1 / 4 / tanh in float64, q_index, q_dequant)
// operation by operation: M * N is a few thousand outputs, so the float64 activation and the IEEE division per output cost
// nothing and give ONE definition at every shape (no staircase table, no fit).  In its own translation unit: the register
// allocation of the tiled kernels does not see it.
#include <algorithm>

#include "tq_device.h"
#include "tq_host.h"

namespace tq {

typedef int v4i __attribute__((ext_vector_type(4)));

enum { SK_ACT_NONE = 0, SK_ACT_RELU = 1, SK_ACT_GELU = 2, SK_ACT_TANH = 3 };

constexpr int kSkRows = 8;                       // rows per wave
constexpr uint64_t kSkMaxM = 256, kSkMaxK = 16384;

struct Skinny16Args {
  const int8_t* x_hi;     // hi plane or null (8-bit form); row r at x_* + r * x_stride
  const int8_t* x_lo;
  uint64_t x_stride;
  const int32_t* x_rows;  // [M] row numbers or null (row m is m)
  uint32_t x_row_top;     // x_n_rows - 1
  const int8_t* w;        // [N, K]
  const int32_t* w_rowsum;
  const float* bias;      // [N] or null
  void* y;                // [M, N] or null
  int8_t* y_hi;           // [M, N] or null
  int8_t* y_lo;           // [M, N] or null
  uint32_t M, N, K;
  const float* x_delta;
  const float* x_zero_float;
  float x_eps;
  int x_n_bits;
  const float* w_delta;   // [1] or [N]
  uint32_t w_n_params;
  float w_eps;
  int act;
  int has_q;
  tq_quantizer q_out;
};

__device__ __forceinline__ float skinny16_act(float pre, int act) {
  switch (act) {   // wave-uniform
    case SK_ACT_RELU: return pre > 0.0f ? pre : 0.0f;
    case SK_ACT_GELU: {                                  // correctly rounded erf form: csrc/tq_stair.hip act64, oracle code 4
      const double v = (double)pre;
      return (float)(0.5 * v * (1.0 + erf(v * 0.70710678118654752440)));
    }
    case SK_ACT_TANH: return (float)tanh((double)pre);
    default: return pre;
  }
}

__device__ __forceinline__ uint32_t pinned_uniform_u32(uint32_t v) {
  uint32_t b = __builtin_amdgcn_readfirstlane(v);
  asm volatile("" : "+s"(b));
  return b;
}

// the (unclamped) row numbers of rows m0 .. m0 + 7: loads with a table, m itself without
__device__ __forceinline__ void skinny16_fetch_rows(const Skinny16Args& p, uint32_t m0, int32_t (&rows)[kSkRows]) {
#pragma unroll
  for (int r = 0; r < kSkRows; ++r) {
    const uint32_t m = m0 + r < p.M ? m0 + r : p.M - 1;
    rows[r] = p.x_rows != nullptr ? p.x_rows[m] : (int32_t)m;
  }
}

template <int YDT, bool HI>
__global__ __launch_bounds__(kBlock) void linear_i16x8_skinny_k(Skinny16Args p) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t groups = (p.M + kSkRows - 1) / kSkRows;
  const uint64_t pairs = (uint64_t)p.N * groups;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t chunks = p.K / 16;
  uint64_t pair = (uint64_t)blockIdx.x * (kBlock / kWave) + wave;
  if (pair >= pairs) return;

  // one batch of parameter loads with the first pair's row numbers among them, pinned below
  float dx = p.x_delta[0], zx = p.x_zero_float[0];
  QRaw qr = load_qraw(p.q_out, 0, p.x_delta);            // has_q == 0: reads x_delta, unused
  int32_t rows[kSkRows];
  skinny16_fetch_rows(p, (uint32_t)(pair % groups) * kSkRows, rows);

  dx = pinned_uniform(dx);
  zx = pinned_uniform(zx);
  qraw_arrived(qr);
  const float sx = dx < p.x_eps ? p.x_eps : dx;
  const int shift = 128 - (int)clamp_nanprop(rintf(zx), 0.0f, grid_top_small(p.x_n_bits));
  QP qo = QP{1.0f, 0.0f, 0.0f, 0.0f};
  if (p.has_q) qo = qp_from_raw(p.q_out, qr);

  for (;;) {
    const uint32_t n = (uint32_t)(pair / groups), m0 = (uint32_t)(pair % groups) * kSkRows;
    const int8_t* wp = p.w + (size_t)n * p.K;
    uint64_t xo[kSkRows];                               // byte offset of the row in both planes (scalar)
#pragma unroll
    for (int r = 0; r < kSkRows; ++r) {
      int32_t row = (int32_t)pinned_uniform_u32((uint32_t)rows[r]);
      row = row < 0 ? 0 : row;
      const uint32_t ru = (uint32_t)row > p.x_row_top ? p.x_row_top : (uint32_t)row;
      xo[r] = (uint64_t)ru * p.x_stride;
    }
    int acc[kSkRows], acc_hi[HI ? kSkRows : 1];
#pragma unroll
    for (int r = 0; r < kSkRows; ++r) acc[r] = 0;
#pragma unroll
    for (int r = 0; r < (HI ? kSkRows : 1); ++r) acc_hi[r] = 0;
    for (uint32_t c = lane; c < chunks; c += kWave) {
      // all loads of the chunk first (9 or 17 in flight), then the dot products
      const v4i wv = *reinterpret_cast<const v4i*>(wp + (size_t)c * 16);
      v4i xl[kSkRows], xh[HI ? kSkRows : 1];
#pragma unroll
      for (int r = 0; r < kSkRows; ++r) xl[r] = *reinterpret_cast<const v4i*>(p.x_lo + xo[r] + (size_t)c * 16);
      if (HI) {
#pragma unroll
        for (int r = 0; r < (HI ? kSkRows : 1); ++r) xh[r] = *reinterpret_cast<const v4i*>(p.x_hi + xo[r] + (size_t)c * 16);
      }
#pragma unroll
      for (int r = 0; r < kSkRows; ++r) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r] = __builtin_amdgcn_sdot4(xl[r][e], wv[e], acc[r], false);
      }
      if (HI) {
#pragma unroll
        for (int r = 0; r < (HI ? kSkRows : 1); ++r) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc_hi[r] = __builtin_amdgcn_sdot4(xh[r][e], wv[e], acc_hi[r], false);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kSkRows; ++r) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o, 64);
    }
    if (HI) {
#pragma unroll
      for (int r = 0; r < (HI ? kSkRows : 1); ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc_hi[r] += __shfl_xor(acc_hi[r], o, 64);
      }
    }
    int mine = acc[0], mine_hi = acc_hi[0];
#pragma unroll
    for (int r = 1; r < kSkRows; ++r) {
      mine = lane == r ? acc[r] : mine;
      if (HI) mine_hi = lane == r ? acc_hi[HI ? r : 0] : mine_hi;
    }
    const uint32_t m = m0 + lane;
    if (lane < kSkRows && m < p.M) {
      const int rs = p.w_rowsum[n];
      float ft;
      if (HI) {
        // |tot| up to ~2^37: every term and the sum are integers below 2^53 (the fma's product included), one rounding
        const double tot = __builtin_fma((double)mine_hi, 256.0, (double)mine) + (double)rs * (double)(shift + 32768);
        ft = (float)tot;
      } else {
        ft = (float)(mine + rs * shift);
      }
      const float dw = p.w_delta[p.w_n_params == 1 ? 0 : n];
      const float sw = sx * (dw < p.w_eps ? p.w_eps : dw);
      const float b = p.bias != nullptr ? p.bias[n] : 0.0f;
      float v = ft * sw + b;                              // separate mul and add (-ffp-contract=off)
      v = skinny16_act(v, p.act);
      const size_t at = (size_t)m * p.N + n;
      if (p.has_q) {
        const float xi = q_index(v, qo);
        v = q_dequant(xi, qo);
        const uint32_t idx = (uint32_t)(int32_t)xi;        // b - 128 as a byte: top bit flipped (csrc/tq_quantize_hilo.hip)
        if (p.y_lo != nullptr) p.y_lo[at] = (int8_t)(int)((idx & 255u) ^ 128u);
        if (p.y_hi != nullptr) p.y_hi[at] = (int8_t)(int)(((idx >> 8) & 255u) ^ 128u);
      }
      if (p.y != nullptr) Store<YDT>::store1(static_cast<typename Store<YDT>::elem_t*>(p.y) + at, v);
    }
    pair += n_waves;
    if (pair >= pairs) break;
    skinny16_fetch_rows(p, (uint32_t)(pair % groups) * kSkRows, rows);
  }
}

template <int YDT>
static int launch_skinny16(const Skinny16Args& a, unsigned blocks, hipStream_t st) {
  if (a.x_hi != nullptr)
    hipLaunchKernelGGL((linear_i16x8_skinny_k<YDT, true>), dim3(blocks), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((linear_i16x8_skinny_k<YDT, false>), dim3(blocks), dim3(kBlock), 0, st, a);
  return check_launch("linear_i16x8_skinny_k");
}

// Every argument check (all of them before any device access), then the launch, for both C entries: `who` is the entry's name.
static int skinny_fwd(const char* who, const int8_t* x_hi, const int8_t* x_lo, uint64_t x_row_stride, const int32_t* x_rows,
                      uint64_t x_n_rows, const int8_t* w_idx, const int32_t* w_rowsum, const float* bias, void* y, int8_t* y_hi,
                      int8_t* y_lo, int y_dtype, uint64_t M, uint64_t N, uint64_t K, const float* x_delta,
                      const float* x_zero_float, int x_n_bits, float x_eps, const float* w_delta, uint64_t w_n_params,
                      float w_eps, int activation, const tq_quantizer* q_out, tq_stream_t stream) {
  if (M == 0 || N == 0) return TQ_OK;
  TQ_REQUIRE(x_lo && w_idx && w_rowsum && (y || y_lo) && x_delta && x_zero_float && w_delta, "%s: NULL pointer", who);
  TQ_REQUIRE(y_hi == nullptr || y_lo != nullptr, "%s: y_hi needs y_lo (the index is both planes)", who);
  TQ_REQUIRE(y_dtype == TQ_F32 || y_dtype == TQ_BF16, "%s: y dtype must be fp32 or bf16", who);
  TQ_REQUIRE(M <= kSkMaxM && N < (1ull << 31) && K % 16 == 0 && K >= 16 && K <= kSkMaxK,
             "%s: unsupported shape M=%llu N=%llu K=%llu (1 <= M <= 256, N < 2^31, K %% 16, 16 <= K <= 16384)", who,
             (unsigned long long)M, (unsigned long long)N, (unsigned long long)K);
  const uint64_t stride = x_row_stride == 0 ? K : x_row_stride;
  TQ_REQUIRE(stride >= K && stride % 16 == 0 && stride < (1ull << 40),
             "%s: x_row_stride %llu must be 0 or a multiple of 16 that is >= K", who, (unsigned long long)x_row_stride);
  if (x_rows != nullptr) {
    TQ_REQUIRE(reinterpret_cast<uintptr_t>(x_rows) % 4 == 0, "%s: x_rows must be 4-byte aligned", who);
    TQ_REQUIRE(x_n_rows >= 1 && x_n_rows <= (1ull << 31) && x_n_rows <= (1ull << 56) / stride,
               "%s: x_n_rows %llu must be in [1, 2^31] with x_n_rows * stride <= 2^56", who, (unsigned long long)x_n_rows);
  }
  TQ_REQUIRE(x_n_bits >= 1 && x_n_bits <= (x_hi != nullptr ? 16 : 8),
             "%s: input quantizer must have <= 8 bits (<= 16 with the hi plane)", who);
  TQ_REQUIRE(w_n_params == 1 || w_n_params == N, "%s: weight scales must be per-tensor or per-output-channel", who);
  TQ_REQUIRE(activation >= SK_ACT_NONE && activation <= SK_ACT_TANH, "%s: unknown activation %d", who, activation);
  TQ_REQUIRE((x_hi == nullptr || aligned16(x_hi)) && aligned16(x_lo) && aligned16(w_idx),
             "%s: 16-byte alignment required for the x planes and w_idx", who);
  const size_t es = elem_size(y_dtype);
  TQ_REQUIRE(y == nullptr || reinterpret_cast<uintptr_t>(y) % es == 0, "%s: y must be aligned to its element size", who);
  if (y_hi != nullptr)
    TQ_REQUIRE(q_out != nullptr && !q_out->symmetric && !q_out->log_domain && q_out->n_bits <= 16,
               "%s: index planes need an asymmetric linear-domain <= 16-bit output quantizer", who);
  else
    TQ_REQUIRE(y_lo == nullptr || (q_out != nullptr && !q_out->symmetric && q_out->n_bits <= 8),
               "%s: y_lo alone needs an asymmetric <= 8-bit output quantizer", who);
  Skinny16Args a{};
  a.has_q = q_out != nullptr;
  if (q_out != nullptr) {
    if (int e = check_quantizer(q_out, M * N, who)) return e;
    TQ_REQUIRE(q_out->n_params == 1, "%s: per-tensor output quantizer only", who);
    a.q_out = *q_out;
  }
  a.x_hi = x_hi; a.x_lo = x_lo; a.x_stride = stride; a.x_rows = x_rows;
  a.x_row_top = x_rows != nullptr ? (uint32_t)(x_n_rows - 1) : (uint32_t)(M - 1);
  a.w = w_idx; a.w_rowsum = w_rowsum; a.bias = bias; a.y = y; a.y_hi = y_hi; a.y_lo = y_lo;
  a.M = (uint32_t)M; a.N = (uint32_t)N; a.K = (uint32_t)K;
  a.x_delta = x_delta; a.x_zero_float = x_zero_float; a.x_eps = x_eps; a.x_n_bits = x_n_bits;
  a.w_delta = w_delta; a.w_n_params = (uint32_t)w_n_params; a.w_eps = w_eps; a.act = activation;
  // one wave per (column, row group); beyond kMaxGrid * 16 blocks the waves stride over the pairs
  const uint64_t pairs = N * ceil_div(M, kSkRows);
  const unsigned blocks = (unsigned)std::min<uint64_t>(ceil_div(pairs, kBlock / kWave), (uint64_t)kMaxGrid * 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return y_dtype == TQ_F32 ? launch_skinny16<TQ_F32>(a, blocks, st) : launch_skinny16<TQ_BF16>(a, blocks, st);
}

}  // namespace tq

using namespace tq;

extern "C" int tq_linear_i16x8_skinny_fwd(const int8_t* x_hi, const int8_t* x_lo, uint64_t x_row_stride, const int32_t* x_rows,
                                          uint64_t x_n_rows, const int8_t* w_idx, const int32_t* w_rowsum, const float* bias,
                                          void* y, int8_t* y_hi, int8_t* y_lo, int y_dtype, uint64_t M, uint64_t N, uint64_t K,
                                          const float* x_delta, const float* x_zero_float, int x_n_bits, float x_eps,
                                          const float* w_delta, uint64_t w_n_params, float w_eps, int activation,
                                          const tq_quantizer* q_out, tq_stream_t stream) {
  return skinny_fwd("tq_linear_i16x8_skinny_fwd", x_hi, x_lo, x_row_stride, x_rows, x_n_rows, w_idx, w_rowsum, bias, y, y_hi,
                    y_lo, y_dtype, M, N, K, x_delta, x_zero_float, x_n_bits, x_eps, w_delta, w_n_params, w_eps, activation,
                    q_out, stream);
}

// the 16-bit entry without planes and without a row table
extern "C" int tq_linear_i8_skinny_fwd(const int8_t* x_idx, uint64_t x_row_stride, const int8_t* w_idx, const int32_t* w_rowsum,
                                       const float* bias, void* y, int8_t* y_idx, int y_dtype, uint64_t M, uint64_t N, uint64_t K,
                                       const float* x_delta, const float* x_zero_float, int x_n_bits, float x_eps,
                                       const float* w_delta, uint64_t w_n_params, float w_eps, int activation,
                                       const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_linear_i8_skinny_fwd";
  // the one check whose message names an argument that only this entry has (skinny_fwd would say y_lo)
  if (M != 0 && N != 0)
    TQ_REQUIRE(y_idx == nullptr || (q_out != nullptr && !q_out->symmetric && q_out->n_bits <= 8),
               "%s: y_idx needs an asymmetric <= 8-bit output quantizer", who);
  return skinny_fwd(who, nullptr, x_idx, x_row_stride, nullptr, 0, w_idx, w_rowsum, bias, y, nullptr, y_idx, y_dtype, M, N, K,
                    x_delta, x_zero_float, x_n_bits, x_eps, w_delta, w_n_params, w_eps, activation, q_out, stream);
}
