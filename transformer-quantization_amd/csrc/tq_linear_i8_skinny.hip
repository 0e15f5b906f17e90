// Integer Linear for SKINNY shapes (tq_linear_i8_skinny_fwd): few rows (1 <= M <= 256), any number of output features, K a
// multiple of 16 -- BERT's pooler (M = batch, 768 -> 768, Tanh) and classifier (M = batch, N = num_labels), which no tile of
// csrc/tq_linear_i8.hip covers and which therefore ran as fp32 GEMMs whose bits depend on the BLAS build.  The contraction is
// the same exact int32 sum as tq_linear_i8_fwd's, so its order is free and the matrix cores are not needed:
//
//   * one wave per (output column n, group of 8 rows); the groups of a column are neighbouring waves (W row from L2);
//   * lanes stride over K in 16-byte chunks; a lane loads its W chunk ONCE and multiplies it into the 8 x rows
//     (4 v_dot4 per row and chunk); rows past M re-read row M - 1 (in bounds, result dropped);
//   * a butterfly over the wave leaves all 8 sums in every lane; lanes 0..7 run the epilogue for one row each and store with
//     element-sized vector stores (y / y_idx need element alignment only: N = 2 has unaligned rows).
//
// Epilogue = oracle/tq_int_oracle.c (lin_pre, act_fn codes 0 / 1 / 4 / tanh in float64, q_index, q_dequant) operation by
// operation: M * N is a few thousand outputs, so the float64 activation and the IEEE division per output cost nothing and
// give ONE definition at every shape (no staircase table, no fit).  In its own translation unit: the register allocation of
// the tiled kernels does not see it.
#include <algorithm>

#include "tq_device.h"
#include "tq_host.h"

namespace tq {

typedef int v4i __attribute__((ext_vector_type(4)));

enum { SK_ACT_NONE = 0, SK_ACT_RELU = 1, SK_ACT_GELU = 2, SK_ACT_TANH = 3 };

constexpr int kSkRows = 8;                       // rows per wave
constexpr uint64_t kSkMaxM = 256, kSkMaxK = 16384;

struct SkinnyArgs {
  const int8_t* x;        // row m at x + m * x_stride: int8(index - 128)
  uint64_t x_stride;
  const int8_t* w;        // [N, K]
  const int32_t* w_rowsum;
  const float* bias;      // [N] or null
  void* y;                // [M, N] or null (index-only)
  int8_t* y_idx;          // [M, N] or null
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

__device__ __forceinline__ float skinny_act(float pre, int act) {
  switch (act) {   // wave-uniform
    case SK_ACT_RELU: return pre > 0.0f ? pre : 0.0f;
    case SK_ACT_GELU: {                                   // correctly rounded erf form: csrc/tq_stair.hip act64, oracle code 4
      const double v = (double)pre;
      return (float)(0.5 * v * (1.0 + erf(v * 0.70710678118654752440)));
    }
    case SK_ACT_TANH: return (float)tanh((double)pre);
    default: return pre;
  }
}

template <int YDT>
__global__ __launch_bounds__(kBlock) void linear_i8_skinny_k(SkinnyArgs p) {
  const int lane = threadIdx.x & 63;
  // one batch of parameter loads, pinned below once the first operand chunk is on its way
  float dx = p.x_delta[0], zx = p.x_zero_float[0];
  QRaw qr = load_qraw(p.q_out, 0, p.x_delta);            // has_q == 0: reads x_delta, unused

  const uint32_t groups = (p.M + kSkRows - 1) / kSkRows;
  const uint64_t pairs = (uint64_t)p.N * groups;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const uint32_t chunks = p.K / 16;
  uint64_t pair = (uint64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (pair >= pairs) return;

  dx = pinned_uniform(dx);
  zx = pinned_uniform(zx);
  qraw_arrived(qr);
  const float sx = dx < p.x_eps ? p.x_eps : dx;
  const int shift = 128 - (int)clamp_nanprop(rintf(zx), 0.0f, grid_top_small(p.x_n_bits));
  QP qo = QP{1.0f, 0.0f, 0.0f, 0.0f};
  if (p.has_q) qo = qp_from_raw(p.q_out, qr);

  for (; pair < pairs; pair += n_waves) {
    const uint32_t n = (uint32_t)(pair / groups), m0 = (uint32_t)(pair % groups) * kSkRows;
    const int8_t* wp = p.w + (size_t)n * p.K;
    const int8_t* xr[kSkRows];
#pragma unroll
    for (int r = 0; r < kSkRows; ++r) {
      const uint32_t m = m0 + r < p.M ? m0 + r : p.M - 1;
      xr[r] = p.x + (size_t)m * p.x_stride;
    }
    int acc[kSkRows];
#pragma unroll
    for (int r = 0; r < kSkRows; ++r) acc[r] = 0;
    for (uint32_t c = lane; c < chunks; c += kWave) {
      const v4i wv = *reinterpret_cast<const v4i*>(wp + (size_t)c * 16);
#pragma unroll
      for (int r = 0; r < kSkRows; ++r) {
        const v4i xv = *reinterpret_cast<const v4i*>(xr[r] + (size_t)c * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r] = __builtin_amdgcn_sdot4(xv[e], wv[e], acc[r], false);
      }
    }
#pragma unroll
    for (int r = 0; r < kSkRows; ++r) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[r] += __shfl_xor(acc[r], o, 64);
    }
    int mine = acc[0];
#pragma unroll
    for (int r = 1; r < kSkRows; ++r) mine = lane == r ? acc[r] : mine;
    const uint32_t m = m0 + lane;
    if (lane < kSkRows && m < p.M) {
      const int tot = mine + p.w_rowsum[n] * shift;
      const float dw = p.w_delta[p.w_n_params == 1 ? 0 : n];
      const float sw = sx * (dw < p.w_eps ? p.w_eps : dw);
      const float b = p.bias != nullptr ? p.bias[n] : 0.0f;
      float v = (float)tot * sw + b;                      // separate mul and add (-ffp-contract=off)
      v = skinny_act(v, p.act);
      const size_t at = (size_t)m * p.N + n;
      if (p.has_q) {
        const float xi = q_index(v, qo);
        v = q_dequant(xi, qo);
        if (p.y_idx != nullptr) p.y_idx[at] = (int8_t)((int)xi - 128);
      }
      if (p.y != nullptr) Store<YDT>::store1(static_cast<typename Store<YDT>::elem_t*>(p.y) + at, v);
    }
  }
}

}  // namespace tq

using namespace tq;

extern "C" int tq_linear_i8_skinny_fwd(const int8_t* x_idx, uint64_t x_row_stride, const int8_t* w_idx, const int32_t* w_rowsum,
                                       const float* bias, void* y, int8_t* y_idx, int y_dtype, uint64_t M, uint64_t N, uint64_t K,
                                       const float* x_delta, const float* x_zero_float, int x_n_bits, float x_eps,
                                       const float* w_delta, uint64_t w_n_params, float w_eps, int activation,
                                       const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_linear_i8_skinny_fwd";
  if (M == 0 || N == 0) return TQ_OK;
  TQ_REQUIRE(x_idx && w_idx && w_rowsum && (y || y_idx) && x_delta && x_zero_float && w_delta, "%s: NULL pointer", who);
  TQ_REQUIRE(y_dtype == TQ_F32 || y_dtype == TQ_BF16, "%s: y dtype must be fp32 or bf16", who);
  TQ_REQUIRE(M <= kSkMaxM && N < (1ull << 31) && K % 16 == 0 && K >= 16 && K <= kSkMaxK,
             "%s: unsupported shape M=%llu N=%llu K=%llu (1 <= M <= 256, N < 2^31, K %% 16, 16 <= K <= 16384)", who,
             (unsigned long long)M, (unsigned long long)N, (unsigned long long)K);
  const uint64_t stride = x_row_stride == 0 ? K : x_row_stride;
  TQ_REQUIRE(stride >= K && stride % 16 == 0 && stride < (1ull << 40),
             "%s: x_row_stride %llu must be 0 or a multiple of 16 that is >= K", who, (unsigned long long)x_row_stride);
  TQ_REQUIRE(x_n_bits >= 1 && x_n_bits <= 8, "%s: input quantizer must have <= 8 bits", who);
  TQ_REQUIRE(w_n_params == 1 || w_n_params == N, "%s: weight scales must be per-tensor or per-output-channel", who);
  TQ_REQUIRE(activation >= SK_ACT_NONE && activation <= SK_ACT_TANH, "%s: unknown activation %d", who, activation);
  TQ_REQUIRE(aligned16(x_idx) && aligned16(w_idx), "%s: 16-byte alignment required for x_idx and w_idx", who);
  const size_t es = elem_size(y_dtype);
  TQ_REQUIRE(y == nullptr || reinterpret_cast<uintptr_t>(y) % es == 0, "%s: y must be aligned to its element size", who);
  TQ_REQUIRE(y_idx == nullptr || (q_out != nullptr && !q_out->symmetric && q_out->n_bits <= 8),
             "%s: y_idx needs an asymmetric <= 8-bit output quantizer", who);
  SkinnyArgs a{};
  a.has_q = q_out != nullptr;
  if (q_out != nullptr) {
    if (int e = check_quantizer(q_out, M * N, who)) return e;
    TQ_REQUIRE(q_out->n_params == 1, "%s: per-tensor output quantizer only", who);
    a.q_out = *q_out;
  }
  a.x = x_idx; a.x_stride = stride; a.w = w_idx; a.w_rowsum = w_rowsum; a.bias = bias; a.y = y; a.y_idx = y_idx;
  a.M = (uint32_t)M; a.N = (uint32_t)N; a.K = (uint32_t)K;
  a.x_delta = x_delta; a.x_zero_float = x_zero_float; a.x_eps = x_eps; a.x_n_bits = x_n_bits;
  a.w_delta = w_delta; a.w_n_params = (uint32_t)w_n_params; a.w_eps = w_eps; a.act = activation;
  // one wave per (column, row group); beyond kMaxGrid * 16 blocks the waves stride over the pairs
  const uint64_t pairs = N * ceil_div(M, kSkRows);
  const uint64_t blocks = std::min<uint64_t>(ceil_div(pairs, kBlock / kWave), (uint64_t)kMaxGrid * 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (y_dtype == TQ_F32)
    hipLaunchKernelGGL(linear_i8_skinny_k<TQ_F32>, dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(linear_i8_skinny_k<TQ_BF16>, dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
  return check_launch("linear_i8_skinny_k");
}
