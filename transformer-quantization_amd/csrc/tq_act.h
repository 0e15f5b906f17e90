// What the Linear-epilogue training pairs share (csrc/tq_act_bwd.hip: per-tensor output quantizer; csrc/tq_act_axis_bwd.hip: one
// parameter per column): the activation function with its derivative, the strip grid and the argument checks.  The text is
// tq_act_bwd.hip's, moved here unchanged; the bounds of the GELU evaluation are stated at the head of that file.
#pragma once

#include <algorithm>

#include "tq_device.h"
#include "tq_host.h"

namespace tq {

constexpr int kActStripVec = 64;                 // 16-byte vectors per strip: one wave
constexpr int kActGroups = kBlock / kActStripVec;   // row groups per block
constexpr unsigned kActMaxBlocks = 2048;

// E = erf(a / sqrt 2): gelu_erf_n of csrc/tq_linear_i8.hip for one value
__device__ __forceinline__ float erf_fit(float v) {
  const float a = v * 0.70710678118654752440f;
  const float t = fabsf(a);
  float q = __builtin_fmaf(t, -4.5358574425335974e-05f, 0.00044550743768922985f);
  q = __builtin_fmaf(t, q, -0.0014894409105181694f);
  q = __builtin_fmaf(t, q, -0.0007746309274807572f);
  q = __builtin_fmaf(t, q, 0.02825368195772171f);
  q = __builtin_fmaf(t, q, -0.14848162233829498f);
  q = __builtin_fmaf(t, q, -0.9184163808822632f);
  q = __builtin_fmaf(t, q, -1.6279085874557495f);
  q = q * t;
  const float e = 1.0f - __builtin_amdgcn_exp2f(q);
  return __builtin_copysignf(e, a);
}

// h = act(a); DERIV: also dact = act'(a)
template <int ACT, bool DERIV>
__device__ __forceinline__ float act_eval(float a, float& dact) {
  dact = 1.0f;
  if (ACT == TQ_ACT_RELU) {
    if (DERIV) dact = a > 0.0f ? 1.0f : 0.0f;
    return a <= 0.0f ? 0.0f : a;
  }
  if (ACT == TQ_ACT_GELU) {
    const float one_e = 1.0f + erf_fit(a);
    if (DERIV) {
      const float phi = __builtin_amdgcn_exp2f((a * a) * -0.72134752044448170368f) * 0.39894228040143267794f;
      const float ap = fabsf(a) < 14.0f ? a * phi : 0.0f;
      dact = 0.5f * one_e + ap;
    }
    return (a * 0.5f) * one_e;
  }
  return a;
}

// ---- host side
struct ActGrid {
  uint64_t nvec;
  unsigned strips, chunks;
};

inline ActGrid act_grid(uint64_t rows, uint64_t cols) {
  ActGrid g;
  g.nvec = cols / 4;
  g.strips = (unsigned)ceil_div(g.nvec, kActStripVec);
  g.chunks = (unsigned)std::min<uint64_t>(ceil_div(rows, kActGroups), std::max<unsigned>(1u, kActMaxBlocks / std::max(g.strips, 1u)));
  return g;
}

// the checks every entry of both pairs shares, up to the quantizer's own (check_quantizer); -> TQ_OK with rows, cols > 0.  What a
// pair asks of the quantizer's layout comes behind it, in the pair's file.
inline int act_check(const char* who, const float* gemm, const float* bias, uint64_t rows, uint64_t cols, int act, const tq_quantizer* q) {
  TQ_REQUIRE(act == TQ_ACT_NONE || act == TQ_ACT_RELU || act == TQ_ACT_GELU, "%s: activation %d unsupported (none, relu, gelu)", who, act);
  TQ_REQUIRE(cols > 0 && cols % 4 == 0, "%s: cols=%llu must be a positive multiple of 4", who, (unsigned long long)cols);
  TQ_REQUIRE(cols <= (1ull << 32) && rows <= (1ull << 62) / cols, "%s: shape too large", who);
  TQ_REQUIRE(gemm != nullptr, "%s: NULL pointer", who);
  TQ_REQUIRE(aligned16(gemm) && aligned16(bias), "%s: 16-byte alignment required", who);
  if (q != nullptr) {
    if (int e = check_quantizer(q, rows * cols, who)) return e;
  }
  return TQ_OK;
}

}  // namespace tq
