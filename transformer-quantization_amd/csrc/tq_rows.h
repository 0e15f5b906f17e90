// Row pieces shared by the kernels that keep one row in the registers of a lane group (csrc/tq_fused_ln.hip: the fused
// tails and the attention-probability chain; csrc/tq_softmax_bwd.hip: that chain's backward; csrc/tq_ln_bwd.hip: the LayerNorm
// tail's backward).
#pragma once

#include "tq_device.h"

namespace tq {

// Sum over the LPR lanes that own one row (every lane gets the total).  The first four butterfly steps run on the
// VALU's data-parallel-primitive path (quad permutes, half-row / row mirrors: one v_add_f32_dpp each, no index
// arithmetic, no LDS crossbar round trip); lanes 16 apart through ds_swizzle, 32 apart through ds_bpermute.
// (__shfl_xor costs 4 VALU instructions of index math + a dependent ds_bpermute per step: 10 steps per LayerNorm row
// were ~110 instructions and the longest dependency chain of the kernel.)
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
  static_assert(LPR >= 4 && LPR <= 64 && (LPR & (LPR - 1)) == 0, "LPR");
  v += dpp_f32<0xB1>(v);                        // quad_perm [1, 0, 3, 2]
  v += dpp_f32<0x4E>(v);                        // quad_perm [2, 3, 0, 1]
  if (LPR >= 8) v += dpp_f32<0x141>(v);         // row_half_mirror: the other quad of the 8 (all its lanes agree by now)
  if (LPR >= 16) v += dpp_f32<0x140>(v);        // row_mirror: the other half of the 16
  if (LPR >= 32) v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));   // lane ^ 16
  if (LPR >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

template <int LPR>
__device__ __forceinline__ float group_max(float v) {      // fmaxf butterfly on the same paths as group_sum
  v = max_raw(v, dpp_f32<0xB1>(v));
  v = max_raw(v, dpp_f32<0x4E>(v));
  if (LPR >= 8) v = max_raw(v, dpp_f32<0x141>(v));
  if (LPR >= 16) v = max_raw(v, dpp_f32<0x140>(v));
  if (LPR >= 32) v = max_raw(v, __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F)));
  if (LPR >= 64) v = max_raw(v, __shfl_xor(v, 32, 64));
  return v;
}

// Which body the attention-probability chain runs, from the derived parameters of its two quantizers: the branch-free exact
// one (Markstein quotients, QF quantizers) needs both quantizers, scales the exact-quotient identities hold for and a
// denominator whose reciprocal is harmless.  ONE predicate for the forward and for the backward that recomputes it: the
// backward's masks and indices have to be the ones of the body the forward ran.
__device__ __forceinline__ bool softmax_fast_ok(const QP& p1, const QP& p2, int on1, int on2, float denom) {
  if (!on1 || !on2) return false;
  const float ad = fabsf(denom);
  return make_qf(p1).ok && make_qf(p2).ok && p1.scale >= 0x1p-60f && p1.scale <= 0x1p60f && p2.scale >= 0x1p-60f &&
         p2.scale <= 0x1p60f && ad >= 0x1p-20f && ad <= 0x1p20f;
}

// ---- one quantizer of the branch-free body of a BACKWARD that recomputes its forward (tq_softmax_bwd.hip, tq_ln_bwd.hip):
// scale, its negative and reciprocal, the same of scale^2 (range gradients of the softmax chain), the grid ends relative to
// the zero point and the operand bounds of the grid widened by one step.
struct SmQW {
  float s, ns, rc, nss, rcss, klo, khi, ylo, yhi;
};
__device__ __forceinline__ SmQW make_qw(const QP& p) {
  SmQW w;
  w.s = p.scale; w.ns = -p.scale; w.rc = guarded_rcp(p.scale);
  const float ss = p.scale * p.scale;
  w.nss = -ss; w.rcss = 1.0f / ss;
  w.klo = p.lo - p.zp; w.khi = p.hi - p.zp;
  w.ylo = p.scale * (w.klo - 1.0f); w.yhi = p.scale * (w.khi + 1.0f);
  return w;
}
// RN(a / b) from rc = RN(1 / b), nb = -b (Markstein; tq_device.h (1))
__device__ __forceinline__ float div_rn(float a, float nb, float rc) {
  const float q0 = a * rc;
  return __builtin_fmaf(__builtin_fmaf(q0, nb, a), rc, q0);
}
// h = clamp(rint(v / s), k_lo - 1, k_hi + 1) (NaN for a NaN v): `in` and the forward's index follow from it
__device__ __forceinline__ float qw_index(float v, const SmQW& w) {
  const float h = rintf(div_rn(__builtin_amdgcn_fmed3f(v, w.ylo, w.yhi), w.ns, w.rc));
  return v != v ? v : h;
}

// ---- one quantizer of the division body of the fused tails (csrc/tq_fused_ln.hip) and of their backward
struct FusedQ {
  QP p;
  int on;
  float rcp;     // guarded_rcp(p.scale): three quantizers per element make these kernels VALU-bound with the division
};

__device__ __forceinline__ FusedQ make_fq(const QP& p, int on) {
  FusedQ f = {QP{1.f, 0.f, 0.f, 0.f}, on, 1.f};
  if (on) { f.p = p; f.rcp = guarded_rcp(f.p.scale); }
  return f;
}

// x_int of v under q (bit-identical to q_index: rne_quot1 falls back to the division near ties)
__device__ __forceinline__ float index_q(float v, const FusedQ& q) {
  return clamp_nanprop(rne_quot1(v, q.p.scale, q.rcp) + q.p.zp, q.p.lo, q.p.hi);
}

// The three quantizers as the kernel entry derived them (once, from one batch of loads: tq_device.h load_qraw).
struct TailQ {
  QP p1, p2, p3;
};

}  // namespace tq

// ---- row pieces of the LayerNorm tails as macros (why macros, and the names each one uses and declares: the list at the
// head of csrc/tq_fused_ln.hip).  The forward kernels and the tail's backward (csrc/tq_ln_bwd.hip) expand the same text: the
// backward's statistics, body vote and staged affine parameters ARE the forward's.

// The lanes of this wave that own the same row as this lane, as a ballot mask.
#define TQ_GROUP_MASK (LPR == 64 ? ~0ull : (((1ull << (LPR % 64)) - 1) << ((threadIdx.x & 63) / LPR * LPR)))

// The statistics of the row held in u -> mean, rstd, row_nan.  Two chains for the row sum (s2, s2b: fed by the front); centred
// sum of squares in two independent packed accumulators fed by fma (a single `ss2 = ss2 + c * c` chain was 2 packed ops per
// pair plus a wait state after each: 46 s_nop per 24-element lane row in the round-3 ISA).  The statistics carry a tolerance
// contract (tests/test_fused_ln.py; order: oracle/ln_sum.py).  FAST: rows with a NaN input have NaN statistics upstream, hence
// every output of the row (GRP: TQ_GROUP_MASK, or a variable that holds it).
#define TQ_ROW_STATISTICS(GRP)                                                                                  \
  s2 = s2 + s2b;                                                                                                \
  float mean = group_sum<LPR>(s2.x + s2.y) * inv_d;                                                             \
  bool row_nan = false;                                                                                         \
  f32x2 ssa = {0.f, 0.f}, ssb = {0.f, 0.f};                                                                     \
  {                                                                                                             \
    const f32x2 m2 = {mean, mean};                                                                              \
    _Pragma("unroll") for (int v = 0; v < NV; ++v)                                                              \
      _Pragma("unroll") for (int j = 0; j < H; ++j) {                                                           \
        const f32x2 c = u[v][j] - m2;                                                                           \
        if ((v * H + j) & 1) ssb = __builtin_elementwise_fma(c, c, ssb);                                        \
        else ssa = __builtin_elementwise_fma(c, c, ssa);                                                        \
      }                                                                                                         \
  }                                                                                                             \
  const f32x2 ss2 = ssa + ssb;                                                                                  \
  const float rstd = 1.0f / sqrtf(group_sum<LPR>(ss2.x + ss2.y) * inv_d + ln_eps);                              \
  if (FAST) {                                                                                                   \
    const uint64_t m = __ballot(lane_nan);                                                                      \
    if (m & (GRP)) { mean = __builtin_nanf(""); row_nan = true; }                                               \
  }

// The prologue pieces of the per-tensor tail kernels (the order they go in: csrc/tq_fused_ln.hip, above struct FusedF).
#define TQ_AFFINE_REQUEST                                                                                       \
  float aw[NA], ab[NA];                                                                                         \
  _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                              \
    const uint32_t c = threadIdx.x + i * kBlock;                                                                \
    const uint32_t cc = c < d ? c : d - 1;                                                                      \
    aw[i] = ln_w[cc];                                                                                           \
    ab[i] = ln_b[cc];                                                                                           \
  }
#define TQ_AFFINE_STAGE                                                                                         \
  _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                              \
    const uint32_t c = threadIdx.x + i * kBlock;                                                                \
    if (c < d) { s_w[c] = aw[i]; s_b[c] = ab[i]; }                                                              \
  }                                                                                                             \
  __syncthreads();
#define TQ_TAIL_QUANTIZERS                                                                                      \
  const QP none = {1.f, 0.f, 0.f, 0.f};                                                                         \
  const TailQ tq = {on1 ? qp_from_raw(q1, w1) : none, on2 ? qp_from_raw(q2, w2) : none, on3 ? qp_from_raw(q3, w3) : none};
#define TQ_TAIL_VOTE                                                                                            \
  bool fast = true;                                                                                             \
  if (on1) fast = fast && make_qf(tq.p1).ok;                                                                    \
  if (on2) fast = fast && make_qf(tq.p2).ok;                                                                    \
  if (on3) fast = fast && make_qf(tq.p3).ok;
