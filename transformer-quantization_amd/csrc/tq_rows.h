// Row pieces shared by the kernels that keep one row in the registers of a lane group (csrc/tq_fused_ln.hip: the fused
// tails and the attention-probability chain; csrc/tq_softmax_bwd.hip: that chain's backward).
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

}  // namespace tq
