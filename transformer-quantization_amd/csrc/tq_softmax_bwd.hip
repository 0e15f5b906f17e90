// Backward of the attention-probability chain for QAT (forward: csrc/tq_fused_ln.hip softmax_quant_k)
//     probs = Q_probs( softmax( Q_scores(scores) / denom + mask , dim=-1 ) )
// under the straight-through estimator, as ONE launch over [rows, cols] (+ one two-block launch for the range gradients):
// 2 reads (scores, grad_probs) + 1 write (grad_scores) = 12 B per score element, against four autograd nodes and the two
// quantizers' parameter-gradient launches of the layered chain.  Nothing but `scores` is kept from the forward: the row is
// RECOMPUTED here -- one exp per element beside 12 B of HBM traffic -- with the forward's own arithmetic in the forward's own
// order, because the clamp masks of the two quantizers and the index x_int of Q_probs have to be the ones the forward used.
//
// Per row (every fp32 operation rounded on its own; s1, zp1, lo1, hi1 / s2, .. the derived parameters):
//     u_j  = Q_scores(x_j)          r1_j = rint(x_j / s1) + zp1     in1_j = lo1 <= r1_j <= hi1
//     t_j  = u_j / denom + m_j      p = softmax(t)
//     r2_j = rint(p_j / s2) + zp2   in2_j = lo2 <= r2_j <= hi2      xi2_j = clamp(r2_j)
//     gp_j = in2_j ? (gy_j * s2) / s2 : 0
//     dot  = sum_j gp_j * p_j       (lane-local in element order, then the group butterfly)
//     gt_j = p_j * (gp_j - dot),    gu_j = gt_j / denom,    gx_j = in1_j ? (gu_j * s1) / s1 : 0
// and the range-gradient terms of tq_fake_quant_bwd (ste_bwd_elem), once with (g, v, s) = (gy, p, s2), once with (gu, x, s1):
//     d += g (xi - zp) - in (g s v) / (s s)        z += in ? 0 : -(g s)
//
// Design (gfx950):
//  * The forward's layout: LPR lanes x NV 16-byte vectors own one row, R independent rows per lane group in flight, one
//    instantiation per row length.  A row never leaves its lanes' registers; the three row reductions (max, sum, dot) are the
//    forward's DPP / swizzle butterflies (tq_rows.h), no LDS.
//  * Three input streams.  The first step's loads of scores, grad_probs and the mask row are issued together with the six
//    quantizer-buffer reads (load_qraw) before anything depends on either: the parameter derivation (two dependent round
//    trips per quantizer otherwise) hides under the data loads.  Later steps load at the loop's bottom.
//  * R: the backward holds x, gy, the mask / then p, and (with range gradients) xi1 - zp1 per element, twice the forward's
//    registers per row, so it keeps HALF the forward's rows in flight: R = 2 for one vector per lane (96 registers, 5 waves
//    per SIMD, without range gradients; 154 / 3 waves with them), R = 1 for longer rows and small grids (72 / 7 waves and
//    105 / 4 waves at one vector; T = 1024 with range gradients is the widest at 256 + 12 registers, one wave per SIMD, no
//    scratch).  Numbers: lib/kernel_resources.json, profiles/r22/kernel_resources_diff.txt.
//  * Both bodies of the forward, chosen by the same predicate (softmax_fast_ok) from the same parameters.  In the
//    branch-free body the clamp masks come out of the SAME Markstein quotient as the index: the operand is bounded by
//    the grid ends widened by ONE step, Q(med3(x, s (k_lo - 1), s (k_hi + 1))) = clamp(Q(x), k_lo - 1, k_hi + 1) (identity
//    (2) of tq_device.h on the wider grid), so `in` is k_lo <= h <= k_hi and clamping h gives the forward's index -- no second
//    quotient, no IEEE division.  Its gradient divisions are Markstein quotients with the reciprocals of s1, s2, denom, s1^2
//    and s2^2 (correctly rounded = the IEEE result wherever the fma residual is exact; a gradient in the subnormal range or
//    an infinite one may differ from v_div's result, within the tolerance contract of the chain).
//  * Range gradients: four lane-local sums over all rows of a thread, one wave butterfly + one LDS hop per block at the very
//    end, block partials in `workspace`, and a two-block final kernel (one block per quantizer) that adds them in float64 in
//    a fixed order and applies the chain through clamp(delta, eps) | exp(delta) and the zero-point clamp.  No atomics:
//    deterministic.  Without range gradients (PG = false) none of this is compiled in.
//  * A row index past the end is clamped for the loads (the forward recomputes the last row there); such a row stores
//    nothing and its terms are replaced by zero with a select, so a NaN in the duplicated row cannot leak either.
// The recomputed quantizers, the block-end and final sums and the chain are the shared pieces of csrc/tq_ste_bwd.h.  The
// backward terms stay here: the branch-free body forms the range term as a Markstein quotient with the reciprocal of s^2,
// which no other backward does.
#include <algorithm>

#include "tq_device.h"
#include "tq_host.h"
#include "tq_rows.h"
#include "tq_ste_bwd.h"

namespace tq {

struct SmAcc { float d1, z1, d2, z2; };

// The constants of both bodies.  Deriving only the running body's (the choice is wave-uniform and fixed for the launch) means
// two copies of the row loop, one per body, each with its own loads at the bottom; built that way every variant needed MORE
// registers (T = 128, R = 2: 96 -> 120 without range gradients, 155 -> 168 with; T = 1024: 168 -> 204 and 256 + 12 -> 256 + 35),
// so the loop stays single and both sets stay live.
struct SmBwdParams {
  SmQW f1, f2;       // branch-free body
  FusedQ d1, d2;     // division body
  float denom, rd, nd;
};

// R rows of one lane group from loaded registers to stored gradients.  FAST: the forward's branch-free body, else its
// IEEE-division body.  g holds grad_probs on entry and is overwritten (gp).
template <int LPR, int NV, int R, bool PG, bool FAST>
__device__ __forceinline__ void sm_bwd_step(const f32x4 (&x)[R][NV], f32x4 (&g)[R][NV], const f32x4 (&mk)[R][NV], uint64_t row0,
                                            uint64_t rows, bool has_mask, f32x4* __restrict__ gxv, f32x4* __restrict__ yv,
                                            int lane, const SmBwdParams& c, SmAcc& acc) {
  constexpr uint32_t T4 = LPR * NV;
  float p[R][NV][4], hm1[R][NV][4], mx[R], sum[R], dot[R];
  uint32_t in1[R];
  // ---- forward, first half: u = Q_scores(x), t = u / c.denom + m, row max
#pragma unroll
  for (int r = 0; r < R; ++r) {
    in1[r] = 0;
    mx[r] = -__builtin_huge_valf();
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xv = x[r][k][j];
        bool in;
        float hc;
        const float u = q_recompute<FAST, true>(xv, c.f1, c.d1, FAST || c.d1.on, in, hc);      // (the branch-free body: both present)
        in1[r] |= (uint32_t)in << (k * 4 + j);
        hm1[r][k][j] = hc;
        float t = FAST ? div_rn(u, c.nd, c.rd) : u / c.denom;                                  // the forward's t / c.denom
        if (has_mask) t = t + mk[r][k][j];
        p[r][k][j] = t;
        mx[r] = FAST ? max_raw(mx[r], t) : fmaxf(mx[r], t);
      }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) mx[r] = group_max<LPR>(mx[r]);
  // ---- exp and row sum, in the forward's element order
#pragma unroll
  for (int r = 0; r < R; ++r) {
    sum[r] = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = FAST ? exp_nonpos_fast(p[r][k][j] - mx[r]) : expf(p[r][k][j] - mx[r]);
        p[r][k][j] = e;
        sum[r] += e;
      }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) sum[r] = group_sum<LPR>(sum[r]);
  // ---- p = e / sum, Q_probs, its STE backward and range-gradient terms, the row's dot product
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool valid = row0 + r < rows;
    const float rs = 1.0f / sum[r], ns = -sum[r];
    dot[r] = 0.f;
    f32x4 o[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gy = g[r][k][j];
        float hc, gp, gs, t2;
        bool in;
        const float pv = FAST ? div_rn(p[r][k][j], ns, rs) : p[r][k][j] / sum[r];
        const float yq = q_recompute<FAST, true>(pv, c.f2, c.d2, FAST || c.d2.on, in, hc);
        if constexpr (FAST) {
          gs = gy * c.f2.s;
          gp = div_rn(gs, c.f2.ns, c.f2.rc);
          t2 = div_rn(gs * pv, c.f2.nss, c.f2.rcss);
        } else {
          gs = gy; gp = gy; t2 = 0.f;
          if (c.d2.on) {
            gs = gy * c.d2.p.scale;
            gp = gs / c.d2.p.scale;
            if (PG) t2 = (gs * pv) / (c.d2.p.scale * c.d2.p.scale);
          }
        }
        gp = in ? gp : 0.0f;
        if (PG) {
          float dd = gy * hc;
          if (in) dd -= t2;
          acc.d2 += valid ? dd : 0.0f;
          acc.z2 += (valid && !in) ? -gs : 0.0f;
        }
        p[r][k][j] = pv;
        g[r][k][j] = gp;
        o[k][j] = yq;
        dot[r] += gp * pv;
      }
    if (yv != nullptr && valid) {
#pragma unroll
      for (int k = 0; k < NV; ++k) yv[(row0 + r) * T4 + k * LPR + lane] = o[k];
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) dot[r] = group_sum<LPR>(dot[r]);
  // ---- softmax backward, / c.denom, Q_scores' STE backward and range-gradient terms
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool valid = row0 + r < rows;
    f32x4 o[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = (in1[r] >> (k * 4 + j)) & 1u;
        const float gt = p[r][k][j] * (g[r][k][j] - dot[r]);
        const float xv = x[r][k][j];
        float gu, gs, gxe, t2 = 0.f;
        if constexpr (FAST) {
          gu = div_rn(gt, c.nd, c.rd);
          gs = gu * c.f1.s;
          gxe = div_rn(gs, c.f1.ns, c.f1.rc);
          if (PG) t2 = div_rn(gs * xv, c.f1.nss, c.f1.rcss);
        } else {
          gu = gt / c.denom;
          gs = gu; gxe = gu;
          if (c.d1.on) {
            gs = gu * c.d1.p.scale;
            gxe = gs / c.d1.p.scale;
            if (PG) t2 = (gs * xv) / (c.d1.p.scale * c.d1.p.scale);
          }
        }
        if (PG) {
          float dd = gu * hm1[r][k][j];
          if (in) dd -= t2;
          acc.d1 += valid ? dd : 0.0f;
          acc.z1 += (valid && !in) ? -gs : 0.0f;
        }
        o[k][j] = in ? gxe : 0.0f;
      }
    if (valid) {
#pragma unroll
      for (int k = 0; k < NV; ++k) gxv[(row0 + r) * T4 + k * LPR + lane] = o[k];
    }
  }
}

template <int LPR, int NV, int R, bool PG>
__global__ __launch_bounds__(kBlock) void softmax_quant_bwd_k(const f32x4* __restrict__ s, const f32x4* __restrict__ gyv,
                                                              f32x4* __restrict__ gxv, f32x4* __restrict__ yv, uint64_t rows,
                                                              const float* __restrict__ mask, uint64_t rows_per_mask,
                                                              float denom, tq_quantizer q1, tq_quantizer q2, int on1, int on2,
                                                              int allow_fast, float* __restrict__ partial) {
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t T4 = LPR * NV;              // float4 vectors per row
  const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
  const uint64_t stride = (uint64_t)gridDim.x * RPB * R;
  uint64_t row0 = ((uint64_t)blockIdx.x * RPB + sub) * R;

  f32x4 x[R][NV], g[R][NV], mk[R][NV];
  // (a macro: the loop's bottom issues the same loads for the next step)
#define TQ_SMB_LOAD()                                                                                           \
  {                                                                                                             \
    const uint64_t rb = row0 < rows ? row0 : rows - 1;          /* a lane group without rows: loads the last row, unused */ \
    const uint64_t m0 = mask ? rb / rows_per_mask : 0, rem0 = rb - m0 * rows_per_mask;                          \
    _Pragma("unroll") for (int r = 0; r < R; ++r) {                                                             \
      const uint64_t row = rb + r < rows ? rb + r : rows - 1;                                                   \
      const uint64_t mi = rem0 + r < rows_per_mask ? m0 : row / rows_per_mask;                                  \
      const f32x4* mrow = mask ? reinterpret_cast<const f32x4*>(mask + mi * (uint64_t)T4 * 4) : nullptr;        \
      _Pragma("unroll") for (int k = 0; k < NV; ++k) {                                                          \
        x[r][k] = s[row * T4 + k * LPR + lane];                                                                 \
        g[r][k] = gyv[row * T4 + k * LPR + lane];                                                               \
        mk[r][k] = mrow ? mrow[k * LPR + lane] : f32x4{0.f, 0.f, 0.f, 0.f};                                     \
      }                                                                                                         \
    }                                                                                                           \
  }
  const float* safe = reinterpret_cast<const float*>(s);
  QRaw w1 = load_qraw(q1, 0, safe), w2 = load_qraw(q2, 0, safe);
  TQ_SMB_LOAD()
  qraw_arrived(w1); qraw_arrived(w2);
  const QP none = {1.f, 0.f, 0.f, 0.f};
  const QP p1 = on1 ? qp_from_raw<true>(q1, w1) : none, p2 = on2 ? qp_from_raw<true>(q2, w2) : none;
  const bool fast = allow_fast && softmax_fast_ok(p1, p2, on1, on2, denom);          // wave-uniform
  const SmBwdParams c = {make_qw(p1), make_qw(p2), make_fq(p1, on1), make_fq(p2, on2), denom, 1.0f / denom, -denom};
  SmAcc acc = {0.f, 0.f, 0.f, 0.f};
  while (row0 < rows) {
    if (fast) sm_bwd_step<LPR, NV, R, PG, true>(x, g, mk, row0, rows, mask != nullptr, gxv, yv, lane, c, acc);
    else sm_bwd_step<LPR, NV, R, PG, false>(x, g, mk, row0, rows, mask != nullptr, gxv, yv, lane, c, acc);
    row0 += stride;
    if (row0 < rows) TQ_SMB_LOAD()
  }
#undef TQ_SMB_LOAD
  if constexpr (PG) {
    const float sums[4] = {acc.d1, acc.z1, acc.d2, acc.z2};
    block_range_sums(sums, partial + 4 * (uint64_t)blockIdx.x);
  }
}

// block 0: Q_scores, block 1: Q_probs.  out = [d loss / d _delta, d loss / d _zero_float]: float64 sum of the block partials in
// a fixed order, then the chain (final_range_sums, range_chain: tq_ste_bwd.h).
__global__ __launch_bounds__(kBlock) void softmax_quant_bwd_final_k(const float* __restrict__ partial, uint32_t nb, tq_quantizer q1,
                                                                    tq_quantizer q2, float* __restrict__ g1,
                                                                    float* __restrict__ g2) {
  const int which = blockIdx.x;
  float* out = which ? g2 : g1;
  if (out == nullptr) return;                    // block-uniform
  double dsum, zsum;
  final_range_sums(partial, nb, 4, 2 * which, dsum, zsum);
  if (threadIdx.x == 0) {
    const RangeGrad g = range_chain(which ? q2 : q1, 0, dsum, zsum);
    out[0] = g.delta;
    out[1] = g.zero_float;
  }
}

}  // namespace tq

using namespace tq;

// lanes per row of the instantiation for `cols`, 0 if there is none
static int sm_bwd_lpr(uint64_t cols) {
  switch (cols) {
    case 32: return 8;
    case 64: return 16;
    case 128: return 32;
    case 256: case 512: case 1024: return 64;
    default: return 0;
  }
}

// blocks of the launch with R rows per lane group in flight
static unsigned sm_bwd_grid(uint64_t rows, int lpr, int R) {
  return (unsigned)std::min<uint64_t>(std::max<uint64_t>(ceil_div(rows, (uint64_t)(kBlock / lpr) * R), 1), kMaxGrid);
}

// four floats per block; sized for R = 1, the launch with the most blocks
extern "C" size_t tq_scores_softmax_quant_bwd_workspace_bytes(uint64_t rows, uint64_t cols) {
  const int lpr = sm_bwd_lpr(cols);
  if (rows == 0 || lpr == 0) return 0;
  return (size_t)sm_bwd_grid(rows, lpr, 1) * 4 * sizeof(float);
}

extern "C" int tq_scores_softmax_quant_bwd(const float* scores, const float* grad_probs, float* grad_scores, uint64_t rows,
                                           uint64_t cols, const float* mask, uint64_t rows_per_mask, float denom,
                                           const tq_quantizer* q_scores, const tq_quantizer* q_probs, float* grad_q_scores,
                                           float* grad_q_probs, float* probs, void* workspace, size_t workspace_bytes,
                                           tq_stream_t stream) {
  const char* who = "tq_scores_softmax_quant_bwd";
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(scores && grad_probs && grad_scores, "%s: NULL pointer", who);
  TQ_REQUIRE(aligned16(scores) && aligned16(grad_probs) && aligned16(grad_scores) && aligned16(probs) &&
                 (mask == nullptr || aligned16(mask)), "%s: 16-byte alignment required", who);
  TQ_REQUIRE(mask == nullptr || (rows_per_mask >= 1 && rows % rows_per_mask == 0), "%s: bad mask layout", who);
  if (mask == nullptr) rows_per_mask = rows;      // unused without a mask; keeps the kernel's row -> mask arithmetic away from / 0
  TQ_REQUIRE(denom != 0.0f, "%s: denom == 0", who);
  for (const tq_quantizer* q : {q_scores, q_probs})
    if (q != nullptr) {
      if (int e = check_quantizer(q, rows * cols, who)) return e;
      TQ_REQUIRE(q->n_params == 1, "%s: per-tensor quantizers only", who);
    }
  TQ_REQUIRE((grad_q_scores == nullptr || q_scores != nullptr) && (grad_q_probs == nullptr || q_probs != nullptr),
             "%s: range gradients asked for an absent quantizer", who);
  TQ_REQUIRE(((reinterpret_cast<uintptr_t>(grad_q_scores) | reinterpret_cast<uintptr_t>(grad_q_probs)) & 3u) == 0,
             "%s: range gradients must be 4-byte aligned", who);
  const int lpr = sm_bwd_lpr(cols);
  if (lpr == 0)
    return set_error(TQ_EUNSUPPORTED, "%s: row length %llu unsupported (32..1024, power of two)", who, (unsigned long long)cols);
  const bool pg = grad_q_scores != nullptr || grad_q_probs != nullptr;
  // rows in flight per lane group: as many as the registers allow (see the head of this file), while the grid still covers
  // the chip twice (the forward's rule)
  const int allow_fast = tuning("TQ_SM_FAST", 1);      // read per call, as the forward does: both must run the same body
  int R = cols > 128 ? 1 : 2;
  while (R > 1 && rows / ((uint64_t)(kBlock / lpr) * R) < 512) R >>= 1;
  const unsigned grid = sm_bwd_grid(rows, lpr, R);
  if (pg && (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0 ||
             workspace_bytes < (size_t)grid * 4 * sizeof(float)))
    return set_error(TQ_EWORKSPACE, "%s: workspace %zu < %zu bytes (or NULL / misaligned)", who, workspace_bytes,
                     (size_t)grid * 4 * sizeof(float));
  const tq_quantizer none{};
  const tq_quantizer &c1 = q_scores ? *q_scores : none, &c2 = q_probs ? *q_probs : none;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const auto sv = reinterpret_cast<const f32x4*>(scores);
  const auto gv = reinterpret_cast<const f32x4*>(grad_probs);
  auto ov = reinterpret_cast<f32x4*>(grad_scores);
  auto yv = reinterpret_cast<f32x4*>(probs);
  float* ws = static_cast<float*>(workspace);
#define TQ_SMB_GO(LPR, NV, RV, PGV)                                                                             \
  hipLaunchKernelGGL((softmax_quant_bwd_k<LPR, NV, RV, PGV>), dim3(grid), dim3(kBlock), 0, st, sv, gv, ov, yv, rows, mask, \
                     rows_per_mask, denom, c1, c2, q_scores != nullptr, q_probs != nullptr, allow_fast, ws)
#define TQ_SMB(LPR, NV, RMAX)                                                                                   \
  if (cols == (uint64_t)(LPR) * (NV) * 4) {                                                                     \
    if constexpr ((RMAX) == 2) {                                                                                \
      if (R == 2) { if (pg) TQ_SMB_GO(LPR, NV, 2, true); else TQ_SMB_GO(LPR, NV, 2, false); }                   \
      else        { if (pg) TQ_SMB_GO(LPR, NV, 1, true); else TQ_SMB_GO(LPR, NV, 1, false); }                   \
    } else {                                                                                                    \
      if (pg) TQ_SMB_GO(LPR, NV, 1, true); else TQ_SMB_GO(LPR, NV, 1, false);                                   \
    }                                                                                                           \
  }
  TQ_SMB(8, 1, 2) TQ_SMB(16, 1, 2) TQ_SMB(32, 1, 2) TQ_SMB(64, 1, 1) TQ_SMB(64, 2, 1) TQ_SMB(64, 4, 1)
#undef TQ_SMB
#undef TQ_SMB_GO
  if (int e = check_launch("softmax_quant_bwd_k")) return e;
  if (pg) {
    hipLaunchKernelGGL(softmax_quant_bwd_final_k, dim3(2), dim3(kBlock), 0, st, ws, grid, c1, c2, grad_q_scores, grad_q_probs);
    return check_launch("softmax_quant_bwd_final_k");
  }
  return TQ_OK;
}
