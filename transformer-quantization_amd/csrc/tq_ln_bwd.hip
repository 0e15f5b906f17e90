// Backward of the residual + LayerNorm tail for QAT (forward: csrc/tq_fused_ln.hip res_ln_quant_k)
//     y = Q_out( layer_norm( Q_sum( Q_dense(dense_out) + residual ); w, b, eps ) )
// under the straight-through estimator, as ONE launch over [rows, d] plus one small final launch for the sums over rows
// (the affine gradients, per column, and the range gradients of the three quantizers): 3 reads (dense_out, residual, grad_y)
// + 2 writes (grad_dense, grad_residual) = 20 B per fp32 element, against three fake-quant backwards with their
// parameter-gradient launches, the add and LayerNorm's backward with its column reductions.  Nothing but dense_out and
// residual is kept from the forward: the row is RECOMPUTED with the forward's own arithmetic in the forward's own order,
// because the clamp masks of the three quantizers and Q_out's index have to be the ones the forward used.
//
// Per row (every fp32 operation rounded on its own; s_k, zp_k, lo_k, hi_k the derived parameters of quantizer k):
//     a_j  = Q1(g_j)                 in1_j = lo1 <= rint(g_j / s1) + zp1 <= hi1
//     t_j  = a_j + r_j               u_j = Q2(t_j), in2_j likewise on t_j
//     mean, rstd = TQ_ROW_STATISTICS of u          xh_j = (u_j - mean) * rstd          z_j = xh_j * w_j + b_j
//     y_j  = Q3(z_j), in3_j, xi3_j
//     gz_j = in3_j ? (gy_j * s3) / s3 : 0          (a NaN z_j: gz_j = NaN)
//     grad_ln_bias_c += gz_j         grad_ln_weight_c += gz_j * xh_j                   (over all rows, per column)
//     gxh_j = gz_j * w_j
//     m1 = (1/d) sum_j gxh_j         m2 = (1/d) sum_j gxh_j * xh_j                     (lane-local in element order, group_sum)
//     gu_j = rstd * ((gxh_j - m1) - xh_j * m2)
//     gt_j = in2_j ? (gu_j * s2) / s2 : 0   -> grad_residual
//     gg_j = in1_j ? (gt_j * s1) / s1 : 0   -> grad_dense
// and the range-gradient terms of tq_fake_quant_bwd (ste_bwd_elem) with (g, v, s) = (gy, z, s3), (gu, t, s2), (gt, g, s1):
//     d += g (xi - zp) - in (g s v) / (s s)        z += in ? 0 : -(g s)
//
// Design (gfx950):
//  * The forward's layout: LPR lanes x NV 16-byte vectors own one row, one instantiation per row length, 256 / LPR lane groups
//    (rows) per block.  A row never leaves its lanes' registers; the four row reductions (sum, centred squares, m1, m2) are the
//    DPP / swizzle butterflies of tq_rows.h, no LDS.  The statistics, the staged affine parameters, the quantizer derivation
//    and the body vote are the forward's macros (tq_rows.h), expanded here: the same text, hence the same bits.
//  * Three input streams.  The first row's loads of dense_out, residual and grad_y are issued together with the affine
//    parameters and the nine quantizer-buffer reads (load_qraw) before anything depends on either; later rows load at the
//    loop's bottom into the same registers (no second set: the row state below is already the register budget).
//  * Both bodies of the forward, chosen by the forward's vote.  In the branch-free body mask and index come out of ONE
//    Markstein quotient on the grid widened by one step (q_recompute, tq_ste_bwd.h; identity (2) of tq_device.h on the wider grid),
//    and the data-gradient divisions are Markstein quotients; the range-gradient term (g s v) / (s s) stays an IEEE division:
//    the vote admits scales down to 2^-100, whose square has no reciprocal.  The front always dequantises with the "+ 0" fma:
//    where the forward's all-quantizers variant skips it, a -0 cannot reach z's grid index or y (its own argument).
//  * Row state per element: g, gy -> gxh, u -> xh, and with range gradients t and the two clamped indices; masks as bits.  One
//    row per lane group in flight.  d = 1024 with everything asked for is the widest instantiation (lib/kernel_resources.json,
//    profiles/r23/kernel_resources_diff.txt); no scratch anywhere.
//  * Affine gradients: a lane owns the same 4 NV columns for every row it visits, so it adds gz and gz * xh into 2 x 4 NV
//    registers across the block's grid-stride trips.  At block end the 256 / LPR lane groups meet in LDS -- ONE [groups, d]
//    buffer used twice, weight then bias (16 KiB at most; with the 2 d floats of staged affine parameters 24 KiB at d = 1024,
//    where the registers allow two blocks per CU anyway) -- are added in group order by the thread that owns the column
//    vector, and go out as the block's [2, d] partial.
//  * Range gradients: six lane-local sums over all rows of a thread, one wave butterfly + one LDS hop per block, eight floats
//    per block in `workspace` behind the column partials.
//  * The final launch: 64 columns x 4 slices per block add the block partials of a column in float64 in a fixed order (slice s
//    takes blocks s, s + 4, ..; then slice 0 + 1 + 2 + 3), and ONE more block finishes the six range sums in float64 and
//    applies the chain through clamp(delta, eps) | exp(delta) and the zero-point clamp (range_chain, tq_ste_bwd.h).  No
//    atomics anywhere: two runs give identical bits.
//  * The grid is capped (kLnBwdMaxGrid blocks: two for each of the MI355X's 256 CUs) and strides over the rows, so the workspace is bounded:
//    grid * (2 d + 8) floats.  The trip count is block-uniform: a lane group past the last row loads the last row, stores
//    nothing and selects its terms to zero, so a NaN in the duplicated row cannot leak and every wave stays whole for the
//    ballots and the block-end barriers.
//  * PG (range gradients) and AG (affine gradients) are template parameters: without them none of their code, registers or
//    LDS is compiled in.
// The recomputed quantizer, its STE backward, the block-end and final sums and the chain are the shared pieces of
// csrc/tq_ste_bwd.h; the checks and the launch dispatch of the entry are shared in csrc/tq_host.h.
#include <algorithm>

#include "tq_device.h"
#include "tq_host.h"
#include "tq_rows.h"
#include "tq_ste_bwd.h"

namespace tq {

constexpr int kLnBwdMaxGrid = 512;

struct LnAcc { float d1, z1, d2, z2, d3, z3; };

struct LnBwdParams {
  SmQW f1, f2, f3;          // branch-free body
  FusedQ g1, g2, g3;        // division body
  int on1, on2, on3;
  float ln_eps;
};

// One row of one lane group from loaded registers to stored gradients.
template <int LPR, int NV, bool PG, bool AG, bool FAST>
__device__ __forceinline__ void ln_bwd_row(const f32x4 (&xa)[NV], const f32x4 (&xr)[NV], f32x4 (&xg)[NV], uint64_t row, bool valid,
                                           int lane, const float* s_w, const float* s_b, const LnBwdParams& c,
                                           f32x4* __restrict__ gdv, f32x4* __restrict__ grv, f32x4* __restrict__ yv, LnAcc& acc,
                                           float (&gw)[AG ? NV : 1][4], float (&gb)[AG ? NV : 1][4]) {
  constexpr int H = 2;
  constexpr uint32_t T4 = LPR * NV;
  constexpr uint32_t d = T4 * 4;
  const float inv_d = 1.0f / (float)d, ln_eps = c.ln_eps;
  f32x2 u[NV][H];
  float tt[PG ? NV : 1][4], hm1[PG ? NV : 1][4], hm2[PG ? NV : 1][4];
  uint32_t in1 = 0, in2 = 0;
  f32x2 s2 = {0.f, 0.f}, s2b = {0.f, 0.f};
  bool lane_nan = false;
  // ---- the forward's front: u = Q2(Q1(g) + r), the two row-sum chains
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool i1, i2;
      float h1, h2;
      const float a = q_recompute<FAST, false>(xa[v][e], c.f1, c.g1, c.on1, i1, h1);
      const float t = a + xr[v][e];
      const float uu = q_recompute<FAST, false>(t, c.f2, c.g2, c.on2, i2, h2);
      if (FAST) lane_nan = lane_nan || __builtin_isunordered(xa[v][e], xr[v][e]);
      in1 |= (uint32_t)i1 << (v * 4 + e);
      in2 |= (uint32_t)i2 << (v * 4 + e);
      if (PG) { tt[v][e] = t; hm1[v][e] = h1; hm2[v][e] = h2; }
      u[v][e >> 1][e & 1] = uu;
    }
#pragma unroll
    for (int j = 0; j < H; ++j) {
      if (j & 1) s2b = s2b + u[v][j];
      else s2 = s2 + u[v][j];
    }
  }
  TQ_ROW_STATISTICS(TQ_GROUP_MASK)
  (void)row_nan;                                   // a flagged row has mean = NaN: every z of it is NaN below
  // ---- xh, z = xh * w + b, Q3 with its STE backward, the column terms, the two row sums of LayerNorm's backward
  float l1 = 0.f, l2 = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t col = (v * LPR + lane) * 4 + e;
      const float w = s_w[col], b = s_b[col];
      const float xh = (u[v][e >> 1][e & 1] - mean) * rstd;
      const float z = xh * w + b;
      const float gy = xg[v][e];
      float y = z, gz = gy;
      if (c.on3) {                                 // (ONE uniform branch around both pieces: two cost a mask move per element)
        bool in;
        float hc;
        y = q_recompute<FAST, true>(z, c.f3, c.g3, 1, in, hc);
        gz = ste_backward<PG, FAST>(gy, z, hc, in, valid, c.f3, c.g3, 1, acc.d3, acc.z3);
      }
      gz = z != z ? z : gz;                        // NaN rule: a row the forward turns NaN has NaN gradients
      if (AG) {
        gb[v][e] += valid ? gz : 0.0f;
        gw[v][e] += valid ? gz * xh : 0.0f;
      }
      const float gxh = gz * w;
      l1 += gxh;
      l2 += gxh * xh;
      u[v][e >> 1][e & 1] = xh;
      xg[v][e] = gxh;
      o[e] = y;
    }
    if (yv != nullptr && valid) yv[row * T4 + v * LPR + lane] = o;
  }
  const float m1 = group_sum<LPR>(l1) * inv_d, m2 = group_sum<LPR>(l2) * inv_d;
  // ---- LayerNorm's backward, Q2's and Q1's STE backward
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    f32x4 ot, og;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = u[v][e >> 1][e & 1];
      const float gu = rstd * ((xg[v][e] - m1) - xh * m2);
      const bool i1 = (in1 >> (v * 4 + e)) & 1u, i2 = (in2 >> (v * 4 + e)) & 1u;
      const float gt = ste_backward<PG, FAST>(gu, PG ? tt[v][e] : 0.f, PG ? hm2[v][e] : 0.f, i2, valid, c.f2, c.g2, c.on2, acc.d2, acc.z2);
      const float gg = ste_backward<PG, FAST>(gt, xa[v][e], PG ? hm1[v][e] : 0.f, i1, valid, c.f1, c.g1, c.on1, acc.d1, acc.z1);
      ot[e] = gt;
      og[e] = gg;
    }
    if (valid) {
      if (grv != nullptr) grv[row * T4 + v * LPR + lane] = ot;
      if (gdv != nullptr) gdv[row * T4 + v * LPR + lane] = og;
    }
  }
}

// The block's column sums -> its [2, d] partial: the lane groups meet in one [groups, d] LDS buffer, weight then bias, and the
// thread that owns a column vector adds them in group order.
template <int LPR, int NV>
__device__ __forceinline__ void ln_col_reduce(const float (&gw)[NV][4], const float (&gb)[NV][4], int lane, int sub,
                                              f32x4* __restrict__ colpart) {
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t T4 = LPR * NV;
  __shared__ f32x4 s_col[RPB * T4];
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    if (which) __syncthreads();                    // the first pass's reads are done
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float* src = which ? gb[v] : gw[v];
      s_col[sub * T4 + v * LPR + lane] = f32x4{src[0], src[1], src[2], src[3]};
    }
    __syncthreads();
    for (uint32_t cv = threadIdx.x; cv < T4; cv += kBlock) {
      f32x4 t = s_col[cv];
#pragma unroll
      for (int s = 1; s < RPB; ++s) t = t + s_col[s * T4 + cv];
      colpart[((uint64_t)blockIdx.x * 2 + which) * T4 + cv] = t;
    }
  }
}

template <int LPR, int NV, bool PG, bool AG>
__global__ __launch_bounds__(kBlock) void ln_quant_bwd_k(const f32x4* __restrict__ a, const f32x4* __restrict__ r,
                                                         const f32x4* __restrict__ gyv, f32x4* __restrict__ gdv,
                                                         f32x4* __restrict__ grv, f32x4* __restrict__ yv, uint64_t rows,
                                                         const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                         float ln_eps, tq_quantizer q1, tq_quantizer q2, tq_quantizer q3, int on1,
                                                         int on2, int on3, f32x4* __restrict__ colpart,
                                                         float* __restrict__ rngpart) {
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t T4 = LPR * NV;
  constexpr uint32_t d = T4 * 4;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d];
  const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
  const uint64_t stride = (uint64_t)gridDim.x * RPB;
  uint64_t rowb = (uint64_t)blockIdx.x * RPB;          // block-uniform; the host launches no block without a row

  f32x4 xa[NV], xr[NV], xg[NV];
  // (a macro: the loop's bottom issues the same loads for the next trip)
#define TQ_LNB_LOAD()                                                                                           \
  {                                                                                                             \
    const uint64_t rl = rowb + sub < rows ? rowb + sub : rows - 1;      /* past the end: the last row, unused */ \
    _Pragma("unroll") for (int k = 0; k < NV; ++k) {                                                            \
      xa[k] = a[rl * T4 + k * LPR + lane];                                                                      \
      xr[k] = r[rl * T4 + k * LPR + lane];                                                                      \
      xg[k] = gyv[rl * T4 + k * LPR + lane];                                                                    \
    }                                                                                                           \
  }
  TQ_LNB_LOAD()
  TQ_AFFINE_REQUEST
  QRaw w1 = load_qraw(q1, 0, ln_w), w2 = load_qraw(q2, 0, ln_w), w3 = load_qraw(q3, 0, ln_w);
  qraw_arrived(w1); qraw_arrived(w2); qraw_arrived(w3);
  TQ_AFFINE_STAGE
  TQ_TAIL_QUANTIZERS
  TQ_TAIL_VOTE
  const LnBwdParams c = {make_qw(tq.p1), make_qw(tq.p2), make_qw(tq.p3), make_fq(tq.p1, on1), make_fq(tq.p2, on2),
                         make_fq(tq.p3, on3), on1, on2, on3, ln_eps};
  LnAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float gw[AG ? NV : 1][4], gb[AG ? NV : 1][4];
#pragma unroll
  for (int v = 0; v < (AG ? NV : 1); ++v)
#pragma unroll
    for (int e = 0; e < 4; ++e) gw[v][e] = gb[v][e] = 0.f;
  while (rowb < rows) {
    const uint64_t row = rowb + sub;
    const bool valid = row < rows;
    if (fast) ln_bwd_row<LPR, NV, PG, AG, true>(xa, xr, xg, row, valid, lane, s_w, s_b, c, gdv, grv, yv, acc, gw, gb);
    else ln_bwd_row<LPR, NV, PG, AG, false>(xa, xr, xg, row, valid, lane, s_w, s_b, c, gdv, grv, yv, acc, gw, gb);
    rowb += stride;
    if (rowb < rows) TQ_LNB_LOAD()
  }
#undef TQ_LNB_LOAD
  if constexpr (AG) ln_col_reduce<LPR, NV>(gw, gb, lane, sub, colpart);
  if constexpr (PG) {
    const float sums[6] = {acc.d1, acc.z1, acc.d2, acc.z2, acc.d3, acc.z3};
    block_range_sums(sums, rngpart + 8 * (uint64_t)blockIdx.x);
  }
}

// Blocks 0 .. ncb - 1: 64 of the 2 d columns of the [2, d] block partials each (weight, then bias), 4 slices of the nb blocks per
// column, float64 (col_sum_f64).  Block ncb (only with range gradients): the six range sums in float64, then the chain
// (final_range_sums, range_chain: tq_ste_bwd.h).
__global__ __launch_bounds__(kBlock) void ln_quant_bwd_final_k(const float* __restrict__ colpart, const float* __restrict__ rngpart,
                                                               uint32_t nb, uint32_t d, uint32_t ncb, float* __restrict__ gw,
                                                               float* __restrict__ gb, tq_quantizer q1, tq_quantizer q2,
                                                               tq_quantizer q3, float* __restrict__ g1, float* __restrict__ g2,
                                                               float* __restrict__ g3) {
  if (blockIdx.x < ncb) {
    const uint32_t col = blockIdx.x * 64 + (threadIdx.x & 63);     // < 2 d: 2 d is a multiple of 64
    const double t = col_sum_f64<64, 4>(colpart + col, nb, 2 * (uint64_t)d);
    float* out = col < d ? gw : gb;
    if (threadIdx.x < 64 && out != nullptr) out[col < d ? col : col - d] = (float)t;
    return;
  }
  for (int which = 0; which < 3; ++which) {
    float* out = which == 0 ? g1 : which == 1 ? g2 : g3;
    if (out == nullptr) continue;                  // block-uniform
    double dsum, zsum;
    final_range_sums(rngpart, nb, 8, 2 * which, dsum, zsum);
    if (threadIdx.x == 0) {
      const RangeGrad g = range_chain(which == 0 ? q1 : which == 1 ? q2 : q3, 0, dsum, zsum);
      out[0] = g.delta;
      out[1] = g.zero_float;
    }
  }
}

}  // namespace tq

using namespace tq;

static unsigned ln_bwd_grid(uint64_t rows, int lpr) {
  return (unsigned)std::min<uint64_t>(ceil_div(rows, (uint64_t)(kBlock / lpr)), kLnBwdMaxGrid);
}

// per block: its [2, d] column partial and eight floats for the six range sums
extern "C" size_t tq_residual_layernorm_quant_bwd_workspace_bytes(uint64_t rows, uint64_t d) {
  const int lpr = ln_bwd_lpr(d);
  if (rows == 0 || lpr == 0) return 0;
  return (size_t)ln_bwd_grid(rows, lpr) * (2 * d + 8) * sizeof(float);
}

extern "C" int tq_residual_layernorm_quant_bwd(const float* dense_out, const float* residual, const float* grad_y, uint64_t rows,
                                               uint64_t d, const tq_quantizer* q_dense, const tq_quantizer* q_sum,
                                               const float* ln_weight, const float* ln_bias, float ln_eps,
                                               const tq_quantizer* q_out, float* grad_dense, float* grad_residual,
                                               float* grad_ln_weight, float* grad_ln_bias, float* grad_q_dense, float* grad_q_sum,
                                               float* grad_q_out, float* y, void* workspace, size_t workspace_bytes,
                                               tq_stream_t stream) {
  const char* who = "tq_residual_layernorm_quant_bwd";
  if (rows == 0) return TQ_OK;
  if (int e = tail_bwd_check(who, dense_out, residual, grad_y, ln_weight, ln_bias, grad_dense, grad_residual, y, rows, d,
                             {q_dense, q_sum, q_out}, {grad_q_dense, grad_q_sum, grad_q_out}, false))
    return e;
  TQ_REQUIRE(aligned4({grad_q_dense, grad_q_sum, grad_q_out, grad_ln_weight, grad_ln_bias}), "%s: gradients must be 4-byte aligned",
             who);
  const int lpr = ln_bwd_lpr(d);
  if (lpr == 0)
    return set_error(TQ_EUNSUPPORTED, "%s: row length %llu has no instantiation (64, 128, 256, 384, 512, 768, 1024)", who,
                     (unsigned long long)d);
  const bool pg = grad_q_dense != nullptr || grad_q_sum != nullptr || grad_q_out != nullptr;
  const bool ag = grad_ln_weight != nullptr || grad_ln_bias != nullptr;
  const unsigned grid = ln_bwd_grid(rows, lpr);
  const size_t need = (size_t)grid * (2 * d + 8) * sizeof(float);
  if (int e = bwd_workspace_check(who, pg || ag, workspace, workspace_bytes, need)) return e;
  const tq_quantizer none{};
  const tq_quantizer &c1 = q_dense ? *q_dense : none, &c2 = q_sum ? *q_sum : none, &c3 = q_out ? *q_out : none;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const auto av = reinterpret_cast<const f32x4*>(dense_out);
  const auto rv = reinterpret_cast<const f32x4*>(residual);
  const auto gv = reinterpret_cast<const f32x4*>(grad_y);
  auto gdv = reinterpret_cast<f32x4*>(grad_dense);
  auto grv = reinterpret_cast<f32x4*>(grad_residual);
  auto yv = reinterpret_cast<f32x4*>(y);
  float* colpart = static_cast<float*>(workspace);
  float* rngpart = colpart ? colpart + (size_t)grid * 2 * d : nullptr;
#define TQ_LNB_GO(PGV, AGV, LPR, NV)                                                                            \
  hipLaunchKernelGGL((ln_quant_bwd_k<LPR, NV, PGV, AGV>), dim3(grid), dim3(kBlock), 0, st, av, rv, gv, gdv, grv, yv, rows,  \
                     ln_weight, ln_bias, ln_eps, c1, c2, c3, q_dense != nullptr, q_sum != nullptr, q_out != nullptr,        \
                     reinterpret_cast<f32x4*>(colpart), rngpart)
#define TQ_LNB(LPR, NV) if (d == (uint64_t)(LPR) * (NV) * 4) TQ_PG_AG_DISPATCH(pg, ag, TQ_LNB_GO, LPR, NV);
  TQ_TAIL_BWD_FORMS(TQ_LNB)
#undef TQ_LNB
#undef TQ_LNB_GO
  if (int e = check_launch("ln_quant_bwd_k")) return e;
  if (pg || ag) {
    const unsigned ncb = ag ? (unsigned)(2 * d / 64) : 0;
    hipLaunchKernelGGL(ln_quant_bwd_final_k, dim3(ncb + (pg ? 1 : 0)), dim3(kBlock), 0, st, colpart, rngpart, grid, (uint32_t)d,
                       ncb, grad_ln_weight, grad_ln_bias, c1, c2, c3, grad_q_dense, grad_q_sum, grad_q_out);
    return check_launch("ln_quant_bwd_final_k");
  }
  return TQ_OK;
}
