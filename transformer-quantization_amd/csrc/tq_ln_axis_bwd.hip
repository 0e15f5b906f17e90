// Backward of the residual + LayerNorm tail with quantizer parameters PER COLUMN (forward: csrc/tq_fused_ln.hip
// res_ln_quant_axis_k; per-embedding and per-embedding-group quantizers hold `_delta[d]` / `_zero_float[d]`)
//     y = Q_out( layer_norm( Q_sum( Q_dense(dense_out) + residual ); w, b, eps ) )
// under the straight-through estimator, as ONE launch over [rows, d] plus one small final launch for the sums over rows: the
// affine gradients and the range gradients of the three quantizers, all of them PER COLUMN here.  The formulas are the ones at
// the head of csrc/tq_ln_bwd.hip with s_k, zp_k and the reciprocal taken per column; the chain through clamp(delta, eps) and the
// zero-point clamp is applied per parameter.  3 reads + 2 writes = 20 B per fp32 element; nothing but dense_out and residual is
// kept from the forward, the row is recomputed with the forward's arithmetic so that masks and indices are the forward's.
//
// Design (gfx950), and where it leaves the per-tensor kernel:
//  * The forward's layout: LPR lanes x NV 16-byte vectors own one row, 256 / LPR lane groups per block, the statistics macro of
//    tq_rows.h (the recomputed row has the forward's bits), a grid-stride loop with a block-uniform trip count (lane groups
//    past the end load the last row, store nothing and select their terms to zero), the first row's three streams issued
//    together with the affine and the raw quantizer parameters of this thread's columns.
//  * Quantizer constants: derived once per block in the prologue (qp_from_raw per column, as res_ln_quant_axis_k does) and
//    staged in LDS next to s_w / s_b as THREE floats per column and quantizer -- scale, guarded reciprocal, zero point -- read
//    by the row loop as 16-byte vectors of a lane's consecutive columns.  The forward stages four (it keeps the operand bounds
//    of its grid); here both bodies share one table: the grid ends relative to the zero point and the operand bounds of the
//    grid widened by one step (qw_index's, tq_rows.h) are two subtractions and two products per element from the table and the
//    per-quantizer limits, and scale^2 of the range term (g s v) / (s s) is one product.  A per-tensor quantizer in the mix is
//    broadcast into its table.  Both bodies of the forward, exact (Markstein) and division, chosen by the forward's block-wide
//    vote over every column of every enabled quantizer.
//  * Column accumulators: a lane owns the same 4 NV columns for every row it visits, so the affine sums AND the six range sums
//    per column are lane-local registers across the trips: 8 x 4 NV of them.  To make room the row state is cut to the three
//    loaded vectors and u / xh: t, both clamped indices and both masks of the front are NOT kept across the statistics but
//    recomputed from the loaded g and r in the last pass (two more quotients per element against 12 NV + 2 registers).
//    PG (range gradients) and AG (affine gradients) are template parameters: none of that state is compiled in where it is
//    not asked for.  Registers per instantiation: lib/kernel_resources.json; no scratch anywhere.
//  * Block end: the lane groups meet in ONE [groups, d] LDS buffer, reused once per accumulated quantity and added in group
//    order by the thread that owns the column vector; the block writes its [8, d] partial (weight, bias, then d and z of
//    Q_dense, Q_sum, Q_out) into `workspace`.  With LPR >= 32 the buffer aliases the quantizer tables behind a barrier (the row
//    loop is done): 11 d floats of LDS in all, 44 KB at d = 1024; at LPR = 16 (d = 64) the tables are too small and the buffer
//    is its own 4 KB.
//  * Final launch: 64 columns x 4 slices per block add the block partials of a column in float64 in a fixed order (slice s
//    takes blocks s, s + 4, ..; then slice 0 + 1 + 2 + 3), then the chain per parameter.  For a PER-TENSOR quantizer in the
//    mix the float64 column sums go to the workspace's tail instead and one more one-block launch adds them over the columns
//    in float64 in a fixed order and applies the chain: [2, 1].  (A third launch only for such a mix: one block that reads all
//    grid x d partials itself would take longer than the launch.)  No atomics anywhere: two runs give identical bits.
//  * The grid is capped at kLnAxisBwdMaxGrid = 512 blocks (two per CU), so the workspace is bounded:
//    512 x 8 x d floats + 6 d doubles <= 16 MiB + 48 KiB at d = 1024.
//  * NaN rule: a row the forward turns NaN has NaN data gradients inside the clamp ranges and 0 outside; a NaN term reaches
//    only its own column's sums (and, through the column sum, every per-tensor sum); other rows are untouched.
// The recomputed quantizer (on a column's scale, reciprocal and zero point), its STE backward, the float64 column sums and the
// chain are the shared pieces of csrc/tq_ste_bwd.h; the checks and the launch dispatch of the entry are shared in csrc/tq_host.h.
#include <algorithm>

#include "tq_device.h"
#include "tq_host.h"
#include "tq_rows.h"
#include "tq_ste_bwd.h"

namespace tq {

constexpr int kLnAxisBwdMaxGrid = 512;
constexpr int kLnAxisBwdQuantities = 8;      // ln_weight, ln_bias, then (d, z) of q_dense, q_sum, q_out

struct AxbLim {           // what is the same for every column: the integer limits of the three quantizers and who is there
  float lo[3], hi[3];
  int on[3];
};

struct AxbCol {           // the table entries of one quantizer for a lane's four consecutive columns
  f32x4 s, rc, zp;
};
__device__ __forceinline__ AxbCol axb_cols(const float* tab, uint32_t d, uint32_t c0) {
  return AxbCol{*reinterpret_cast<const f32x4*>(tab + c0), *reinterpret_cast<const f32x4*>(tab + d + c0),
                *reinterpret_cast<const f32x4*>(tab + 2 * d + c0)};
}

// One row of one lane group from loaded registers to stored gradients.  acc = [quantity][vector][element]: the lane's column sums.
template <int LPR, int NV, bool PG, bool AG, bool FAST>
__device__ __forceinline__ void ln_axis_bwd_row(const f32x4 (&xa)[NV], const f32x4 (&xr)[NV], f32x4 (&xg)[NV], uint64_t row, bool valid,
                                                int lane, const float* s_w, const float* s_b, const float* s_q, const AxbLim& lim,
                                                float ln_eps, f32x4* __restrict__ gdv, f32x4* __restrict__ grv,
                                                f32x4* __restrict__ yv, float (&gw)[AG ? NV : 1][4], float (&gb)[AG ? NV : 1][4],
                                                float (&rd)[3][PG ? NV : 1][4], float (&rz)[3][PG ? NV : 1][4]) {
  constexpr int H = 2;
  constexpr uint32_t T4 = LPR * NV;
  constexpr uint32_t d = T4 * 4;
  const float *t1 = s_q, *t2 = s_q + 3 * d, *t3 = s_q + 6 * d;
  const float inv_d = 1.0f / (float)d;
  f32x2 u[NV][H];
  f32x2 s2 = {0.f, 0.f}, s2b = {0.f, 0.f};
  bool lane_nan = false;
  // ---- the forward's front: u = Q2(Q1(g) + r), the two row-sum chains
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const uint32_t c0 = (v * LPR + lane) * 4;
    const AxbCol k1 = axb_cols(t1, d, c0), k2 = axb_cols(t2, d, c0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool in;
      float hc;
      const float a = q_recompute<FAST, false>(xa[v][e], k1.s[e], k1.rc[e], k1.zp[e], lim.lo[0], lim.hi[0], lim.on[0], in, hc);
      u[v][e >> 1][e & 1] = q_recompute<FAST, false>(a + xr[v][e], k2.s[e], k2.rc[e], k2.zp[e], lim.lo[1], lim.hi[1], lim.on[1], in, hc);
      if (FAST) lane_nan = lane_nan || __builtin_isunordered(xa[v][e], xr[v][e]);
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
    const uint32_t c0 = (v * LPR + lane) * 4;
    const f32x4 wv = *reinterpret_cast<const f32x4*>(s_w + c0), bv = *reinterpret_cast<const f32x4*>(s_b + c0);
    const AxbCol k3 = axb_cols(t3, d, c0);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (u[v][e >> 1][e & 1] - mean) * rstd;
      const float z = xh * wv[e] + bv[e];
      bool in;
      float hc;
      const float y = q_recompute<FAST, true>(z, k3.s[e], k3.rc[e], k3.zp[e], lim.lo[2], lim.hi[2], lim.on[2], in, hc);
      float gz = ste_backward<PG, FAST>(xg[v][e], z, hc, in, valid, k3.s[e], k3.rc[e], lim.on[2], rd[2][PG ? v : 0][e], rz[2][PG ? v : 0][e]);
      gz = z != z ? z : gz;                        // NaN rule: a row the forward turns NaN has NaN gradients
      if (AG) {
        gb[v][e] += valid ? gz : 0.0f;
        gw[v][e] += valid ? gz * xh : 0.0f;
      }
      const float gxh = gz * wv[e];
      l1 += gxh;
      l2 += gxh * xh;
      u[v][e >> 1][e & 1] = xh;
      xg[v][e] = gxh;
      o[e] = y;
    }
    if (yv != nullptr && valid) yv[row * T4 + v * LPR + lane] = o;
  }
  const float m1 = group_sum<LPR>(l1) * inv_d, m2 = group_sum<LPR>(l2) * inv_d;
  // ---- LayerNorm's backward; the front once more for t, masks and indices; Q2's and Q1's STE backward
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const uint32_t c0 = (v * LPR + lane) * 4;
    const AxbCol k1 = axb_cols(t1, d, c0), k2 = axb_cols(t2, d, c0);
    f32x4 ot, og;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool i1, i2;
      float h1, h2;
      const float t = q_recompute<FAST, false>(xa[v][e], k1.s[e], k1.rc[e], k1.zp[e], lim.lo[0], lim.hi[0], lim.on[0], i1, h1) + xr[v][e];
      (void)q_recompute<FAST, false>(t, k2.s[e], k2.rc[e], k2.zp[e], lim.lo[1], lim.hi[1], lim.on[1], i2, h2);
      const float xh = u[v][e >> 1][e & 1];
      const float gu = rstd * ((xg[v][e] - m1) - xh * m2);
      const float gt = ste_backward<PG, FAST>(gu, t, h2, i2, valid, k2.s[e], k2.rc[e], lim.on[1], rd[1][PG ? v : 0][e], rz[1][PG ? v : 0][e]);
      const float gg = ste_backward<PG, FAST>(gt, xa[v][e], h1, i1, valid, k1.s[e], k1.rc[e], lim.on[0], rd[0][PG ? v : 0][e], rz[0][PG ? v : 0][e]);
      ot[e] = gt;
      og[e] = gg;
    }
    if (valid) {
      if (grv != nullptr) grv[row * T4 + v * LPR + lane] = ot;
      if (gdv != nullptr) gdv[row * T4 + v * LPR + lane] = og;
    }
  }
}

// One accumulated quantity of the block -> row `qn` of its [8, d] partial: the lane groups meet in s_col = [groups, d] and the
// thread that owns a column vector adds them in group order.  The leading barrier: the previous quantity's reads (the first
// time: the row loop's reads of the tables s_col may alias) are done.
template <int LPR, int NV>
__device__ __forceinline__ void axb_col_reduce(const float (&src)[NV][4], int qn, int lane, int sub, f32x4* s_col,
                                               f32x4* __restrict__ colpart) {
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t T4 = LPR * NV;
  __syncthreads();
#pragma unroll
  for (int v = 0; v < NV; ++v) s_col[sub * T4 + v * LPR + lane] = f32x4{src[v][0], src[v][1], src[v][2], src[v][3]};
  __syncthreads();
  for (uint32_t cv = threadIdx.x; cv < T4; cv += kBlock) {
    f32x4 t = s_col[cv];
#pragma unroll
    for (int s = 1; s < RPB; ++s) t = t + s_col[s * T4 + cv];
    colpart[((uint64_t)blockIdx.x * kLnAxisBwdQuantities + qn) * T4 + cv] = t;
  }
}

// raw parameters of column c (or of the only parameter of a per-tensor quantizer); an absent buffer reads `safe`
__device__ __forceinline__ void axb_load_raw(const tq_quantizer& q, uint32_t c, const float* safe, float& dl, float& zf) {
  const uint64_t p = q.n_params == 1 ? 0 : c;
  dl = *(q.delta != nullptr ? q.delta + p : safe);
  zf = *(q.zero_float != nullptr ? q.zero_float + p : safe);
}

template <int LPR, int NV, bool PG, bool AG>
__global__ __launch_bounds__(kBlock) void ln_quant_axis_bwd_k(const f32x4* __restrict__ a, const f32x4* __restrict__ r,
                                                              const f32x4* __restrict__ gyv, f32x4* __restrict__ gdv,
                                                              f32x4* __restrict__ grv, f32x4* __restrict__ yv, uint64_t rows,
                                                              const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                              float ln_eps, tq_quantizer q1, tq_quantizer q2, tq_quantizer q3,
                                                              int on1, int on2, int on3, f32x4* __restrict__ colpart) {
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t T4 = LPR * NV;
  constexpr uint32_t d = T4 * 4;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  constexpr bool ALIAS = LPR >= 32;                    // 9 d floats of tables >= the [groups, d] = 1024 NV floats of s_col
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d], s_q[3 * 3 * d], s_own[ALIAS ? 4 : RPB * d];
  const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
  const uint64_t stride = (uint64_t)gridDim.x * RPB;
  uint64_t rowb = (uint64_t)blockIdx.x * RPB;          // block-uniform; the host launches no block without a row

  f32x4 xa[NV], xr[NV], xg[NV];
  // (a macro: the loop's bottom issues the same loads for the next trip)
#define TQ_LNAB_LOAD()                                                                                          \
  {                                                                                                             \
    const uint64_t rl = rowb + sub < rows ? rowb + sub : rows - 1;      /* past the end: the last row, unused */ \
    _Pragma("unroll") for (int k = 0; k < NV; ++k) {                                                            \
      xa[k] = a[rl * T4 + k * LPR + lane];                                                                      \
      xr[k] = r[rl * T4 + k * LPR + lane];                                                                      \
      xg[k] = gyv[rl * T4 + k * LPR + lane];                                                                    \
    }                                                                                                           \
  }
  TQ_LNAB_LOAD()
  // ---- prologue of res_ln_quant_axis_k: the affine and the raw parameters of this thread's columns, all in flight together
  // with the first row; every column's constants derived with qp_from_raw; the forward's block-wide vote
  float aw[NA], ab[NA], pd[3][NA], pz[3][NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const uint32_t c = threadIdx.x + i * kBlock;
    const uint32_t cc = c < d ? c : d - 1;
    aw[i] = ln_w[cc];
    ab[i] = ln_b[cc];
    axb_load_raw(q1, cc, ln_w, pd[0][i], pz[0][i]);
    axb_load_raw(q2, cc, ln_w, pd[1][i], pz[1][i]);
    axb_load_raw(q3, cc, ln_w, pd[2][i], pz[2][i]);
  }
  uint32_t sg[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const tq_quantizer& q = k == 0 ? q1 : (k == 1 ? q2 : q3);
    sg[k] = *(q.signed_flag != nullptr ? q.signed_flag : reinterpret_cast<const uint8_t*>(ln_w));
  }
  AxbLim lim;
  int ok = 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const tq_quantizer& q = k == 0 ? q1 : (k == 1 ? q2 : q3);
    sg[k] = __builtin_amdgcn_readfirstlane(sg[k]);
    lim.on[k] = k == 0 ? on1 : (k == 1 ? on2 : on3);
    lim.lo[k] = lim.hi[k] = 0.f;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      asm volatile("" : "+v"(pd[k][i]), "+v"(pz[k][i]));        // the loads stay where they were issued
      const QP p = lim.on[k] ? qp_from_raw(q, QRaw{pd[k][i], pz[k][i], sg[k]}) : QP{1.f, 0.f, 0.f, 0.f};
      const QF f = make_qf(p);
      ok = ok && (!lim.on[k] || f.ok);
      lim.lo[k] = p.lo;
      lim.hi[k] = p.hi;
      const uint32_t c = threadIdx.x + i * kBlock;
      if (c < d) {
        float* t = s_q + k * 3 * d;
        t[c] = p.scale;
        t[d + c] = f.rcp.x;
        t[2 * d + c] = p.zp;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const uint32_t c = threadIdx.x + i * kBlock;
    if (c < d) { s_w[c] = aw[i]; s_b[c] = ab[i]; }
  }
  const int fast = __syncthreads_and(ok);              // (the barrier behind the tables as well)

  float gw[AG ? NV : 1][4], gb[AG ? NV : 1][4], rd[3][PG ? NV : 1][4], rz[3][PG ? NV : 1][4];
#pragma unroll
  for (int v = 0; v < (AG ? NV : 1); ++v)
#pragma unroll
    for (int e = 0; e < 4; ++e) gw[v][e] = gb[v][e] = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int v = 0; v < (PG ? NV : 1); ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) rd[k][v][e] = rz[k][v][e] = 0.f;
  while (rowb < rows) {
    const uint64_t row = rowb + sub;
    const bool valid = row < rows;
    if (fast) ln_axis_bwd_row<LPR, NV, PG, AG, true>(xa, xr, xg, row, valid, lane, s_w, s_b, s_q, lim, ln_eps, gdv, grv, yv, gw, gb, rd, rz);
    else ln_axis_bwd_row<LPR, NV, PG, AG, false>(xa, xr, xg, row, valid, lane, s_w, s_b, s_q, lim, ln_eps, gdv, grv, yv, gw, gb, rd, rz);
    rowb += stride;
    if (rowb < rows) TQ_LNAB_LOAD()
  }
#undef TQ_LNAB_LOAD
  f32x4* s_col = reinterpret_cast<f32x4*>(ALIAS ? s_q : s_own);
  if constexpr (AG) {
    axb_col_reduce<LPR, NV>(gw, 0, lane, sub, s_col, colpart);
    axb_col_reduce<LPR, NV>(gb, 1, lane, sub, s_col, colpart);
  }
  if constexpr (PG) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (!lim.on[k]) continue;                        // block-uniform; the final launch reads no row of an absent quantizer
      axb_col_reduce<LPR, NV>(rd[k], 2 + 2 * k, lane, sub, s_col, colpart);
      axb_col_reduce<LPR, NV>(rz[k], 3 + 2 * k, lane, sub, s_col, colpart);
    }
  }
}

// 64 of the 8 d columns of the [8, d] block partials per block (d is a multiple of 64: one quantity per block), 4 slices of
// the nb blocks per column, float64.  A quantity nobody asked for returns at once (its rows of the partials were not written).
__global__ __launch_bounds__(kBlock) void ln_quant_axis_bwd_final_k(const float* __restrict__ colpart, uint32_t nb, uint32_t d,
                                                                    float* __restrict__ gw, float* __restrict__ gb,
                                                                    tq_quantizer q1, tq_quantizer q2, tq_quantizer q3,
                                                                    float* __restrict__ g1, float* __restrict__ g2,
                                                                    float* __restrict__ g3, double* __restrict__ colsum) {
  const uint32_t qn = blockIdx.x * 64 / d, c = blockIdx.x * 64 - qn * d + (threadIdx.x & 63);
  const int k = qn < 2 ? -1 : (int)(qn - 2) >> 1, which = qn & 1;
  float* out = qn == 0 ? gw : qn == 1 ? gb : k == 0 ? g1 : k == 1 ? g2 : g3;
  if (out == nullptr) return;                          // block-uniform
  const double t = col_sum_f64<64, 4>(colpart + (uint64_t)qn * d + c, nb, (uint64_t)kLnAxisBwdQuantities * d);
  if (threadIdx.x >= 64) return;
  if (k < 0) { out[c] = (float)t; return; }
  const tq_quantizer& q = k == 0 ? q1 : k == 1 ? q2 : q3;
  if (q.n_params == 1) colsum[(uint64_t)(qn - 2) * d + c] = t;
  else out[(uint64_t)which * d + c] = which ? chain_zero_float(q, c, t) : chain_delta(q, c, t);
}

// The per-tensor quantizers of a mix: their float64 column sums over the d columns in a fixed order (thread, wave, block), the chain.
__global__ __launch_bounds__(kBlock) void ln_quant_axis_bwd_tensor_k(const double* __restrict__ colsum, uint32_t d, tq_quantizer q1,
                                                                     tq_quantizer q2, tq_quantizer q3, float* __restrict__ g1,
                                                                     float* __restrict__ g2, float* __restrict__ g3) {
  __shared__ double s_red[kBlock / kWave];
  for (int j = 0; j < 6; ++j) {
    const int k = j >> 1, which = j & 1;
    float* out = k == 0 ? g1 : k == 1 ? g2 : g3;
    const tq_quantizer& q = k == 0 ? q1 : k == 1 ? q2 : q3;
    if (out == nullptr || q.n_params != 1) continue;   // block-uniform
    double t = 0.0;
    for (uint32_t c = threadIdx.x; c < d; c += kBlock) t += colsum[(uint64_t)j * d + c];
    t = wave_sum(t);
    __syncthreads();                                   // the previous quantity's reads of s_red are done
    if ((threadIdx.x & (kWave - 1)) == 0) s_red[threadIdx.x / kWave] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
      t = 0.0;
      for (int w = 0; w < kBlock / kWave; ++w) t += s_red[w];
      out[which] = which ? chain_zero_float(q, 0, t) : chain_delta(q, 0, t);
    }
  }
}

}  // namespace tq

using namespace tq;

static unsigned ln_axis_bwd_grid(uint64_t rows, int lpr) {
  return (unsigned)std::min<uint64_t>(ceil_div(rows, (uint64_t)(kBlock / lpr)), kLnAxisBwdMaxGrid);
}

// per block its [8, d] column partial; behind them the [6, d] float64 column sums of per-tensor quantizers
static size_t ln_axis_bwd_need(unsigned grid, uint64_t d) {
  return (size_t)grid * kLnAxisBwdQuantities * d * sizeof(float) + 6 * d * sizeof(double);
}

extern "C" size_t tq_residual_layernorm_quant_axis_bwd_workspace_bytes(uint64_t rows, uint64_t d) {
  const int lpr = ln_bwd_lpr(d);
  if (rows == 0 || lpr == 0) return 0;
  return ln_axis_bwd_need(ln_axis_bwd_grid(rows, lpr), d);
}

extern "C" int tq_residual_layernorm_quant_axis_bwd(const float* dense_out, const float* residual, const float* grad_y,
                                                    uint64_t rows, uint64_t d, const tq_quantizer* q_dense,
                                                    const tq_quantizer* q_sum, const float* ln_weight, const float* ln_bias,
                                                    float ln_eps, const tq_quantizer* q_out, float* grad_dense,
                                                    float* grad_residual, float* grad_ln_weight, float* grad_ln_bias,
                                                    float* grad_q_dense, float* grad_q_sum, float* grad_q_out, float* y,
                                                    void* workspace, size_t workspace_bytes, tq_stream_t stream) {
  const char* who = "tq_residual_layernorm_quant_axis_bwd";
  if (rows == 0) return TQ_OK;
  const tq_quantizer* const qs[3] = {q_dense, q_sum, q_out};
  const float* const gq[3] = {grad_q_dense, grad_q_sum, grad_q_out};
  if (int e = tail_bwd_check(who, dense_out, residual, grad_y, ln_weight, ln_bias, grad_dense, grad_residual, y, rows, d, qs, gq, true))
    return e;
  bool tensor_sums = false;
  for (int k = 0; k < 3; ++k) tensor_sums = tensor_sums || (gq[k] != nullptr && qs[k]->n_params == 1);
  TQ_REQUIRE(aligned4({grad_q_dense, grad_q_sum, grad_q_out, grad_ln_weight, grad_ln_bias}), "%s: gradients must be 4-byte aligned",
             who);
  const int lpr = ln_bwd_lpr(d);
  if (lpr == 0)
    return set_error(TQ_EUNSUPPORTED, "%s: row length %llu has no instantiation (64, 128, 256, 384, 512, 768, 1024)", who,
                     (unsigned long long)d);
  const bool pg = grad_q_dense != nullptr || grad_q_sum != nullptr || grad_q_out != nullptr;
  const bool ag = grad_ln_weight != nullptr || grad_ln_bias != nullptr;
  const unsigned grid = ln_axis_bwd_grid(rows, lpr);
  const size_t need = ln_axis_bwd_need(grid, d);
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
  double* colsum = colpart ? reinterpret_cast<double*>(colpart + (size_t)grid * kLnAxisBwdQuantities * d) : nullptr;
#define TQ_LNAB_GO(PGV, AGV, LPR, NV)                                                                           \
  hipLaunchKernelGGL((ln_quant_axis_bwd_k<LPR, NV, PGV, AGV>), dim3(grid), dim3(kBlock), 0, st, av, rv, gv, gdv, grv, yv, rows, \
                     ln_weight, ln_bias, ln_eps, c1, c2, c3, q_dense != nullptr, q_sum != nullptr, q_out != nullptr,            \
                     reinterpret_cast<f32x4*>(colpart))
#define TQ_LNAB(LPR, NV) if (d == (uint64_t)(LPR) * (NV) * 4) TQ_PG_AG_DISPATCH(pg, ag, TQ_LNAB_GO, LPR, NV);
  TQ_TAIL_BWD_FORMS(TQ_LNAB)
#undef TQ_LNAB
#undef TQ_LNAB_GO
  if (int e = check_launch("ln_quant_axis_bwd_k")) return e;
  if (pg || ag) {
    hipLaunchKernelGGL(ln_quant_axis_bwd_final_k, dim3((unsigned)(kLnAxisBwdQuantities * d / 64)), dim3(kBlock), 0, st, colpart,
                       grid, (uint32_t)d, grad_ln_weight, grad_ln_bias, c1, c2, c3, grad_q_dense, grad_q_sum, grad_q_out, colsum);
    if (int e = check_launch("ln_quant_axis_bwd_final_k")) return e;
  }
  if (tensor_sums) {
    hipLaunchKernelGGL(ln_quant_axis_bwd_tensor_k, dim3(1), dim3(kBlock), 0, st, colsum, (uint32_t)d, c1, c2, c3, grad_q_dense,
                       grad_q_sum, grad_q_out);
    return check_launch("ln_quant_axis_bwd_tensor_k");
  }
  return TQ_OK;
}
