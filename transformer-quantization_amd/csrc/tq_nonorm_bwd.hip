// Backward of the residual + NoNorm tail for QAT (forward: csrc/tq_fused_ln.hip res_ln_quant_k, the AFF variant behind
// tq_residual_nonorm_quant_fwd; MobileBERT's `dense -> + residual -> quantizer -> NoNorm -> quantizer`)
//     y = Q_out( Q_sum( Q_dense(dense_out) + residual ) * w + b )
// under the straight-through estimator, as ONE launch over [rows, d] plus one small final launch for the sums over rows (the
// affine gradients, per column, and the range gradients of the three quantizers): 3 reads (dense_out, residual, grad_y) + 2
// writes (grad_dense, grad_residual) = 20 B per fp32 element, against three fake-quant backwards with their parameter-gradient
// launches, the multiply's and the add's backward and two column sums.  Nothing but dense_out and residual is kept from the
// forward: a, t, u, z, the three clamp masks and Q_out's index are RECOMPUTED with the forward's arithmetic.
//
// Per element (every fp32 operation rounded on its own; s_k, zp_k, lo_k, hi_k the derived parameters of quantizer k):
//     a  = Q1(g), in1        t = a + r        u = Q2(t), in2        z = u * w_c + b_c      (mul, then add: the forward's two roundings)
//     y  = Q3(z), in3, xi3
//     gz = in3 ? (gy * s3) / s3 : 0
//     grad_bias_c += gz      grad_weight_c += gz * u                                       (over all rows, per column)
//     gu = gz * w_c
//     gt = in2 ? (gu * s2) / s2 : 0  -> grad_residual          gg = in1 ? (gt * s1) / s1 : 0  -> grad_dense
// and the range-gradient terms of tq_fake_quant_bwd (ste_bwd_elem) with (g, v, s) = (gy, z, s3), (gu, t, s2), (gt, g, s1):
//     d += g (xi - zp) - in (g s v) / (s s)        z += in ? 0 : -(g s)
// NaN rule, element-local like the forward's NoNorm rule: an element whose z is NaN has gz = gt = gg = NaN (a NaN has no grid
// index, so the masks alone would give 0 or NaN depending on the body), hence NaN in its column of both affine gradients and in
// the _delta gradients; every other element and column is what it is without the NaN.
//
// This is not ln_quant_bwd_k without its statistics: nothing is reduced along a row, so a row does not have to live in one
// lane group.  No per-row-length instantiation, no butterflies inside the loop, no [groups, d] buffer; d is a run-time stride.
//
// Work split (gfx950):
//  * A lane owns ONE 16-byte vector of columns for its whole life: its 4 w and 4 b are loaded once and stay in registers, and so
//    do its 8 column accumulators (gz, gz * u) and the 6 range accumulators.
//  * Rows of at most 64 vectors (d = 64, 128, 256): 16, 32 or 64 lanes per row, so a wave holds 4, 2 or 1 ROW SLOTS and covers
//    that many consecutive rows per trip -- 64 consecutive vectors, one full 1 KiB load per stream whatever d is (MobileBERT's
//    intra-bottleneck width 128 keeps every lane busy).  A block is 4 waves = 4, 8 or 16 consecutive rows per trip.
//  * Wider rows (384 .. 3072): strips of 64 vectors, grid = strips x row chunks (bias_act_quant_bwd_k's split); the lanes past
//    the last vector of a ragged strip (d = 384: 96 vectors) load and store nothing and contribute zeros.
//  * Three input streams: the first trip's loads of dense_out, residual and grad_y are issued together with the lane's affine
//    parameters and the nine quantizer-buffer reads (load_qraw) before anything depends on either; inside the loop the next
//    trip's three loads are issued before the current trip's arithmetic.  The loop has no cross-lane operation, so every lane
//    runs its own trip count: a row slot past the last row simply leaves early.
//  * Both bodies of the forward, chosen by the forward's vote (make_qf(p).ok of every present quantizer).  Branch-free body: mask
//    and index from ONE Markstein quotient on the grid widened by one step (q_recompute, tq_ste_bwd.h), data-gradient divisions as
//    Markstein quotients; the range term (g s v) / (s s) stays an IEEE division.  The front always dequantises with the "+ 0"
//    fma: where the forward's all-quantizers variant skips it, a -0 can reach z only as a -0, which Q_out normalises.
//  * Block end: the 4 waves x (4 | 2 | 1) row slots meet ONCE in LDS (8 KiB: weight and bias sums side by side); the first 128
//    threads add the partial vectors of a column in (wave, slot) order and write the block's segment of the [chunks, 2, d]
//    column partials; the range sums take one wave butterfly + an LDS hop of their own (block_range_sums): 8 floats per block behind the column
//    partials.
//  * Final launch (nonorm_quant_bwd_final_k): 16 of the 2 d columns x 16 slices per block add a column's `chunks` partials in
//    float64 in a fixed order (slice s takes chunks s, s + 16, ..; then slice 0 + 1 + .. + 15: with 64 x 4, the split of
//    ln_quant_bwd_final_k, a thread added 512 partials one after the other at [16384, 128] and the launch took 135 us); ONE more
//    block finishes the six range sums over the chunks x strips block partials in float64 and applies the chain through
//    clamp(delta, eps) | exp(delta) and the zero-point clamp (range_chain, tq_ste_bwd.h).  ln_quant_bwd_final_k has ONE partial count for both parts; here the column sums have
//    `chunks` partials and the range sums chunks x strips, so the kernel is written here.  No atomics: two runs, identical bits.
//  * Grid cap kNnMaxBlocks = 2048 (256 CUs x 8 resident blocks): chunks = min(ceil(rows / rows per block trip), 2048 / strips);
//    blocks stride over the rows, so the workspace is bounded by 2048 x (2 x 256 + 8) floats.
//  * PG (range gradients), AG (affine gradients) and the body are template parameters: what is not asked for is not compiled
//    in.  No scratch in any instantiation (lib/kernel_resources.json).
// The recomputed quantizer, its STE backward, the block-end and final sums and the chain are the shared pieces of
// csrc/tq_ste_bwd.h; the checks and the launch dispatch of the entry are shared in csrc/tq_host.h.
#include <algorithm>

#include "tq_device.h"
#include "tq_host.h"
#include "tq_rows.h"
#include "tq_ste_bwd.h"

namespace tq {

constexpr int kNnStripVec = 64;                  // 16-byte vectors per strip: one wave
constexpr int kNnWaves = kBlock / kWave;
constexpr unsigned kNnMaxBlocks = 2048;
constexpr int kNnFinalCols = 16;                 // the final launch: 16 columns x 16 slices of the chunks per block
constexpr int kNnSlices = kBlock / kNnFinalCols;

struct NnAcc { float d1, z1, d2, z2, d3, z3; };

struct NnParams {
  SmQW f1, f2, f3;          // branch-free body
  FusedQ g1, g2, g3;        // division body
  int on1, on2, on3;
};

// The rows of one lane: its column vector `cv` of rows row, row + stride, ..; xa / xr / xg hold the first row's loads.
template <bool PG, bool AG, bool FAST>
__device__ __forceinline__ void nn_bwd_rows(const f32x4* __restrict__ a, const f32x4* __restrict__ r, const f32x4* __restrict__ gyv,
                                            f32x4* __restrict__ gdv, f32x4* __restrict__ grv, f32x4* __restrict__ yv, uint64_t rows,
                                            uint64_t nvec, uint64_t row, uint64_t stride, uint64_t cv, f32x4 xa, f32x4 xr, f32x4 xg,
                                            const f32x4& w, const f32x4& b, const NnParams& c, NnAcc& acc, float (&gw)[4],
                                            float (&gb)[4]) {
  for (;;) {
    const uint64_t nxt = row + stride;
    f32x4 na = xa, nr = xr, ng = xg;
    if (nxt < rows) {
      const uint64_t nat = nxt * nvec + cv;
      na = a[nat];
      nr = r[nat];
      ng = gyv[nat];
    }
    f32x4 oy, ot, og;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool i1, i2, i3;
      float h1, h2, h3;
      const float aq = q_recompute<FAST, true>(xa[e], c.f1, c.g1, c.on1, i1, h1);
      const float t = aq + xr[e];
      float u = q_recompute<FAST, true>(t, c.f2, c.g2, c.on2, i2, h2);
      // (the forward's front works on v_med3, which drops a NaN, and restores it from the input pair: the same here, so that a
      // NaN behind an ABSENT quantizer and one behind a present quantizer are the same NaN element)
      if (FAST) u = __builtin_isunordered(xa[e], xr[e]) ? __builtin_nanf("") : u;
      const float z = u * w[e] + b[e];
      float y = q_recompute<FAST, true>(z, c.f3, c.g3, c.on3, i3, h3);
      if (FAST) y = z != z ? z : y;                  // the forward passes the NaN itself through
      const bool nz = z != z;
      float gz = ste_backward<PG, FAST>(xg[e], z, h3, i3, true, c.f3, c.g3, c.on3, acc.d3, acc.z3);
      gz = nz ? z : gz;
      if (AG) {
        gb[e] += gz;
        gw[e] += gz * u;
      }
      const float gu = gz * w[e];
      float gt = ste_backward<PG, FAST>(gu, t, h2, i2, true, c.f2, c.g2, c.on2, acc.d2, acc.z2);
      gt = nz ? z : gt;
      float gg = ste_backward<PG, FAST>(gt, xa[e], h1, i1, true, c.f1, c.g1, c.on1, acc.d1, acc.z1);
      gg = nz ? z : gg;
      oy[e] = y;
      ot[e] = gt;
      og[e] = gg;
    }
    const uint64_t at = row * nvec + cv;
    if (yv != nullptr) yv[at] = oy;
    if (grv != nullptr) grv[at] = ot;
    if (gdv != nullptr) gdv[at] = og;
    if (nxt >= rows) break;
    row = nxt;
    xa = na;
    xr = nr;
    xg = ng;
  }
}

// grid = (strips, chunks).  sh = log2(lanes per row slot): 4, 5 or 6 (d = 64, 128, >= 256); a wave holds 64 >> sh row slots.
template <bool PG, bool AG>
__global__ __launch_bounds__(kBlock) void nonorm_quant_bwd_k(const f32x4* __restrict__ a, const f32x4* __restrict__ r,
                                                             const f32x4* __restrict__ gyv, f32x4* __restrict__ gdv,
                                                             f32x4* __restrict__ grv, f32x4* __restrict__ yv, uint64_t rows,
                                                             uint32_t nvec, uint32_t sh, const float* __restrict__ ln_w,
                                                             const float* __restrict__ ln_b, tq_quantizer q1, tq_quantizer q2,
                                                             tq_quantizer q3, int on1, int on2, int on3,
                                                             f32x4* __restrict__ colpart, float* __restrict__ rngpart) {
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const uint32_t slots = kWave >> sh;                  // row slots per wave
  const uint32_t slot = lane >> sh, j = lane & ((1u << sh) - 1);
  const uint64_t cv = (uint64_t)blockIdx.x * kNnStripVec + j;
  const uint64_t rpb = (uint64_t)kNnWaves * slots;     // rows per block trip
  const uint64_t row0 = (uint64_t)blockIdx.y * rpb + wave * slots + slot;
  const uint64_t stride = (uint64_t)gridDim.y * rpb;
  const bool live = cv < nvec && row0 < rows;          // a lane past a ragged strip's end, a row slot past the last row
  f32x4 xa = {0.f, 0.f, 0.f, 0.f}, xr = xa, xg = xa, w = xa, b = xa;
  if (live) {
    const uint64_t at = row0 * nvec + cv;
    xa = a[at];
    xr = r[at];
    xg = gyv[at];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      w[e] = ln_w[cv * 4 + e];
      b[e] = ln_b[cv * 4 + e];
    }
  }
  QRaw w1 = load_qraw(q1, 0, ln_w), w2 = load_qraw(q2, 0, ln_w), w3 = load_qraw(q3, 0, ln_w);
  qraw_arrived(w1); qraw_arrived(w2); qraw_arrived(w3);
  TQ_TAIL_QUANTIZERS
  TQ_TAIL_VOTE
  const NnParams c = {make_qw(tq.p1), make_qw(tq.p2), make_qw(tq.p3), make_fq(tq.p1, on1), make_fq(tq.p2, on2),
                      make_fq(tq.p3, on3), on1, on2, on3};
  NnAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float gw[4] = {0.f, 0.f, 0.f, 0.f}, gb[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    if (fast) nn_bwd_rows<PG, AG, true>(a, r, gyv, gdv, grv, yv, rows, nvec, row0, stride, cv, xa, xr, xg, w, b, c, acc, gw, gb);
    else nn_bwd_rows<PG, AG, false>(a, r, gyv, gdv, grv, yv, rows, nvec, row0, stride, cv, xa, xr, xg, w, b, c, acc, gw, gb);
  }
  // ---- block end: every thread arrives (lanes that were not live hold zeros)
  if constexpr (PG) {
    const float sums[6] = {acc.d1, acc.z1, acc.d2, acc.z2, acc.d3, acc.z3};
    block_range_sums(sums, rngpart + 8 * ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x));
  }
  __shared__ f32x4 s_col[AG ? 2 * kBlock : 1];
  if (AG) {
    s_col[threadIdx.x] = f32x4{gw[0], gw[1], gw[2], gw[3]};
    s_col[kBlock + threadIdx.x] = f32x4{gb[0], gb[1], gb[2], gb[3]};
    __syncthreads();
  }
  if (AG && threadIdx.x < 2 * kNnStripVec) {
    const uint32_t which = threadIdx.x / kNnStripVec, jj = threadIdx.x & (kNnStripVec - 1);      // weight, then bias
    const uint64_t cvo = (uint64_t)blockIdx.x * kNnStripVec + jj;
    if (jj < (1u << sh) && cvo < nvec) {
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      for (uint32_t wv = 0; wv < (uint32_t)kNnWaves; ++wv)
        for (uint32_t s = 0; s < slots; ++s) t = t + s_col[which * kBlock + wv * kWave + (s << sh) + jj];
      colpart[((uint64_t)blockIdx.y * 2 + which) * nvec + cvo] = t;
    }
  }
}

// Blocks 0 .. ncb - 1: 16 of the 2 d columns of the [chunks, 2, d] block partials each (weight, then bias), 16 slices of the
// chunks per column, float64.  Block ncb (only with range gradients): the six range sums over the nbr = chunks x strips block
// partials in float64, then the chain (final_range_sums, range_chain: tq_ste_bwd.h).
__global__ __launch_bounds__(kBlock) void nonorm_quant_bwd_final_k(const float* __restrict__ colpart, const float* __restrict__ rngpart,
                                                                   uint32_t chunks, uint32_t nbr, uint32_t d, uint32_t ncb,
                                                                   float* __restrict__ gw, float* __restrict__ gb, tq_quantizer q1,
                                                                   tq_quantizer q2, tq_quantizer q3, float* __restrict__ g1,
                                                                   float* __restrict__ g2, float* __restrict__ g3) {
  if (blockIdx.x < ncb) {
    const uint32_t col = blockIdx.x * kNnFinalCols + threadIdx.x % kNnFinalCols;     // < 2 d: 2 d is a multiple of 16
    const double t = col_sum_f64<kNnFinalCols, kNnSlices>(colpart + col, chunks, 2 * (uint64_t)d);
    float* out = col < d ? gw : gb;
    if (threadIdx.x < kNnFinalCols && out != nullptr) out[col < d ? col : col - d] = (float)t;
    return;
  }
  for (int which = 0; which < 3; ++which) {
    float* out = which == 0 ? g1 : which == 1 ? g2 : g3;
    if (out == nullptr) continue;                  // block-uniform
    double dsum, zsum;
    final_range_sums(rngpart, nbr, 8, 2 * which, dsum, zsum);
    if (threadIdx.x == 0) {
      const RangeGrad g = range_chain(which == 0 ? q1 : which == 1 ? q2 : q3, 0, dsum, zsum);
      out[0] = g.delta;
      out[1] = g.zero_float;
    }
  }
}

}  // namespace tq

using namespace tq;

namespace {

struct NnGrid {
  uint32_t nvec, sh;
  unsigned strips, chunks;
};

// -> false where the forward's fp32 tail has no instantiation for d (d / 4 in 16, 32, 64, 96, 128, 192, 256, 384, 512, 768)
bool nn_grid(uint64_t rows, uint64_t d, NnGrid& g) {
  bool known = false;
  for (uint64_t v : {16, 32, 64, 96, 128, 192, 256, 384, 512, 768}) known = known || d == 4 * v;
  if (!known) return false;
  g.nvec = (uint32_t)(d / 4);
  g.sh = g.nvec == 16 ? 4 : g.nvec == 32 ? 5 : 6;
  g.strips = (unsigned)ceil_div((uint64_t)g.nvec, (uint64_t)kNnStripVec);
  const uint64_t rpb = (uint64_t)kNnWaves * (kWave >> g.sh);
  g.chunks = (unsigned)std::min<uint64_t>(ceil_div(rows, rpb), kNnMaxBlocks / g.strips);
  return true;
}

size_t nn_workspace(const NnGrid& g) {
  return ((size_t)g.chunks * 2 * g.nvec * 4 + (size_t)g.chunks * g.strips * 8) * sizeof(float);
}

}  // namespace

// per row chunk its [2, d] column partial, then eight floats per block for the six range sums
extern "C" size_t tq_residual_nonorm_quant_bwd_workspace_bytes(uint64_t rows, uint64_t d) {
  NnGrid g;
  if (rows == 0 || !nn_grid(rows, d, g)) return 0;
  return nn_workspace(g);
}

extern "C" int tq_residual_nonorm_quant_bwd(const float* dense_out, const float* residual, const float* grad_y, uint64_t rows,
                                            uint64_t d, const tq_quantizer* q_dense, const tq_quantizer* q_sum, const float* weight,
                                            const float* bias, const tq_quantizer* q_out, float* grad_dense, float* grad_residual,
                                            float* grad_weight, float* grad_bias, float* grad_q_dense, float* grad_q_sum,
                                            float* grad_q_out, float* y, void* workspace, size_t workspace_bytes,
                                            tq_stream_t stream) {
  const char* who = "tq_residual_nonorm_quant_bwd";
  if (rows == 0) return TQ_OK;
  if (int e = tail_bwd_check(who, dense_out, residual, grad_y, weight, bias, grad_dense, grad_residual, y, rows, d,
                             {q_dense, q_sum, q_out}, {grad_q_dense, grad_q_sum, grad_q_out}, false))
    return e;
  TQ_REQUIRE(aligned4({grad_q_dense, grad_q_sum, grad_q_out, grad_weight, grad_bias, weight, bias}),
             "%s: affine parameters and gradients must be 4-byte aligned", who);
  NnGrid g;
  if (!nn_grid(rows, d, g))
    return set_error(TQ_EUNSUPPORTED, "%s: row length %llu is not one of the forward's (64, 128, 256, 384, 512, 768, 1024, 1536, "
                     "2048, 3072)", who, (unsigned long long)d);
  const bool pg = grad_q_dense != nullptr || grad_q_sum != nullptr || grad_q_out != nullptr;
  const bool ag = grad_weight != nullptr || grad_bias != nullptr;
  const size_t need = nn_workspace(g);
  if (int e = bwd_workspace_check(who, pg || ag, workspace, workspace_bytes, need)) return e;
  const tq_quantizer none{};
  const tq_quantizer &c1 = q_dense ? *q_dense : none, &c2 = q_sum ? *q_sum : none, &c3 = q_out ? *q_out : none;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* colpart = (pg || ag) ? static_cast<float*>(workspace) : nullptr;
  float* rngpart = colpart ? colpart + (size_t)g.chunks * 2 * d : nullptr;
#define TQ_NNB_GO(PGV, AGV)                                                                                                   \
  hipLaunchKernelGGL((nonorm_quant_bwd_k<PGV, AGV>), dim3(g.strips, g.chunks), dim3(kBlock), 0, st,                           \
                     reinterpret_cast<const f32x4*>(dense_out), reinterpret_cast<const f32x4*>(residual),                     \
                     reinterpret_cast<const f32x4*>(grad_y), reinterpret_cast<f32x4*>(grad_dense),                            \
                     reinterpret_cast<f32x4*>(grad_residual), reinterpret_cast<f32x4*>(y), rows, g.nvec, g.sh, weight, bias,   \
                     c1, c2, c3, q_dense != nullptr, q_sum != nullptr, q_out != nullptr, reinterpret_cast<f32x4*>(colpart),   \
                     rngpart)
  TQ_PG_AG_DISPATCH(pg, ag, TQ_NNB_GO);
#undef TQ_NNB_GO
  if (int e = check_launch("nonorm_quant_bwd_k")) return e;
  if (pg || ag) {
    const unsigned ncb = ag ? (unsigned)(2 * d / kNnFinalCols) : 0;
    hipLaunchKernelGGL(nonorm_quant_bwd_final_k, dim3(ncb + (pg ? 1 : 0)), dim3(kBlock), 0, st, colpart, rngpart, g.chunks,
                       g.chunks * g.strips, (uint32_t)d, ncb, grad_weight, grad_bias, c1, c2, c3, grad_q_dense, grad_q_sum,
                       grad_q_out);
    return check_launch("nonorm_quant_bwd_final_k");
  }
  return TQ_OK;
}
