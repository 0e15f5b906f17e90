// Bias + activation function + PER-COLUMN output quantizer behind a Linear's GEMM, and its backward for QAT:
//     y = Q_c( act( gemm + bias_c ) )                  act = none | ReLU | GELU (erf form), Q_c: one parameter per column
// The per-column form of csrc/tq_act_bwd.hip (per-embedding / per-embedding-group output quantizers of the query, key and value
// Linears hold `_delta[cols]` / `_zero_float[cols]` in natural column order: n_params == cols, inner == 1).  Layered, the bias
// add, the activation function and tq_fake_quant_fwd are sweeps of their own and the backward is tq_fake_quant_bwd with `cols`
// parameters and its per-parameter reductions, the activation's backward and the bias gradient's column sum.  Here the forward
// is ONE launch (8 B per element) and the backward ONE launch (12 B per element) plus one small final launch when a sum over
// rows is asked for; only `gemm` is kept from the forward.
//
// Per element, every fp32 operation rounded on its own (s_c, zp_c of column c, lo, hi of the grid: tq_device.h make_qp(q, c)):
//     a = g + bias_c          h = act(a)          r = rint(h / s_c) + zp_c        in = lo <= r <= hi
//     xi = clamp(r, lo, hi)   y = s_c * (xi - zp_c)
//     gh = in ? (gy * s_c) / s_c : 0                ga = gh * act'(a)  -> grad_gemm          (act, act': csrc/tq_act.h)
//     grad_bias_c = sum over rows of ga
//     d_c = sum over rows of gy (xi - zp_c) - in (gy s_c h) / (s_c s_c)      z_c = sum over rows of (in ? 0 : -(gy s_c))
// and the chain per column through clamp(delta_c, eps) and the zero-point clamp (range_chain, tq_ste_bwd.h).  NaN rule (the one
// of tq_act_bwd.hip): an element whose h is NaN has ga = NaN, so ITS column of grad_bias and of the _delta gradient are NaN;
// every other element and column is what it is without the NaN.
//
// Work split (gfx950): tq_act_bwd.hip's grid, which suits a per-column quantizer better than the LayerNorm tail's did.
//  * grid = (strips of 64 16-byte vectors = 256 columns) x (row chunks); a block is 4 waves = 4 ROW GROUPS over the same strip;
//    wave w of chunk c walks rows 4 c + w, + 4 chunks, .. (grid stride), one row per trip, the next row's loads issued before
//    the current row's arithmetic.  chunks = min(ceil(rows / 4), max(1, 2048 / strips)): at most 2048 blocks.
//  * A lane owns ONE vector of columns for its whole life, so everything per column is lane-local REGISTERS: the bias (4), the
//    quantizer constants of its four columns -- scale, guarded reciprocal, zero point (12; the grid ends lo, hi are the same for
//    every column and stay scalar) -- and, in the backward, four bias column sums and four d and four z accumulators.  No LDS
//    table, no instantiation per row length, and NO cross-lane operation in the loop: a range sum here is a column sum.
//  * Body vote PER STRIP: a lane votes make_qf(p).ok for its four columns (a lane past the end of a ragged strip votes "ok"), the
//    wave takes the ballot.  Every wave of a block holds the same 64 vectors, so the four waves agree without meeting, and the
//    forward and the backward (same grid, same text: strip_vote) agree per strip.  Branch-free body: q_recompute<true, true>
//    (tq_ste_bwd.h: one Markstein quotient on the grid widened by one step) and a Markstein quotient for gh.  Division body
//    (a scale outside [2^-100, 2^100] or a grid of 2^22 steps and more somewhere in the strip): tq_fake_quant_fwd's q_index /
//    q_dequant text and IEEE divisions.  Either gives the bits of tq_fake_quant_fwd (n_params = cols, inner = 1) on the kernel's
//    own h; both are compiled in.  The range term (gy s h) / (s s) is an IEEE division in both.
//  * Block end: the four row groups meet ONCE in LDS (up to three planes -- bias, d, z -- of [4][64] vectors: 12 KiB); wave p adds
//    plane p's four partial vectors in group order and writes it: the block's [3][256] partial (a plane nobody asked for is
//    neither staged nor written nor read).  workspace = chunks x strips x 3 x 256 floats.
//  * Final launch: 64 columns per block, 4 slices of the `chunks` block partials per column and plane in float64
//    (col_sum_f64<64, 4>: slice s takes chunks s, s + 4, ..; then 0 + 1 + 2 + 3 -- the order of bias_act_quant_bwd_final_k), then
//    range_chain per column.  No atomics: two runs give identical bits.
//  * ACT, PG (range gradients) and CG (the bias column sum) are template parameters.  Registers: lib/kernel_resources.json and
//    DESIGN.md section 8; no scratch in any instantiation.
#include "tq_act.h"
#include "tq_device.h"
#include "tq_host.h"
#include "tq_rows.h"
#include "tq_ste_bwd.h"

namespace tq {

constexpr int kActAxisPlanes = 3;                // bias, d, z: a block's partial is [3][256]
constexpr int kActStripCols = kActStripVec * 4;

// the quantizer constants of a lane's four columns; lo, hi are wave-uniform
struct AxisQ {
  f32x4 s, rc, zp;
  float lo, hi;
};

// Derives the constants of columns 4 cv .. 4 cv + 3 (`live`: the lane has a vector) and takes the strip's vote.
__device__ __forceinline__ bool strip_vote(const tq_quantizer& q, uint64_t cv, bool live, AxisQ& c) {
  bool ok = true;
  c.lo = c.hi = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    QP p = QP{1.f, 0.f, 0.f, 0.f};
    if (live) p = make_qp(q, cv * 4 + e);
    const QF f = make_qf(p);
    ok = ok && f.ok;
    c.s[e] = p.scale;
    c.rc[e] = f.rcp.x;
    c.zp[e] = p.zp;
    if (live) { c.lo = p.lo; c.hi = p.hi; }
  }
  // (lane 0 of a strip always has a vector: the grid ends become scalars)
  c.lo = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, c.lo)));
  c.hi = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(uint32_t, c.hi)));
  return __builtin_amdgcn_ballot_w64(ok) == ~0ull;
}

// The forward of one element from a = g + bias_c: h (through hh), y, and for the backward the clamp mask and xi - zp_c.
template <int ACT, bool DERIV, bool FAST>
__device__ __forceinline__ float act_axis_elem(float a, float s, float rc, float zp, float lo, float hi, float& hh, float& dact,
                                               bool& in, float& hc) {
  const float h = act_eval<ACT, DERIV>(a, dact);
  hh = h;
  if constexpr (FAST) {
    return q_recompute<true, true>(h, s, rc, zp, lo, hi, 1, in, hc);
  } else {                                         // tq_fake_quant_fwd's division body: q_index / q_dequant, an IEEE division
    const float r = rintf(h / s) + zp;
    in = r >= lo && r <= hi;
    const float xi = clamp_nanprop(r, lo, hi);
    hc = xi - zp;
    return s * hc;
  }
}

// ------------------------------------------------------------------------------ forward
template <int ACT, bool FAST>
__device__ __forceinline__ void act_axis_fwd_rows(const f32x4* __restrict__ gv, f32x4* __restrict__ yv, const f32x4& b, uint64_t rows,
                                                  uint64_t nvec, uint64_t cv, const AxisQ& c) {
  const uint64_t stride = (uint64_t)gridDim.y * kActGroups;
  uint64_t row = (uint64_t)blockIdx.y * kActGroups + threadIdx.x / kActStripVec;
  if (row >= rows) return;
  f32x4 xg = gv[row * nvec + cv];
  for (;;) {
    const uint64_t nxt = row + stride;
    f32x4 ng = xg;
    if (nxt < rows) ng = gv[nxt * nvec + cv];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float hh, dact, hc;
      bool in;
      o[e] = act_axis_elem<ACT, false, FAST>(xg[e] + b[e], c.s[e], c.rc[e], c.zp[e], c.lo, c.hi, hh, dact, in, hc);
    }
    yv[row * nvec + cv] = o;
    if (nxt >= rows) break;
    row = nxt;
    xg = ng;
  }
}

template <int ACT>
__global__ __launch_bounds__(kBlock) void bias_act_quant_axis_fwd_k(const f32x4* __restrict__ gv, const f32x4* __restrict__ bias,
                                                                    f32x4* __restrict__ yv, uint64_t rows, uint64_t nvec,
                                                                    tq_quantizer q) {
  const uint64_t cv = (uint64_t)blockIdx.x * kActStripVec + (threadIdx.x & (kActStripVec - 1));
  AxisQ c;
  const bool fast = strip_vote(q, cv, cv < nvec, c);
  if (cv >= nvec) return;                          // ragged strip: no barrier follows
  const f32x4 b = bias != nullptr ? bias[cv] : f32x4{0.f, 0.f, 0.f, 0.f};
  if (fast) act_axis_fwd_rows<ACT, true>(gv, yv, b, rows, nvec, cv, c);
  else act_axis_fwd_rows<ACT, false>(gv, yv, b, rows, nvec, cv, c);
}

// ------------------------------------------------------------------------------ backward
struct AxisAcc {
  f32x4 col, d, z;
};

template <int ACT, bool PG, bool CG, bool FAST>
__device__ __forceinline__ void act_axis_bwd_rows(const f32x4* __restrict__ gv, const f32x4* __restrict__ gyv,
                                                  f32x4* __restrict__ gav, f32x4* __restrict__ hv, f32x4* __restrict__ yv,
                                                  const f32x4& b, uint64_t rows, uint64_t nvec, uint64_t cv, const AxisQ& c,
                                                  AxisAcc& acc) {
  const uint64_t stride = (uint64_t)gridDim.y * kActGroups;
  uint64_t row = (uint64_t)blockIdx.y * kActGroups + threadIdx.x / kActStripVec;
  if (row >= rows) return;
  f32x4 xg = gv[row * nvec + cv], xy = gyv[row * nvec + cv];
  for (;;) {
    const uint64_t nxt = row + stride;
    f32x4 ng = xg, ny = xy;
    if (nxt < rows) {
      ng = gv[nxt * nvec + cv];
      ny = gyv[nxt * nvec + cv];
    }
    f32x4 oa, oh, oy;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float h, dact, hc;
      bool in;
      const float gy = xy[e], s = c.s[e];
      oy[e] = act_axis_elem<ACT, true, FAST>(xg[e] + b[e], s, c.rc[e], c.zp[e], c.lo, c.hi, h, dact, in, hc);
      oh[e] = h;
      // act_bwd_rows' STE terms (csrc/tq_act_bwd.hip; the mask applied BEFORE the range terms, as there), on column e's scale
      const float gs = gy * s;
      float gh = FAST ? div_rn(gs, -s, c.rc[e]) : gs / s;
      gh = in ? gh : 0.0f;
      if (PG) {
        float dd = gy * hc;
        if (in) dd -= (gs * h) / (s * s);
        acc.d[e] += dd;
        acc.z[e] += in ? 0.0f : -gs;
      }
      float ga = gh * dact;
      ga = h != h ? h : ga;                        // NaN rule
      if (CG) acc.col[e] += ga;
      oa[e] = ga;
    }
    const uint64_t at = row * nvec + cv;
    gav[at] = oa;
    if (hv != nullptr) hv[at] = oh;
    if (yv != nullptr) yv[at] = oy;
    if (nxt >= rows) break;
    row = nxt;
    xg = ng;
    xy = ny;
  }
}

template <int ACT, bool PG, bool CG>
__global__ __launch_bounds__(kBlock) void bias_act_quant_axis_bwd_k(const f32x4* __restrict__ gv, const f32x4* __restrict__ bias,
                                                                    const f32x4* __restrict__ gyv, f32x4* __restrict__ gav,
                                                                    f32x4* __restrict__ hv, f32x4* __restrict__ yv, uint64_t rows,
                                                                    uint64_t nvec, tq_quantizer q, f32x4* __restrict__ part) {
  const int lane = threadIdx.x & (kActStripVec - 1), grp = threadIdx.x / kActStripVec;
  const uint64_t cv = (uint64_t)blockIdx.x * kActStripVec + lane;
  AxisQ c;
  const bool fast = strip_vote(q, cv, cv < nvec, c);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  AxisAcc acc = {zero, zero, zero};
  if (cv < nvec) {                                 // lanes past a ragged strip's end keep zeros and meet the others below
    const f32x4 b = bias != nullptr ? bias[cv] : zero;
    if (fast) act_axis_bwd_rows<ACT, PG, CG, true>(gv, gyv, gav, hv, yv, b, rows, nvec, cv, c, acc);
    else act_axis_bwd_rows<ACT, PG, CG, false>(gv, gyv, gav, hv, yv, b, rows, nvec, cv, c, acc);
  }
  if constexpr (PG || CG) {
    // plane 0: bias, 1: d, 2: z.  Wave p adds plane p over the four row groups in group order.
    constexpr int P0 = CG ? 0 : 1, P1 = PG ? kActAxisPlanes : 1;
    __shared__ f32x4 s_part[P1 - P0][kBlock];
    if (CG) s_part[0][threadIdx.x] = acc.col;
    if (PG) {
      s_part[1 - P0][threadIdx.x] = acc.d;
      s_part[2 - P0][threadIdx.x] = acc.z;
    }
    __syncthreads();
    const int plane = P0 + grp;
    if (plane < P1) {
      f32x4 t = s_part[grp][lane];
#pragma unroll
      for (int g = 1; g < kActGroups; ++g) t = t + s_part[grp][g * kActStripVec + lane];
      const uint64_t blk = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
      part[(blk * kActAxisPlanes + plane) * kActStripVec + lane] = t;
    }
  }
}

// 64 columns per block: per plane asked for, the float64 sum of the column's `chunks` block partials; then the chain per column.
__global__ __launch_bounds__(kBlock) void bias_act_quant_axis_bwd_final_k(const float* __restrict__ part, uint32_t chunks,
                                                                          uint32_t strips, uint64_t cols,
                                                                          float* __restrict__ grad_bias, tq_quantizer q,
                                                                          float* __restrict__ grad_q) {
  const uint64_t col = (uint64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = col < cols;
  const float* src = part + (live ? (col / kActStripCols) * (kActAxisPlanes * kActStripCols) + col % kActStripCols : 0);
  const uint32_t n = live ? chunks : 0;
  const uint64_t stride = (uint64_t)strips * (kActAxisPlanes * kActStripCols);
  if (grad_bias != nullptr) {                      // (block-uniform, as grad_q below)
    const double t = col_sum_f64<64, 4>(src, n, stride);
    if (threadIdx.x < 64 && live) grad_bias[col] = (float)t;
  }
  if (grad_q != nullptr) {
    __syncthreads();                               // col_sum_f64's buffer: the previous sum's reads are done
    const double dsum = col_sum_f64<64, 4>(src + kActStripCols, n, stride);
    __syncthreads();
    const double zsum = col_sum_f64<64, 4>(src + 2 * kActStripCols, n, stride);
    if (threadIdx.x < 64 && live) {
      const RangeGrad g = range_chain(q, col, dsum, zsum);
      grad_q[col] = g.delta;
      grad_q[cols + col] = g.zero_float;
    }
  }
}

}  // namespace tq

using namespace tq;

namespace {

// act_check (tq_act.h) and this pair's rule for the quantizer: required, one parameter per column in natural order
int act_check_axis(const char* who, const float* gemm, const float* bias, uint64_t rows, uint64_t cols, int act, const tq_quantizer* q) {
  TQ_REQUIRE(q != nullptr, "%s: q_out is required (an absent or per-tensor quantizer: tq_bias_act_quant_*)", who);
  if (int e = act_check(who, gemm, bias, rows, cols, act, q)) return e;
  TQ_REQUIRE(q->n_params == cols && q->inner == 1,
             "%s: one quantizer parameter per column (n_params = cols = %llu, inner = 1); got n_params = %llu, inner = %llu", who,
             (unsigned long long)cols, (unsigned long long)q->n_params, (unsigned long long)q->inner);
  TQ_REQUIRE(!q->log_domain, "%s: linear scale domain only", who);
  TQ_REQUIRE(aligned4({q->delta, q->zero_float}), "%s: quantizer parameters must be 4-byte aligned", who);
  return TQ_OK;
}

size_t act_axis_need(const ActGrid& g) { return (size_t)g.chunks * g.strips * kActAxisPlanes * kActStripCols * sizeof(float); }

}  // namespace

extern "C" int tq_bias_act_quant_axis_fwd(const float* gemm, const float* bias, float* y, uint64_t rows, uint64_t cols, int act,
                                          const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_bias_act_quant_axis_fwd";
  if (rows == 0) return TQ_OK;
  if (int e = act_check_axis(who, gemm, bias, rows, cols, act, q_out)) return e;
  TQ_REQUIRE(y != nullptr && aligned16(y), "%s: y must be a 16-byte aligned pointer", who);
  const ActGrid g = act_grid(rows, cols);
  hipStream_t st = static_cast<hipStream_t>(stream);
#define TQ_ACTXF(A)                                                                                                   \
  hipLaunchKernelGGL((bias_act_quant_axis_fwd_k<A>), dim3(g.strips, g.chunks), dim3(kBlock), 0, st,                   \
                     reinterpret_cast<const f32x4*>(gemm), reinterpret_cast<const f32x4*>(bias), reinterpret_cast<f32x4*>(y), \
                     rows, g.nvec, *q_out)
  if (act == TQ_ACT_GELU) TQ_ACTXF(TQ_ACT_GELU);
  else if (act == TQ_ACT_RELU) TQ_ACTXF(TQ_ACT_RELU);
  else TQ_ACTXF(TQ_ACT_NONE);
#undef TQ_ACTXF
  return check_launch("bias_act_quant_axis_fwd_k");
}

extern "C" size_t tq_bias_act_quant_axis_bwd_workspace_bytes(uint64_t rows, uint64_t cols) {
  if (rows == 0 || cols == 0 || cols % 4 != 0) return 0;
  return act_axis_need(act_grid(rows, cols));
}

extern "C" int tq_bias_act_quant_axis_bwd(const float* gemm, const float* bias, const float* grad_y, uint64_t rows, uint64_t cols,
                                          int act, const tq_quantizer* q_out, float* grad_gemm, float* grad_bias,
                                          float* grad_q_out, float* h, float* y, void* workspace, size_t workspace_bytes,
                                          tq_stream_t stream) {
  const char* who = "tq_bias_act_quant_axis_bwd";
  if (rows == 0) return TQ_OK;
  if (int e = act_check_axis(who, gemm, bias, rows, cols, act, q_out)) return e;
  TQ_REQUIRE(grad_y != nullptr && grad_gemm != nullptr, "%s: NULL pointer", who);
  TQ_REQUIRE(aligned16(grad_y) && aligned16(grad_gemm) && aligned16(h) && aligned16(y), "%s: 16-byte alignment required", who);
  TQ_REQUIRE(grad_bias == nullptr || bias != nullptr, "%s: grad_bias asked for an absent bias", who);
  TQ_REQUIRE(aligned4({grad_bias, grad_q_out}), "%s: gradients must be 4-byte aligned", who);
  const ActGrid g = act_grid(rows, cols);
  const bool pg = grad_q_out != nullptr, cg = grad_bias != nullptr;
  if (int e = bwd_workspace_check(who, pg || cg, workspace, workspace_bytes, act_axis_need(g))) return e;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = (pg || cg) ? static_cast<float*>(workspace) : nullptr;
#define TQ_ACTXB_GO(PGV, CGV, A)                                                                                      \
  hipLaunchKernelGGL((bias_act_quant_axis_bwd_k<A, PGV, CGV>), dim3(g.strips, g.chunks), dim3(kBlock), 0, st,         \
                     reinterpret_cast<const f32x4*>(gemm), reinterpret_cast<const f32x4*>(bias),                      \
                     reinterpret_cast<const f32x4*>(grad_y), reinterpret_cast<f32x4*>(grad_gemm), reinterpret_cast<f32x4*>(h), \
                     reinterpret_cast<f32x4*>(y), rows, g.nvec, *q_out, reinterpret_cast<f32x4*>(part))
  if (act == TQ_ACT_GELU) TQ_PG_AG_DISPATCH(pg, cg, TQ_ACTXB_GO, TQ_ACT_GELU);
  else if (act == TQ_ACT_RELU) TQ_PG_AG_DISPATCH(pg, cg, TQ_ACTXB_GO, TQ_ACT_RELU);
  else TQ_PG_AG_DISPATCH(pg, cg, TQ_ACTXB_GO, TQ_ACT_NONE);
#undef TQ_ACTXB_GO
  if (int e = check_launch("bias_act_quant_axis_bwd_k")) return e;
  if (pg || cg) {
    hipLaunchKernelGGL(bias_act_quant_axis_bwd_final_k, dim3((unsigned)ceil_div(cols, 64)), dim3(kBlock), 0, st, part, g.chunks,
                       g.strips, cols, grad_bias, *q_out, grad_q_out);
    return check_launch("bias_act_quant_axis_bwd_final_k");
  }
  return TQ_OK;
}
