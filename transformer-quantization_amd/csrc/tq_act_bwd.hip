// Bias + activation function + output quantizer behind a Linear's GEMM, and its backward for QAT:
//     y = Q( act( gemm + bias ) )                       act = none | ReLU | GELU (erf form), Q per-tensor or absent
// The layered modules run F.linear's bias add, nn.GELU() and the quantizer as sweeps of their own and keep two [rows, cols]
// tensors for the backward, whose three nodes (fake-quant, GELU, the bias gradient's column sum) are three more sweeps.  Here
// the forward is ONE launch (read gemm, write y: 8 B per element) and the backward ONE launch (read gemm and grad_y, write
// grad_gemm: 12 B per element) plus one small final launch when a sum over rows is asked for.  Only `gemm` is kept from the
// forward: a, h, the clamp mask and the index are RECOMPUTED by the forward's own function (act_q_elem below: ONE text for both
// kernels, hence the same bits).
//
// Per element, every fp32 operation rounded on its own (s, zp, lo, hi the derived parameters of q_out, tq_device.h make_qp):
//     a = g + bias_c          h = act(a)          r = rint(h / s) + zp          in = lo <= r <= hi
//     xi = clamp(r, lo, hi)   y = s * (xi - zp)                                              (q_out NULL: y = h)
//     gh = in ? (gy * s) / s : 0                                                             (q_out NULL: gh = gy)
//     ga = gh * act'(a)       act' = 1 | [a > 0] | Phi(a) + a phi(a)                         -> grad_gemm
//     grad_bias_c = sum over rows of ga
//     d += gy (xi - zp) - in (gy s h) / (s s)      z += in ? 0 : -(gy s)                     (tq_fake_quant_bwd's terms)
// NaN rule (the one of ln_quant_bwd_k): an element whose h is NaN has ga = NaN, so its column of grad_bias and d are NaN; every
// other element and column is what it is without the NaN.  (A NaN has no grid index: `in` is false for it, and without the
// rule ReLU's and the identity's gradient of such an element would be a finite number.)
//
// Activation functions.  ReLU: h = a <= 0 ? +0 : a (a NaN stays).  GELU: the erfc fit of csrc/tq_linear_i8.hip (gelu_erf_n), one
// element at a time: t = |a| / sqrt 2, erfc(t) = 2^(t Q(t)), Q of degree 7 (absolute error of erf 8.5e-8: fit + fp32 evaluation
// with the hardware's 2^x), E = copysign(1 - erfc(t), a), Phi = 0.5 (1 + E), h = (0.5 a)(1 + E); and
// phi(a) = 2^(-(a a) log2(e) / 2) / sqrt(2 pi), act' = Phi + a phi (a phi taken as 0 from |a| = 14 on, where phi underflows: no
// inf * 0).  Against float64, 0.5 a (1 + erf(a / sqrt 2)) and Phi(a) + a phi(a), established on the CPU with this evaluation
// in numpy fp32 (fma through float64) over 4e6 equidistant points of [-12, 12], 2e6 draws of N(0, 1.5^2) and +-1e-3 downwards in
// relative steps of 2^-10, plus one ulp of each hardware 2^x (numpy's is correctly rounded to half of one):
//     |h    - GELU (a)| <= 9.0e-8 |a| + 2^-23 |GELU(a)|      (sweep: 5.1e-8 |a| + ..; 2^x: 2^-24 on erf, times |a| / 2)
//     |act' - GELU'(a)| <= 2.5e-7                             (sweep: 1.56e-7; 2^x: 3e-8 through Phi, 1.5e-8 through a phi)
// The largest absolute error of h in the sweep is 4.7e-7 (a = 4.4: one ulp of h).  Beyond |a| = 12 h is a or a zero and act' 1
// or 0 to within the same bounds.
//
// The quantizer arithmetic is the library's: make_qp, and tq_fake_quant_fwd's body vote (make_qf(p).ok).  Branch-free body: ONE
// Markstein quotient on the grid widened by one step gives mask and index (q_recompute, tq_ste_bwd.h; identity (2) of tq_device.h on
// the wider grid), y = fma(s, xi - zp, +0), and gh is a Markstein quotient (the IEEE result for normal operands).  Division
// body (scales outside [2^-100, 2^100], grids of 2^22 steps and more): q_index / q_dequant and IEEE divisions.  Either way y
// has the bits tq_fake_quant_fwd gives for the kernel's own h.  The range term (gy s h) / (s s) is an IEEE division in both.
//
// Work split (gfx950).  Column sums and whole-tensor sums without atomics:
//  * grid = (column strips) x (row chunks).  A strip is 64 16-byte vectors = 256 columns: one wave reads 1 KiB of a row with one
//    instruction.  A block is 4 waves = 4 ROW GROUPS over the same strip; wave w of chunk c walks rows 4 c + w, + 4 chunks, ..
//    (grid stride), one row per trip, the next row's two loads issued before the current row's arithmetic.
//  * A lane owns ONE vector of columns for its whole life: its bias strip (4 floats) is loaded once and stays in registers, and
//    so do its four column accumulators and the two range accumulators.  Lanes past the last vector of a ragged strip (cols is
//    any multiple of 4) load and store nothing and contribute zeros.
//  * At block end the four row groups meet in LDS once (4 KiB): wave 0 adds the four partial vectors of a column in group
//    order and writes the block's [256] partial; the range sums take one wave butterfly + an LDS hop of their own (block_range_sums).
//  * workspace = [chunks x strips x 256] column partials, then [chunks x strips x 2] range partials.  The final launch adds a
//    column's `chunks` partials in float64 in a fixed order (64 columns x 4 slices per block: slice s takes chunks s, s + 4, ..;
//    then 0 + 1 + 2 + 3), and one more block finishes the two range sums in float64 and applies the chain through
//    clamp(delta, eps) | exp(delta) and the zero-point clamp (final_range_sums, range_chain: tq_ste_bwd.h).  Two runs give identical bits.
//  * Grid cap: kActMaxBlocks = 2048 blocks (256 CUs x 8 resident blocks): chunks = min(ceil(rows / 4), max(1, 2048 / strips)), so
//    the workspace is bounded by 2048 x 258 floats for cols <= 2048 x 256.  FFN1 of BERT-base ([M, 3072]: 12 strips) runs 170 chunks.
//  * ACT, PG (range gradients) and CG (the column sum) are template parameters: without them none of their code or registers is
//    compiled in; both quantizer bodies are, chosen by the wave-uniform vote.  No scratch in any instantiation.
// The recomputed quantizer of the branch-free body, the block-end and final sums and the chain are the shared pieces of
// csrc/tq_ste_bwd.h; the division body of act_q_elem (tq_fake_quant_fwd's text) and the STE terms in act_bwd_rows are this file's own.
// act_eval, the strip grid and the shared argument checks live in csrc/tq_act.h (the per-column pair, tq_act_axis_bwd.hip, uses them too).
#include "tq_act.h"
#include "tq_device.h"
#include "tq_host.h"
#include "tq_rows.h"
#include "tq_ste_bwd.h"

namespace tq {

struct ActQ {
  SmQW f;        // branch-free body
  QP p;          // division body
  int on, fast;
};

__device__ __forceinline__ ActQ make_actq(const tq_quantizer& q, int on) {
  ActQ c;
  c.p = QP{1.f, 0.f, 0.f, 0.f};
  c.on = on;
  if (on) c.p = make_qp(q, 0);
  c.f = make_qw(c.p);
  c.fast = on && make_qf(c.p).ok;                // tq_fake_quant_fwd's vote (fq_tensor)
  return c;
}

// The forward of one element from a = g + bias: h (returned through hh), y, and for the backward the clamp mask and xi - zp.
template <int ACT, bool DERIV, bool FAST>
__device__ __forceinline__ float act_q_elem(float a, const ActQ& c, float& hh, float& dact, bool& in, float& hc) {
  const float h = act_eval<ACT, DERIV>(a, dact);
  hh = h;
  in = true;
  hc = 0.0f;
  if (!c.on) return h;
  if constexpr (FAST) {
    return q_recompute<true, true>(h, c.f.s, c.f.rc, 0.0f, c.f.klo, c.f.khi, 1, in, hc);
  } else {                                         // tq_fake_quant_fwd's division body: q_index / q_dequant, an IEEE division
    const float r = rintf(h / c.p.scale) + c.p.zp;
    in = r >= c.p.lo && r <= c.p.hi;
    const float xi = clamp_nanprop(r, c.p.lo, c.p.hi);
    hc = xi - c.p.zp;
    return q_dequant(xi, c.p);
  }
}

// ------------------------------------------------------------------------------ forward
template <int ACT, bool FAST>
__device__ __forceinline__ void act_fwd_rows(const f32x4* __restrict__ gv, f32x4* __restrict__ yv, const f32x4& b, uint64_t rows,
                                             uint64_t nvec, uint64_t cv, const ActQ& c) {
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
      o[e] = act_q_elem<ACT, false, FAST>(xg[e] + b[e], c, hh, dact, in, hc);
    }
    yv[row * nvec + cv] = o;
    if (nxt >= rows) break;
    row = nxt;
    xg = ng;
  }
}

template <int ACT>
__global__ __launch_bounds__(kBlock) void bias_act_quant_fwd_k(const f32x4* __restrict__ gv, const f32x4* __restrict__ bias,
                                                               f32x4* __restrict__ yv, uint64_t rows, uint64_t nvec,
                                                               tq_quantizer q, int on) {
  const uint64_t cv = (uint64_t)blockIdx.x * kActStripVec + (threadIdx.x & (kActStripVec - 1));
  const ActQ c = make_actq(q, on);
  if (cv >= nvec) return;                          // ragged strip: no barrier follows
  const f32x4 b = bias != nullptr ? bias[cv] : f32x4{0.f, 0.f, 0.f, 0.f};
  if (c.fast) act_fwd_rows<ACT, true>(gv, yv, b, rows, nvec, cv, c);
  else act_fwd_rows<ACT, false>(gv, yv, b, rows, nvec, cv, c);
}

// ------------------------------------------------------------------------------ backward
struct ActAcc {
  float col[4];
  float d, z;
};

template <int ACT, bool PG, bool CG, bool FAST>
__device__ __forceinline__ void act_bwd_rows(const f32x4* __restrict__ gv, const f32x4* __restrict__ gyv,
                                             f32x4* __restrict__ gav, f32x4* __restrict__ hv, f32x4* __restrict__ yv,
                                             const f32x4& b, uint64_t rows, uint64_t nvec, uint64_t cv, const ActQ& c,
                                             ActAcc& acc) {
  const uint64_t stride = (uint64_t)gridDim.y * kActGroups;
  uint64_t row = (uint64_t)blockIdx.y * kActGroups + threadIdx.x / kActStripVec;
  if (row >= rows) return;
  const float s = FAST ? c.f.s : c.p.scale;
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
      const float gy = xy[e];
      oy[e] = act_q_elem<ACT, true, FAST>(xg[e] + b[e], c, h, dact, in, hc);
      oh[e] = h;
      // (ste_backward's arithmetic, tq_ste_bwd.h, with the mask applied BEFORE the range terms: with the select behind them, as
      // the tails have it, every instantiation with range gradients needs 4 more registers and three lose an occupancy step)
      float gh = gy;
      if (c.on) {
        const float gs = gy * s;
        gh = FAST ? div_rn(gs, c.f.ns, c.f.rc) : gs / s;
        gh = in ? gh : 0.0f;
        if (PG) {
          float dd = gy * hc;
          if (in) dd -= (gs * h) / (s * s);
          acc.d += dd;
          acc.z += in ? 0.0f : -gs;
        }
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
__global__ __launch_bounds__(kBlock) void bias_act_quant_bwd_k(const f32x4* __restrict__ gv, const f32x4* __restrict__ bias,
                                                               const f32x4* __restrict__ gyv, f32x4* __restrict__ gav,
                                                               f32x4* __restrict__ hv, f32x4* __restrict__ yv, uint64_t rows,
                                                               uint64_t nvec, tq_quantizer q, int on,
                                                               f32x4* __restrict__ colpart, float* __restrict__ rngpart) {
  const int lane = threadIdx.x & (kActStripVec - 1), grp = threadIdx.x / kActStripVec;
  const uint64_t cv = (uint64_t)blockIdx.x * kActStripVec + lane;
  const ActQ c = make_actq(q, on);
  ActAcc acc = {{0.f, 0.f, 0.f, 0.f}, 0.f, 0.f};
  if (cv < nvec) {                                 // lanes past a ragged strip's end keep zeros and meet the others below
    const f32x4 b = bias != nullptr ? bias[cv] : f32x4{0.f, 0.f, 0.f, 0.f};
    if (c.fast) act_bwd_rows<ACT, PG, CG, true>(gv, gyv, gav, hv, yv, b, rows, nvec, cv, c, acc);
    else act_bwd_rows<ACT, PG, CG, false>(gv, gyv, gav, hv, yv, b, rows, nvec, cv, c, acc);
  }
  const uint64_t blk = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if constexpr (PG) {
    const float sums[2] = {acc.d, acc.z};
    block_range_sums(sums, rngpart + 2 * blk);
  }
  __shared__ f32x4 s_col[CG ? kBlock : 1];
  if (CG) {
    s_col[threadIdx.x] = f32x4{acc.col[0], acc.col[1], acc.col[2], acc.col[3]};
    __syncthreads();
  }
  if (CG && grp == 0) {
    f32x4 t = s_col[lane];
#pragma unroll
    for (int g = 1; g < kActGroups; ++g) t = t + s_col[g * kActStripVec + lane];
    colpart[blk * kActStripVec + lane] = t;
  }
}

// Blocks 0 .. ncb - 1: 64 columns each, 4 slices of the `chunks` block partials per column, float64.  Block ncb (only with range
// gradients): the two range sums over all chunks x strips partials in float64, then the chain (tq_ste_bwd.h).
__global__ __launch_bounds__(kBlock) void bias_act_quant_bwd_final_k(const float* __restrict__ colpart,
                                                                     const float* __restrict__ rngpart, uint32_t chunks,
                                                                     uint32_t strips, uint64_t cols, uint32_t ncb,
                                                                     float* __restrict__ grad_bias, tq_quantizer q,
                                                                     float* __restrict__ grad_q) {
  if (blockIdx.x < ncb) {
    const uint64_t col = (uint64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const uint64_t strip = col / (kActStripVec * 4), within = col % (kActStripVec * 4);
    const double t = col_sum_f64<64, 4>(colpart + (col < cols ? strip * (kActStripVec * 4) + within : 0), col < cols ? chunks : 0,
                                        (uint64_t)strips * (kActStripVec * 4));
    if (threadIdx.x < 64 && col < cols) grad_bias[col] = (float)t;
    return;
  }
  double dsum, zsum;
  final_range_sums(rngpart, (uint64_t)chunks * strips, 2, 0, dsum, zsum);
  if (threadIdx.x == 0) {
    const RangeGrad g = range_chain(q, 0, dsum, zsum);
    grad_q[0] = g.delta;
    grad_q[1] = g.zero_float;
  }
}

}  // namespace tq

using namespace tq;

namespace {

// act_check (tq_act.h) and this pair's rule for the quantizer
int act_check_tensor(const char* who, const float* gemm, const float* bias, uint64_t rows, uint64_t cols, int act, const tq_quantizer* q) {
  if (int e = act_check(who, gemm, bias, rows, cols, act, q)) return e;
  TQ_REQUIRE(q == nullptr || q->n_params == 1, "%s: per-tensor quantizers only", who);
  return TQ_OK;
}

}  // namespace

extern "C" int tq_bias_act_quant_fwd(const float* gemm, const float* bias, float* y, uint64_t rows, uint64_t cols, int act,
                                     const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_bias_act_quant_fwd";
  if (rows == 0) return TQ_OK;
  if (int e = act_check_tensor(who, gemm, bias, rows, cols, act, q_out)) return e;
  TQ_REQUIRE(y != nullptr && aligned16(y), "%s: y must be a 16-byte aligned pointer", who);
  const ActGrid g = act_grid(rows, cols);
  const tq_quantizer none{};
  const tq_quantizer& c = q_out ? *q_out : none;
  hipStream_t st = static_cast<hipStream_t>(stream);
#define TQ_ACTF(A)                                                                                                    \
  hipLaunchKernelGGL((bias_act_quant_fwd_k<A>), dim3(g.strips, g.chunks), dim3(kBlock), 0, st,                        \
                     reinterpret_cast<const f32x4*>(gemm), reinterpret_cast<const f32x4*>(bias), reinterpret_cast<f32x4*>(y), \
                     rows, g.nvec, c, q_out != nullptr)
  if (act == TQ_ACT_GELU) TQ_ACTF(TQ_ACT_GELU);
  else if (act == TQ_ACT_RELU) TQ_ACTF(TQ_ACT_RELU);
  else TQ_ACTF(TQ_ACT_NONE);
#undef TQ_ACTF
  return check_launch("bias_act_quant_fwd_k");
}

extern "C" size_t tq_bias_act_quant_bwd_workspace_bytes(uint64_t rows, uint64_t cols) {
  if (rows == 0 || cols == 0 || cols % 4 != 0) return 0;
  const ActGrid g = act_grid(rows, cols);
  return (size_t)g.chunks * g.strips * (kActStripVec * 4 + 2) * sizeof(float);
}

extern "C" int tq_bias_act_quant_bwd(const float* gemm, const float* bias, const float* grad_y, uint64_t rows, uint64_t cols,
                                     int act, const tq_quantizer* q_out, float* grad_gemm, float* grad_bias, float* grad_q_out,
                                     float* h, float* y, void* workspace, size_t workspace_bytes, tq_stream_t stream) {
  const char* who = "tq_bias_act_quant_bwd";
  if (rows == 0) return TQ_OK;
  if (int e = act_check_tensor(who, gemm, bias, rows, cols, act, q_out)) return e;
  TQ_REQUIRE(grad_y != nullptr && grad_gemm != nullptr, "%s: NULL pointer", who);
  TQ_REQUIRE(aligned16(grad_y) && aligned16(grad_gemm) && aligned16(h) && aligned16(y), "%s: 16-byte alignment required", who);
  TQ_REQUIRE(grad_q_out == nullptr || q_out != nullptr, "%s: range gradients asked for an absent quantizer", who);
  TQ_REQUIRE(grad_bias == nullptr || bias != nullptr, "%s: grad_bias asked for an absent bias", who);
  TQ_REQUIRE(((reinterpret_cast<uintptr_t>(grad_bias) | reinterpret_cast<uintptr_t>(grad_q_out)) & 3u) == 0,
             "%s: gradients must be 4-byte aligned", who);
  const ActGrid g = act_grid(rows, cols);
  const bool pg = grad_q_out != nullptr, cg = grad_bias != nullptr;
  const size_t ncol = (size_t)g.chunks * g.strips * kActStripVec * 4;
  const size_t need = ncol * sizeof(float) + (size_t)g.chunks * g.strips * 2 * sizeof(float);
  if (int e = bwd_workspace_check(who, pg || cg, workspace, workspace_bytes, need)) return e;
  const tq_quantizer none{};
  const tq_quantizer& c = q_out ? *q_out : none;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* colpart = (pg || cg) ? static_cast<float*>(workspace) : nullptr;
  float* rngpart = colpart ? colpart + ncol : nullptr;
#define TQ_ACTB_GO(PGV, CGV, A)                                                                                       \
  hipLaunchKernelGGL((bias_act_quant_bwd_k<A, PGV, CGV>), dim3(g.strips, g.chunks), dim3(kBlock), 0, st,              \
                     reinterpret_cast<const f32x4*>(gemm), reinterpret_cast<const f32x4*>(bias),                      \
                     reinterpret_cast<const f32x4*>(grad_y), reinterpret_cast<f32x4*>(grad_gemm), reinterpret_cast<f32x4*>(h), \
                     reinterpret_cast<f32x4*>(y), rows, g.nvec, c, q_out != nullptr, reinterpret_cast<f32x4*>(colpart), rngpart)
  if (act == TQ_ACT_GELU) TQ_PG_AG_DISPATCH(pg, cg, TQ_ACTB_GO, TQ_ACT_GELU);
  else if (act == TQ_ACT_RELU) TQ_PG_AG_DISPATCH(pg, cg, TQ_ACTB_GO, TQ_ACT_RELU);
  else TQ_PG_AG_DISPATCH(pg, cg, TQ_ACTB_GO, TQ_ACT_NONE);
#undef TQ_ACTB_GO
  if (int e = check_launch("bias_act_quant_bwd_k")) return e;
  if (pg || cg) {
    const unsigned ncb = cg ? (unsigned)ceil_div(cols, 64) : 0;
    hipLaunchKernelGGL(bias_act_quant_bwd_final_k, dim3(ncb + (pg ? 1 : 0)), dim3(kBlock), 0, st, colpart, rngpart, g.chunks,
                       g.strips, cols, ncb, grad_bias, c, grad_q_out);
    return check_launch("bias_act_quant_bwd_final_k");
  }
  return TQ_OK;
}
