// Pieces shared by the one-launch STE backwards for QAT (csrc/tq_softmax_bwd.hip, tq_ln_bwd.hip, tq_ln_axis_bwd.hip,
// tq_act_bwd.hip, tq_nonorm_bwd.hip) and by the final kernels of tq_fake_quant.hip.  The rule of these kernels is "the
// backward's masks and indices ARE the forward's": one text for the recomputed quantizer, its STE backward, the block-end
// sums and the float64 final sums with the chain, so that a fix lands in every backward at once.  Kept out of tq_rows.h and
// tq_device.h: the forward tails and the fake-quant kernels do not read this file (tests/test_abi.py on what a shared-header
// change once did to a kernel that had no use for it).
//
// Deliberately NOT here (arithmetic, not accident): the softmax chain's Markstein quotient for the range term, act's
// rintf(h / s) division body, ste_bwd_elem / bwd_block_reduce of the fake-quant headline kernels, the float64 chain of
// tq_double.hip.  tq_act_bwd.hip also keeps its own text of the STE terms (same arithmetic; see there).  DESIGN.md,
// "Training backwards, shared pieces".
#pragma once

#include "tq_device.h"
#include "tq_rows.h"

namespace tq {

// ---- one quantizer recomputed at one element: returns Q(v); in = the clamp mask, hc = clamped index minus zero point.
// The forward's own quotient, clamp and dequantise text on scalars: scale s, its guarded reciprocal rc, zero point zp, grid
// ends lo, hi.  FAST (branch-free body): ONE Markstein quotient on the grid widened by one step gives mask and index
// (identity (2) of tq_device.h on the wider grid), dequantised with the "+ 0" fma (qf_dequant2).  NANPROP: a NaN v comes back
// as NaN (qw_index); without it a NaN v gives a grid end, as the v_med3 front of the LayerNorm tails does (they flag the row
// through lane_nan instead).  Division body: rne_quot1 with the stored reciprocal, q_dequant; a NaN stays a NaN either way.
// An absent quantizer (!on) passes v through with in = true.
template <bool FAST, bool NANPROP>
__device__ __forceinline__ float q_recompute(float v, float s, float rc, float zp, float lo, float hi, int on, bool& in, float& hc) {
  in = true; hc = 0.f;
  if (!on) return v;
  if constexpr (FAST) {
    const float klo = lo - zp, khi = hi - zp;
    float h = rintf(div_rn(__builtin_amdgcn_fmed3f(v, s * (klo - 1.0f), s * (khi + 1.0f)), -s, rc));
    if (NANPROP) h = v != v ? v : h;
    in = h >= klo && h <= khi;
    hc = clamp_nanprop(h, klo, khi);
    return __builtin_fmaf(s, hc, 0.0f);
  } else {
    const float q = rne_quot1(v, s, rc) + zp;
    in = q >= lo && q <= hi;
    hc = clamp_nanprop(q, lo, hi) - zp;
    return s * hc;
  }
}
// The same for a per-tensor quantizer held as SmQW (branch-free body: grid ends relative to the zero point) and FusedQ
// (division body).
template <bool FAST, bool NANPROP>
__device__ __forceinline__ float q_recompute(float v, const SmQW& f, const FusedQ& g, int on, bool& in, float& hc) {
  if constexpr (FAST) return q_recompute<true, NANPROP>(v, f.s, f.rc, 0.0f, f.klo, f.khi, on, in, hc);
  else return q_recompute<false, NANPROP>(v, g.p.scale, g.rcp, g.p.zp, g.p.lo, g.p.hi, on, in, hc);
}

// ---- one quantizer's STE backward at one element (tq_fake_quant_bwd's terms): returns in ? (gr * s) / s : 0 and, with PG,
// adds the element's range-gradient terms d += gr hc - in (gr s v) / (s s), z += in ? 0 : -(gr s); an element of a padded
// row (!valid) adds zeros.  FAST: the data-gradient division is a Markstein quotient; the range term stays an IEEE division
// (the body vote admits scales down to 2^-100, whose square has no reciprocal).  An absent quantizer passes gr through.
template <bool PG, bool FAST>
__device__ __forceinline__ float ste_backward(float gr, float v, float hc, bool in, bool valid, float s, float rc, int on,
                                              float& accd, float& accz) {
  if (!on) return gr;
  const float gs = gr * s;
  const float gx = FAST ? div_rn(gs, -s, rc) : gs / s;
  if (PG) {
    float dd = gr * hc;
    if (in) dd -= (gs * v) / (s * s);
    accd += valid ? dd : 0.0f;
    accz += (valid && !in) ? -gs : 0.0f;
  }
  return in ? gx : 0.0f;
}
template <bool PG, bool FAST>
__device__ __forceinline__ float ste_backward(float gr, float v, float hc, bool in, bool valid, const SmQW& f, const FusedQ& g,
                                              int on, float& accd, float& accz) {
  return ste_backward<PG, FAST>(gr, v, hc, in, valid, FAST ? f.s : g.p.scale, f.rc, on, accd, accz);
}

// ---- a block's N range sums -> dst[0 .. N - 1]: one wave butterfly each, one LDS hop, the waves added in index order.
// Every thread of the block arrives.
template <int N>
__device__ __forceinline__ void block_range_sums(const float (&v)[N], float* __restrict__ dst) {
  __shared__ float s_red[N][kBlock / kWave];
  float t[N];
#pragma unroll
  for (int k = 0; k < N; ++k) t[k] = wave_sum(v[k]);
  if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) s_red[k][threadIdx.x / kWave] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    float a = 0.f;
    for (int k = 0; k < kBlock / kWave; ++k) a += s_red[threadIdx.x][k];
    dst[threadIdx.x] = a;
  }
}

// ---- the float64 sum of n block partials (d at part[i * stride + off], z behind it) in a fixed order (thread over i, wave
// butterfly, waves in index order) -> thread 0's dsum, zsum.  One block of kBlock threads, all of them arrive; may be called
// again (the leading barrier: the previous call's reads are done).
__device__ __forceinline__ void final_range_sums(const float* __restrict__ part, uint64_t n, uint32_t stride, uint32_t off,
                                                 double& dsum, double& zsum) {
  __shared__ double s_red[2][kBlock / kWave];
  double d = 0.0, z = 0.0;
  for (uint64_t i = threadIdx.x; i < n; i += kBlock) {
    d += (double)part[i * stride + off];
    z += (double)part[i * stride + off + 1];
  }
  d = wave_sum(d);
  z = wave_sum(z);
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) { s_red[0][threadIdx.x / kWave] = d; s_red[1][threadIdx.x / kWave] = z; }
  __syncthreads();
  dsum = zsum = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kBlock / kWave; ++k) { dsum += s_red[0][k]; zsum += s_red[1][k]; }
}

// ---- the chain from the sums over elements to the gradients of parameter p's `_delta` and `_zero_float`, through
// scale = clamp(delta, eps) | exp(delta) and zp = clamp(round_ste(zero_float), lo, hi); a symmetric quantizer has no zero
// point: 0.  (The halves by themselves: the per-column final kernel holds one sum per block.)
__device__ __forceinline__ float chain_delta(const tq_quantizer& q, uint64_t p, double dsum) {
  const float delta = q.delta[p];
  return (float)dsum * (q.log_domain ? expf(delta) : (delta >= q.eps ? 1.0f : 0.0f));
}
__device__ __forceinline__ float chain_zero_float(const tq_quantizer& q, uint64_t p, double zsum) {
  if (q.symmetric) return 0.0f;
  const QP qp = make_qp(q, p);
  const float zf = rintf(q.zero_float[p]);
  return (zf >= qp.lo && zf <= qp.hi) ? (float)zsum : 0.0f;
}
struct RangeGrad { float delta, zero_float; };
__device__ __forceinline__ RangeGrad range_chain(const tq_quantizer& q, uint64_t p, double dsum, double zsum) {
  return RangeGrad{chain_delta(q, p, dsum), chain_zero_float(q, p, zsum)};
}

// ---- the float64 sum of a column's n block partials src[i * stride]: COLS columns x SLICES slices per block
// (thread = slice * COLS + column); slice s adds partials s, s + SLICES, ..; then slice 0 + 1 + .. in order.  Every thread
// arrives (a column past the end passes n = 0); the sum is returned to the column's thread of slice 0.
template <int COLS, int SLICES>
__device__ __forceinline__ double col_sum_f64(const float* __restrict__ src, uint32_t n, uint64_t stride) {
  static_assert(COLS * SLICES == kBlock, "one thread per (column, slice)");
  __shared__ double s_red[SLICES][COLS];
  const uint32_t cl = threadIdx.x % COLS, slice = threadIdx.x / COLS;
  double t = 0.0;
  for (uint32_t i = slice; i < n; i += SLICES) t += (double)src[(uint64_t)i * stride];
  s_red[slice][cl] = t;
  __syncthreads();
  if (slice == 0)
    for (int k = 1; k < SLICES; ++k) t += s_red[k][cl];
  return t;
}

}  // namespace tq
