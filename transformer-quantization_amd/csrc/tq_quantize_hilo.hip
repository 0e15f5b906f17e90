// Index producer of the 16-bit integer Linear (tq_linear_i16x8_fwd): the grid index of a per-tensor asymmetric quantizer of
// up to 16 bits, written as two int8 byte planes
//     hi = int8((index >> 8) - 128)        lo = int8((index & 255) - 128)
// so that index = 256 (hi + 128) + (lo + 128) and each plane is a signed operand of the i8 matrix cores.  The index itself is
// tq_fake_quant_fwd's, bit for bit: the exact branch-free quotient of tq_device.h where it applies (QF::ok), the IEEE division
// otherwise.  One lane turns 16 consecutive elements (four 16-byte loads of fp32, two of bf16 / fp16) into one 16-byte
// store per plane; 6 (fp32) or 4 bytes of traffic per element.
#include <algorithm>

#include "tq_device.h"
#include "tq_host.h"

namespace tq {

template <int DT, bool FAST>
__device__ __forceinline__ void hilo_vec16(const u32x4* __restrict__ x, int8_t* __restrict__ hi, int8_t* __restrict__ lo, uint64_t g,
                                           const QP& p, const QF& qf) {
  constexpr int V = Store<DT>::kVec, NV = 16 / V;
  u32x4 in[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) in[v] = x[g * NV + v];
  u32x4 oh, ol;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    float f[V], xi[V];
    Store<DT>::unpack(in[v], f);
    if (FAST) {
      constexpr int H = V / 2;
      f32x2 x2[H], h[H];
#pragma unroll
      for (int j = 0; j < H; ++j) x2[j] = f32x2{f[2 * j], f[2 * j + 1]};
      qf_round2_n<H>(x2, qf, h);
      const f32x2 zp2 = {qf.zp, qf.zp};
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const f32x2 t = h[j] + zp2;
        xi[2 * j] = (f[2 * j] != f[2 * j]) ? f[2 * j] : t.x;                   // torch.clamp keeps NaN; v_med3 does not
        xi[2 * j + 1] = (f[2 * j + 1] != f[2 * j + 1]) ? f[2 * j + 1] : t.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) xi[j] = q_index(f[j], p);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int e = v * V + j;                       // element 0..15 of this lane's group: byte e of both stores
      const uint32_t idx = (uint32_t)(int32_t)xi[j];
      const uint32_t bh = ((idx >> 8) & 255u) ^ 128u, bl = (idx & 255u) ^ 128u;      // b - 128 as a byte: top bit flipped
      if (e % 4 == 0) { oh[e / 4] = bh; ol[e / 4] = bl; }
      else { oh[e / 4] |= bh << (8 * (e % 4)); ol[e / 4] |= bl << (8 * (e % 4)); }
    }
  }
  *reinterpret_cast<u32x4*>(hi + g * 16) = oh;
  *reinterpret_cast<u32x4*>(lo + g * 16) = ol;
}

// VEC: x, hi and lo are 16-byte aligned -> groups of 16 elements per lane, then the ragged end (< 16 elements: the first
// lanes of block 0); otherwise every element on its own.
template <int DT, bool VEC>
__global__ __launch_bounds__(kBlock) void quantize_hilo_k(const void* __restrict__ x, int8_t* __restrict__ hi, int8_t* __restrict__ lo,
                                                          uint64_t n, tq_quantizer q) {
  typedef typename Store<DT>::elem_t E;
  const QP p = make_qp(q, 0);
  const QF qf = make_qf(p);
  const uint64_t n_grp = VEC ? n / 16 : 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  if (VEC) {
    const u32x4* xv = static_cast<const u32x4*>(x);
    if (qf.ok) for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < n_grp; g += stride) hilo_vec16<DT, true>(xv, hi, lo, g, p, qf);
    else       for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < n_grp; g += stride) hilo_vec16<DT, false>(xv, hi, lo, g, p, qf);
  }
  for (uint64_t k = n_grp * 16 + (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
    const uint32_t idx = (uint32_t)(int32_t)q_index(Store<DT>::load1(static_cast<const E*>(x) + k), p);
    hi[k] = (int8_t)(int)(((idx >> 8) & 255u) ^ 128u);
    lo[k] = (int8_t)(int)((idx & 255u) ^ 128u);
  }
}

template <int DT>
static int launch_hilo(const void* x, int8_t* hi, int8_t* lo, uint64_t n, const tq_quantizer& q, hipStream_t st) {
  const bool vec = aligned16(x) && aligned16(hi) && aligned16(lo);
  const uint64_t work = vec ? ceil_div(n, 16) : n;
  const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>(ceil_div(work, kBlock), 1), kMaxGrid * 8);
  if (vec) hipLaunchKernelGGL((quantize_hilo_k<DT, true>), dim3(grid), dim3(kBlock), 0, st, x, hi, lo, n, q);
  else     hipLaunchKernelGGL((quantize_hilo_k<DT, false>), dim3(grid), dim3(kBlock), 0, st, x, hi, lo, n, q);
  return check_launch("quantize_hilo_k");
}

}  // namespace tq

using namespace tq;

extern "C" int tq_quantize_hilo_fwd(const void* x, int8_t* hi, int8_t* lo, uint64_t n, int dtype, const tq_quantizer* q,
                                    tq_stream_t stream) {
  const char* who = "tq_quantize_hilo_fwd";
  if (n == 0) return TQ_OK;
  TQ_REQUIRE(x != nullptr && hi != nullptr && lo != nullptr, "%s: NULL pointer", who);
  TQ_REQUIRE(dtype == TQ_F32 || dtype == TQ_BF16 || dtype == TQ_F16, "%s: bad dtype %d", who, dtype);
  if (int e = check_quantizer(q, n, who)) return e;
  TQ_REQUIRE(q->n_params == 1 && !q->symmetric && q->n_bits >= 1 && q->n_bits <= 16 && q->zero_float != nullptr,
             "%s: per-tensor asymmetric quantizer of <= 16 bits only", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case TQ_F32: return launch_hilo<TQ_F32>(x, hi, lo, n, *q, st);
    case TQ_BF16: return launch_hilo<TQ_BF16>(x, hi, lo, n, *q, st);
    default: return launch_hilo<TQ_F16>(x, hi, lo, n, *q, st);
  }
}
