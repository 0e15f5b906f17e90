// (f2) Fused residual-add -> quantize -> LayerNorm -> quantize for gfx950.
//
// The tail of BertSelfOutput / BertOutput in the reference (models/quantized_bert.py:238-248,
// 264-280 with quantization/hijacker.py:98-116 and autoquant_utils.py:55-66) is five separate
// tensor sweeps after the GEMM:
//     t = Q1(dense_out)        activation quantizer of the QuantLinear
//     s = t + residual
//     u = Q2(s)                res_act_quantizer
//     v = layer_norm(u; Q(w), Q(b), eps)
//     y = Q3(v)                activation quantizer of the QuantLayerNorm
// = 5 reads + 4 writes of [B*T, d] plus ~20 launches.  With fixed ranges the chain only needs the
// row it is working on, so it collapses to 2 reads + 1 write (6 B/elem bf16, 12 B/elem fp32):
// LPR lanes (16/32/64) own one row, keep it in registers (d/LPR values per lane), do the two
// row reductions (mean, centred variance) with __shfl_xor inside the lane group, and stream out.
// Any of the three quantizers may be absent (NULL).
#include <algorithm>
#include <initializer_list>

#include "tq_device.h"
#include "tq_host.h"

namespace tq {

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
__device__ __forceinline__ FusedQ make_fq(const tq_quantizer& q, int on) { return make_fq(on ? make_qp(q, 0) : QP{1.f, 0.f, 0.f, 0.f}, on); }

// x_int of v under q (bit-identical to q_index: rne_quot1 falls back to the division near ties)
__device__ __forceinline__ float index_q(float v, const FusedQ& q) {
  return clamp_nanprop(rne_quot1(v, q.p.scale, q.rcp) + q.p.zp, q.p.lo, q.p.hi);
}

__device__ __forceinline__ float apply_q(float v, const FusedQ& q) {
  return q.on ? q_dequant(index_q(v, q), q.p) : v;
}

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

// ---- row pieces that every tail body spells the same way, as macros: a function with the row as array-reference
// parameters compiles to other register allocations (profiles/r18/kernel_resources_diff.txt), the expanded text does not.
// They use the names of the body or kernel they expand in and declare names into it; a body that renames one fails to
// compile at the macro's use.
//   TQ_GROUP_MASK       uses LPR
//   TQ_ROW_STATISTICS   uses LPR, NV, H, FAST, u, s2, s2b, lane_nan, inv_d, ln_eps; declares mean, rstd, row_nan, ssa, ssb, ss2
//   TQ_ROW_STORE        uses LPR, NV, V, y, base, lane, nt, packed, row_nan; declares (in the rare branch) pn, nanv
//   TQ_TAIL_FRONT       uses H, FAST, ALLON, v, fa, f1, f2, g1, g2, u, lane_nan; declares (in its own block) t
//   TQ_PLANE_STORE      uses LPR, v, base, lane, y_hi, y_lo; declares wh, wl
//   TQ_AFFINE_REQUEST   uses NA, d, ln_w, ln_b; declares aw, ab        TQ_AFFINE_STAGE   uses NA, d, aw, ab, s_w, s_b
//   TQ_TAIL_QUANTIZERS  uses q1..q3, w1..w3, on1..on3; declares none, tq      TQ_TAIL_VOTE   uses tq, on1..on3; declares fast

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

// packed[] goes out (streaming for tensors that cannot stay in L2 / MALL anyway); where PATCH holds (the exact path behind
// Q_out, whose outputs are grid values) a row with a NaN input is overwritten AFTER the stores, in a branch that is
// practically never taken: patching the elements before they are packed became one select per element of every row.
// NAN_ROW declares `pn`, the row of NaNs: TQ_NAN_ROW_OF(DT) for any storage type, TQ_NAN_ROW_F32 as a constant.
#define TQ_NAN_ROW_OF(DT)                                                                                       \
  float nanv[V];                                                                                                \
  _Pragma("unroll") for (int e = 0; e < V; ++e) nanv[e] = __builtin_nanf("");                                   \
  const u32x4 pn = Store<DT>::pack(nanv);
#define TQ_NAN_ROW_F32 const u32x4 pn = {0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0x7fc00000u};
#define TQ_ROW_STORE(PATCH, NAN_ROW)                                                                               \
  if (nt) {                                                                                                     \
    _Pragma("unroll") for (int v = 0; v < NV; ++v) st_stream(y + base + v * LPR + lane, packed[v]);             \
  } else {                                                                                                      \
    _Pragma("unroll") for (int v = 0; v < NV; ++v) y[base + v * LPR + lane] = packed[v];                        \
  }                                                                                                             \
  if ((PATCH) && __ballot(row_nan)) {                                                                           \
    if (row_nan) {                                                                                              \
      NAN_ROW                                                                                                   \
      _Pragma("unroll") for (int v = 0; v < NV; ++v) y[base + v * LPR + lane] = pn;                             \
    }                                                                                                           \
  }

// One 16-byte vector (fa, residual FR) through the front of the chain into u[v]: Q2(Q1(a) + r) on the exact path (FAST: the H
// pairs move through the stages side by side, qf_*_n) or the division path.  ALLON: Q3 follows, so a -0 out of Q1 / Q2 cannot
// reach y (Q1(a) + r, the statistics and the affine map treat -0 like +0 unless every term is a zero, and Q3 normalises a
// surviving zero): skip their "+ 0".  v_med3 does not keep a NaN, so the exact path records an unordered input pair: for
// LayerNorm in lane_nan (any NaN turns the WHOLE row NaN -> one compare per element, masks OR-ed), for NoNorm (AFF) as an
// element-local NaN output.
#define TQ_TAIL_FRONT(FR, AFF)                                                                                  \
  if (FAST) {                                                                                                   \
    f32x2 t[H];                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < H; ++j) t[j] = f32x2{fa[2 * j], fa[2 * j + 1]};                       \
    if (ALLON) qf_fake_quant2_n_signed_zero<H>(t, f1.f);                                                        \
    else if (f1.on) qf_fake_quant2_n<H>(t, f1.f);                                                               \
    _Pragma("unroll") for (int j = 0; j < H; ++j) t[j] = t[j] + f32x2{FR[2 * j], FR[2 * j + 1]};                \
    if (ALLON) qf_fake_quant2_n_signed_zero<H>(t, f2.f);                                                        \
    else if (f2.on) qf_fake_quant2_n<H>(t, f2.f);                                                               \
    if (AFF) {                                                                                                  \
      _Pragma("unroll") for (int j = 0; j < H; ++j) {                                                           \
        t[j].x = __builtin_isunordered(fa[2 * j], FR[2 * j]) ? __builtin_nanf("") : t[j].x;                     \
        t[j].y = __builtin_isunordered(fa[2 * j + 1], FR[2 * j + 1]) ? __builtin_nanf("") : t[j].y;             \
      }                                                                                                         \
    } else {                                                                                                    \
      _Pragma("unroll") for (int j = 0; j < H; ++j)                                                             \
        lane_nan = lane_nan || __builtin_isunordered(fa[2 * j], FR[2 * j]) ||                                   \
                   __builtin_isunordered(fa[2 * j + 1], FR[2 * j + 1]);                                         \
    }                                                                                                           \
    _Pragma("unroll") for (int j = 0; j < H; ++j) u[v][j] = t[j];                                               \
  } else {                                                                                                      \
    _Pragma("unroll") for (int j = 0; j < H; ++j)                                                               \
      u[v][j] = f32x2{apply_q(apply_q(fa[2 * j], g1) + FR[2 * j], g2),                                          \
                      apply_q(apply_q(fa[2 * j + 1], g1) + FR[2 * j + 1], g2)};                                 \
  }

// The two byte planes of the N grid indices INDEX[] (< 2^16) of column vector v go out as one 4-byte word each: byte k is
// element k's plane byte b, stored as b - 128 (top bit flipped), like the bytes of y_idx.
#define TQ_PLANE_STORE(INDEX, N)                                                                                \
  uint32_t wh = 0, wl = 0;                                                                                      \
  _Pragma("unroll") for (int k = 0; k < (N); ++k) {                                                             \
    wh |= ((INDEX[k] >> 8) & 255u) << (8 * k);                                                                  \
    wl |= (INDEX[k] & 255u) << (8 * k);                                                                         \
  }                                                                                                             \
  y_hi[base + v * LPR + lane] = wh ^ 0x80808080u;                                                               \
  y_lo[base + v * LPR + lane] = wl ^ 0x80808080u;

// The prologue of the per-tensor tail kernels, in steps around each kernel's own quantizer fetch (QRaw w.. = load_qraw;
// qraw_arrived).  At a model's inference shapes ([1024, 768]: 4 rows per block) such a kernel IS its prologue, so everything
// it reads is requested before anything is waited for: the first row of every lane group (the kernel, first), the affine
// parameters (TQ_AFFINE_REQUEST; staged in LDS by TQ_AFFINE_STAGE once the quantizers have arrived, read as 8-byte pairs
// where they are used: keeping this lane's 2 x d / LPR values in registers cost 48 VGPRs on bf16 rows and with them half
// the occupancy), and the raw buffers of the quantizers -- one memory round trip where the chain rows <- affine staging <-
// code-path choice <- quantizer by quantizer took ~13 (7.6 -> 4.x us per launch).  TQ_TAIL_QUANTIZERS derives the three
// quantizers, TQ_TAIL_VOTE the wave-uniform vote: every enabled quantizer admits the branch-free exact path (tq_device.h, QF).
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

struct FusedF {
  QF f;
  int on;
};
__device__ __forceinline__ FusedF make_ff(const QP& p, int on) {
  FusedF r;
  r.on = on;
  r.f = make_qf(on ? p : QP{1.f, 0.f, 0.f, 1.f});
  return r;
}
__device__ __forceinline__ f32x2 apply_f2(f32x2 v, const FusedF& q) { return q.on ? qf_fake_quant2(v, q.f) : v; }

// NV = 16-byte vectors per lane per row (d == LPR * NV * V).  All element math runs on register pairs with the exact
// branch-free quantizer of tq_device.h (QF): three quantizers per element made the scalar version VALU- / latency-bound
// on bf16 rows (3.1-3.3 TB/s).  NaN: an unordered input pair poisons its element before the statistics (so a LayerNorm
// row turns NaN as a whole, like the reference) and a NaN pre-quantizer value is passed through at the end.  FAST = false
// is the division path (scales outside [2^-100, 2^100], grids of 2^22+ steps); IDX also emits int8(index - 128).
// BERT's embedding block through the same body (EMB): the "dense output" row is word[word_ids[row]] + type[type_ids[row]]
// (one fp32 addition, like the reference's `inputs_embeds + token_type_embeddings`, models/quantized_bert.py:95-111), the
// "residual" row is pos[pos_ids[row]].  An id outside its table (torch's CPU F.embedding raises IndexError there; a GPU
// look-up would read out of bounds) reads the clamped row for memory safety, turns the WHOLE output row NaN (a corrupt
// batch or a vocabulary mismatch must not produce plausible activations) and raises `*bad` (optional; host-visible
// memory: the Python side turns it into the IndexError of the layered CPU route, quantization/_hip.py).
struct EmbArgs {
  const int64_t *a_rows, *a2_rows, *r_rows;
  const u32x4* a2;
  uint64_t a_n, a2_n, r_n;        // rows of the three tables
  int32_t* bad;                   // set to 1 by any row with an out-of-range id (nullptr: not reported)
};

// One row's 16-byte vectors of this lane (dense output, residual, and the token-type row in EMB mode) -> registers.
// Streaming hints only for tensors that cannot stay in L2 / MALL anyway: in a model forward the inputs were just written by
// the GEMM and the output is read by the next layer.  ONE uniform branch per group of loads.
template <int DT, int LPR, int NV, bool EMB>
__device__ __forceinline__ void ln_load_row(const u32x4* __restrict__ a, const u32x4* __restrict__ r, const EmbArgs& emb, int nt,
                                            int lane, uint64_t row, u32x4 (&pa)[NV], u32x4 (&pr)[NV], u32x4 (&pa2)[EMB ? NV : 1]) {
  constexpr int V = Store<DT>::kVec;
  constexpr uint32_t d = LPR * NV * V;
  if (EMB) {
    bool bad = false;
    auto pick = [&bad](const int64_t* ids, uint64_t row_, uint64_t n) {
      const int64_t id = ids[row_];
      const bool out = id < 0 || (uint64_t)id >= n;
      bad = bad || out;
      return out ? (uint64_t)0 : (uint64_t)id;
    };
    const uint64_t oa = pick(emb.a_rows, row, emb.a_n) * (d / V) + lane;
    const uint64_t o2 = pick(emb.a2_rows, row, emb.a2_n) * (d / V) + lane;
    const uint64_t orr = pick(emb.r_rows, row, emb.r_n) * (d / V) + lane;
#pragma unroll
    for (int v = 0; v < NV; ++v) { pa[v] = a[oa + v * LPR]; pa2[v] = emb.a2[o2 + v * LPR]; pr[v] = r[orr + v * LPR]; }
    if (bad) {                       // row-uniform and rare: poison the word row (NaN rule of the body: the row turns NaN)
      const u32x4 nan4 = {0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0x7fc00000u};
#pragma unroll
      for (int v = 0; v < NV; ++v) pa[v] = nan4;
      if (lane == 0 && emb.bad) __hip_atomic_store(emb.bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }
  const uint64_t o = row * (d / V) + lane;
  if (nt) {
#pragma unroll
    for (int v = 0; v < NV; ++v) { pa[v] = ld_stream(a + o + v * LPR); pr[v] = ld_stream(r + o + v * LPR); }
  } else {
#pragma unroll
    for (int v = 0; v < NV; ++v) { pa[v] = a[o + v * LPR]; pr[v] = r[o + v * LPR]; }
  }
}

// The three quantizers as the kernel entry derived them (once, from one batch of loads: tq_device.h load_qraw).
struct TailQ {
  QP p1, p2, p3;
};

template <int DT, int LPR, int NV, bool IDX, bool FAST, bool ALLON, bool AFF, bool EMB>
__device__ __forceinline__ void res_ln_body(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                            u32x4* __restrict__ y, int8_t* __restrict__ y_idx, uint64_t rows,
                                            const float* s_w, const float* s_b,
                                            float ln_eps, const TailQ& tq, int on1_, int on2_, int on3_, int nt, uint32_t iters,
                                            const EmbArgs& emb, u32x4 (&va)[NV], u32x4 (&vr)[NV], u32x4 (&va2)[EMB ? NV : 1]) {
  // AFF (NoNorm: affine map only, no statistics) is a compile-time property: as a run-time flag every NaN rule of BOTH
  // variants was evaluated per element and selected (4-5 v_cndmask / v_cmp per element of ~29 VALU instructions on the
  // bf16 LayerNorm rows, found in the ISA in round 4)
  constexpr bool affine_only = AFF;
  // ALLON: the three quantizers are present (the configuration the tails exist for) -> compile-time flags, no uniform
  // branch around every quantizer application (those branches split the row into ~40 basic blocks and serialised it)
  const int on1 = ALLON ? 1 : on1_, on2 = ALLON ? 1 : on2_, on3 = ALLON ? 1 : on3_;
  constexpr int V = Store<DT>::kVec;
  constexpr int H = V / 2;                          // register pairs per 16-byte vector
  constexpr int RPB = kBlock / LPR;                 // rows per block iteration
  constexpr uint32_t d = LPR * NV * V;
  const FusedF f1 = make_ff(tq.p1, on1), f2 = make_ff(tq.p2, on2), f3 = make_ff(tq.p3, on3);
  const FusedQ g1 = make_fq(tq.p1, on1), g2 = make_fq(tq.p2, on2), g3 = make_fq(tq.p3, on3);     // division path (FAST = false)
  const int lane = threadIdx.x % LPR;
  const int sub = threadIdx.x / LPR;
  const float inv_d = 1.0f / (float)d;

  // A block owns `iters` consecutive groups of RPB rows (one-shot tiles in row order: the resident blocks sweep one
  // contiguous window of HBM); the loads of group i + 1 are issued before group i is computed, and the affine
  // parameters / quantizer constants are set up once per block instead of once per RPB rows.  Measured on
  // [131072, 768] (tools/tuning/tail_sweep.py): bf16 LayerNorm 3.6 / 4.6 / 4.9 / 4.9 TB/s for iters = 1 / 2 / 4 / 8,
  // fp32 5.4 / 5.8 / 5.4 / 5.2 -> 8 for 2-byte storage, 2 for fp32 (launch_res_ln).  The first group's loads were issued by
  // the kernel entry, ahead of everything else.
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + sub;
  u32x4 na[NV], nr[NV];
  u32x4 na2[EMB ? NV : 1];
  auto load_row = [&](uint64_t row, u32x4 (&pa)[NV], u32x4 (&pr)[NV], u32x4 (&pa2)[EMB ? NV : 1]) {
    ln_load_row<DT, LPR, NV, EMB>(a, r, emb, nt, lane, row, pa, pr, pa2);
  };
  for (uint32_t it = 0; it < iters; ++it) {
    const uint64_t row = row0 + (uint64_t)it * RPB;
    if (row >= rows) break;
    const uint64_t base = row * (d / V);
    const uint64_t nrow = row + RPB;
    if (it + 1 < iters && nrow < rows) load_row(nrow, na, nr, na2);
    f32x2 u[NV][H];
    f32x2 s2 = {0.f, 0.f}, s2b = {0.f, 0.f};      // two chains for the row sum (LayerNorm only)
    bool lane_nan = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      float fa[V], fr[V];
      Store<DT>::unpack(va[v], fa);
      Store<DT>::unpack(vr[v], fr);
      if (EMB) {                                    // word row + token-type row: ONE fp32 addition in front of Q1
        float f2[V];
        Store<DT>::unpack(va2[v], f2);
#pragma unroll
        for (int k = 0; k < V; ++k) fa[k] = fa[k] + f2[k];
      }
      TQ_TAIL_FRONT(fr, affine_only)
      if (!affine_only) {
#pragma unroll
        for (int j = 0; j < H; ++j) {
          if (j & 1) s2b = s2b + u[v][j];
          else s2 = s2 + u[v][j];
        }
      }
    }
    s2 = s2 + s2b;
    // MobileBERT's NoNorm (models/quantized_mobilebert.py:58-72) is the affine part alone: u * w + b.  With
    // mean = 0 and rstd = 1 the expression below evaluates exactly that ((u - 0) * 1 is exact).
    float mean = 0.0f, rstd = 1.0f;
    bool row_nan = false;                 // LayerNorm: the whole row is NaN (wave-uniform branch at the store, rare)
    if (!affine_only) {
      mean = group_sum<LPR>(s2.x + s2.y) * inv_d;
      const f32x2 m2 = {mean, mean};
      // centred sum of squares: two independent packed accumulators fed by fma (a single `ss2 = ss2 + c * c` chain was
      // 2 packed ops per pair plus a wait state after each: 46 s_nop per 24-element lane row in the round-3 ISA).  The
      // LayerNorm statistics carry a tolerance contract (tests/test_fused_ln.py); NoNorm has no statistics.
      f32x2 ssa = {0.f, 0.f}, ssb = {0.f, 0.f};
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int j = 0; j < H; ++j) {
          const f32x2 c = u[v][j] - m2;
          if ((v * H + j) & 1) ssb = __builtin_elementwise_fma(c, c, ssb);
          else ssa = __builtin_elementwise_fma(c, c, ssa);
        }
      const f32x2 ss2 = ssa + ssb;
      rstd = 1.0f / sqrtf(group_sum<LPR>(ss2.x + ss2.y) * inv_d + ln_eps);
      if (FAST) {
        // rows with a NaN input: the statistics are NaN upstream, hence every output of the row
        const uint64_t m = __ballot(lane_nan);
        const uint64_t grp = TQ_GROUP_MASK;
        if (m & grp) { mean = __builtin_nanf(""); row_nan = true; }
      }
    }
    const f32x2 m2 = {mean, mean}, r2 = {rstd, rstd};
    u32x4 packed[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      float o[V];
      struct alignas(V) { int8_t e[V]; } oi;
      f32x2 t[H];
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const uint32_t c = (v * LPR + lane) * V + 2 * j;
        const f32x2 wv = *reinterpret_cast<const f32x2*>(s_w + c), bv = *reinterpret_cast<const f32x2*>(s_b + c);
        t[j] = (u[v][j] - m2) * r2 * wv + bv;
      }
      if (f3.on) {
        if (FAST) {
          f32x2 h[H];
          qf_round2_n<H>(t, f3.f, h);
#pragma unroll
          for (int j = 0; j < H; ++j) {
            if (IDX) {
              oi.e[2 * j] = (int8_t)((int)(h[j].x + f3.f.zp) - 128);
              oi.e[2 * j + 1] = (int8_t)((int)(h[j].y + f3.f.zp) - 128);
            }
            const f32x2 yq = qf_dequant2(h[j], f3.f);                     // -0 -> +0 like (x_int - zp), one fma
            if (affine_only) {            // NoNorm: element-local NaN passes through
              t[j].x = (t[j].x != t[j].x) ? t[j].x : yq.x;
              t[j].y = (t[j].y != t[j].y) ? t[j].y : yq.y;
            } else {
              t[j] = yq;                  // LayerNorm: NaN rows are patched below
            }
          }
          // (LayerNorm rows with a NaN input are overwritten AFTER the stores below, in a branch that is practically never
          // taken: patching t[] here became one select per element of every row)
        } else {
#pragma unroll
          for (int j = 0; j < H; ++j) {
            const float x0 = index_q(t[j].x, g3), x1 = index_q(t[j].y, g3);
            if (IDX) {
              oi.e[2 * j] = (int8_t)((int)x0 - 128);
              oi.e[2 * j + 1] = (int8_t)((int)x1 - 128);
            }
            t[j] = f32x2{q_dequant(x0, g3.p), q_dequant(x1, g3.p)};
          }
        }
      }
#pragma unroll
      for (int j = 0; j < H; ++j) { o[2 * j] = t[j].x; o[2 * j + 1] = t[j].y; }
      packed[v] = Store<DT>::pack(o);
      if (IDX) *reinterpret_cast<decltype(oi)*>(y_idx + (base + v * LPR + lane) * V) = oi;
    }
    TQ_ROW_STORE(FAST && !affine_only && f3.on, TQ_NAN_ROW_OF(DT))
#pragma unroll
    for (int v = 0; v < NV; ++v) { va[v] = na[v]; vr[v] = nr[v]; }
    if (EMB) {
#pragma unroll
      for (int v = 0; v < NV; ++v) va2[v] = na2[v];
    }
  }
}

template <int DT, int LPR, int NV, bool IDX, bool AFF, bool EMB = false>
__global__ __launch_bounds__(kBlock) void res_ln_quant_k(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                         u32x4* __restrict__ y, int8_t* __restrict__ y_idx, uint64_t rows,
                                                         const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                         float ln_eps, tq_quantizer q1, tq_quantizer q2, tq_quantizer q3,
                                                         int on1, int on2, int on3, int nt, uint32_t iters, EmbArgs emb) {
  constexpr int V = Store<DT>::kVec;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d];
  u32x4 va[NV], vr[NV];
  u32x4 va2[EMB ? NV : 1];
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + threadIdx.x / LPR;
  if (row0 < rows) ln_load_row<DT, LPR, NV, EMB>(a, r, emb, nt, threadIdx.x % LPR, row0, va, vr, va2);
  TQ_AFFINE_REQUEST
  QRaw w1 = load_qraw(q1, 0, ln_w), w2 = load_qraw(q2, 0, ln_w), w3 = load_qraw(q3, 0, ln_w);
  qraw_arrived(w1); qraw_arrived(w2); qraw_arrived(w3);
  TQ_AFFINE_STAGE
  TQ_TAIL_QUANTIZERS
  TQ_TAIL_VOTE
  if (fast && on1 && on2 && on3)
    res_ln_body<DT, LPR, NV, IDX, true, true, AFF, EMB>(a, r, y, y_idx, rows, s_w, s_b, ln_eps, tq, 1, 1, 1, nt, iters, emb, va, vr, va2);
  else if (fast)
    res_ln_body<DT, LPR, NV, IDX, true, false, AFF, EMB>(a, r, y, y_idx, rows, s_w, s_b, ln_eps, tq, on1, on2, on3, nt, iters, emb, va, vr, va2);
  else
    res_ln_body<DT, LPR, NV, IDX, false, false, AFF, EMB>(a, r, y, y_idx, rows, s_w, s_b, ln_eps, tq, on1, on2, on3, nt, iters, emb, va, vr, va2);
}

// The (lanes per row, vectors per lane) forms every tail kernel is instantiated for; a row is LPR * NV 16-byte vectors.
// d (bf16 | fp32): 768 -> 96 | 192 vectors, 3072 -> 384 | 768, 512 -> 64 | 128, 128 -> 16 | 32, 1024 -> 128 | 256
#define TQ_TAIL_SHAPES(X) X(32, 3) X(64, 3) X(64, 6) X(64, 12) X(64, 1) X(64, 2) X(64, 4) X(16, 1) X(32, 1) X(64, 8)

// How a tail of `rows` rows of d elements is launched with LPR lanes per row: rows per block iteration from the lane group,
// iterations per block (res_ln_body: 8 for 2-byte storage, 2 for fp32; TQ_TAIL_ITERS overrides), the grid, and streaming
// loads / stores for tensors that cannot stay in L2 / MALL.
struct TailGeom {
  uint32_t iters;
  unsigned grid;
  int nt;
};
static TailGeom tail_geom(uint64_t rows, uint64_t d, int lpr, size_t elem_bytes) {
  const unsigned rpb = kBlock / lpr;
  TailGeom g;
  g.iters = (uint32_t)std::max<int>(1, std::min<uint64_t>(tuning("TQ_TAIL_ITERS", elem_bytes == 4 ? 2 : 8), ceil_div(rows, (uint64_t)rpb * 2048)));
  g.grid = (unsigned)std::max<uint64_t>(ceil_div(rows, (uint64_t)rpb * g.iters), 1);
  g.nt = rows * d * elem_bytes >= (64ull << 20);
  return g;
}

template <int DT>
static int launch_res_ln(const void* a, const void* r, void* y, int8_t* y_idx, uint64_t rows, uint64_t d, const float* w, const float* b,
                         float eps, const tq_quantizer* q1, const tq_quantizer* q2, const tq_quantizer* q3, int affine_only,
                         hipStream_t st, const EmbArgs* emb_in = nullptr) {
  const EmbArgs emb = emb_in ? *emb_in : EmbArgs{};
  constexpr int V = Store<DT>::kVec;
  const tq_quantizer none{};
  const tq_quantizer &c1 = q1 ? *q1 : none, &c2 = q2 ? *q2 : none, &c3 = q3 ? *q3 : none;
  const auto av = static_cast<const u32x4*>(a);
  const auto rv = static_cast<const u32x4*>(r);
  auto yv = static_cast<u32x4*>(y);
#define TQ_LN_GO(DTV, LPR, NV, IDXV, AFFV, EMBV, NT)                                                            \
  hipLaunchKernelGGL((res_ln_quant_k<DTV, LPR, NV, IDXV, AFFV, EMBV>), dim3(g.grid), dim3(kBlock), 0, st, av, rv, yv, y_idx, \
                     rows, w, b, eps, c1, c2, c3, q1 != nullptr, q2 != nullptr, q3 != nullptr, NT, g.iters, emb)
#define TQ_LN(LPR, NV)                                                                                          \
  if (d == (uint64_t)(LPR) * (NV) * V) {                                                                        \
    const TailGeom g = tail_geom(rows, d, LPR, elem_size(DT));                                                  \
    if (DT == TQ_F32 && emb_in != nullptr) {                                                                    \
      if (y_idx != nullptr) TQ_LN_GO(TQ_F32, LPR, NV, true, false, true, 0);                                    \
      else                  TQ_LN_GO(TQ_F32, LPR, NV, false, false, true, 0);                                   \
      return check_launch("res_ln_quant_k (embeddings)");                                                       \
    }                                                                                                           \
    if (y_idx != nullptr && affine_only)      TQ_LN_GO(DT, LPR, NV, true, true, false, g.nt);                   \
    else if (y_idx != nullptr)                TQ_LN_GO(DT, LPR, NV, true, false, false, g.nt);                  \
    else if (affine_only)                     TQ_LN_GO(DT, LPR, NV, false, true, false, g.nt);                  \
    else                                      TQ_LN_GO(DT, LPR, NV, false, false, false, g.nt);                 \
    return check_launch("res_ln_quant_k");                                                                      \
  }
  TQ_TAIL_SHAPES(TQ_LN)
#undef TQ_LN
#undef TQ_LN_GO
  return set_error(TQ_EUNSUPPORTED, "tq_residual_layernorm_quant_fwd: row length %llu has no instantiation",
                   (unsigned long long)d);
}

// ---------------------------------------------------------------------------------------------------
// The fp32 LayerNorm tail with its residual as int8 INDICES (tq_residual_layernorm_quant_ires_fwd).  On the integer route
// the residual of a tail is the output of an earlier quantizer launch that also emitted int8(index - 128): reading those
// (1 B per element) and dequantizing in registers gives the bits the producer wrote as fp32 -- scale * (index - zp), one
// exact subtraction and one rounded multiplication, what qf_dequant2 / q_dequant compute -- and with y optional a tail
// whose fp32 output nobody reads moves 6 B per element (GEMM 4, residual index 1, y_idx 1) instead of 13.  What the
// indices cannot carry is the NaN rule (a row with an unordered input is NaN as a whole; its indices are unspecified): one
// byte per row travels beside them, raised by the launch that made the row NaN (y_row_nan) and read by the launches that
// take the row as residual (res_row_nan), which turn it back into a row of NaNs before anything else happens to it.
// Lane layout, statistics order, NaN rule, parameter fetch and first-row prefetch are res_ln_quant_k's.  One body,
// res_ln_ires_body<LPR, NV, RK, WY, IDX, ., ., PL>, serves this entry and tq_residual_layernorm_quant_pres_fwd (the two tails of a
// W8A16 layer whose site x travels as byte planes: planes out and no y -- F1, the attention-output tail, RK = 0 | 1, PL -- and
// planes in -- F2, the feed-forward tail, RK = 2, y and optionally y_idx out).  RK says how the residual arrives: 0 as fp32
// (only the flags are added), 1 as int8 indices, 2 as the two byte planes of a <= 16-bit index (`ri` is the high plane, `ri2`
// the low one, read as the planes kernel below stores them -- one 4-byte word per plane and column vector).
template <int LPR, int NV, int RK>
struct IresRow {                  // what one lane holds of one row between its loads and its arithmetic
  u32x4 a[NV];
  u32x4 r[RK != 0 ? 1 : NV];
  uint32_t ri[RK == 1 ? NV : RK == 2 ? 2 * NV : 1];     // 4 residual indices per 16-byte column vector (planes: hi, then lo)
  uint32_t flag;                  // the row's NaN flag (RK != 0)
};

template <int LPR, int NV, int RK>
__device__ __forceinline__ void ires_load_row(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                              const uint32_t* __restrict__ ri, const uint8_t* __restrict__ rflag, int nt,
                                              int lane, uint64_t row, IresRow<LPR, NV, RK>& p,
                                              const uint32_t* __restrict__ ri2 = nullptr) {
  constexpr bool RIDX = RK != 0;
  const uint64_t o = row * (uint64_t)(LPR * NV) + lane;
  if (nt) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      p.a[v] = ld_stream(a + o + v * LPR);
      if (!RIDX) p.r[v] = ld_stream(r + o + v * LPR);
    }
  } else {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      p.a[v] = a[o + v * LPR];
      if (!RIDX) p.r[v] = r[o + v * LPR];
    }
  }
  if (RIDX) {
#pragma unroll
    for (int v = 0; v < NV; ++v) p.ri[v] = ri[o + v * LPR];
    if (RK == 2) {
#pragma unroll
      for (int v = 0; v < NV; ++v) p.ri[(RK == 2 ? NV : 0) + v] = ri2[o + v * LPR];
    }
    p.flag = rflag != nullptr ? rflag[row] : 0u;
  }
}

// PL: the output's index also leaves as its two byte planes (y_hi / y_lo, stored as res_ln_planes_body stores them; needs Q_out)
template <int LPR, int NV, int RK, bool WY, bool IDX, bool FAST, bool ALLON, bool PL = false>
__device__ __forceinline__ void res_ln_ires_body(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                 const uint32_t* __restrict__ ri, const uint8_t* __restrict__ rflag,
                                                 u32x4* __restrict__ y, int8_t* __restrict__ y_idx, uint8_t* __restrict__ yflag,
                                                 uint64_t rows, const float* s_w, const float* s_b, float ln_eps,
                                                 const TailQ& tq, float res_scale, float res_zp, int on1_, int on2_, int on3_,
                                                 int nt, uint32_t iters, IresRow<LPR, NV, RK>& cur,
                                                 const uint32_t* __restrict__ ri2 = nullptr,
                                                 uint32_t* __restrict__ y_hi = nullptr, uint32_t* __restrict__ y_lo = nullptr) {
  constexpr bool RIDX = RK != 0;
  const int on1 = ALLON ? 1 : on1_, on2 = ALLON ? 1 : on2_, on3 = ALLON ? 1 : on3_;
  constexpr int V = 4;
  constexpr int H = 2;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  const FusedF f1 = make_ff(tq.p1, on1), f2 = make_ff(tq.p2, on2), f3 = make_ff(tq.p3, on3);
  const FusedQ g1 = make_fq(tq.p1, on1), g2 = make_fq(tq.p2, on2), g3 = make_fq(tq.p3, on3);     // division path (FAST = false)
  const int lane = threadIdx.x % LPR;
  const int sub = threadIdx.x / LPR;
  const float inv_d = 1.0f / (float)d;
  const uint64_t grp = TQ_GROUP_MASK;
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + sub;
  IresRow<LPR, NV, RK> nxt;
  for (uint32_t it = 0; it < iters; ++it) {
    const uint64_t row = row0 + (uint64_t)it * RPB;
    if (row >= rows) break;
    const uint64_t base = row * (d / V);
    const uint64_t nrow = row + RPB;
    if (it + 1 < iters && nrow < rows) ires_load_row<LPR, NV, RK>(a, r, ri, rflag, nt, lane, nrow, nxt, ri2);
    // the residual row of this lane as fp32: the producer's bits
    float fr[NV][V];
    if (RIDX) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const uint32_t w = cur.ri[v] ^ 0x80808080u;                 // int8(index - 128) -> index, four at a time
        if (RK == 2) {                                              // planes: index = 256 (hi + 128) + (lo + 128) < 2^16, exact as fp32
          const uint32_t wl = cur.ri[(RK == 2 ? NV : 0) + v] ^ 0x80808080u;
#pragma unroll
          for (int k = 0; k < V; ++k)
            fr[v][k] = res_scale * ((float)((((w >> (8 * k)) & 0xffu) << 8) | ((wl >> (8 * k)) & 0xffu)) - res_zp);
        } else {
          fr[v][0] = res_scale * ((float)(w & 0xffu) - res_zp);
          fr[v][1] = res_scale * ((float)((w >> 8) & 0xffu) - res_zp);
          fr[v][2] = res_scale * ((float)((w >> 16) & 0xffu) - res_zp);
          fr[v][3] = res_scale * ((float)(w >> 24) - res_zp);
        }
      }
      if (__ballot(cur.flag != 0)) {               // rare: a NaN row arrives as its flag, its indices mean nothing
        if (cur.flag != 0) {
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int k = 0; k < V; ++k) fr[v][k] = __builtin_nanf("");
        }
      }
    } else {
#pragma unroll
      for (int v = 0; v < NV; ++v) Store<TQ_F32>::unpack(cur.r[v], fr[v]);
    }
    f32x2 u[NV][H];
    f32x2 s2 = {0.f, 0.f}, s2b = {0.f, 0.f};      // two chains for the row sum
    bool lane_nan = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      float fa[V];
      Store<TQ_F32>::unpack(cur.a[v], fa);
      TQ_TAIL_FRONT(fr[v], false)
#pragma unroll
      for (int j = 0; j < H; ++j) {
        if (j & 1) s2b = s2b + u[v][j];
        else s2 = s2 + u[v][j];
      }
    }
    TQ_ROW_STATISTICS(grp)
    const f32x2 m2 = {mean, mean}, r2 = {rstd, rstd};
    u32x4 packed[WY ? NV : 1];
    // Outside the exact path behind Q_out (whose outputs are grid values: never NaN unless patched below) a row is NaN
    // where its outputs are: the division path propagates NaN through every stage, and without Q_out the statistics do.
    bool out_nan = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      float o[V];
      struct alignas(V) { int8_t e[V]; } oi;
      uint32_t pi[PL ? V : 1] = {};                 // PL: the grid index of the four elements of this column vector
      f32x2 t[H];
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const uint32_t c = (v * LPR + lane) * V + 2 * j;
        const f32x2 wv = *reinterpret_cast<const f32x2*>(s_w + c), bv = *reinterpret_cast<const f32x2*>(s_b + c);
        t[j] = (u[v][j] - m2) * r2 * wv + bv;
      }
      if (f3.on) {
        if (FAST) {
          f32x2 h[H];
          qf_round2_n<H>(t, f3.f, h);
#pragma unroll
          for (int j = 0; j < H; ++j) {
            if (IDX) {
              oi.e[2 * j] = (int8_t)((int)(h[j].x + f3.f.zp) - 128);
              oi.e[2 * j + 1] = (int8_t)((int)(h[j].y + f3.f.zp) - 128);
            }
            if (PL) {
              pi[PL ? 2 * j : 0] = (uint32_t)(int)(h[j].x + f3.f.zp);
              pi[PL ? 2 * j + 1 : 0] = (uint32_t)(int)(h[j].y + f3.f.zp);
            }
            if (WY) t[j] = qf_dequant2(h[j], f3.f);      // NaN rows are patched below
          }
        } else {
#pragma unroll
          for (int j = 0; j < H; ++j) {
            const float x0 = index_q(t[j].x, g3), x1 = index_q(t[j].y, g3);
            if (IDX) {
              oi.e[2 * j] = (int8_t)((int)x0 - 128);
              oi.e[2 * j + 1] = (int8_t)((int)x1 - 128);
            }
            if (PL) {
              pi[PL ? 2 * j : 0] = (uint32_t)(int)x0;
              pi[PL ? 2 * j + 1 : 0] = (uint32_t)(int)x1;
            }
            t[j] = f32x2{q_dequant(x0, g3.p), q_dequant(x1, g3.p)};
          }
        }
      }
      if (!(FAST && ALLON)) {
        if (!(FAST && f3.on)) {
#pragma unroll
          for (int j = 0; j < H; ++j) out_nan = out_nan || t[j].x != t[j].x || t[j].y != t[j].y;
        }
      }
      if (WY) {
#pragma unroll
        for (int j = 0; j < H; ++j) { o[2 * j] = t[j].x; o[2 * j + 1] = t[j].y; }
        packed[v] = Store<TQ_F32>::pack(o);
      }
      if (IDX) *reinterpret_cast<decltype(oi)*>(y_idx + (base + v * LPR + lane) * V) = oi;
      if (PL) {
        TQ_PLANE_STORE(pi, PL ? V : 1)
      }
    }
    if (WY) {
      TQ_ROW_STORE(FAST && f3.on, TQ_NAN_ROW_F32)
    }
    if (yflag != nullptr) {                               // one ordinary byte store per row
      if (!(FAST && ALLON)) row_nan = row_nan || (__ballot(out_nan) & grp) != 0;
      if (lane == 0) yflag[row] = row_nan ? 1 : 0;
    }
    cur = nxt;
  }
}

// The forms of tq_residual_layernorm_quant_ires_fwd (RK = RIDX, no planes either way) and, below, those of
// tq_residual_layernorm_quant_pres_fwd: two thin kernels over the one body, the first without the plane pointers it has no
// use for.
template <int LPR, int NV, bool RIDX, bool WY, bool IDX>
__global__ __launch_bounds__(kBlock) void res_ln_quant_ires_k(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                              const uint32_t* __restrict__ ri, const uint8_t* __restrict__ rflag,
                                                              u32x4* __restrict__ y, int8_t* __restrict__ y_idx,
                                                              uint8_t* __restrict__ yflag, uint64_t rows,
                                                              const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                              float ln_eps, tq_quantizer q1, tq_quantizer q2, tq_quantizer q3,
                                                              tq_quantizer qr, int on1, int on2, int on3, int nt, uint32_t iters) {
  constexpr int V = 4;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d];
  IresRow<LPR, NV, RIDX> cur;
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + threadIdx.x / LPR;
  if (row0 < rows) ires_load_row<LPR, NV, RIDX>(a, r, ri, rflag, nt, threadIdx.x % LPR, row0, cur);
  TQ_AFFINE_REQUEST
  QRaw w1 = load_qraw(q1, 0, ln_w), w2 = load_qraw(q2, 0, ln_w), w3 = load_qraw(q3, 0, ln_w), wr = load_qraw(qr, 0, ln_w);
  qraw_arrived(w1); qraw_arrived(w2); qraw_arrived(w3); qraw_arrived(wr);
  TQ_AFFINE_STAGE
  TQ_TAIL_QUANTIZERS
  const QP pr = RIDX ? qp_from_raw(qr, wr) : none;
  TQ_TAIL_VOTE
  if (fast && on1 && on2 && on3)
    res_ln_ires_body<LPR, NV, RIDX, WY, IDX, true, true>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, ln_eps, tq, pr.scale, pr.zp, 1, 1, 1, nt, iters, cur);
  else if (fast)
    res_ln_ires_body<LPR, NV, RIDX, WY, IDX, true, false>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, ln_eps, tq, pr.scale, pr.zp, on1, on2, on3, nt, iters, cur);
  else
    res_ln_ires_body<LPR, NV, RIDX, WY, IDX, false, false>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, ln_eps, tq, pr.scale, pr.zp, on1, on2, on3, nt, iters, cur);
}

template <int LPR, int NV, int RK, bool WY, bool IDX, bool PL>
__global__ __launch_bounds__(kBlock) void res_ln_quant_pres_k(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                              const uint32_t* __restrict__ ri, const uint32_t* __restrict__ ri2,
                                                              const uint8_t* __restrict__ rflag, u32x4* __restrict__ y,
                                                              int8_t* __restrict__ y_idx, uint32_t* __restrict__ y_hi,
                                                              uint32_t* __restrict__ y_lo, uint8_t* __restrict__ yflag,
                                                              uint64_t rows, const float* __restrict__ ln_w,
                                                              const float* __restrict__ ln_b, float ln_eps, tq_quantizer q1,
                                                              tq_quantizer q2, tq_quantizer q3, tq_quantizer qr, int on1, int on2,
                                                              int on3, int nt, uint32_t iters) {
  constexpr int V = 4;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d];
  IresRow<LPR, NV, RK> cur;
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + threadIdx.x / LPR;
  if (row0 < rows) ires_load_row<LPR, NV, RK>(a, r, ri, rflag, nt, threadIdx.x % LPR, row0, cur, ri2);
  TQ_AFFINE_REQUEST
  QRaw w1 = load_qraw(q1, 0, ln_w), w2 = load_qraw(q2, 0, ln_w), w3 = load_qraw(q3, 0, ln_w), wr = load_qraw(qr, 0, ln_w);
  qraw_arrived(w1); qraw_arrived(w2); qraw_arrived(w3); qraw_arrived(wr);
  TQ_AFFINE_STAGE
  TQ_TAIL_QUANTIZERS
  const QP pr = RK != 0 ? qp_from_raw(qr, wr) : none;
  TQ_TAIL_VOTE
  if (fast && on1 && on2 && on3)
    res_ln_ires_body<LPR, NV, RK, WY, IDX, true, true, PL>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, ln_eps, tq, pr.scale, pr.zp, 1, 1, 1, nt, iters, cur, ri2, y_hi, y_lo);
  else if (fast)
    res_ln_ires_body<LPR, NV, RK, WY, IDX, true, false, PL>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, ln_eps, tq, pr.scale, pr.zp, on1, on2, on3, nt, iters, cur, ri2, y_hi, y_lo);
  else
    res_ln_ires_body<LPR, NV, RK, WY, IDX, false, false, PL>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, ln_eps, tq, pr.scale, pr.zp, on1, on2, on3, nt, iters, cur, ri2, y_hi, y_lo);
}
// ---------------------------------------------------------------------------------------------------
// The fp32 LayerNorm tail that writes the two byte planes of its output's index (tq_residual_layernorm_quant_planes_fwd).
// Where the consumer of y is the 16-bit integer Linear, the index the tail holds in registers behind Q_out -- (int)(h + zp)
// on the exact path, index_q on the division path -- is what tq_quantize_hilo_fwd would re-derive from y in a launch of its
// own (a fixed-range quantizer is idempotent on its own grid), so its two bytes go out here: per 16-byte column vector one
// 4-byte store per plane, the byte b ^ 0x80 for b - 128, next to the 16-byte store of y (2 B per element beside 12).  Lane
// layout, statistics order, NaN rule, parameter fetch and first-row prefetch are res_ln_quant_k's fp32 forms; Q_out is always
// present.  A body of its own beside res_ln_ires_body<0, true, false, ., ., true>, which computes the same: as that form the
// tail read 1.7 % behind this body at [131072, 768] in one A/B run.  The cause was not found in the ISA, and the figure lies
// within what a later control (one library against its own copy) shows for identical code, so it is no established cost:
// the body stays because that keeps this kernel's code what it was.  The planes of a NaN row are unspecified.
template <int LPR, int NV, bool FAST, bool ALLON>
__device__ __forceinline__ void res_ln_planes_body(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                   u32x4* __restrict__ y, uint32_t* __restrict__ y_hi, uint32_t* __restrict__ y_lo,
                                                   uint64_t rows, const float* s_w, const float* s_b, float ln_eps,
                                                   const TailQ& tq, int on1_, int on2_, int nt, uint32_t iters,
                                                   u32x4 (&va)[NV], u32x4 (&vr)[NV]) {
  const int on1 = ALLON ? 1 : on1_, on2 = ALLON ? 1 : on2_;
  constexpr int V = 4;
  constexpr int H = 2;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  const FusedF f1 = make_ff(tq.p1, on1), f2 = make_ff(tq.p2, on2), f3 = make_ff(tq.p3, 1);
  const FusedQ g1 = make_fq(tq.p1, on1), g2 = make_fq(tq.p2, on2), g3 = make_fq(tq.p3, 1);     // division path (FAST = false)
  const int lane = threadIdx.x % LPR;
  const int sub = threadIdx.x / LPR;
  const float inv_d = 1.0f / (float)d;
  const EmbArgs no_emb{};
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + sub;
  u32x4 na[NV], nr[NV];
  u32x4 unused[1];
  for (uint32_t it = 0; it < iters; ++it) {
    const uint64_t row = row0 + (uint64_t)it * RPB;
    if (row >= rows) break;
    const uint64_t base = row * (d / V);
    const uint64_t nrow = row + RPB;
    if (it + 1 < iters && nrow < rows) ln_load_row<TQ_F32, LPR, NV, false>(a, r, no_emb, nt, lane, nrow, na, nr, unused);
    f32x2 u[NV][H];
    f32x2 s2 = {0.f, 0.f}, s2b = {0.f, 0.f};      // two chains for the row sum
    bool lane_nan = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      float fa[V], fr[V];
      Store<TQ_F32>::unpack(va[v], fa);
      Store<TQ_F32>::unpack(vr[v], fr);
      TQ_TAIL_FRONT(fr, false)
#pragma unroll
      for (int j = 0; j < H; ++j) {
        if (j & 1) s2b = s2b + u[v][j];
        else s2 = s2 + u[v][j];
      }
    }
    TQ_ROW_STATISTICS(TQ_GROUP_MASK)
    const f32x2 m2 = {mean, mean}, r2 = {rstd, rstd};
    u32x4 packed[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      float o[V];
      uint32_t idx[V];                              // the grid index of the four elements of this column vector
      f32x2 t[H];
#pragma unroll
      for (int j = 0; j < H; ++j) {
        const uint32_t c = (v * LPR + lane) * V + 2 * j;
        const f32x2 wv = *reinterpret_cast<const f32x2*>(s_w + c), bv = *reinterpret_cast<const f32x2*>(s_b + c);
        t[j] = (u[v][j] - m2) * r2 * wv + bv;
      }
      if (FAST) {
        f32x2 h[H];
        qf_round2_n<H>(t, f3.f, h);
#pragma unroll
        for (int j = 0; j < H; ++j) {
          idx[2 * j] = (uint32_t)(int)(h[j].x + f3.f.zp);
          idx[2 * j + 1] = (uint32_t)(int)(h[j].y + f3.f.zp);
          t[j] = qf_dequant2(h[j], f3.f);           // NaN rows are patched below
        }
      } else {
#pragma unroll
        for (int j = 0; j < H; ++j) {
          const float x0 = index_q(t[j].x, g3), x1 = index_q(t[j].y, g3);
          idx[2 * j] = (uint32_t)(int)x0;
          idx[2 * j + 1] = (uint32_t)(int)x1;
          t[j] = f32x2{q_dequant(x0, g3.p), q_dequant(x1, g3.p)};
        }
      }
#pragma unroll
      for (int j = 0; j < H; ++j) { o[2 * j] = t[j].x; o[2 * j + 1] = t[j].y; }
      packed[v] = Store<TQ_F32>::pack(o);
      TQ_PLANE_STORE(idx, V)
    }
    TQ_ROW_STORE(FAST, TQ_NAN_ROW_F32)
#pragma unroll
    for (int v = 0; v < NV; ++v) { va[v] = na[v]; vr[v] = nr[v]; }
  }
}

template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void res_ln_quant_planes_k(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                                u32x4* __restrict__ y, uint32_t* __restrict__ y_hi,
                                                                uint32_t* __restrict__ y_lo, uint64_t rows,
                                                                const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                                float ln_eps, tq_quantizer q1, tq_quantizer q2, tq_quantizer q3,
                                                                int on1, int on2, int nt, uint32_t iters) {
  // Prologue as in res_ln_quant_k: the first row of every lane group, the affine parameters and the raw buffers of the
  // three quantizers are requested together and waited for once.
  constexpr int V = 4;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d];
  u32x4 va[NV], vr[NV];
  u32x4 unused[1];
  const EmbArgs no_emb{};
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + threadIdx.x / LPR;
  if (row0 < rows) ln_load_row<TQ_F32, LPR, NV, false>(a, r, no_emb, nt, threadIdx.x % LPR, row0, va, vr, unused);
  TQ_AFFINE_REQUEST
  QRaw w1 = load_qraw(q1, 0, ln_w), w2 = load_qraw(q2, 0, ln_w), w3 = load_qraw(q3, 0, ln_w);
  qraw_arrived(w1); qraw_arrived(w2); qraw_arrived(w3);
  TQ_AFFINE_STAGE
  const QP none = {1.f, 0.f, 0.f, 0.f};
  const TailQ tq = {on1 ? qp_from_raw(q1, w1) : none, on2 ? qp_from_raw(q2, w2) : none, qp_from_raw(q3, w3)};
  bool fast = make_qf(tq.p3).ok;
  if (on1) fast = fast && make_qf(tq.p1).ok;
  if (on2) fast = fast && make_qf(tq.p2).ok;
  if (fast && on1 && on2)
    res_ln_planes_body<LPR, NV, true, true>(a, r, y, y_hi, y_lo, rows, s_w, s_b, ln_eps, tq, 1, 1, nt, iters, va, vr);
  else if (fast)
    res_ln_planes_body<LPR, NV, true, false>(a, r, y, y_hi, y_lo, rows, s_w, s_b, ln_eps, tq, on1, on2, nt, iters, va, vr);
  else
    res_ln_planes_body<LPR, NV, false, false>(a, r, y, y_hi, y_lo, rows, s_w, s_b, ln_eps, tq, on1, on2, nt, iters, va, vr);
}

// The (RK, WY, IDX, PL) forms that exist: the index-residual entry's six (res_ln_quant_ires_k) and the two planes-in and the
// two planes-out forms of the plane-residual entry (res_ln_quant_pres_k).  The eleventh form, y beside its planes with an fp32
// residual and no row flags (0, 1, 0, 1), is the plane tail: res_ln_quant_planes_k.
#define TQ_IRES_FORMS(X, LPR, NV)                                                                               \
  X(LPR, NV, 0, false, true, false) X(LPR, NV, 0, true, true, false) X(LPR, NV, 0, true, false, false)          \
  X(LPR, NV, 1, false, true, false) X(LPR, NV, 1, true, true, false) X(LPR, NV, 1, true, false, false)
#define TQ_PRES_FORMS(X, LPR, NV)                                                                               \
  X(LPR, NV, 2, true, true, false) X(LPR, NV, 2, true, false, false)                                            \
  X(LPR, NV, 1, false, false, true) X(LPR, NV, 0, false, false, true)

// The form follows from which pointers are given: the residual as planes (rh / rl), as indices (ri) or as fp32 (r); y,
// y_idx and the output planes each where their pointer is not NULL.  The plane tail takes no row flags and needs Q_out: with
// either missing the call is no form that exists.
static int launch_res_ln_ires(const char* who, const float* a, const float* r, const int8_t* ri, const int8_t* rh,
                              const int8_t* rl, const uint8_t* rflag, float* y, int8_t* y_idx, int8_t* y_hi, int8_t* y_lo,
                              uint8_t* yflag, uint64_t rows, uint64_t d, const float* w, const float* b, float eps,
                              const tq_quantizer* q1, const tq_quantizer* q2, const tq_quantizer* q3, const tq_quantizer* qr,
                              hipStream_t st) {
  const tq_quantizer none{};
  const tq_quantizer &c1 = q1 ? *q1 : none, &c2 = q2 ? *q2 : none, &c3 = q3 ? *q3 : none, &cr = qr ? *qr : none;
  const auto av = reinterpret_cast<const u32x4*>(a);
  const auto rv = reinterpret_cast<const u32x4*>(r);
  const auto iv = reinterpret_cast<const uint32_t*>(rh != nullptr ? rh : ri);
  const auto lv = reinterpret_cast<const uint32_t*>(rl);
  auto yv = reinterpret_cast<u32x4*>(y);
  auto yh = reinterpret_cast<uint32_t*>(y_hi);
  auto yl = reinterpret_cast<uint32_t*>(y_lo);
  const int rk = rh != nullptr ? 2 : ri != nullptr ? 1 : 0;
  const bool wy = y != nullptr, idx = y_idx != nullptr, pl = y_hi != nullptr;
#define TQ_LNI_GO(LPR, NV, RKV, WYV, IDXV, PLV)                                                                 \
  if (rk == RKV && wy == WYV && idx == IDXV && pl == PLV) {                                                     \
    hipLaunchKernelGGL((res_ln_quant_ires_k<LPR, NV, RKV != 0, WYV, IDXV>), dim3(g.grid), dim3(kBlock), 0, st, av, rv, iv, rflag, \
                       yv, y_idx, yflag, rows, w, b, eps, c1, c2, c3, cr, q1 != nullptr, q2 != nullptr, q3 != nullptr, g.nt,    \
                       g.iters);                                                                                \
    return check_launch("res_ln_quant_ires_k");                                                                 \
  }
#define TQ_LNR_GO(LPR, NV, RKV, WYV, IDXV, PLV)                                                                 \
  if (rk == RKV && wy == WYV && idx == IDXV && pl == PLV) {                                                     \
    hipLaunchKernelGGL((res_ln_quant_pres_k<LPR, NV, RKV, WYV, IDXV, PLV>), dim3(g.grid), dim3(kBlock), 0, st, av, rv, iv, lv, \
                       rflag, yv, y_idx, yh, yl, yflag, rows, w, b, eps, c1, c2, c3, cr, q1 != nullptr, q2 != nullptr,         \
                       q3 != nullptr, g.nt, g.iters);                                                           \
    return check_launch("res_ln_quant_pres_k");                                                                 \
  }
#define TQ_LNI(LPR, NV)                                                                                         \
  if (d == (uint64_t)(LPR) * (NV) * 4) {                                                                        \
    const TailGeom g = tail_geom(rows, d, LPR, 4);                                                              \
    if (rk == 0 && wy && !idx && pl && rflag == nullptr && yflag == nullptr && q3 != nullptr) {                 \
      hipLaunchKernelGGL((res_ln_quant_planes_k<LPR, NV>), dim3(g.grid), dim3(kBlock), 0, st, av, rv, yv, yh, yl, rows, w, b, eps, \
                         c1, c2, c3, q1 != nullptr, q2 != nullptr, g.nt, g.iters);                              \
      return check_launch("res_ln_quant_planes_k");                                                             \
    }                                                                                                           \
    TQ_IRES_FORMS(TQ_LNI_GO, LPR, NV)                                                                           \
    TQ_PRES_FORMS(TQ_LNR_GO, LPR, NV)                                                                           \
    return set_error(TQ_EUNSUPPORTED,                                                                           \
                     "%s: supported are (1) residual as fp32 or res_idx with y_hi / y_lo [and y_row_nan] as the only outputs " \
                     "(y == NULL, y_idx == NULL) and (2) residual as res_hi / res_lo with y [, y_idx] [, y_row_nan] and no "  \
                     "output planes", who);                                                                     \
  }
  TQ_TAIL_SHAPES(TQ_LNI)
#undef TQ_LNI
#undef TQ_LNI_GO
#undef TQ_LNR_GO
  return set_error(TQ_EUNSUPPORTED, "%s: row length %llu has no instantiation", who, (unsigned long long)d);
}

// ---------------------------------------------------------------------------------------------------
// The LayerNorm tail with quantizer parameters PER COLUMN (tq_residual_layernorm_quant_axis_fwd): per-embedding and
// per-embedding-group (PEG) activation quantizers hold `_delta[d]` / `_zero_float[d]` in natural column order.  Same lane
// layout, statistics and element arithmetic as res_ln_quant_k above (oracle/ln_sum.py applies unchanged); only the
// quantizer constants differ from column to column.  A lane owns 12-24 columns and three quantizers' constants do not
// fit in registers next to the row, so every block derives them ONCE (make_qp's arithmetic per column, in the prologue,
// from loads that are in flight together with the first rows and the affine parameters) and stages them in LDS next to
// s_w / s_b: four floats per column and quantizer, as four arrays that the row loop reads as 16-byte vectors of
// consecutive columns --
//     exact path:     scale, RN(1 / scale), y_lo, y_hi        (QF of tq_device.h; + zp of Q_out when indices are emitted)
//     division path:  scale, guarded_rcp(scale), zp           (lo / hi are per quantizer, not per column)
// The exact path is taken when EVERY column of every enabled quantizer admits it (one block-wide vote); both paths give
// the bits of tq_fake_quant_fwd with n_params = d.  A per-tensor quantizer in the mix is broadcast into its table.
// LDS: (14 + IDX) x 4 x d bytes -- 43 / 46 KB at d = 768 (3 blocks per CU), 57 / 61 KB at d = 1024 (2 blocks per CU); wider
// rows do not fit the 64 KB a block may declare and are refused by the launcher.
constexpr uint64_t kAxisMaxD = 1024;

template <int H>
__device__ __forceinline__ void lds_pairs(const float* s, uint32_t c0, f32x2 (&o)[H]) {      // H pairs = 2 H consecutive columns
#pragma unroll
  for (int k = 0; k < H / 2; ++k) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(s + c0 + 4 * k);
    o[2 * k] = f32x2{t[0], t[1]};
    o[2 * k + 1] = f32x2{t[2], t[3]};
  }
}

// qf_round2_n with the constants of each pair's own columns: tab = [4][D] (scale, rcp, y_lo, y_hi); sc returns the scales
template <int H, uint32_t D>
__device__ __forceinline__ void axq_round(const f32x2 (&x)[H], const float* tab, uint32_t c0, f32x2 (&h)[H], f32x2 (&sc)[H]) {
  f32x2 rc[H], lo[H], hi[H], xc[H], q0[H], e[H];
  lds_pairs<H>(tab, c0, sc);
  lds_pairs<H>(tab + D, c0, rc);
  lds_pairs<H>(tab + 2 * D, c0, lo);
  lds_pairs<H>(tab + 3 * D, c0, hi);
#pragma unroll
  for (int i = 0; i < H; ++i) {
    xc[i].x = __builtin_amdgcn_fmed3f(x[i].x, lo[i].x, hi[i].x);
    xc[i].y = __builtin_amdgcn_fmed3f(x[i].y, lo[i].y, hi[i].y);
  }
#pragma unroll
  for (int i = 0; i < H; ++i) q0[i] = xc[i] * rc[i];
#pragma unroll
  for (int i = 0; i < H; ++i) e[i] = __builtin_elementwise_fma(q0[i], -sc[i], xc[i]);
#pragma unroll
  for (int i = 0; i < H; ++i) q0[i] = __builtin_elementwise_fma(e[i], rc[i], q0[i]);
#pragma unroll
  for (int i = 0; i < H; ++i) h[i] = f32x2{rintf(q0[i].x), rintf(q0[i].y)};
}
// PLUS0 = false: the "+ 0" that turns -0 into +0 is skipped (qf_fake_quant2_n_signed_zero: another quantizer follows)
template <int H, uint32_t D, bool PLUS0>
__device__ __forceinline__ void axq_fake_quant(f32x2 (&x)[H], const float* tab, uint32_t c0) {
  f32x2 h[H], sc[H];
  axq_round<H, D>(x, tab, c0, h, sc);
#pragma unroll
  for (int i = 0; i < H; ++i) x[i] = PLUS0 ? __builtin_elementwise_fma(sc[i], h[i], f32x2{0.0f, 0.0f}) : sc[i] * h[i];
}

struct AxisLim {          // int_min / int_max of the three quantizers (division path)
  float lo[3], hi[3];
};
template <uint32_t D>
__device__ __forceinline__ FusedQ axis_fq(const float* tab, uint32_t c, const AxisLim& lim, int k, int on) {
  FusedQ f = {QP{1.f, 0.f, 0.f, 0.f}, on, 1.f};
  if (on) { f.p = QP{tab[c], tab[2 * D + c], lim.lo[k], lim.hi[k]}; f.rcp = tab[D + c]; }
  return f;
}

// The two row pieces of the per-column bodies, as macros for the reason given at TQ_GROUP_MASK (they expand to the text the
// axis body held before there were two bodies):
//   TQ_AXIS_FRONT        one 16-byte vector (fa, residual FR) of the columns from c0 through the front of the chain into u[v];
//                        uses H, d, FAST, ALLON, on1, on2, t1, t2, lim, c0, fa, u, v, lane_nan; declares (in its own block) t
//   TQ_AXIS_AFFINE_QOUT  the affine map and Q_out of column vector v: t[] holds the outputs, oi the indices (IDX);
//                        uses H, d, FAST, IDX, on3, s_w, s_b, s_zp3, t3, lim, c0, u, v, m2, r2, oi; declares t, wv, bv
#define TQ_AXIS_FRONT(FR)                                                                                       \
  if (FAST) {                                                                                                   \
    f32x2 t[H];                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < H; ++j) t[j] = f32x2{fa[2 * j], fa[2 * j + 1]};                       \
    if (ALLON) axq_fake_quant<H, d, false>(t, t1, c0);                                                          \
    else if (on1) axq_fake_quant<H, d, true>(t, t1, c0);                                                        \
    _Pragma("unroll") for (int j = 0; j < H; ++j) t[j] = t[j] + f32x2{FR[2 * j], FR[2 * j + 1]};                \
    if (ALLON) axq_fake_quant<H, d, false>(t, t2, c0);                                                          \
    else if (on2) axq_fake_quant<H, d, true>(t, t2, c0);                                                        \
    _Pragma("unroll") for (int j = 0; j < H; ++j)                                                               \
      lane_nan = lane_nan || __builtin_isunordered(fa[2 * j], FR[2 * j]) ||                                     \
                 __builtin_isunordered(fa[2 * j + 1], FR[2 * j + 1]);                                           \
    _Pragma("unroll") for (int j = 0; j < H; ++j) u[v][j] = t[j];                                               \
  } else {                                                                                                      \
    _Pragma("unroll") for (int j = 0; j < H; ++j) {                                                             \
      const uint32_t c = c0 + 2 * j;                                                                            \
      u[v][j] = f32x2{apply_q(apply_q(fa[2 * j], axis_fq<d>(t1, c, lim, 0, on1)) + FR[2 * j], axis_fq<d>(t2, c, lim, 1, on2)),\
                      apply_q(apply_q(fa[2 * j + 1], axis_fq<d>(t1, c + 1, lim, 0, on1)) + FR[2 * j + 1],       \
                              axis_fq<d>(t2, c + 1, lim, 1, on2))};                                             \
    }                                                                                                           \
  }

#define TQ_AXIS_AFFINE_QOUT                                                                                     \
  f32x2 t[H], wv[H], bv[H];                                                                                     \
  lds_pairs<H>(s_w, c0, wv);                                                                                    \
  lds_pairs<H>(s_b, c0, bv);                                                                                    \
  _Pragma("unroll") for (int j = 0; j < H; ++j) t[j] = (u[v][j] - m2) * r2 * wv[j] + bv[j];                     \
  if (on3) {                                                                                                    \
    if (FAST) {                                                                                                 \
      f32x2 h[H], sc[H], zp[H];                                                                                 \
      axq_round<H, d>(t, t3, c0, h, sc);                                                                        \
      if (IDX) lds_pairs<H>(s_zp3, c0, zp);                                                                     \
      _Pragma("unroll") for (int j = 0; j < H; ++j) {                                                           \
        if (IDX) {                                                                                              \
          oi.e[2 * j] = (int8_t)((int)(h[j].x + zp[j].x) - 128);                                                \
          oi.e[2 * j + 1] = (int8_t)((int)(h[j].y + zp[j].y) - 128);                                            \
        }                                                                                                       \
        t[j] = __builtin_elementwise_fma(sc[j], h[j], f32x2{0.0f, 0.0f});                                       \
      }                                                                                                         \
    } else {                                                                                                    \
      _Pragma("unroll") for (int j = 0; j < H; ++j) {                                                           \
        const FusedQ ga = axis_fq<d>(t3, c0 + 2 * j, lim, 2, 1), gb = axis_fq<d>(t3, c0 + 2 * j + 1, lim, 2, 1);\
        const float x0 = index_q(t[j].x, ga), x1 = index_q(t[j].y, gb);                                         \
        if (IDX) {                                                                                              \
          oi.e[2 * j] = (int8_t)((int)x0 - 128);                                                                \
          oi.e[2 * j + 1] = (int8_t)((int)x1 - 128);                                                            \
        }                                                                                                       \
        t[j] = f32x2{q_dequant(x0, ga.p), q_dequant(x1, gb.p)};                                                 \
      }                                                                                                         \
    }                                                                                                           \
  }

template <int DT, int LPR, int NV, bool IDX, bool FAST, bool ALLON>
__device__ __forceinline__ void res_ln_axis_body(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                 u32x4* __restrict__ y, int8_t* __restrict__ y_idx, uint64_t rows,
                                                 const float* s_w, const float* s_b, const float* s_q, const float* s_zp3,
                                                 float ln_eps, const AxisLim& lim, int on1_, int on2_, int on3_, int nt,
                                                 uint32_t iters, u32x4 (&va)[NV], u32x4 (&vr)[NV]) {
  const int on1 = ALLON ? 1 : on1_, on2 = ALLON ? 1 : on2_, on3 = ALLON ? 1 : on3_;
  constexpr int V = Store<DT>::kVec;
  constexpr int H = V / 2;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  const float *t1 = s_q, *t2 = s_q + 4 * d, *t3 = s_q + 8 * d;
  const int lane = threadIdx.x % LPR;
  const int sub = threadIdx.x / LPR;
  const float inv_d = 1.0f / (float)d;
  const EmbArgs emb{};
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + sub;
  u32x4 na[NV], nr[NV], dummy[1];
  for (uint32_t it = 0; it < iters; ++it) {
    const uint64_t row = row0 + (uint64_t)it * RPB;
    if (row >= rows) break;
    const uint64_t base = row * (d / V);
    const uint64_t nrow = row + RPB;
    if (it + 1 < iters && nrow < rows) ln_load_row<DT, LPR, NV, false>(a, r, emb, nt, lane, nrow, na, nr, dummy);
    f32x2 u[NV][H];
    f32x2 s2 = {0.f, 0.f}, s2b = {0.f, 0.f};
    bool lane_nan = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const uint32_t c0 = (v * LPR + lane) * V;
      float fa[V], fr[V];
      Store<DT>::unpack(va[v], fa);
      Store<DT>::unpack(vr[v], fr);
      TQ_AXIS_FRONT(fr)
#pragma unroll
      for (int j = 0; j < H; ++j) {
        if (j & 1) s2b = s2b + u[v][j];
        else s2 = s2 + u[v][j];
      }
    }
    TQ_ROW_STATISTICS(TQ_GROUP_MASK)
    const f32x2 m2 = {mean, mean}, r2 = {rstd, rstd};
    u32x4 packed[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const uint32_t c0 = (v * LPR + lane) * V;
      float o[V];
      struct alignas(V) { int8_t e[V]; } oi;
      TQ_AXIS_AFFINE_QOUT
#pragma unroll
      for (int j = 0; j < H; ++j) { o[2 * j] = t[j].x; o[2 * j + 1] = t[j].y; }
      packed[v] = Store<DT>::pack(o);
      if (IDX) *reinterpret_cast<decltype(oi)*>(y_idx + (base + v * LPR + lane) * V) = oi;
    }
    TQ_ROW_STORE(FAST && on3, TQ_NAN_ROW_OF(DT))
#pragma unroll
    for (int v = 0; v < NV; ++v) { va[v] = na[v]; vr[v] = nr[v]; }
  }
}

// raw parameters of column c (or of the only parameter of a per-tensor quantizer); an absent buffer reads `safe`
__device__ __forceinline__ void axis_load_raw(const tq_quantizer& q, uint32_t c, const float* safe, float& dl, float& zf) {
  const uint64_t p = q.n_params == 1 ? 0 : c;
  dl = *(q.delta != nullptr ? q.delta + p : safe);
  zf = *(q.zero_float != nullptr ? q.zero_float + p : safe);
}
__device__ __forceinline__ uint32_t axis_load_flag(const tq_quantizer& q, const float* safe) {
  return *(q.signed_flag != nullptr ? q.signed_flag : reinterpret_cast<const uint8_t*>(safe));
}
__device__ __forceinline__ void pin_lane(float& v) { asm volatile("" : "+v"(v)); }

// The prologue of the per-column kernels in three steps (macros: see TQ_GROUP_MASK), around what a kernel adds of its own:
//   TQ_AXIS_REQUEST  the affine parameters and the raw parameters of this thread's columns for the three quantizers, and
//                    their signed flags; uses NA, d, ln_w, ln_b, q1..q3; declares aw, ab, rd, rz, sg
//   TQ_AXIS_DERIVE   waits for them, derives every column's constants and takes the block-wide vote for the exact path (the
//                    limits are the same for every column: they depend on n_bits / symmetric / signed alone);
//                    uses on1..on3; declares on, qf, ok, lim, fast
//   TQ_AXIS_STAGE    the tables into LDS, and the barrier; uses IDX, s_w, s_b, s_q, s_zp3
#define TQ_AXIS_REQUEST                                                                                         \
  float aw[NA], ab[NA], rd[3][NA], rz[3][NA];                                                                   \
  _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                              \
    const uint32_t c = threadIdx.x + i * kBlock;                                                                \
    const uint32_t cc = c < d ? c : d - 1;                                                                      \
    aw[i] = ln_w[cc];                                                                                           \
    ab[i] = ln_b[cc];                                                                                           \
    axis_load_raw(q1, cc, ln_w, rd[0][i], rz[0][i]);                                                            \
    axis_load_raw(q2, cc, ln_w, rd[1][i], rz[1][i]);                                                            \
    axis_load_raw(q3, cc, ln_w, rd[2][i], rz[2][i]);                                                            \
  }                                                                                                             \
  uint32_t sg[3] = {axis_load_flag(q1, ln_w), axis_load_flag(q2, ln_w), axis_load_flag(q3, ln_w)};

#define TQ_AXIS_DERIVE                                                                                          \
  _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                               \
    sg[k] = __builtin_amdgcn_readfirstlane(sg[k]);                                                              \
    _Pragma("unroll") for (int i = 0; i < NA; ++i) { pin_lane(rd[k][i]); pin_lane(rz[k][i]); }                  \
  }                                                                                                             \
  const int on[3] = {on1, on2, on3};                                                                            \
  QF qf[3][NA];                                                                                                 \
  int ok = 1;                                                                                                   \
  AxisLim lim;                                                                                                  \
  _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                               \
    const tq_quantizer& q = k == 0 ? q1 : (k == 1 ? q2 : q3);                                                   \
    lim.lo[k] = 0.f;                                                                                            \
    lim.hi[k] = 0.f;                                                                                            \
    _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                            \
      const QP p = on[k] ? qp_from_raw(q, QRaw{rd[k][i], rz[k][i], sg[k]}) : QP{1.f, 0.f, 0.f, 0.f};            \
      qf[k][i] = make_qf(p);                                                                                    \
      ok = ok && (!on[k] || qf[k][i].ok);                                                                       \
      lim.lo[k] = p.lo;                                                                                         \
      lim.hi[k] = p.hi;                                                                                         \
    }                                                                                                           \
  }                                                                                                             \
  const int fast = __syncthreads_and(ok);

#define TQ_AXIS_STAGE                                                                                           \
  _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                              \
    const uint32_t c = threadIdx.x + i * kBlock;                                                                \
    if (c < d) {                                                                                                \
      s_w[c] = aw[i];                                                                                           \
      s_b[c] = ab[i];                                                                                           \
      _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                           \
        float* t = s_q + k * 4 * d;                                                                             \
        const QF& f = qf[k][i];                                                                                 \
        t[c] = f.scale.x;                                                                                       \
        t[d + c] = f.rcp.x;                                                                                     \
        t[2 * d + c] = fast ? f.ylo : f.zp;                                                                     \
        t[3 * d + c] = f.yhi;                                                                                   \
      }                                                                                                         \
      if (IDX) s_zp3[c] = qf[2][i].zp;                                                                          \
    }                                                                                                           \
  }                                                                                                             \
  __syncthreads();

template <int DT, int LPR, int NV, bool IDX>
__global__ __launch_bounds__(kBlock) void res_ln_quant_axis_k(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                              u32x4* __restrict__ y, int8_t* __restrict__ y_idx, uint64_t rows,
                                                              const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                              float ln_eps, tq_quantizer q1, tq_quantizer q2, tq_quantizer q3,
                                                              int on1, int on2, int on3, int nt, uint32_t iters) {
  // Prologue as in res_ln_quant_k: everything the block reads before its row loop is requested first (first rows, affine
  // parameters, the raw parameters of this thread's columns for the three quantizers), then waited for once.
  constexpr int V = Store<DT>::kVec;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  static_assert(d <= kAxisMaxD, "per-column tables must fit in LDS");
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d], s_q[3 * 4 * d], s_zp3[IDX ? d : 4];
  u32x4 va[NV], vr[NV], dummy[1];
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + threadIdx.x / LPR;
  if (row0 < rows) ln_load_row<DT, LPR, NV, false>(a, r, EmbArgs{}, nt, threadIdx.x % LPR, row0, va, vr, dummy);
  TQ_AXIS_REQUEST
  TQ_AXIS_DERIVE
  TQ_AXIS_STAGE
  if (fast && on1 && on2 && on3)
    res_ln_axis_body<DT, LPR, NV, IDX, true, true>(a, r, y, y_idx, rows, s_w, s_b, s_q, s_zp3, ln_eps, lim, 1, 1, 1, nt, iters, va, vr);
  else if (fast)
    res_ln_axis_body<DT, LPR, NV, IDX, true, false>(a, r, y, y_idx, rows, s_w, s_b, s_q, s_zp3, ln_eps, lim, on1, on2, on3, nt, iters, va, vr);
  else
    res_ln_axis_body<DT, LPR, NV, IDX, false, false>(a, r, y, y_idx, rows, s_w, s_b, s_q, s_zp3, ln_eps, lim, on1, on2, on3, nt, iters, va, vr);
}

template <int DT>
static int launch_res_ln_axis(const void* a, const void* r, void* y, int8_t* y_idx, uint64_t rows, uint64_t d, const float* w,
                              const float* b, float eps, const tq_quantizer* q1, const tq_quantizer* q2, const tq_quantizer* q3,
                              hipStream_t st) {
  constexpr int V = Store<DT>::kVec;
  const tq_quantizer none{};
  const tq_quantizer &c1 = q1 ? *q1 : none, &c2 = q2 ? *q2 : none, &c3 = q3 ? *q3 : none;
  const auto av = static_cast<const u32x4*>(a);
  const auto rv = static_cast<const u32x4*>(r);
  auto yv = static_cast<u32x4*>(y);
  // Of the shared shapes those whose tables fit: rows of 16 / 32 / 64 / 96 / 128 / 192 / 256 vectors for fp32, of 16 / 32 /
  // 64 / 96 / 128 for 2-byte storage.
#define TQ_LNA_GO(LPR, NV, IDXV)                                                                                \
  hipLaunchKernelGGL((res_ln_quant_axis_k<DT, LPR, NV, IDXV>), dim3(g.grid), dim3(kBlock), 0, st, av, rv, yv, y_idx, rows, w, b, \
                     eps, c1, c2, c3, q1 != nullptr, q2 != nullptr, q3 != nullptr, g.nt, g.iters)
#define TQ_LNA(LPR, NV)                                                                                         \
  if constexpr ((uint64_t)(LPR) * (NV) * V <= kAxisMaxD) {                                                      \
    if (d == (uint64_t)(LPR) * (NV) * V) {                                                                      \
      const TailGeom g = tail_geom(rows, d, LPR, elem_size(DT));                                                \
      if (y_idx != nullptr) TQ_LNA_GO(LPR, NV, true);                                                           \
      else                  TQ_LNA_GO(LPR, NV, false);                                                          \
      return check_launch("res_ln_quant_axis_k");                                                               \
    }                                                                                                           \
  }
  TQ_TAIL_SHAPES(TQ_LNA)
#undef TQ_LNA
#undef TQ_LNA_GO
  return set_error(TQ_EUNSUPPORTED,
                   "tq_residual_layernorm_quant_axis_fwd: row length %llu has no instantiation (rows of 16 / 32 / 64 / 96 / 128 / "
                   "192 / 256 16-byte vectors, at most %llu columns: the per-column tables live in LDS)",
                   (unsigned long long)d, (unsigned long long)kAxisMaxD);
}

// ---------------------------------------------------------------------------------------------------
// BERT's embedding block behind per-column quantizers (tq_embeddings_layernorm_quant_axis_fwd, fp32): row r is
//     Q_out(LN(Q_sum2(Q_sum1(word[word_ids[r]] + type[type_ids[r]]) + pos[pos_ids[r]])))
// with the gather, the ONE fp32 addition in front of Q_sum1, the clamped read / NaN row / `bad` flag of an out-of-range id
// from the per-tensor tail's embedding mode (EmbArgs, ln_load_row<., ., ., true>) and the LDS tables, block-wide vote and row
// pieces of the per-column tail (the TQ_AXIS_* macros): the bits of res_ln_quant_axis_k on the gathered rows.  A kernel of its
// own, not another template parameter of res_ln_quant_axis_k / res_ln_axis_body (see TQ_GROUP_MASK: that moves the register
// allocation of the kernels that exist).  The gather is a dependent chain, id -> row address -> row: the first row's three
// ids are requested before anything else, its row loads go out right behind the parameter requests (the parameters'
// derivation and the barrier run under them), and the loop fetches the next row's ids and rows before it computes this one.
// The first row is read for every lane group, clamped to the last row (a group past the end computes nothing): loads that
// are not under a branch keep the order above.
template <int LPR, int NV, bool IDX, bool FAST, bool ALLON>
__device__ __forceinline__ void emb_ln_axis_body(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                 u32x4* __restrict__ y, int8_t* __restrict__ y_idx, uint64_t rows,
                                                 const float* s_w, const float* s_b, const float* s_q, const float* s_zp3,
                                                 float ln_eps, const AxisLim& lim, int on1_, int on2_, int on3_,
                                                 uint32_t iters, const EmbArgs& emb, u32x4 (&va)[NV], u32x4 (&vr)[NV],
                                                 u32x4 (&va2)[NV]) {
  const int on1 = ALLON ? 1 : on1_, on2 = ALLON ? 1 : on2_, on3 = ALLON ? 1 : on3_;
  constexpr int V = 4;
  constexpr int H = V / 2;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  constexpr int nt = 0;                             // the output is read by the first layer: no streaming stores
  const float *t1 = s_q, *t2 = s_q + 4 * d, *t3 = s_q + 8 * d;
  const int lane = threadIdx.x % LPR;
  const int sub = threadIdx.x / LPR;
  const float inv_d = 1.0f / (float)d;
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + sub;
  u32x4 na[NV], nr[NV], na2[NV];
  for (uint32_t it = 0; it < iters; ++it) {
    const uint64_t row = row0 + (uint64_t)it * RPB;
    if (row >= rows) break;
    const uint64_t base = row * (d / V);
    const uint64_t nrow = row + RPB;
    if (it + 1 < iters && nrow < rows) ln_load_row<TQ_F32, LPR, NV, true>(a, r, emb, nt, lane, nrow, na, nr, na2);
    f32x2 u[NV][H];
    f32x2 s2 = {0.f, 0.f}, s2b = {0.f, 0.f};
    bool lane_nan = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const uint32_t c0 = (v * LPR + lane) * V;
      float fa[V], f2[V], fr[V];
      Store<TQ_F32>::unpack(va[v], fa);
      Store<TQ_F32>::unpack(va2[v], f2);
      Store<TQ_F32>::unpack(vr[v], fr);
#pragma unroll
      for (int k = 0; k < V; ++k) fa[k] = fa[k] + f2[k];          // word row + token-type row: ONE fp32 addition in front of Q1
      TQ_AXIS_FRONT(fr)
#pragma unroll
      for (int j = 0; j < H; ++j) {
        if (j & 1) s2b = s2b + u[v][j];
        else s2 = s2 + u[v][j];
      }
    }
    TQ_ROW_STATISTICS(TQ_GROUP_MASK)
    const f32x2 m2 = {mean, mean}, r2 = {rstd, rstd};
    u32x4 packed[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const uint32_t c0 = (v * LPR + lane) * V;
      float o[V];
      struct alignas(V) { int8_t e[V]; } oi;
      TQ_AXIS_AFFINE_QOUT
#pragma unroll
      for (int j = 0; j < H; ++j) { o[2 * j] = t[j].x; o[2 * j + 1] = t[j].y; }
      packed[v] = Store<TQ_F32>::pack(o);
      if (IDX) *reinterpret_cast<decltype(oi)*>(y_idx + (base + v * LPR + lane) * V) = oi;
    }
    TQ_ROW_STORE(FAST && on3, TQ_NAN_ROW_F32)
#pragma unroll
    for (int v = 0; v < NV; ++v) { va[v] = na[v]; vr[v] = nr[v]; va2[v] = na2[v]; }
  }
}

// (Three prefetched rows beside the row in work: at d = 384 / 768 the allocator, left alone, takes 170-190 VGPRs where 168 are
// three waves per SIMD -- what the LDS tables of these widths allow -- so those instantiations ask for three; no spills.)
template <int LPR, int NV, bool IDX>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(NV == 3 ? 3 : 1))) void emb_ln_quant_axis_k(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                              u32x4* __restrict__ y, int8_t* __restrict__ y_idx, uint64_t rows,
                                                              const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                              float ln_eps, tq_quantizer q1, tq_quantizer q2, tq_quantizer q3,
                                                              int on1, int on2, int on3, uint32_t iters, EmbArgs emb) {
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * 4;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  static_assert(d <= kAxisMaxD, "per-column tables must fit in LDS");
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d], s_q[3 * 4 * d], s_zp3[IDX ? d : 4];
  u32x4 va[NV], vr[NV], va2[NV];
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + threadIdx.x / LPR;
  const uint64_t first = row0 < rows ? row0 : rows - 1;
  // the ids of the first row: the same three loads ln_load_row makes below, requested ahead of the parameters
  const int64_t ia = emb.a_rows[first], ia2 = emb.a2_rows[first], ir = emb.r_rows[first];
  TQ_AXIS_REQUEST
  ln_load_row<TQ_F32, LPR, NV, true>(a, r, emb, 0, threadIdx.x % LPR, first, va, vr, va2);
  (void)ia; (void)ia2; (void)ir;
  TQ_AXIS_DERIVE
  TQ_AXIS_STAGE
  if (fast && on1 && on2 && on3)
    emb_ln_axis_body<LPR, NV, IDX, true, true>(a, r, y, y_idx, rows, s_w, s_b, s_q, s_zp3, ln_eps, lim, 1, 1, 1, iters, emb, va, vr, va2);
  else if (fast)
    emb_ln_axis_body<LPR, NV, IDX, true, false>(a, r, y, y_idx, rows, s_w, s_b, s_q, s_zp3, ln_eps, lim, on1, on2, on3, iters, emb, va, vr, va2);
  else
    emb_ln_axis_body<LPR, NV, IDX, false, false>(a, r, y, y_idx, rows, s_w, s_b, s_q, s_zp3, ln_eps, lim, on1, on2, on3, iters, emb, va, vr, va2);
}

static int launch_emb_ln_axis(const float* word, const float* pos, float* y, int8_t* y_idx, uint64_t rows, uint64_t d,
                              const float* w, const float* b, float eps, const tq_quantizer* q1, const tq_quantizer* q2,
                              const tq_quantizer* q3, const EmbArgs& emb, hipStream_t st) {
  const tq_quantizer none{};
  const tq_quantizer &c1 = q1 ? *q1 : none, &c2 = q2 ? *q2 : none, &c3 = q3 ? *q3 : none;
  const auto av = reinterpret_cast<const u32x4*>(word);
  const auto rv = reinterpret_cast<const u32x4*>(pos);
  auto yv = reinterpret_cast<u32x4*>(y);
  // the fp32 shapes of the per-column tail: d = 64 / 128 / 256 / 384 / 512 / 768 / 1024; geometry as the per-tensor embedding launch
#define TQ_LNE_GO(LPR, NV, IDXV)                                                                                \
  hipLaunchKernelGGL((emb_ln_quant_axis_k<LPR, NV, IDXV>), dim3(g.grid), dim3(kBlock), 0, st, av, rv, yv, y_idx, rows, w, b, eps, \
                     c1, c2, c3, q1 != nullptr, q2 != nullptr, q3 != nullptr, g.iters, emb)
#define TQ_LNE(LPR, NV)                                                                                         \
  if constexpr ((uint64_t)(LPR) * (NV) * 4 <= kAxisMaxD) {                                                      \
    if (d == (uint64_t)(LPR) * (NV) * 4) {                                                                      \
      const TailGeom g = tail_geom(rows, d, LPR, 4);                                                            \
      if (y_idx != nullptr) TQ_LNE_GO(LPR, NV, true);                                                           \
      else                  TQ_LNE_GO(LPR, NV, false);                                                          \
      return check_launch("emb_ln_quant_axis_k");                                                               \
    }                                                                                                           \
  }
  TQ_TAIL_SHAPES(TQ_LNE)
#undef TQ_LNE
#undef TQ_LNE_GO
  return set_error(TQ_EUNSUPPORTED,
                   "tq_embeddings_layernorm_quant_axis_fwd: row length %llu has no instantiation (64 / 128 / 256 / 384 / 512 / "
                   "768 / 1024 columns: the per-column tables live in LDS)", (unsigned long long)d);
}

// ---------------------------------------------------------------------------------------------------
// The per-column fp32 LayerNorm tail with its residual as int8 INDICES (tq_residual_layernorm_quant_axis_ires_fwd): under the
// PEG recipe site x (the attention-output tail's per-column result) is read by the class-ordered integer Linear, as indices,
// and by the feed-forward tail, as residual -- which can dequantize the same indices in registers, so x never has to exist
// as fp32.  res_ln_axis_body's lane layout, per-column tables, block-wide vote, statistics and NaN rule (its row pieces, as
// the macros above), plus what res_ln_ires_body adds to the per-tensor tail: the residual row as 4 bytes per 16-byte column
// vector (IresRow / ires_load_row, first row requested by the kernel entry), its dequantization scale_c * (index - zp_c),
// one flag per row in and out, and y optional.  RK says how the residual arrives: 0 as fp32, 1 as indices on a per-tensor
// grid (scale and zero point in registers: the attention-output tail, whose residual is the previous layer's per-tensor
// output, keeps the axis kernel's LDS), 2 as indices on a per-column grid (two more floats per column, s_rq = [2][d]: 17
// floats per column with y_idx, 52 KB at d = 768 -- three blocks per CU like the axis kernel; at d = 1024 it would be 69.6 KB,
// more than a block may declare, so rows end at 768).
constexpr uint64_t kAxisIresMaxD = 768;

template <int LPR, int NV, int RK, bool WY, bool IDX, bool FAST, bool ALLON>
__device__ __forceinline__ void res_ln_axis_ires_body(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                      const uint32_t* __restrict__ ri, const uint8_t* __restrict__ rflag,
                                                      u32x4* __restrict__ y, int8_t* __restrict__ y_idx,
                                                      uint8_t* __restrict__ yflag, uint64_t rows, const float* s_w,
                                                      const float* s_b, const float* s_q, const float* s_zp3, const float* s_rq,
                                                      float ln_eps, const AxisLim& lim, float res_scale, float res_zp, int on1_,
                                                      int on2_, int on3_, int nt, uint32_t iters,
                                                      IresRow<LPR, NV, (RK != 0)>& cur) {
  constexpr bool RIDX = RK != 0;
  const int on1 = ALLON ? 1 : on1_, on2 = ALLON ? 1 : on2_, on3 = ALLON ? 1 : on3_;
  constexpr int V = 4;
  constexpr int H = 2;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  const float *t1 = s_q, *t2 = s_q + 4 * d, *t3 = s_q + 8 * d;
  const int lane = threadIdx.x % LPR;
  const int sub = threadIdx.x / LPR;
  const float inv_d = 1.0f / (float)d;
  const uint64_t grp = TQ_GROUP_MASK;
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + sub;
  IresRow<LPR, NV, RIDX> nxt;
  for (uint32_t it = 0; it < iters; ++it) {
    const uint64_t row = row0 + (uint64_t)it * RPB;
    if (row >= rows) break;
    const uint64_t base = row * (d / V);
    const uint64_t nrow = row + RPB;
    if (it + 1 < iters && nrow < rows) ires_load_row<LPR, NV, RIDX>(a, r, ri, rflag, nt, lane, nrow, nxt);
    // the residual row of this lane as fp32: the producer's bits
    float fr[NV][V];
    if (RIDX) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const uint32_t w = cur.ri[v] ^ 0x80808080u;                 // int8(index - 128) -> index, four at a time
        const float x[V] = {(float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu), (float)(w >> 24)};
        if (RK == 2) {
          const uint32_t c0 = (v * LPR + lane) * V;
          const f32x4 sc = *reinterpret_cast<const f32x4*>(s_rq + c0), zp = *reinterpret_cast<const f32x4*>(s_rq + d + c0);
#pragma unroll
          for (int k = 0; k < V; ++k) fr[v][k] = sc[k] * (x[k] - zp[k]);
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) fr[v][k] = res_scale * (x[k] - res_zp);
        }
      }
      if (__ballot(cur.flag != 0)) {               // rare: a NaN row arrives as its flag, its indices mean nothing
        if (cur.flag != 0) {
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int k = 0; k < V; ++k) fr[v][k] = __builtin_nanf("");
        }
      }
    } else {
#pragma unroll
      for (int v = 0; v < NV; ++v) Store<TQ_F32>::unpack(cur.r[v], fr[v]);
    }
    f32x2 u[NV][H];
    f32x2 s2 = {0.f, 0.f}, s2b = {0.f, 0.f};
    bool lane_nan = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const uint32_t c0 = (v * LPR + lane) * V;
      float fa[V];
      Store<TQ_F32>::unpack(cur.a[v], fa);
      TQ_AXIS_FRONT(fr[v])
#pragma unroll
      for (int j = 0; j < H; ++j) {
        if (j & 1) s2b = s2b + u[v][j];
        else s2 = s2 + u[v][j];
      }
    }
    TQ_ROW_STATISTICS(grp)
    const f32x2 m2 = {mean, mean}, r2 = {rstd, rstd};
    u32x4 packed[WY ? NV : 1];
    // as in res_ln_ires_body: outside the exact path behind Q_out a row is NaN where its outputs are
    bool out_nan = false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const uint32_t c0 = (v * LPR + lane) * V;
      float o[V];
      struct alignas(V) { int8_t e[V]; } oi;
      TQ_AXIS_AFFINE_QOUT
      if (!(FAST && ALLON)) {
        if (!(FAST && on3)) {
#pragma unroll
          for (int j = 0; j < H; ++j) out_nan = out_nan || t[j].x != t[j].x || t[j].y != t[j].y;
        }
      }
      if (WY) {
#pragma unroll
        for (int j = 0; j < H; ++j) { o[2 * j] = t[j].x; o[2 * j + 1] = t[j].y; }
        packed[v] = Store<TQ_F32>::pack(o);
      }
      if (IDX) *reinterpret_cast<decltype(oi)*>(y_idx + (base + v * LPR + lane) * V) = oi;
    }
    if (WY) {
      TQ_ROW_STORE(FAST && on3, TQ_NAN_ROW_F32)
    }
    if (yflag != nullptr) {                               // one ordinary byte store per row
      if (!(FAST && ALLON)) row_nan = row_nan || (__ballot(out_nan) & grp) != 0;
      if (lane == 0) yflag[row] = row_nan ? 1 : 0;
    }
    cur = nxt;
  }
}

template <int LPR, int NV, int RK, bool WY, bool IDX>
__global__ __launch_bounds__(kBlock) void res_ln_quant_axis_ires_k(const u32x4* __restrict__ a, const u32x4* __restrict__ r,
                                                                   const uint32_t* __restrict__ ri,
                                                                   const uint8_t* __restrict__ rflag, u32x4* __restrict__ y,
                                                                   int8_t* __restrict__ y_idx, uint8_t* __restrict__ yflag,
                                                                   uint64_t rows, const float* __restrict__ ln_w,
                                                                   const float* __restrict__ ln_b, float ln_eps, tq_quantizer q1,
                                                                   tq_quantizer q2, tq_quantizer q3, tq_quantizer qr, int on1,
                                                                   int on2, int on3, int nt, uint32_t iters) {
  // res_ln_quant_axis_k's prologue; the residual's grid is requested with the rest: one parameter pair into registers (RK = 1),
  // or this thread's columns for the table (RK = 2)
  constexpr int V = 4;
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t d = LPR * NV * V;
  constexpr int NA = (d + kBlock - 1) / kBlock;
  static_assert(d <= kAxisIresMaxD, "per-column tables must fit in LDS");
  __shared__ __attribute__((aligned(16))) float s_w[d], s_b[d], s_q[3 * 4 * d], s_zp3[IDX ? d : 4], s_rq[RK == 2 ? 2 * d : 4];
  IresRow<LPR, NV, (RK != 0)> cur;
  const uint64_t row0 = (uint64_t)blockIdx.x * RPB * iters + threadIdx.x / LPR;
  if (row0 < rows) ires_load_row<LPR, NV, (RK != 0)>(a, r, ri, rflag, nt, threadIdx.x % LPR, row0, cur);
  TQ_AXIS_REQUEST
  float qd[NA], qz[NA];
  QRaw wr = {1.f, 0.f, 0u};
  if (RK == 2) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const uint32_t c = threadIdx.x + i * kBlock;
      axis_load_raw(qr, c < d ? c : d - 1, ln_w, qd[i], qz[i]);
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) { pin_lane(qd[i]); pin_lane(qz[i]); }
  } else if (RK == 1) {
    wr = load_qraw(qr, 0, ln_w);
    qraw_arrived(wr);
  }
  TQ_AXIS_DERIVE
  const QP pr = RK == 1 ? qp_from_raw(qr, wr) : QP{1.f, 0.f, 0.f, 0.f};
  if (RK == 2) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const uint32_t c = threadIdx.x + i * kBlock;
      if (c < d) {
        const QP p = qp_from_raw(qr, QRaw{qd[i], qz[i], 0u});
        s_rq[c] = p.scale;
        s_rq[d + c] = p.zp;
      }
    }
  }
  TQ_AXIS_STAGE
  if (fast && on1 && on2 && on3)
    res_ln_axis_ires_body<LPR, NV, RK, WY, IDX, true, true>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, s_q, s_zp3, s_rq, ln_eps, lim, pr.scale, pr.zp, 1, 1, 1, nt, iters, cur);
  else if (fast)
    res_ln_axis_ires_body<LPR, NV, RK, WY, IDX, true, false>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, s_q, s_zp3, s_rq, ln_eps, lim, pr.scale, pr.zp, on1, on2, on3, nt, iters, cur);
  else
    res_ln_axis_ires_body<LPR, NV, RK, WY, IDX, false, false>(a, r, ri, rflag, y, y_idx, yflag, rows, s_w, s_b, s_q, s_zp3, s_rq, ln_eps, lim, pr.scale, pr.zp, on1, on2, on3, nt, iters, cur);
}

// The (RK, WY, IDX) forms: the residual as fp32, as indices on a per-tensor grid or as indices on a per-column grid, times
// y_idx alone, y with y_idx, and y alone.  Geometry as every tail's (tail_geom).
#define TQ_AXIS_IRES_FORMS(X, LPR, NV)                                                                          \
  X(LPR, NV, 0, false, true) X(LPR, NV, 0, true, true) X(LPR, NV, 0, true, false)                               \
  X(LPR, NV, 1, false, true) X(LPR, NV, 1, true, true) X(LPR, NV, 1, true, false)                               \
  X(LPR, NV, 2, false, true) X(LPR, NV, 2, true, true) X(LPR, NV, 2, true, false)

template <int DT>
static int launch_res_ln_axis_ires(const char* who, const float* a, const float* r, const int8_t* ri, const uint8_t* rflag,
                                   float* y, int8_t* y_idx, uint8_t* yflag, uint64_t rows, uint64_t d, const float* w,
                                   const float* b, float eps, const tq_quantizer* q1, const tq_quantizer* q2,
                                   const tq_quantizer* q3, const tq_quantizer* qr, hipStream_t st) {
  const tq_quantizer none{};
  const tq_quantizer &c1 = q1 ? *q1 : none, &c2 = q2 ? *q2 : none, &c3 = q3 ? *q3 : none, &cr = qr ? *qr : none;
  const auto av = reinterpret_cast<const u32x4*>(a);
  const auto rv = reinterpret_cast<const u32x4*>(r);
  const auto iv = reinterpret_cast<const uint32_t*>(ri);
  auto yv = reinterpret_cast<u32x4*>(y);
  const int rk = ri == nullptr ? 0 : cr.n_params == 1 ? 1 : 2;
  const bool wy = y != nullptr, idx = y_idx != nullptr;
  constexpr int V = Store<DT>::kVec;
  static_assert(DT == TQ_F32, "fp32 rows only");
#define TQ_LNAI_GO(LPR, NV, RKV, WYV, IDXV)                                                                     \
  if (rk == RKV && wy == WYV && idx == IDXV) {                                                                  \
    hipLaunchKernelGGL((res_ln_quant_axis_ires_k<LPR, NV, RKV, WYV, IDXV>), dim3(g.grid), dim3(kBlock), 0, st, av, rv, iv, rflag, \
                       yv, y_idx, yflag, rows, w, b, eps, c1, c2, c3, cr, q1 != nullptr, q2 != nullptr, q3 != nullptr, g.nt,    \
                       g.iters);                                                                                \
    return check_launch("res_ln_quant_axis_ires_k");                                                            \
  }
#define TQ_LNAI(LPR, NV)                                                                                        \
  if constexpr ((uint64_t)(LPR) * (NV) * V <= kAxisIresMaxD) {                                                  \
    if (d == (uint64_t)(LPR) * (NV) * V) {                                                                      \
      const TailGeom g = tail_geom(rows, d, LPR, 4);                                                            \
      TQ_AXIS_IRES_FORMS(TQ_LNAI_GO, LPR, NV)                                                                   \
    }                                                                                                           \
  }
  TQ_TAIL_SHAPES(TQ_LNAI)
#undef TQ_LNAI
#undef TQ_LNAI_GO
  return set_error(TQ_EUNSUPPORTED, "%s: row length %llu has no instantiation (fp32 rows of d = 64, 128, 256, 384, 512 or 768)",
                   who, (unsigned long long)d);
}

// ---------------------------------------------------------------------------------------------------
// Attention probabilities with fixed ranges (reference models/quantized_bert.py:153-198):
//     p = Q_probs( softmax( Q_scores(scores) / denom + mask , dim=-1 ) )
// = quantizer, division, mask add, softmax, quantizer: five sweeps of [B, H, T, T] in the reference,
// here 1 read + 1 write.  LPR lanes own one row of T = LPR * NV * 4 fp32 values.
// Branch-free exact variant of the element math (both quantizers on, tq_device.h QF): ~30 VALU issue slots per element
// instead of ~75 with four IEEE divisions -- the scalar version was VALU-bound at 40 % of the HBM rate.
//   scores quantizer, probs quantizer: QF pairs (med3 clamp + Markstein quotient);
//   t / denom: Markstein with rd = RN(1 / denom): the operand is a grid value (>= 2^-60 or 0, < 2^82), so the fma
//     residual is exact and the quotient correctly rounded -- the same value v_div_* returns;
//   e / sum: the same with rs = RN(1 / sum), one IEEE division per row.  1 <= sum <= T and e in [0, 1]: the residual
//     is exact for e >= 2^-62; below that the probability is < scale / 4 and the probs quantizer returns index 0
//     whatever the last bit of the quotient (which is why this path needs the probs quantizer).
// NaN: v_med3 does not keep it, so a NaN score poisons the row sum (the reference's row is NaN as a whole) and rows
// with a NaN sum are patched after the last quantizer.
__device__ __forceinline__ bool softmax_fast_ok(const tq_quantizer& q1, const tq_quantizer& q2, int on1, int on2, float denom) {
  if (!on1 || !on2) return false;
  // (make_qp's select form in the softmax chain: with the branch form of round 6 the [256,12,128,128] launch went from 75 to
  // 82-86 us in the kernel table; 86 -> 80 us on one box with the select, profiles/r06/softmax_select_ab.txt)
  const QP p1 = make_qp<true>(q1, 0), p2 = make_qp<true>(q2, 0);
  const float ad = fabsf(denom);
  return make_qf(p1).ok && make_qf(p2).ok && p1.scale >= 0x1p-60f && p1.scale <= 0x1p60f && p2.scale >= 0x1p-60f &&
         p2.scale <= 0x1p60f && ad >= 0x1p-20f && ad <= 0x1p20f;
}

template <int LPR, int NV, int R>
__device__ __forceinline__ void softmax_fast_body(const f32x4* __restrict__ s, f32x4* __restrict__ y, uint64_t rows,
                                                  const float* __restrict__ mask, uint64_t rows_per_mask, float denom,
                                                  const tq_quantizer& q1, const tq_quantizer& q2) {
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t T4 = LPR * NV;
  constexpr int P = NV * 2;                      // pairs per lane and row
  const QF f1 = make_qf(make_qp<true>(q1, 0)), f2 = make_qf(make_qp<true>(q2, 0));
  const float rdv = 1.0f / denom;
  const f32x2 rd = {rdv, rdv}, nd = {-denom, -denom};
  const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
  for (uint64_t row0 = ((uint64_t)blockIdx.x * RPB + sub) * R; row0 < rows; row0 += (uint64_t)gridDim.x * RPB * R) {
    f32x4 in[R][NV], mk[R][NV];
    const uint64_t m0 = mask ? row0 / rows_per_mask : 0, rem0 = row0 - m0 * rows_per_mask;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t row = row0 + r < rows ? row0 + r : rows - 1;
      const uint64_t mi = rem0 + r < rows_per_mask ? m0 : row / rows_per_mask;
      const f32x4* mrow = mask ? reinterpret_cast<const f32x4*>(mask + mi * (uint64_t)T4 * 4) : nullptr;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        in[r][k] = s[row * T4 + k * LPR + lane];
        mk[r][k] = mrow ? mrow[k * LPR + lane] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    f32x2 t[R][P];
    float mx[R], sum[R];
    bool bad[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      bad[r] = false;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        bad[r] = bad[r] || in[r][k][0] != in[r][k][0] || in[r][k][1] != in[r][k][1] || in[r][k][2] != in[r][k][2] ||
                 in[r][k][3] != in[r][k][3];
        t[r][2 * k] = f32x2{in[r][k][0], in[r][k][1]};
        t[r][2 * k + 1] = f32x2{in[r][k][2], in[r][k][3]};
      }
      qf_fake_quant2_n<P>(t[r], f1);
      f32x2 q0[P], e[P];
#pragma unroll
      for (int i = 0; i < P; ++i) q0[i] = t[r][i] * rd;
#pragma unroll
      for (int i = 0; i < P; ++i) e[i] = __builtin_elementwise_fma(q0[i], nd, t[r][i]);
#pragma unroll
      for (int i = 0; i < P; ++i) t[r][i] = __builtin_elementwise_fma(e[i], rd, q0[i]);
      if (mask) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          t[r][2 * k] = t[r][2 * k] + f32x2{mk[r][k][0], mk[r][k][1]};
          t[r][2 * k + 1] = t[r][2 * k + 1] + f32x2{mk[r][k][2], mk[r][k][3]};
        }
      }
      mx[r] = -__builtin_huge_valf();
#pragma unroll
      for (int i = 0; i < P; ++i) mx[r] = max_raw(mx[r], max_raw(t[r][i].x, t[r][i].y));
    }
#pragma unroll
    for (int r = 0; r < R; ++r) mx[r] = group_max<LPR>(mx[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      sum[r] = 0.f;
#pragma unroll
      for (int i = 0; i < P; ++i) {
        t[r][i].x = exp_nonpos_fast(t[r][i].x - mx[r]);      // tolerance contract (see tq_device.h), ~8 slots instead of ~13
        t[r][i].y = exp_nonpos_fast(t[r][i].y - mx[r]);
        sum[r] += t[r][i].x;             // the scalar kernel's (and the oracle's) left-to-right order
        sum[r] += t[r][i].y;
      }
      if (bad[r]) sum[r] = __builtin_nanf("");
    }
#pragma unroll
    for (int r = 0; r < R; ++r) sum[r] = group_sum<LPR>(sum[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float rsv = 1.0f / sum[r];
      const f32x2 rs = {rsv, rsv}, ns = {-sum[r], -sum[r]};
      f32x2 q0[P], e[P];
#pragma unroll
      for (int i = 0; i < P; ++i) q0[i] = t[r][i] * rs;
#pragma unroll
      for (int i = 0; i < P; ++i) e[i] = __builtin_elementwise_fma(q0[i], ns, t[r][i]);
#pragma unroll
      for (int i = 0; i < P; ++i) t[r][i] = __builtin_elementwise_fma(e[i], rs, q0[i]);
      qf_fake_quant2_n<P>(t[r], f2);
      if (__ballot(sum[r] != sum[r])) {          // rare: a NaN row
        if (sum[r] != sum[r]) {
#pragma unroll
          for (int i = 0; i < P; ++i) t[r][i] = f32x2{__builtin_nanf(""), __builtin_nanf("")};
        }
      }
      if (row0 + r >= rows) continue;
#pragma unroll
      for (int k = 0; k < NV; ++k)
        y[(row0 + r) * T4 + k * LPR + lane] = f32x4{t[r][2 * k].x, t[r][2 * k].y, t[r][2 * k + 1].x, t[r][2 * k + 1].y};
    }
  }
}

template <int LPR, int NV, int R>
__global__ __launch_bounds__(kBlock) void softmax_quant_k(const f32x4* __restrict__ s, f32x4* __restrict__ y, uint64_t rows,
                                                          const float* __restrict__ mask, uint64_t rows_per_mask,
                                                          float denom, tq_quantizer q1, tq_quantizer q2, int on1, int on2,
                                                          int allow_fast) {
  // R rows per lane group and step: R independent load -> reduce -> exp -> reduce -> store chains in flight
  if (allow_fast && softmax_fast_ok(q1, q2, on1, on2, denom)) {          // wave-uniform
    softmax_fast_body<LPR, NV, R>(s, y, rows, mask, rows_per_mask, denom, q1, q2);
    return;
  }
  constexpr int RPB = kBlock / LPR;
  constexpr uint32_t T4 = LPR * NV;              // float4 vectors per row
  const FusedQ f1 = make_fq(q1, on1), f2 = make_fq(q2, on2);
  const int lane = threadIdx.x % LPR, sub = threadIdx.x / LPR;
  for (uint64_t row0 = ((uint64_t)blockIdx.x * RPB + sub) * R; row0 < rows; row0 += (uint64_t)gridDim.x * RPB * R) {
    f32x4 in[R][NV], mk[R][NV];
    const uint64_t m0 = mask ? row0 / rows_per_mask : 0, rem0 = row0 - m0 * rows_per_mask;   // one 64-bit division per step
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t row = row0 + r < rows ? row0 + r : rows - 1;        // clamp: tail rows recompute the last one
      const uint64_t mi = rem0 + r < rows_per_mask ? m0 : row / rows_per_mask;
      const f32x4* mrow = mask ? reinterpret_cast<const f32x4*>(mask + mi * (uint64_t)T4 * 4) : nullptr;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        in[r][k] = s[row * T4 + k * LPR + lane];
        mk[r][k] = mrow ? mrow[k * LPR + lane] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    float v[R][NV][4], mx[R], sum[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      mx[r] = -__builtin_huge_valf();
#pragma unroll
      for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float t = apply_q(in[r][k][j], f1) / denom;
          if (mask) t = t + mk[r][k][j];
          v[r][k][j] = t;
          mx[r] = fmaxf(mx[r], t);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) mx[r] = group_max<LPR>(mx[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      sum[r] = 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[r][k][j] = expf(v[r][k][j] - mx[r]); sum[r] += v[r][k][j]; }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) sum[r] = group_sum<LPR>(sum[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (row0 + r >= rows) continue;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = apply_q(v[r][k][j] / sum[r], f2);
        y[(row0 + r) * T4 + k * LPR + lane] = o;
      }
    }
  }
}

}  // namespace tq

using namespace tq;

// ---- argument checks the tail entries share ----
static int check_tensor_quantizers(const char* who, std::initializer_list<const tq_quantizer*> qs, uint64_t n) {
  for (const tq_quantizer* q : qs)
    if (q != nullptr) {
      if (int e = check_quantizer(q, n, who)) return e;
      TQ_REQUIRE(q->n_params == 1, "%s: per-tensor quantizers only", who);
    }
  return TQ_OK;
}

// The quantizers of the per-column tails: per-tensor, or one parameter per column in natural order.
static int check_column_quantizers(const char* who, std::initializer_list<const tq_quantizer*> qs, uint64_t rows, uint64_t d) {
  for (const tq_quantizer* q : qs)
    if (q != nullptr) {
      if (int e = check_quantizer(q, rows * d, who)) return e;
      TQ_REQUIRE(q->n_params == 1 || (q->n_params == d && q->inner == 1),
                 "%s: quantizers are per-tensor (n_params = 1) or per-column (n_params = d = %llu, inner = 1); got n_params = %llu, "
                 "inner = %llu", who, (unsigned long long)d, (unsigned long long)q->n_params, (unsigned long long)q->inner);
      TQ_REQUIRE((reinterpret_cast<uintptr_t>(q->delta) & 3u) == 0 && (reinterpret_cast<uintptr_t>(q->zero_float) & 3u) == 0,
                 "%s: quantizer parameters must be 4-byte aligned", who);
    }
  return TQ_OK;
}

// y_idx is int8(index - 128): an asymmetric grid of at most 8 bits.  align8: the kernels that store 8 indices at once.
static int check_y_idx(const char* who, const int8_t* y_idx, const tq_quantizer* q_out, bool align8) {
  TQ_REQUIRE(y_idx == nullptr || (q_out != nullptr && !q_out->symmetric && q_out->n_bits <= 8 &&
                                  (!align8 || (reinterpret_cast<uintptr_t>(y_idx) & 7u) == 0)),
             align8 ? "%s: y_idx needs an asymmetric <= 8-bit output quantizer and 8-byte alignment"
                    : "%s: y_idx needs an asymmetric <= 8-bit output quantizer", who);
  return TQ_OK;
}

// A grid whose index goes out as two byte planes: asymmetric, linear domain, 1..16 bits.
static bool plane_grid(const tq_quantizer* q) {
  return q != nullptr && !q->symmetric && !q->log_domain && q->n_bits >= 1 && q->n_bits <= 16 && q->zero_float != nullptr;
}

// The grid of a residual that arrives as indices or planes (`what` names them in the message).
static int check_q_res(const char* who, const char* what, const tq_quantizer* q_res, int max_bits, uint64_t n) {
  TQ_REQUIRE(q_res != nullptr && q_res->delta != nullptr && q_res->zero_float != nullptr, "%s: %s (q_res)", who, what);
  TQ_REQUIRE(!q_res->symmetric && !q_res->log_domain && q_res->n_params == 1 && q_res->n_bits >= 1 && q_res->n_bits <= max_bits,
             "%s: q_res must be a per-tensor asymmetric linear-domain quantizer with n_bits <= %d", who, max_bits);
  return check_quantizer(q_res, n, who);
}

static int residual_tail(const char* who, const void* dense_out, const void* residual, void* y, int8_t* y_idx, uint64_t rows,
                         uint64_t d, int dtype, const tq_quantizer* q_dense, const tq_quantizer* q_sum, const float* weight,
                         const float* bias, float ln_eps, const tq_quantizer* q_out, int affine_only, tq_stream_t stream) {
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(dense_out && residual && y && weight && bias, "%s: NULL pointer", who);
  TQ_REQUIRE(dtype == TQ_F32 || dtype == TQ_BF16 || dtype == TQ_F16, "%s: bad dtype %d", who, dtype);
  TQ_REQUIRE(aligned16(dense_out) && aligned16(residual) && aligned16(y), "%s: 16-byte alignment required", who);
  if (int e = check_y_idx(who, y_idx, q_out, true)) return e;
  if (int e = check_tensor_quantizers(who, {q_dense, q_sum, q_out}, rows * d)) return e;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case TQ_F32: return launch_res_ln<TQ_F32>(dense_out, residual, y, y_idx, rows, d, weight, bias, ln_eps, q_dense, q_sum, q_out, affine_only, st);
    case TQ_BF16: return launch_res_ln<TQ_BF16>(dense_out, residual, y, y_idx, rows, d, weight, bias, ln_eps, q_dense, q_sum, q_out, affine_only, st);
    default: return launch_res_ln<TQ_F16>(dense_out, residual, y, y_idx, rows, d, weight, bias, ln_eps, q_dense, q_sum, q_out, affine_only, st);
  }
}

extern "C" int tq_residual_layernorm_quant_fwd(const void* dense_out, const void* residual, void* y, int8_t* y_idx, uint64_t rows,
                                               uint64_t d, int dtype, const tq_quantizer* q_dense,
                                               const tq_quantizer* q_sum, const float* ln_weight, const float* ln_bias,
                                               float ln_eps, const tq_quantizer* q_out, tq_stream_t stream) {
  return residual_tail("tq_residual_layernorm_quant_fwd", dense_out, residual, y, y_idx, rows, d, dtype, q_dense, q_sum, ln_weight,
                       ln_bias, ln_eps, q_out, 0, stream);
}

extern "C" int tq_residual_layernorm_quant_axis_fwd(const void* dense_out, const void* residual, void* y, int8_t* y_idx,
                                                    uint64_t rows, uint64_t d, int dtype, const tq_quantizer* q_dense,
                                                    const tq_quantizer* q_sum, const float* ln_weight, const float* ln_bias,
                                                    float ln_eps, const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_residual_layernorm_quant_axis_fwd";
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(dense_out && residual && y && ln_weight && ln_bias, "%s: NULL pointer", who);
  TQ_REQUIRE(dtype == TQ_F32 || dtype == TQ_BF16 || dtype == TQ_F16, "%s: bad dtype %d", who, dtype);
  TQ_REQUIRE(d >= 1, "%s: d == 0", who);
  TQ_REQUIRE(aligned16(dense_out) && aligned16(residual) && aligned16(y), "%s: 16-byte alignment required", who);
  if (int e = check_y_idx(who, y_idx, q_out, true)) return e;
  if (int e = check_column_quantizers(who, {q_dense, q_sum, q_out}, rows, d)) return e;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case TQ_F32: return launch_res_ln_axis<TQ_F32>(dense_out, residual, y, y_idx, rows, d, ln_weight, ln_bias, ln_eps, q_dense, q_sum, q_out, st);
    case TQ_BF16: return launch_res_ln_axis<TQ_BF16>(dense_out, residual, y, y_idx, rows, d, ln_weight, ln_bias, ln_eps, q_dense, q_sum, q_out, st);
    default: return launch_res_ln_axis<TQ_F16>(dense_out, residual, y, y_idx, rows, d, ln_weight, ln_bias, ln_eps, q_dense, q_sum, q_out, st);
  }
}

extern "C" int tq_residual_layernorm_quant_ires_fwd(const float* dense_out, const float* residual, const int8_t* res_idx,
                                                    const tq_quantizer* q_res, const uint8_t* res_row_nan, float* y,
                                                    int8_t* y_idx, uint8_t* y_row_nan, uint64_t rows, uint64_t d,
                                                    const tq_quantizer* q_dense, const tq_quantizer* q_sum,
                                                    const float* ln_weight, const float* ln_bias, float ln_eps,
                                                    const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_residual_layernorm_quant_ires_fwd";
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(dense_out && ln_weight && ln_bias, "%s: NULL pointer", who);
  TQ_REQUIRE((residual != nullptr) != (res_idx != nullptr), "%s: the residual comes as fp32 values or as int8 indices, one of the two", who);
  TQ_REQUIRE(res_row_nan == nullptr || res_idx != nullptr, "%s: res_row_nan goes with res_idx", who);
  TQ_REQUIRE(y != nullptr || y_idx != nullptr, "%s: y == NULL needs y_idx", who);
  if (int e = check_y_idx(who, y_idx, q_out, false)) return e;
  if (res_idx != nullptr)
    if (int e = check_q_res(who, "res_idx needs its grid", q_res, 8, rows * d)) return e;
  TQ_REQUIRE(aligned16(dense_out) && (residual == nullptr || aligned16(residual)) && (y == nullptr || aligned16(y)),
             "%s: 16-byte alignment required", who);
  TQ_REQUIRE((reinterpret_cast<uintptr_t>(res_idx) & 3u) == 0 && (reinterpret_cast<uintptr_t>(y_idx) & 3u) == 0,
             "%s: index arrays must be 4-byte aligned", who);
  if (int e = check_tensor_quantizers(who, {q_dense, q_sum, q_out}, rows * d)) return e;
  return launch_res_ln_ires(who, dense_out, residual, res_idx, nullptr, nullptr, res_row_nan, y, y_idx, nullptr, nullptr, y_row_nan,
                            rows, d, ln_weight, ln_bias, ln_eps, q_dense, q_sum, q_out, res_idx != nullptr ? q_res : nullptr,
                            static_cast<hipStream_t>(stream));
}

extern "C" int tq_residual_layernorm_quant_axis_ires_fwd(const float* dense_out, const float* residual, const int8_t* res_idx,
                                                         const tq_quantizer* q_res, const uint8_t* res_row_nan, float* y,
                                                         int8_t* y_idx, uint8_t* y_row_nan, uint64_t rows, uint64_t d,
                                                         const tq_quantizer* q_dense, const tq_quantizer* q_sum,
                                                         const float* ln_weight, const float* ln_bias, float ln_eps,
                                                         const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_residual_layernorm_quant_axis_ires_fwd";
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(dense_out && ln_weight && ln_bias, "%s: NULL pointer", who);
  TQ_REQUIRE(d >= 1, "%s: d == 0", who);
  TQ_REQUIRE((residual != nullptr) != (res_idx != nullptr), "%s: the residual comes as fp32 values or as int8 indices, one of the two", who);
  TQ_REQUIRE(res_row_nan == nullptr || res_idx != nullptr, "%s: res_row_nan goes with res_idx", who);
  TQ_REQUIRE(y != nullptr || y_idx != nullptr, "%s: y == NULL needs y_idx", who);
  if (int e = check_y_idx(who, y_idx, q_out, false)) return e;
  if (res_idx != nullptr) {
    TQ_REQUIRE(q_res != nullptr && q_res->delta != nullptr && q_res->zero_float != nullptr, "%s: res_idx needs its grid (q_res)", who);
    TQ_REQUIRE(!q_res->symmetric && !q_res->log_domain && q_res->n_bits >= 1 && q_res->n_bits <= 8 &&
                   (q_res->n_params == 1 || (q_res->n_params == d && q_res->inner == 1)),
               "%s: q_res must be an asymmetric linear-domain quantizer with n_bits <= 8, per-tensor (n_params = 1) or per-column "
               "(n_params = d = %llu, inner = 1)", who, (unsigned long long)d);
  }
  TQ_REQUIRE(aligned16(dense_out) && (residual == nullptr || aligned16(residual)) && (y == nullptr || aligned16(y)),
             "%s: 16-byte alignment required", who);
  TQ_REQUIRE((reinterpret_cast<uintptr_t>(res_idx) & 3u) == 0 && (reinterpret_cast<uintptr_t>(y_idx) & 3u) == 0,
             "%s: index arrays must be 4-byte aligned", who);
  for (const tq_quantizer* q : {q_dense, q_sum, q_out, res_idx != nullptr ? q_res : nullptr})
    if (q != nullptr) {
      if (int e = check_quantizer(q, rows * d, who)) return e;
      TQ_REQUIRE(q->n_params == 1 || (q->n_params == d && q->inner == 1),
                 "%s: quantizers are per-tensor (n_params = 1) or per-column (n_params = d = %llu, inner = 1); got n_params = %llu, "
                 "inner = %llu", who, (unsigned long long)d, (unsigned long long)q->n_params, (unsigned long long)q->inner);
      TQ_REQUIRE((reinterpret_cast<uintptr_t>(q->delta) & 3u) == 0 && (reinterpret_cast<uintptr_t>(q->zero_float) & 3u) == 0,
                 "%s: quantizer parameters must be 4-byte aligned", who);
    }
  return launch_res_ln_axis_ires<TQ_F32>(who, dense_out, residual, res_idx, res_row_nan, y, y_idx, y_row_nan, rows, d, ln_weight,
                                         ln_bias, ln_eps, q_dense, q_sum, q_out, res_idx != nullptr ? q_res : nullptr,
                                         static_cast<hipStream_t>(stream));
}

extern "C" int tq_residual_layernorm_quant_planes_fwd(const float* dense_out, const float* residual, float* y, int8_t* y_hi,
                                                      int8_t* y_lo, uint64_t rows, uint64_t d, const tq_quantizer* q_dense,
                                                      const tq_quantizer* q_sum, const float* ln_weight, const float* ln_bias,
                                                      float ln_eps, const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_residual_layernorm_quant_planes_fwd";
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(dense_out && residual && y && y_hi && y_lo && ln_weight && ln_bias, "%s: NULL pointer", who);
  TQ_REQUIRE(q_out != nullptr, "%s: the byte planes need an output quantizer", who);
  TQ_REQUIRE(aligned16(dense_out) && aligned16(residual) && aligned16(y), "%s: 16-byte alignment required", who);
  TQ_REQUIRE((reinterpret_cast<uintptr_t>(y_hi) & 3u) == 0 && (reinterpret_cast<uintptr_t>(y_lo) & 3u) == 0,
             "%s: the byte planes must be 4-byte aligned", who);
  if (int e = check_tensor_quantizers(who, {q_dense, q_sum, q_out}, rows * d)) return e;
  TQ_REQUIRE(plane_grid(q_out), "%s: q_out must be a per-tensor asymmetric linear-domain quantizer of 1..16 bits", who);
  return launch_res_ln_ires(who, dense_out, residual, nullptr, nullptr, nullptr, nullptr, y, nullptr, y_hi, y_lo, nullptr, rows, d,
                            ln_weight, ln_bias, ln_eps, q_dense, q_sum, q_out, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int tq_residual_layernorm_quant_pres_fwd(const float* dense_out, const float* residual, const int8_t* res_idx,
                                                    const int8_t* res_hi, const int8_t* res_lo, const tq_quantizer* q_res,
                                                    const uint8_t* res_row_nan, float* y, int8_t* y_idx, int8_t* y_hi,
                                                    int8_t* y_lo, uint8_t* y_row_nan, uint64_t rows, uint64_t d,
                                                    const tq_quantizer* q_dense, const tq_quantizer* q_sum,
                                                    const float* ln_weight, const float* ln_bias, float ln_eps,
                                                    const tq_quantizer* q_out, tq_stream_t stream) {
  const char* who = "tq_residual_layernorm_quant_pres_fwd";
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(dense_out && ln_weight && ln_bias, "%s: NULL pointer", who);
  TQ_REQUIRE((res_hi != nullptr) == (res_lo != nullptr), "%s: the residual's byte planes come as a pair (res_hi and res_lo)", who);
  TQ_REQUIRE((residual != nullptr) + (res_idx != nullptr) + (res_hi != nullptr) == 1,
             "%s: the residual comes as fp32 values, as int8 indices or as byte planes, exactly one of the three", who);
  TQ_REQUIRE(res_row_nan == nullptr || residual == nullptr, "%s: res_row_nan goes with res_idx or with the planes", who);
  TQ_REQUIRE((y_hi != nullptr) == (y_lo != nullptr), "%s: the output's byte planes come as a pair (y_hi and y_lo)", who);
  TQ_REQUIRE(y != nullptr || y_idx != nullptr || y_hi != nullptr, "%s: nothing to write (y, y_idx or y_hi / y_lo)", who);
  if (int e = check_y_idx(who, y_idx, q_out, false)) return e;
  TQ_REQUIRE(y_hi == nullptr || plane_grid(q_out),
             "%s: y_hi / y_lo need a per-tensor asymmetric linear-domain output quantizer of 1..16 bits", who);
  if (residual == nullptr)
    if (int e = check_q_res(who, "res_idx and the planes need their grid", q_res, res_idx != nullptr ? 8 : 16, rows * d)) return e;
  TQ_REQUIRE(aligned16(dense_out) && (residual == nullptr || aligned16(residual)) && (y == nullptr || aligned16(y)),
             "%s: 16-byte alignment required", who);
  for (const void* p : {(const void*)res_idx, (const void*)res_hi, (const void*)res_lo, (const void*)y_idx, (const void*)y_hi,
                        (const void*)y_lo})
    TQ_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3u) == 0, "%s: index arrays and byte planes must be 4-byte aligned", who);
  if (int e = check_tensor_quantizers(who, {q_dense, q_sum, q_out}, rows * d)) return e;
  const bool f1 = res_hi == nullptr && y == nullptr && y_idx == nullptr && y_hi != nullptr;
  const bool f2 = res_hi != nullptr && y != nullptr && y_hi == nullptr;
  if (!f1 && !f2)
    return set_error(TQ_EUNSUPPORTED,
                     "%s: supported are (1) residual as fp32 or res_idx with y_hi / y_lo [and y_row_nan] as the only outputs "
                     "(y == NULL, y_idx == NULL) and (2) residual as res_hi / res_lo with y [, y_idx] [, y_row_nan] and no "
                     "output planes", who);
  return launch_res_ln_ires(who, dense_out, residual, res_idx, res_hi, res_lo, res_row_nan, y, y_idx, y_hi, y_lo, y_row_nan, rows, d,
                            ln_weight, ln_bias, ln_eps, q_dense, q_sum, q_out, residual == nullptr ? q_res : nullptr,
                            static_cast<hipStream_t>(stream));
}

extern "C" int tq_embeddings_layernorm_quant_fwd(const float* word_table, uint64_t word_rows, const int64_t* word_ids,
                                                 const float* type_table, uint64_t type_rows, const int64_t* type_ids,
                                                 const float* pos_table, uint64_t pos_rows, const int64_t* pos_ids, float* y,
                                                 int8_t* y_idx, uint64_t rows, uint64_t d, const tq_quantizer* q_sum1,
                                                 const tq_quantizer* q_sum2, const float* ln_weight, const float* ln_bias,
                                                 float ln_eps, const tq_quantizer* q_out, int32_t* bad_ids,
                                                 tq_stream_t stream) {
  const char* who = "tq_embeddings_layernorm_quant_fwd";
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(word_table && type_table && pos_table && word_ids && type_ids && pos_ids && y && ln_weight && ln_bias, "%s: NULL pointer", who);
  TQ_REQUIRE(word_rows >= 1 && type_rows >= 1 && pos_rows >= 1, "%s: empty table", who);
  TQ_REQUIRE(aligned16(word_table) && aligned16(type_table) && aligned16(pos_table) && aligned16(y), "%s: 16-byte alignment required", who);
  TQ_REQUIRE(d % 4 == 0, "%s: row length %llu is not a whole number of 16-byte vectors", who, (unsigned long long)d);
  if (int e = check_y_idx(who, y_idx, q_out, true)) return e;
  if (int e = check_tensor_quantizers(who, {q_sum1, q_sum2, q_out}, rows * d)) return e;
  TQ_REQUIRE(bad_ids == nullptr || (reinterpret_cast<uintptr_t>(bad_ids) & 3u) == 0, "%s: bad_ids must be 4-byte aligned", who);
  const EmbArgs emb{word_ids, type_ids, pos_ids, reinterpret_cast<const u32x4*>(type_table), word_rows, type_rows, pos_rows, bad_ids};
  return launch_res_ln<TQ_F32>(word_table, pos_table, y, y_idx, rows, d, ln_weight, ln_bias, ln_eps, q_sum1, q_sum2, q_out, 0,
                               static_cast<hipStream_t>(stream), &emb);
}

extern "C" int tq_embeddings_layernorm_quant_axis_fwd(const float* word_table, uint64_t word_rows, const int64_t* word_ids,
                                                      const float* type_table, uint64_t type_rows, const int64_t* type_ids,
                                                      const float* pos_table, uint64_t pos_rows, const int64_t* pos_ids, float* y,
                                                      int8_t* y_idx, uint64_t rows, uint64_t d, const tq_quantizer* q_sum1,
                                                      const tq_quantizer* q_sum2, const float* ln_weight, const float* ln_bias,
                                                      float ln_eps, const tq_quantizer* q_out, int32_t* bad_ids,
                                                      tq_stream_t stream) {
  const char* who = "tq_embeddings_layernorm_quant_axis_fwd";
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(word_table && type_table && pos_table && word_ids && type_ids && pos_ids && y && ln_weight && ln_bias, "%s: NULL pointer", who);
  TQ_REQUIRE(word_rows >= 1 && type_rows >= 1 && pos_rows >= 1, "%s: empty table", who);
  TQ_REQUIRE(aligned16(word_table) && aligned16(type_table) && aligned16(pos_table) && aligned16(y), "%s: 16-byte alignment required", who);
  TQ_REQUIRE(d >= 1 && d % 4 == 0, "%s: row length %llu is not a whole number of 16-byte vectors", who, (unsigned long long)d);
  if (int e = check_y_idx(who, y_idx, q_out, true)) return e;
  if (int e = check_column_quantizers(who, {q_sum1, q_sum2, q_out}, rows, d)) return e;
  TQ_REQUIRE(bad_ids == nullptr || (reinterpret_cast<uintptr_t>(bad_ids) & 3u) == 0, "%s: bad_ids must be 4-byte aligned", who);
  const EmbArgs emb{word_ids, type_ids, pos_ids, reinterpret_cast<const u32x4*>(type_table), word_rows, type_rows, pos_rows, bad_ids};
  return launch_emb_ln_axis(word_table, pos_table, y, y_idx, rows, d, ln_weight, ln_bias, ln_eps, q_sum1, q_sum2, q_out, emb,
                            static_cast<hipStream_t>(stream));
}

extern "C" int tq_residual_nonorm_quant_fwd(const void* dense_out, const void* residual, void* y, int8_t* y_idx, uint64_t rows,
                                            uint64_t d, int dtype, const tq_quantizer* q_dense, const tq_quantizer* q_sum,
                                            const float* weight, const float* bias, const tq_quantizer* q_out,
                                            tq_stream_t stream) {
  return residual_tail("tq_residual_nonorm_quant_fwd", dense_out, residual, y, y_idx, rows, d, dtype, q_dense, q_sum, weight, bias,
                       0.0f, q_out, 1, stream);
}

extern "C" int tq_scores_softmax_quant_fwd(const float* scores, float* probs, uint64_t rows, uint64_t cols,
                                           const float* mask, uint64_t rows_per_mask, float denom,
                                           const tq_quantizer* q_scores, const tq_quantizer* q_probs, tq_stream_t stream) {
  if (rows == 0) return TQ_OK;
  TQ_REQUIRE(scores && probs, "tq_scores_softmax_quant_fwd: NULL pointer");
  TQ_REQUIRE(aligned16(scores) && aligned16(probs) && (mask == nullptr || aligned16(mask)),
             "tq_scores_softmax_quant_fwd: 16-byte alignment required");
  TQ_REQUIRE(mask == nullptr || (rows_per_mask >= 1 && rows % rows_per_mask == 0), "tq_scores_softmax_quant_fwd: bad mask layout");
  if (mask == nullptr) rows_per_mask = rows;      // unused without a mask; keeps the kernels' row -> mask arithmetic away from / 0
  TQ_REQUIRE(denom != 0.0f, "tq_scores_softmax_quant_fwd: denom == 0");
  for (const tq_quantizer* q : {q_scores, q_probs})
    if (q != nullptr) {
      if (int e = check_quantizer(q, rows * cols, "tq_scores_softmax_quant_fwd")) return e;
      TQ_REQUIRE(q->n_params == 1, "tq_scores_softmax_quant_fwd: per-tensor quantizers only");
    }
  const tq_quantizer none{};
  const tq_quantizer &c1 = q_scores ? *q_scores : none, &c2 = q_probs ? *q_probs : none;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const auto sv = reinterpret_cast<const f32x4*>(scores);
  auto yv = reinterpret_cast<f32x4*>(probs);
#define TQ_SM(LPR, NV)                                                                                          \
  if (cols == (uint64_t)(LPR) * (NV) * 4) {                                                                     \
    static const int r_env = tuning("TQ_SM_R", 0);                                                              \
    const int allow_fast = tuning("TQ_SM_FAST", 1);      /* read per call: the parity test flips it */            \
    /* rows in flight per lane group: as many as the registers allow, while the grid still covers the chip twice */ \
    int want = r_env ? r_env : 4;                                                                               \
    while (!r_env && want > 1 && rows / (kBlock / (LPR) * want) < 512) want >>= 1;                              \
    const int R = (want == 4 && (NV) == 1) ? 4 : ((want >= 2 && (NV) <= 2) ? 2 : 1);                            \
    const unsigned rpb = kBlock / (LPR) * R;                                                                    \
    const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>(ceil_div(rows, rpb), 1), 1u << 20);   \
    if (R == 4 && (NV) == 1)                                                                                    \
      hipLaunchKernelGGL((softmax_quant_k<LPR, NV, 4>), dim3(grid), dim3(kBlock), 0, st, sv, yv, rows, mask, rows_per_mask, \
                         denom, c1, c2, q_scores != nullptr, q_probs != nullptr, allow_fast);                               \
    else if (R == 2 && (NV) <= 2)                                                                               \
      hipLaunchKernelGGL((softmax_quant_k<LPR, NV, 2>), dim3(grid), dim3(kBlock), 0, st, sv, yv, rows, mask, rows_per_mask, \
                         denom, c1, c2, q_scores != nullptr, q_probs != nullptr, allow_fast);                               \
    else                                                                                                        \
      hipLaunchKernelGGL((softmax_quant_k<LPR, NV, 1>), dim3(grid), dim3(kBlock), 0, st, sv, yv, rows, mask, rows_per_mask, \
                         denom, c1, c2, q_scores != nullptr, q_probs != nullptr, allow_fast);                               \
    return check_launch("softmax_quant_k");                                                                     \
  }
  TQ_SM(8, 1) TQ_SM(16, 1) TQ_SM(32, 1) TQ_SM(64, 1) TQ_SM(64, 2) TQ_SM(64, 4)
#undef TQ_SM
  return set_error(TQ_EUNSUPPORTED, "tq_scores_softmax_quant_fwd: row length %llu unsupported (32..1024, power of two)",
                   (unsigned long long)cols);
}
