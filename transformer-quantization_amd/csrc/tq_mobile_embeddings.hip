// MobileBERT's embedding block with fixed ranges as ONE exact integer launch (tq_mobile_embeddings_nonorm_quant_fwd).
//
// The reference block (models/quantized_mobilebert.py, QuantizedMobileBertEmbeddings) looks three neighbouring word rows
// up, concatenates them to a [B, T, 3E] "trigram" tensor, sends it through the 3E -> N `embedding_transformation` Linear
// and adds position and token-type rows, with a quantizer behind every step and NoNorm at the end.  The look-up returns
// rows of an already fake-quantized table: the Linear's input is s_e * e_idx with e_idx the signed indices of the word
// table on its symmetric grid, so the GEMM is an exact integer contraction (|sum| <= 384 * 128 * 128 < 2^24: its
// conversion to fp32 is exact too) and everything behind it is single IEEE fp32 operations:
//
//     tri[m, 0:E] = e_idx[ids[b, t+1]]    tri[m, E:2E] = e_idx[ids[b, t]]    tri[m, 2E:3E] = e_idx[ids[b, t-1]]
//     lin[m, n]   = (s_e * s_w[n]) * float(sum_k tri[m, k] * w_idx[n, k]) + bias[n]
//     y           = Q_3( Q_2( Q_1( Q_t(lin) + pos[pos_ids[m]] ) + type[type_ids[m]] ) * nn_w + nn_b )
//
// Work split.  A workgroup (4 waves) owns kR = 16 consecutive tokens of ONE sequence times kTN = 128 output columns; the
// grid is B x ceil(T / 16) x N / 128 (256 workgroups at [8, 128] x 512: one per CU).  It gathers the 16 + 2 word rows of
// its chunk and of the two halo tokens ONCE into LDS as int8 (18 x 128 bytes; a zero row where a halo falls outside
// [0, T), so a chunk never sees another sequence, and for the tokens past T of a partial last chunk).  The three K-thirds
// of the MFMA's token operand are then the SAME LDS array read at row offsets +2 / +1 / +0: the [B, T, 3E] tensor never
// exists.  The workgroup's weight tile (128 columns x 384 bytes = 48 KB, one contiguous block of w_idx) travels through
// registers into LDS in 16-byte pieces, fully coalesced.  Both arrays have rows padded by 16 bytes (pitches of 100 and 36
// dwords: the 16 rows of a fragment read start in 16 different groups of 4 banks).  One barrier; then every wave runs
// 2 x 6 v_mfma_i32_16x16x64_i8 for its 32 columns (weights first operand: a lane's 4 accumulator registers are 4
// consecutive columns of one token) and the epilogue on the accumulator registers.  Everything the epilogue reads --
// quantizer buffers, per-column constants, the position / token-type rows -- is requested before the barrier.
//
// Linear stage: the operation order of tq_linear_i8_fwd's epilogue on x_idx = tri with an input zero point of 128 (its
// zero-point term vanishes): sw = s_e * s_w[n] first, then float(acc) * sw + bias as two operations.  Tail stages: the
// device functions of the fake-quant kernels (tq_device.h) -- the exact branch-free form where a quantizer admits it, the
// IEEE division otherwise; NaN passes through a quantizer in both.
//
// Out-of-range ids never read out of bounds: a word id outside the table stands as a zero row in LDS and turns every row
// whose trigram touches it (t-1, t, t+1 of its sequence) NaN as a whole; a position / token-type id outside its table
// turns its own row NaN.  *bad_ids is raised as by tq_embeddings_layernorm_quant_fwd.  No atomic read-modify-write, no
// scratch memory.
#include "tq_device.h"
#include "tq_host.h"

namespace tq {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kMeE = 128;                 // embedding size: bytes of one word row
constexpr int kMeK = 3 * kMeE;            // the Linear's K
constexpr int kMeR = 16;                  // tokens per workgroup
constexpr int kMeTN = 128;                // output columns per workgroup (32 per wave)
constexpr int kMeWP = kMeK + 16;          // LDS pitch of a weight row
constexpr int kMeXP = kMeE + 16;          // LDS pitch of a word row
constexpr int kMeWChunks = kMeTN * kMeK / 16 / kBlock;   // 16-byte weight pieces per thread (12)

struct MobEmbArgs {
  const int8_t* e_idx;       // [vocab, E] signed indices of the word table
  uint64_t vocab;
  const int64_t* ids;        // [B, T]
  const float* e_delta;      // the word table's symmetric per-tensor quantizer
  float e_eps;
  const int8_t* w;           // [N, 3E]
  const float* w_delta;      // [1] or [N]
  uint32_t w_n_params;
  float w_eps;
  const float* bias;         // [N] or null
  const float* pos;          // [pos_rows, N]
  uint64_t pos_rows;
  const int64_t* pos_ids;    // [B * T]
  const float* typ;          // [type_rows, N]
  uint64_t type_rows;
  const int64_t* type_ids;   // [B * T]
  const float *nn_w, *nn_b;  // [N]
  float* y;                  // [B * T, N]
  int8_t* y_idx;             // optional
  uint32_t B, T, N, chunks;
  tq_quantizer q[4];         // Q_t, Q_1, Q_2, Q_3
  int on[4];
  int32_t* bad;
};

struct MeQ {
  QP p;
  QF f;
  int on;
};

// One quantizer on a pair: the exact form (NaN kept by hand: v_med3 drops it) or the division; xi = grid index of the result
__device__ __forceinline__ f32x2 me_quant(f32x2 v, const MeQ& q, f32x2& xi) {
  if (!q.on) return v;
  if (q.f.ok) {
    const f32x2 h = qf_round2(v, q.f);
    xi = h + f32x2{q.f.zp, q.f.zp};
    f32x2 y = qf_dequant2(h, q.f);
    y.x = v.x != v.x ? v.x : y.x;
    y.y = v.y != v.y ? v.y : y.y;
    return y;
  }
  xi = f32x2{q_index(v.x, q.p), q_index(v.y, q.p)};
  return f32x2{q_dequant(xi.x, q.p), q_dequant(xi.y, q.p)};
}

__global__ __launch_bounds__(kBlock) void mobile_embeddings_k(MobEmbArgs p) {
  __shared__ __attribute__((aligned(16))) int8_t s_w[kMeTN * kMeWP];
  __shared__ __attribute__((aligned(16))) int8_t s_x[(kMeR + 2) * kMeXP];
  __shared__ int s_bad[kMeR + 2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, kg = lane >> 4;
  const uint32_t n_tiles = p.N / kMeTN;
  const uint32_t tile = blockIdx.x % n_tiles, rest = blockIdx.x / n_tiles;
  const uint32_t chunk = rest % p.chunks, b = rest / p.chunks;
  const uint32_t n0 = tile * kMeTN, t0 = chunk * kMeR;

  // ---- requests: the chunk's ids first (the word rows depend on them), then the weight tile
  const int xrow = tid >> 3, xcol = tid & 7;                    // threads 0..143: one 16-byte piece of one word row each
  const int64_t tt = (int64_t)t0 - 1 + xrow;                    // the token LDS row xrow holds
  const bool xmine = tid < (kMeR + 2) * 8;
  const bool xtok = xmine && tt >= 0 && tt < (int64_t)p.T;
  int64_t wid = 0;
  if (xtok) wid = p.ids[(uint64_t)b * p.T + (uint64_t)tt];
  u32x4 wreg[kMeWChunks];
  const u32x4* wsrc = reinterpret_cast<const u32x4*>(p.w + (size_t)n0 * kMeK);      // the tile: one contiguous block
#pragma unroll
  for (int i = 0; i < kMeWChunks; ++i) wreg[i] = wsrc[i * kBlock + tid];

  // this lane's token and its position / token-type ids
  const uint32_t t = t0 + r16;
  const bool live = t < p.T;
  const uint64_t m = (uint64_t)b * p.T + (live ? t : 0);
  int64_t pid = 0, yid = 0;
  if (live) { pid = p.pos_ids[m]; yid = p.type_ids[m]; }

  // quantizer buffers and the word table's scale
  const float* safe = p.e_delta;
  QRaw qr[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) qr[k] = p.on[k] ? load_qraw(p.q[k], 0, safe) : QRaw{1.0f, 0.0f, 0u};
  float de = p.e_delta[0];

  // per-column constants of this lane's 2 x 4 columns
  const uint32_t nw0 = n0 + wave * 32;
  f32x4 c_sw[2], c_b[2], c_nw[2], c_nb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t n = nw0 + i * 16 + kg * 4;
    c_sw[i] = p.w_n_params == 1 ? f32x4{p.w_delta[0], p.w_delta[0], p.w_delta[0], p.w_delta[0]}
                                : *reinterpret_cast<const f32x4*>(p.w_delta + n);
    c_b[i] = p.bias != nullptr ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    c_nw[i] = *reinterpret_cast<const f32x4*>(p.nn_w + n);
    c_nb[i] = *reinterpret_cast<const f32x4*>(p.nn_b + n);
  }

  // ---- the word rows: an id outside the table reads nothing and marks its LDS row
  const bool wbad = xtok && (wid < 0 || (uint64_t)wid >= p.vocab);
  u32x4 xreg = {0u, 0u, 0u, 0u};
  if (xtok && !wbad) xreg = *reinterpret_cast<const u32x4*>(p.e_idx + (size_t)wid * kMeE + xcol * 16);
  // position / token-type rows of this lane's columns (clamped row for memory safety; the row turns NaN below)
  const bool obad = live && (pid < 0 || (uint64_t)pid >= p.pos_rows || yid < 0 || (uint64_t)yid >= p.type_rows);
  const bool pbad = pid < 0 || (uint64_t)pid >= p.pos_rows, ybad = yid < 0 || (uint64_t)yid >= p.type_rows;
  const float* prow = p.pos + (size_t)(pbad ? 0 : pid) * p.N;
  const float* yrow = p.typ + (size_t)(ybad ? 0 : yid) * p.N;
  f32x4 c_pos[2], c_typ[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t n = nw0 + i * 16 + kg * 4;
    c_pos[i] = *reinterpret_cast<const f32x4*>(prow + n);
    c_typ[i] = *reinterpret_cast<const f32x4*>(yrow + n);
  }

  // ---- into LDS
  if (xmine) {
    *reinterpret_cast<u32x4*>(s_x + xrow * kMeXP + xcol * 16) = xreg;
    if (xcol == 0) s_bad[xrow] = wbad ? 1 : 0;
  }
#pragma unroll
  for (int i = 0; i < kMeWChunks; ++i) {
    const int c = i * kBlock + tid;                              // piece c: weight row c / 24, bytes (c % 24) * 16 ..
    *reinterpret_cast<u32x4*>(s_w + (c / (kMeK / 16)) * kMeWP + (c % (kMeK / 16)) * 16) = wreg[i];
  }
  if ((wbad || obad) && p.bad != nullptr && (wbad ? xcol == 0 : kg == 0))
    __hip_atomic_store(p.bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);       // a plain store the host can see
  __syncthreads();

  // ---- 2 column tiles x 6 K steps; K third j (token t+1 / t / t-1) is the word-row array at row offset 2 - j
  v4i acc[2] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}};
  const int8_t* wl = s_w + (wave * 32 + r16) * kMeWP + kg * 16;
  const int8_t* xl = s_x + r16 * kMeXP + kg * 16;
#pragma unroll
  for (int ks = 0; ks < kMeK / 64; ++ks) {
    const v4i fx = *reinterpret_cast<const v4i*>(xl + (2 - ks / 2) * kMeXP + (ks % 2) * 64);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const v4i fw = *reinterpret_cast<const v4i*>(wl + i * 16 * kMeWP + ks * 64);
      acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw, fx, acc[i], 0, 0, 0);
    }
  }
  const bool row_nan = obad || s_bad[r16] != 0 || s_bad[r16 + 1] != 0 || s_bad[r16 + 2] != 0;

  // ---- epilogue
  de = pinned_uniform(de);
  MeQ mq[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    qraw_arrived(qr[k]);
    mq[k].on = p.on[k];
    mq[k].p = p.on[k] ? qp_from_raw(p.q[k], qr[k]) : QP{1.f, 0.f, 0.f, 1.f};
    mq[k].f = make_qf(mq[k].p);
  }
  const float sx = de < p.e_eps ? p.e_eps : de;
  if (!live) return;
  const float nanf_ = __builtin_nanf("");
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t n = nw0 + i * 16 + kg * 4;
    f32x2 v[2], xi[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float d0 = c_sw[i][2 * h], d1 = c_sw[i][2 * h + 1];
      const f32x2 sw = {sx * (d0 < p.w_eps ? p.w_eps : d0), sx * (d1 < p.w_eps ? p.w_eps : d1)};
      const f32x2 a = {(float)acc[i][2 * h], (float)acc[i][2 * h + 1]};
      v[h] = a * sw + f32x2{c_b[i][2 * h], c_b[i][2 * h + 1]};                 // separate mul and add, like the Linear
      v[h] = me_quant(v[h], mq[0], xi[h]);
      v[h] = me_quant(v[h] + f32x2{c_pos[i][2 * h], c_pos[i][2 * h + 1]}, mq[1], xi[h]);
      v[h] = me_quant(v[h] + f32x2{c_typ[i][2 * h], c_typ[i][2 * h + 1]}, mq[2], xi[h]);
      v[h] = v[h] * f32x2{c_nw[i][2 * h], c_nw[i][2 * h + 1]} + f32x2{c_nb[i][2 * h], c_nb[i][2 * h + 1]};
      v[h] = me_quant(v[h], mq[3], xi[h]);
    }
    f32x4 o = {v[0].x, v[0].y, v[1].x, v[1].y};
    if (row_nan) o = f32x4{nanf_, nanf_, nanf_, nanf_};
    const size_t at = (size_t)m * p.N + n;
    *reinterpret_cast<f32x4*>(p.y + at) = o;
    if (p.y_idx != nullptr) {                                                  // int8(index - 128) on Q_3's grid
      struct alignas(4) { int8_t e[4]; } oi = {{(int8_t)((int)xi[0].x - 128), (int8_t)((int)xi[0].y - 128),
                                                (int8_t)((int)xi[1].x - 128), (int8_t)((int)xi[1].y - 128)}};
      *reinterpret_cast<uint32_t*>(p.y_idx + at) = __builtin_bit_cast(uint32_t, oi);
    }
  }
}

}  // namespace tq

using namespace tq;

extern "C" int tq_mobile_embeddings_nonorm_quant_fwd(
    const int8_t* e_idx, uint64_t vocab, uint64_t E, const int64_t* word_ids, const float* e_delta, float e_eps,
    const int8_t* w_idx, const float* w_delta, uint64_t w_n_params, float w_eps, const float* bias, const float* pos_table,
    uint64_t pos_rows, const int64_t* pos_ids, const float* type_table, uint64_t type_rows, const int64_t* type_ids,
    const float* nn_weight, const float* nn_bias, float* y, int8_t* y_idx, uint64_t B, uint64_t T, uint64_t N,
    const tq_quantizer* q_t, const tq_quantizer* q_sum1, const tq_quantizer* q_sum2, const tq_quantizer* q_out,
    int32_t* bad_ids, tq_stream_t stream) {
  const char* who = "tq_mobile_embeddings_nonorm_quant_fwd";
  TQ_REQUIRE(e_idx && word_ids && e_delta && w_idx && w_delta && pos_table && pos_ids && type_table && type_ids && nn_weight &&
                 nn_bias && y, "%s: NULL pointer", who);
  TQ_REQUIRE(B >= 1 && T >= 1 && B * T < (1ull << 31) && vocab >= 1 && pos_rows >= 1 && type_rows >= 1,
             "%s: B, T and the table row counts must be >= 1 (B * T < 2^31)", who);
  if (E != (uint64_t)kMeE || N == 0 || N % kMeTN != 0 || N >= (1u << 20))
    return set_error(TQ_EUNSUPPORTED, "%s: embedding size %llu -> hidden size %llu has no instantiation (E = 128, N a multiple "
                     "of 128)", who, (unsigned long long)E, (unsigned long long)N);
  TQ_REQUIRE(w_n_params == 1 || w_n_params == N, "%s: weight scales must be per-tensor or per-output-channel", who);
  TQ_REQUIRE(aligned16(e_idx) && aligned16(w_idx) && aligned16(pos_table) && aligned16(type_table) && aligned16(nn_weight) &&
                 aligned16(nn_bias) && aligned16(bias) && aligned16(y) && (w_n_params == 1 || aligned16(w_delta)),
             "%s: 16-byte alignment required", who);
  TQ_REQUIRE(aligned4({e_delta, w_delta, y_idx}) && (reinterpret_cast<uintptr_t>(word_ids) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(pos_ids) & 7u) == 0 && (reinterpret_cast<uintptr_t>(type_ids) & 7u) == 0,
             "%s: scales and y_idx must be 4-byte, ids 8-byte aligned", who);
  TQ_REQUIRE(bad_ids == nullptr || (reinterpret_cast<uintptr_t>(bad_ids) & 3u) == 0, "%s: bad_ids must be 4-byte aligned", who);
  TQ_REQUIRE(y_idx == nullptr || (q_out != nullptr && !q_out->symmetric && q_out->n_bits <= 8),
             "%s: y_idx needs an asymmetric <= 8-bit output quantizer", who);
  MobEmbArgs a{};
  const tq_quantizer* qs[4] = {q_t, q_sum1, q_sum2, q_out};
  for (int k = 0; k < 4; ++k) {
    a.on[k] = qs[k] != nullptr;
    if (qs[k] == nullptr) continue;
    if (int e = check_quantizer(qs[k], B * T * N, who)) return e;
    TQ_REQUIRE(qs[k]->n_params == 1, "%s: per-tensor quantizers only", who);
    TQ_REQUIRE(aligned4({qs[k]->delta, qs[k]->zero_float}), "%s: quantizer parameters must be 4-byte aligned", who);
    a.q[k] = *qs[k];
  }
  const uint64_t chunks = ceil_div(T, kMeR);
  const uint64_t blocks = B * chunks * (N / kMeTN);
  TQ_REQUIRE(blocks < (1ull << 31), "%s: %llu workgroups (B * ceil(T / 16) * N / 128 must stay below 2^31)", who,
             (unsigned long long)blocks);
  a.e_idx = e_idx; a.vocab = vocab; a.ids = word_ids; a.e_delta = e_delta; a.e_eps = e_eps;
  a.w = w_idx; a.w_delta = w_delta; a.w_n_params = (uint32_t)w_n_params; a.w_eps = w_eps; a.bias = bias;
  a.pos = pos_table; a.pos_rows = pos_rows; a.pos_ids = pos_ids;
  a.typ = type_table; a.type_rows = type_rows; a.type_ids = type_ids;
  a.nn_w = nn_weight; a.nn_b = nn_bias; a.y = y; a.y_idx = y_idx;
  a.B = (uint32_t)B; a.T = (uint32_t)T; a.N = (uint32_t)N; a.chunks = (uint32_t)chunks;
  a.bad = bad_ids;
  hipLaunchKernelGGL(mobile_embeddings_k, dim3((unsigned)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("mobile_embeddings_k");
}
