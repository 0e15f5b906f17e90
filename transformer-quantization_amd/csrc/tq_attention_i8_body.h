// Body of the attention core's kernels (csrc/tq_attention_i8.hip includes it once per form, inside the kernel's braces).
// TQ_ATTN_RAGGED 0: attention_i8_k, sequences of T = 16 NT_ALL rows.
// TQ_ATTN_RAGGED 1: attention_i8_ragged_k -- the sequences hold p.T <= T valid rows each (any length) and the launch
// computes the problem padded to T keys whose pad keys carry the mask -inf.  A pad key's exponential is exactly 0.0f, its
// probability index the zero point and its term (a'_p + c_p)(a'_v + c_v) of the second contraction 0 whatever its V row
// holds -- so pad rows are never read (every row index is clamped to the last valid row: any in-range bytes do), the
// score of a pad key is replaced by -inf behind the mask add, and pad queries are computed but not stored.  The summation
// tree, the exchanges and the second GEMM are the same instructions in the same order: bit-identical to the padded launch.
// TQ_ATTN_RAGGED 2: attention_i8_varlen_k -- the ragged form over PACKED sequences (tq_attention_i8_varlen_fwd): sequence b
// owns rows seq_start[b] .. seq_start[b + 1] - 1 of the [total_rows, ...] buffers, so its length tv, its row bases, the mask
// index and the output row come from seq_start where the ragged form has p.T and b * p.T.  Everything else is the ragged
// form's text: bit-identical to the ragged launch on the batch padded to p.T rows per sequence.  seq_start and total_rows
// are kernel parameters of that kernel alone.
// TQ_ATTN_HEADS: whether the kernel may be launched with one grid per head (AttnArgs::wide_*); false only for the one
// instantiation whose register allocation the run-time head offset would raise (kRaggedPerTensorOnly in the .hip), which
// has a twin, attention_i8_ragged_heads_k, for those launches.
// The forms are told apart by the preprocessor, not by a template parameter, so that the text -- and with it the
// generated code -- of the kernels that existed before a form was added is what it was.
  static_assert(QW == kAttnWaves || !SPLIT, "the key-split form has two query waves");
  static_assert((NT_ALL * 16) % (16 * QW) == 0, "whole workgroups per row of queries");
  constexpr int T = NT_ALL * 16;
  constexpr int NT = SPLIT ? NT_ALL / 2 : NT_ALL;  // key tiles of this wave
  constexpr int KS = NT / 4;                       // its 64-key MFMA steps of the second GEMM
  constexpr int THREADS = SPLIT ? 2 * kAttnThreads : QW * kWave;
  constexpr int PITCH = T + 32;                    // 32 * odd bytes: conflict-free ds_read_b128 (4 x 16 lane groups, 64 banks)
  constexpr int KSA = SPLIT ? 2 * KS : KS;         // 64-key steps of the wave that finishes the tile (all keys)
  static_assert(!SPLIT || NT_ALL % 8 == 0, "key split needs an even number of 64-key steps");
  __shared__ __attribute__((aligned(16))) int8_t s_vt[DH * PITCH];
  __shared__ float s_red[SPLIT ? 2 : 1][4][16];    // [max | sum][wave][query]
  // key-split form: the kh = 1 wave hands its probability indices (KS operands of 16 bytes per lane) to its kh = 0 partner
  __shared__ __attribute__((aligned(16))) v4i s_fp[SPLIT ? 2 : 1][SPLIT ? KS : 1][64];
  // QW = 8: the K tile of the (batch, head) is fetched ONCE per workgroup (one 16-byte load per thread at T = 128) and read
  // from LDS by the eight waves -- each wave fetching its own copy was 8 of the 13 loads per lane in front of the first
  // instruction, on a launch whose longest phase is that fetch (profiles/r06/attn_phase_profile.txt).  Row pitch DH + 16:
  // conflict-free ds_read_b128 of 16 rows x 16 bytes.
  constexpr bool K_LDS = !SPLIT && QW == 8;
  constexpr int KP = DH + 16;
  __shared__ __attribute__((aligned(16))) int8_t s_k[K_LDS ? T * KP : 16];

  const int tid = threadIdx.x, lane = tid & 63, wave = SPLIT ? (tid >> 6) & 1 : tid >> 6, kh = SPLIT ? tid >> 7 : 0;
  const int r16 = lane & 15, g = lane >> 4;
  const int t0 = kh * NT;                          // first key tile of this wave
  const uint32_t qblocks = T / (16 * QW);
  const uint32_t bh = blockIdx.x / qblocks, qb = blockIdx.x % qblocks;
  const uint32_t b = bh / p.H, h = bh % p.H;
  const size_t row_stride = p.in_stride;
#if TQ_ATTN_RAGGED == 2
  // both seq_start words are requested before anything else: the V, Q and K loads below depend on them, and this launch
  // is its prologue.  Defensive clamps (a consistent seq_start makes each a no-op): start into [0, total_rows], end into
  // [start, total_rows], the length to p.T -- no row outside the total_rows rows is ever addressed.
  const int32_t ss0 = seq_start[b], ss1 = seq_start[b + 1];
  const uint32_t seq0 = ss0 < 0 ? 0u : ((uint32_t)ss0 < total_rows ? (uint32_t)ss0 : total_rows);
  const uint32_t seq1 = ss1 < (int32_t)seq0 ? seq0 : ((uint32_t)ss1 < total_rows ? (uint32_t)ss1 : total_rows);
  const uint32_t tv = seq1 - seq0 < p.T ? seq1 - seq0 : p.T;   // valid rows of this sequence; T = the padded length
  // queries beyond the sequence (all of them when it is empty): the WHOLE workgroup leaves, before any barrier
  if (qb * 16 * QW >= tv) return;
#define TQ_SEQ_ROW0 (size_t)seq0
#define TQ_ROW(r) ((uint32_t)(r) < tv ? (uint32_t)(r) : tv - 1)     /* pad rows: any valid row */
#elif TQ_ATTN_RAGGED
  const uint32_t tv = p.T;                         // valid rows (= keys = queries) of a sequence; T = the padded length
  // a workgroup whose queries are all pad rows has nothing to store: the WHOLE workgroup leaves, before any barrier
  if (qb * 16 * QW >= tv) return;
#define TQ_SEQ_ROWS tv
#define TQ_ROW(r) ((uint32_t)(r) < tv ? (uint32_t)(r) : tv - 1)     /* pad rows: any valid row */
#else
#define TQ_SEQ_ROWS T
#define TQ_ROW(r) (r)
#endif
#ifndef TQ_SEQ_ROW0
#define TQ_SEQ_ROW0 (size_t)b * TQ_SEQ_ROWS                         /* first row of sequence b */
#endif
  const size_t base = TQ_SEQ_ROW0 * row_stride + (size_t)h * DH;
  const size_t v_stride = p.v_stride, base_v = TQ_SEQ_ROW0 * v_stride + (size_t)h * DH;

  TQ_STAMP(0);
  // ---- V tile: loads first (one work item = 4 consecutive keys x 16 head dims, four 16-byte loads) ----------------
  constexpr uint32_t PARTS = DH / 16, ITEMS = (uint32_t)T / 4 * PARTS;
  constexpr int VIT = (ITEMS + THREADS - 1) / THREADS;
  v4i raw[VIT][4];
#pragma unroll
  for (int it = 0; it < VIT; ++it) {
    const uint32_t c = tid + it * THREADS;
    if (ITEMS % THREADS == 0 || c < ITEMS) {
      const uint32_t key4 = (c / PARTS) * 4, part = c % PARTS;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        raw[it][kk] = *reinterpret_cast<const v4i*>(p.v + base_v + (size_t)TQ_ROW(key4 + kk) * v_stride + part * 16);
    }
  }

  // ---- quantizer parameters and this wave's queries: two dependent rounds of loads (kernel argument -> pointer ->
  // value) in flight together with the V tile
  const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
  const v4i zero4 = {0, 0, 0, 0};
  const uint32_t qrow = qb * 16 * QW + wave * 16 + r16;
  const bool kin = g * 16 < DH;                     // lane groups beyond the head dim supply zeros
  v4i fq = zero4;
  if (kin) fq = *reinterpret_cast<const v4i*>(p.q + base + (size_t)TQ_ROW(qrow) * row_stride + g * 16);
  // short rows: the K tiles too -- one exposed memory latency for V, Q, K and the parameters instead of two
  constexpr bool K_EARLY = NT <= 8 && !K_LDS;
  v4i fk_all[K_EARLY ? NT : 1];
  constexpr uint32_t KCH = (uint32_t)T * PARTS;     // 16-byte chunks of the K tile (K_LDS)
  constexpr int KIT = K_LDS ? (KCH + THREADS - 1) / THREADS : 1;
  v4i kraw[KIT];
  if (K_LDS) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const uint32_t c = tid + it * THREADS;
      if (KCH % THREADS == 0 || c < KCH)
        kraw[it] = *reinterpret_cast<const v4i*>(p.k + base + (size_t)TQ_ROW(c / PARTS) * row_stride + (c % PARTS) * 16);
    }
  }
  if (K_EARLY) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      fk_all[t] = zero4;
      if (kin) fk_all[t] = *reinterpret_cast<const v4i*>(p.k + base + (size_t)TQ_ROW((t0 + t) * 16 + r16) * row_stride + g * 16);
    }
  }

  // the raw buffers of all six quantizers as ONE batch of independent loads (tq_device.h load_qraw; quantizer by
  // quantizer, delta -> zero_float, this was ~10 dependent scalar round trips: 3-4 us of a 10 us launch at BERT-base's
  // inference batch), pinned behind the V / Q / K loads
  // Q, K, V and the context may carry one grid per head (AttnArgs::wide_*): this workgroup's head is wave-uniform, so its
  // parameters are the same scalars as a per-tensor grid's, fetched at the head's first column instead of element 0.
  // TQ_ATTN_HEADS (a constant expression of the including kernel) false: this kernel is launched with per-tensor grids
  // only and fetches element 0, as it did before the per-head form existed.
  constexpr bool HEADS = TQ_ATTN_HEADS;
  const uint32_t hcol = HEADS ? __builtin_amdgcn_readfirstlane(h * DH) : 0u;
  QRaw wq = load_qraw(p.qq, p.wide_q ? hcol : 0u, p.qq.delta), wk = load_qraw(p.qk, p.wide_k ? hcol : 0u, p.qq.delta);
  QRaw wv = load_qraw(p.qv, p.wide_v ? hcol : 0u, p.qq.delta), wp = load_qraw(p.q_probs, 0, p.qq.delta);
  QRaw ws = load_qraw(p.q_scores, 0, p.qq.delta), wc = load_qraw(p.q_ctx, p.wide_c ? hcol : 0u, p.qq.delta);
  qraw_arrived(wq); qraw_arrived(wk); qraw_arrived(wv); qraw_arrived(wp); qraw_arrived(ws); qraw_arrived(wc);
  const QP pq = qp_from_raw(p.qq, wq), pk = qp_from_raw(p.qk, wk), pv = qp_from_raw(p.qv, wv), pp = qp_from_raw(p.q_probs, wp);
  const int cq = 128 - (int)pq.zp, ck = 128 - (int)pk.zp, cv = 128 - (int)pv.zp, cp = 128 - (int)pp.zp;
  const float s_qk = pq.scale * pk.scale, s_pv = pp.scale * pv.scale;
  QP ps = {1.f, 0.f, 0.f, 0.f}, pc = {1.f, 0.f, 0.f, 0.f};
  if (p.has_scores) ps = qp_from_raw(p.q_scores, ws);
  if (p.has_ctx) pc = qp_from_raw(p.q_ctx, wc);
  const float rcp_s = guarded_rcp(ps.scale), rcp_p = guarded_rcp(pp.scale);   // rne(x / scale), tq_device.h

  // denom = 2^k (normal range): the division is an exact scaling
  const uint32_t dbits = f32_to_bits(p.denom);
  const bool denom_pow2 = (dbits & 0x007fffffu) == 0 && (dbits >> 23) >= 32 && (dbits >> 23) <= 222;
  const float inv_denom = 1.0f / p.denom;

  // ---- V^T -> LDS with the key permutation of the accumulator layout: 4x4 byte transposes in registers, sixteen
  // 32-bit LDS stores per work item (keys 4m .. 4m+3 are adjacent slots of one V^T row)
#pragma unroll
  for (int it = 0; it < VIT; ++it) {
    const uint32_t c = tid + it * THREADS;
    if (ITEMS % THREADS == 0 || c < ITEMS) {
      const uint32_t key4 = (c / PARTS) * 4, part = c % PARTS;
      const uint32_t slot = key_slot(key4);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t word[4];                              // word[e]: byte kk = head dim 4 w + e of key key4 + kk
        transpose4x4_b8((uint32_t)raw[it][0][w], (uint32_t)raw[it][1][w], (uint32_t)raw[it][2][w], (uint32_t)raw[it][3][w], word);
#pragma unroll
        for (int e = 0; e < 4; ++e) *reinterpret_cast<uint32_t*>(s_vt + (part * 16 + w * 4 + e) * PITCH + slot) = word[e];
      }
    }
  }

  if (K_LDS) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const uint32_t c = tid + it * THREADS;
      if (KCH % THREADS == 0 || c < KCH) *reinterpret_cast<v4i*>(s_k + (c / PARTS) * KP + (c % PARTS) * 16) = kraw[it];
    }
    __syncthreads();                                 // K tile and V^T are in LDS
  }
  TQ_STAMP(1);
  // ---- S^T = K Q^T for this wave's 16 queries --------------------------------------------------------
  const int rsq = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, fq, zero4, 0, 0, 0)[0];   // sum_d a'_q of column r16
  const int q_const = ck * rsq + DH * cq * ck;

  // Wave-uniform: every quantizer of the score / probability chain admits the exact branch-free path (tq_device.h QF)
  // and the Markstein quotients below keep their fma residuals exact (scales within 2^+-60, see tq_fused_ln.hip).
  const QF fs = make_qf(ps), fpq = make_qf(pp);
  const float adn = fabsf(p.denom);
  const bool fast = p.fast_ok && fpq.ok && pp.scale >= 0x1p-60f && pp.scale <= 0x1p60f && adn >= 0x1p-20f && adn <= 0x1p20f &&
                    s_qk >= 0x1p-60f && s_qk <= 0x1p60f &&
                    (!p.has_scores || (fs.ok && ps.scale >= 0x1p-60f && ps.scale <= 0x1p60f));

  TQ_STAMP(2);
  const QF fc = make_qf(pc);
  const bool fast_ctx = p.fast_ok && p.has_ctx && fc.ok;

  // The zero-point corrections ride on the matrix cores (round 6: they were a v_mul_lo + v_add3 per score): the per-query
  // constant is the accumulator's initial value, and c_q sum_d a'_k is one more MFMA of the K tile against an operand whose
  // bytes are all c_q (c_q = 128 - z_q is in [-127, 128]; 128 = two passes with 64).  Same exact integers as before.
  const int cq_b = cq == 128 ? 64 : cq;
  const int cq_w = (int)((uint32_t)(cq_b & 0xff) * 0x01010101u);
  const v4i cq4 = {cq_w, cq_w, cq_w, cq_w};
  const v4i qc4 = {q_const, q_const, q_const, q_const};
  float sc[NT][4];
  auto score_tiles = [&](auto wide) {                // (one wave-uniform branch around the loop, not one per tile)
    if constexpr (K_EARLY) {
      // register-resident K tiles: the NT accumulator chains side by side, pass by pass (a dependent MFMA waits for
      // its predecessor's last pass: tile by tile the second MFMA of every tile stalled the wave)
      v4i acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk_all[t], fq, qc4, 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk_all[t], cq4, acc[t], 0, 0, 0);
      if (decltype(wide)::value) {
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk_all[t], cq4, acc[t], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[t][r] = (float)acc[t][r] * s_qk;
      return;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      v4i fk = zero4;
      if (K_EARLY) fk = fk_all[t];
      else if (K_LDS) { if (kin) fk = *reinterpret_cast<const v4i*>(s_k + ((t0 + t) * 16 + r16) * KP + g * 16); }
      else if (kin) fk = *reinterpret_cast<const v4i*>(p.k + base + (size_t)TQ_ROW((t0 + t) * 16 + r16) * row_stride + g * 16);
      v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk, fq, qc4, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk, cq4, acc, 0, 0, 0);               // + c_q sum_d a'_k of rows 4g + r
      if (decltype(wide)::value) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fk, cq4, acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) sc[t][r] = (float)acc[r] * s_qk;
      // pin the four scores: the scheduler otherwise keeps the integer accumulators of every tile alive
      asm volatile("" : "+v"(sc[t][0]), "+v"(sc[t][1]), "+v"(sc[t][2]), "+v"(sc[t][3]));
    }
  };
  if (cq == 128) score_tiles(std::true_type{});
  else score_tiles(std::false_type{});

  TQ_STAMP(3);
  v4i fp[KS];
  bool bad_row;                                      // NaN row sum (fully masked query): the context row is NaN
  if (NT <= 16 && fast) {       // (longer rows: the stage arrays would spill)
    // ---- branch-free: NT * 2 register pairs move through every stage side by side ---------------------------------
    constexpr int P = NT * 2;
    f32x2 x[P];
#pragma unroll
    for (int t = 0; t < NT; ++t) { x[2 * t] = f32x2{sc[t][0], sc[t][1]}; x[2 * t + 1] = f32x2{sc[t][2], sc[t][3]}; }
    if (p.has_scores) {
#pragma unroll
      for (int c = 0; c < P; c += 4) {
        f32x2 (&xc)[4] = *reinterpret_cast<f32x2(*)[4]>(&x[c]);
        qf_fake_quant2_n<4>(xc, fs);
      }
    }
    if (denom_pow2) {
      const f32x2 rd = {inv_denom, inv_denom};
#pragma unroll
      for (int i = 0; i < P; ++i) x[i] = x[i] * rd;
    } else {                                         // RN(x / denom)
      quot2_n<P>(x, f32x2{inv_denom, inv_denom}, f32x2{-p.denom, -p.denom});
    }
#if TQ_ATTN_RAGGED
    {                                                // mask [B, p.T]: element by element, pad keys -> -inf
      const float ninf = -__builtin_huge_valf();
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const uint32_t k0 = (t0 + t) * 16 + g * 4;
        if (p.mask) {
          float mk[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) mk[r] = p.mask[TQ_SEQ_ROW0 + TQ_ROW(k0 + r)];
          x[2 * t] = x[2 * t] + f32x2{mk[0], mk[1]};
          x[2 * t + 1] = x[2 * t + 1] + f32x2{mk[2], mk[3]};
        }
        x[2 * t].x = k0 + 0 < tv ? x[2 * t].x : ninf;
        x[2 * t].y = k0 + 1 < tv ? x[2 * t].y : ninf;
        x[2 * t + 1].x = k0 + 2 < tv ? x[2 * t + 1].x : ninf;
        x[2 * t + 1].y = k0 + 3 < tv ? x[2 * t + 1].y : ninf;
      }
    }
#else
    if (p.mask) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 mk = *reinterpret_cast<const f32x4*>(p.mask + (size_t)b * T + (t0 + t) * 16 + g * 4);
        x[2 * t] = x[2 * t] + f32x2{mk[0], mk[1]};
        x[2 * t + 1] = x[2 * t + 1] + f32x2{mk[2], mk[3]};
      }
    }
#endif
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int i = 0; i < P; ++i) mx = max_raw(mx, max_raw(x[i].x, x[i].y));
    mx = max_raw(mx, __shfl_xor(mx, 16));
    mx = max_raw(mx, __shfl_xor(mx, 32));
    if (SPLIT) mx = max_raw(mx, pair_exchange(s_red[0], mx, wave, kh, r16, g));   // (the barrier inside also publishes V^T)
    // The denominator's summation order is part of the contract (oracle/tq_int_oracle.c restates it): per key half,
    // a lane group adds its exponentials sequentially (tile-major), groups combine as (s0 + s1) + (s2 + s3), the two
    // halves are added last -- the same tree whether one wave owns the whole row or two waves own a half each.
    float sum = 0.f, sum_hi = 0.f;
    {
      const f32x2 nmx = {-mx, -mx};                    // x - mx == x + (-mx), bit for bit
#pragma unroll
      for (int i = 0; i < P; ++i) x[i] = x[i] + nmx;
    }
    exp_neg_ieee2_n<P>(x);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if (SPLIT || i < P / 2) { sum += x[i].x; sum += x[i].y; }
      else { sum_hi += x[i].x; sum_hi += x[i].y; }
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (SPLIT) {
      sum += pair_exchange(s_red[1], sum, wave, kh, r16, g);
    } else {
      sum_hi += __shfl_xor(sum_hi, 16);
      sum_hi += __shfl_xor(sum_hi, 32);
      sum += sum_hi;
    }
    bad_row = sum != sum;
    const float rsv = 1.0f / sum;                    // RN(e / sum), 1 <= sum <= T
    quot2_n<P>(x, f32x2{rsv, rsv}, f32x2{-sum, -sum});
    f32x2 hq[P];
#pragma unroll
    for (int c = 0; c < P; c += 4) {                 // clamp(rne(p / scale) + zp, lo, hi) - zp
      f32x2 (&xc)[4] = *reinterpret_cast<f32x2(*)[4]>(&x[c]);
      f32x2 (&hc)[4] = *reinterpret_cast<f32x2(*)[4]>(&hq[c]);
      qf_round2_n<4>(xc, fpq, hc);
    }
    const f32x2 zp2 = {pp.zp, pp.zp};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const f32x2 i0 = hq[2 * (s * 4 + tt)] + zp2, i1 = hq[2 * (s * 4 + tt) + 1] + zp2;     // indices in [0, 255]
        uint32_t w = __builtin_amdgcn_cvt_pk_u8_f32(i0.x, 0, 0u);
        w = __builtin_amdgcn_cvt_pk_u8_f32(i0.y, 1, w);
        w = __builtin_amdgcn_cvt_pk_u8_f32(i1.x, 2, w);
        w = __builtin_amdgcn_cvt_pk_u8_f32(i1.y, 3, w);
        fp[s][tt] = (int)(w ^ 0x80808080u);          // int8(index - 128)
      }
  } else {
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 mk = {0.f, 0.f, 0.f, 0.f};
#if TQ_ATTN_RAGGED
      const uint32_t k0 = (t0 + t) * 16 + g * 4;
      if (p.mask) {
#pragma unroll
        for (int r = 0; r < 4; ++r) mk[r] = p.mask[TQ_SEQ_ROW0 + TQ_ROW(k0 + r)];
      }
#else
      if (p.mask) mk = *reinterpret_cast<const f32x4*>(p.mask + (size_t)b * T + (t0 + t) * 16 + g * 4);
#endif
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = sc[t][r];
        if (p.has_scores) {
          v = q_dequant(clamp_nanprop(rne_quot1(v, ps.scale, rcp_s) + ps.zp, ps.lo, ps.hi), ps);
        }
        v = denom_pow2 ? v * inv_denom : v / p.denom;      // x / 2^k == x * 2^-k exactly (sqrt(64) = 8)
        if (p.mask) v = v + mk[r];
#if TQ_ATTN_RAGGED
        if (k0 + r >= tv) v = -__builtin_huge_valf();     // pad key
#endif
        sc[t][r] = v;
        mx = max_raw(mx, v);
      }
    }
    // ---- softmax over the T keys of this lane's query: in-lane, then across the 4 lane groups ------------
    mx = max_raw(mx, __shfl_xor(mx, 16));
    mx = max_raw(mx, __shfl_xor(mx, 32));
    if (SPLIT) mx = max_raw(mx, pair_exchange(s_red[0], mx, wave, kh, r16, g));   // (the barrier inside also publishes V^T)
    float sum = 0.f, sum_hi = 0.f;                     // same summation tree as the branch-free form above
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        sc[t][r] = exp_neg_ieee(sc[t][r] - mx);
        if (SPLIT || t < NT / 2) sum += sc[t][r];
        else sum_hi += sc[t][r];
      }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (SPLIT) {
      sum += pair_exchange(s_red[1], sum, wave, kh, r16, g);
    } else {
      sum_hi += __shfl_xor(sum_hi, 16);
      sum_hi += __shfl_xor(sum_hi, 32);
      sum += sum_hi;
    }
    bad_row = sum != sum;
    const float inv_sum = (sum >= 7.888609052210118e-31f && sum <= 1.2676506002282294e30f) ? 1.0f / sum : __builtin_nanf("");

    // ---- probability indices -> B operand of the second GEMM (byte tt * 4 + r of step s = key 64s + 16tt + 4g + r)
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        uint32_t word = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // rne((e / sum) / scale): e * (1/sum) * (1/scale) carries 4 roundings against the 2 of the exact chain
          // (<= 6 u apart); a band of 8 u (|h| + 1) around the ties decides which elements redo it exactly
          const float e = sc[s * 4 + tt][r];
          const float q0 = (e * inv_sum) * rcp_p;
          float hq = rintf(q0);
          if (!(fabsf(q0 - hq) < __builtin_fmaf(fabsf(hq), -2.0f * kTieTol, 0.5f - 2.0f * kTieTol)))   // 4 roundings: 8 u band
            hq = rintf((e / sum) / pp.scale);
          const int a = (int)clamp_nanprop(hq + pp.zp, pp.lo, pp.hi) - 128;
          word |= ((uint32_t)a & 0xffu) << (8 * r);
        }
        fp[s][tt] = (int)word;
      }
  }

  TQ_STAMP(4);
  if (!SPLIT && !K_LDS) __syncthreads();             // V^T is in LDS
  TQ_STAMP(5);

  // ---- C^T = V^T P^T -------------------------------------------------------------------------------
  // Key-split form (round 6): the kh = 1 wave is done once its probability indices are in LDS; its partner runs the second
  // GEMM over ALL keys.  (Before, both waves ran their half and the kh = 1 wave handed over 1 + 8 d / 16 integer partial
  // sums per lane -- 33 LDS stores, 33 loads and 33 additions per lane against 1 + 1 here; the MFMAs are not the
  // bottleneck.)  The same exact integers either way.
  v4i fpa[KSA];
#pragma unroll
  for (int s = 0; s < KS; ++s) fpa[s] = fp[s];
  if (SPLIT) {
    if (kh == 1) {
#pragma unroll
      for (int s = 0; s < KS; ++s) s_fp[wave][s][lane] = fp[s];
    }
    __syncthreads();
    if (kh == 1) return;
#pragma unroll
    for (int s = 0; s < KS; ++s) fpa[KS + s] = s_fp[wave][s][lane];
  }
  v4i rsp4 = zero4;
#pragma unroll
  for (int s = 0; s < KSA; ++s) rsp4 = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, fpa[s], rsp4, 0, 0, 0);
  v4i accs[DH / 16], csvs[DH / 16];
#pragma unroll
  for (int j = 0; j < DH / 16; ++j) {
    v4i acc = zero4, csv = zero4;
#pragma unroll
    for (int s = 0; s < KSA; ++s) {
      const v4i fv = *reinterpret_cast<const v4i*>(s_vt + (j * 16 + r16) * PITCH + s * 64 + g * 16);
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(fv, fpa[s], acc, 0, 0, 0);
      csv = __builtin_amdgcn_mfma_i32_16x16x64_i8(fv, ones, csv, 0, 0, 0);              // sum_k a'_v of rows 4g + r
    }
    accs[j] = acc;
    csvs[j] = csv;
  }
  const int rsp = rsp4[0];                           // sum_k a'_p of column r16
  const int p_const = cv * rsp + T * cp * cv;
#if TQ_ATTN_RAGGED
  if (qrow >= tv) return;                            // pad query: nothing to store (behind the last barrier)
#endif
  const size_t out_row = (TQ_SEQ_ROW0 + qrow) * ((size_t)p.H * DH) + (size_t)h * DH;
#pragma unroll
  for (int j = 0; j < DH / 16; ++j) {
    const v4i acc = accs[j], csv = csvs[j];
    float o[4];
    uint32_t oi = 0;
    if (fast_ctx) {                                  // exact branch-free quantizer (tq_device.h QF): no IEEE division
      f32x2 v2[2], h2[2];
#pragma unroll
      for (int r = 0; r < 4; ++r) v2[r >> 1][r & 1] = (float)(acc[r] + cp * csv[r] + p_const) * s_pv;
      qf_round2_n<2>(v2, fc, h2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float hh = h2[r >> 1][r & 1];
        oi = __builtin_amdgcn_cvt_pk_u8_f32(hh + pc.zp, r, oi);
        o[r] = bad_row ? __builtin_nanf("") : pc.scale * (hh + 0.0f);
      }
      oi ^= 0x80808080u;                             // int8(index - 128)
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = (float)(acc[r] + cp * csv[r] + p_const) * s_pv;
        if (p.has_ctx) {
          const float xi = q_index(v, pc);
          oi |= ((uint32_t)((int)xi - 128) & 0xffu) << (8 * r);
          v = q_dequant(xi, pc);
        }
        o[r] = bad_row ? __builtin_nanf("") : v;       // softmax of a fully masked row is NaN in the reference
      }
    }
    const size_t off = out_row + j * 16 + g * 4;
    *reinterpret_cast<f32x4*>(p.ctx + off) = f32x4{o[0], o[1], o[2], o[3]};
    if (p.ctx_idx) *reinterpret_cast<uint32_t*>(p.ctx_idx + off) = oi;
  }
  TQ_STAMP(6);
#undef TQ_SEQ_ROWS
#undef TQ_SEQ_ROW0
#undef TQ_ROW
