"""Process-wide switches of the MI355X path (extensions beyond the reference's behaviour)."""
import torch

# Run quantized Linears with fixed ranges as exact integer GEMMs on the i8 matrix cores with bias / activation / output
# quantizer fused into the epilogue (tq_linear_i8_fwd); quantizers with a fixed per-tensor range then also emit their int8
# grid indices in the same launch so that the GEMM can consume them directly, and the harness models run their fused
# fixed-range tails / attention cores.
#   'auto' (default): whenever autograd is off (torch.no_grad()) -- the fixed-range EVALUATION forward (and, for large GEMMs,
#           calibrating forwards: INT8_CALIBRATION below).
#           Training and anything with forward hooks on the modules involved keep the layered route (one launch per
#           quantizer around torch's fp32 GEMM, the reference's module chain); so do the fused tails / attention core / small
#           GEMMs of a calibrating forward (their quantizers are still estimating).
#   True:   also under autograd (QAT forward on the matrix cores, straight-through backward).
#   False:  never -- the layered route everywhere.
# Why 'auto' is the default (round 5, profiles/r05/int_vs_reference.json, tests/test_bert_e2e.py / test_mobilebert_e2e.py
# `..._default_route_...`): against the REFERENCE's own outputs the integer route is as close as the layered GPU route --
# the layered route's hipBLASLt GEMMs differ from the reference's CPU GEMMs by fp32 round-off just as the exact integer
# contraction does, and through 12-24 quantized layers either difference is amplified the same way (BERT-base W8A8,
# reference ranges installed: 24.67 % vs 24.56 % of the last layer's 786 432 outputs on the reference's grid point, mean
# deviation 1.283 vs 1.291 steps; first layer 99.80 % vs 99.20 %) -- while it is deterministic, exact arithmetic and 4x
# faster (3.26 -> 0.80 ms).
# Per-embedding-group (PEG) activation grids: a Linear whose INPUT lies on a PEG grid (classes of 128-column multiples,
# <= 24 of them) and whose output quantizer is per-tensor runs the class-ordered integer Linear (tq_linear_i8_cls_fwd;
# BERT's first feed-forward Linear under {'x', 'h', 'y'}: 'ng6').  Residual + LayerNorm tails whose quantizers are per-column
# run as one launch (tq_residual_layernorm_quant_axis_fwd, rows of <= 1024 columns), which applies BERT's per-column `h` behind
# an integer FFN2 without output quantizer.  Per-column output quantizers INSIDE a Linear's epilogue, NoNorm tails, the
# attention core and calibrating forwards keep the layered route for PEG sites.
# Mixed precision (W8A16, `--quant-dict "{'x': 16, 'h': 16, 'y': 16}"`): BERT's first feed-forward Linear, whose INPUT lies on a
# per-tensor asymmetric grid of 9..16 bits (site x), runs index-only on the 16-bit integer Linear (tq_linear_i16x8_fwd) from
# the two byte planes of its indices (tq_quantize_hilo_fwd, one launch over the fp32 input), inside the fused feed-forward
# block only; 16-bit `h` and `y` are per-tensor quantizers of the fused tail.  A 16-bit PEG input, a Linear on its own (outside
# that block), calibration, autograd and observed modules keep the layered route for 16-bit inputs.
INT8_LINEAR = 'auto'

# Calibrating forwards (ranges still being estimated, autograd off) on the integer route as well: a quantized Linear whose
# INPUT was produced by a quantizer that has just set its range for this batch (per-tensor asymmetric <= 8 bit) and whose
# weight grid is known runs the exact integer GEMM (bias + activation function in the epilogue, fp32 result to the output
# quantizer's estimator) instead of the fp32 simulation -- the GEMMs are 2 of the 4.2 ms of a BERT-base calibrating forward
# at [8,128] and 25 of 33 ms at [128,128].  The statistics each estimator sees are those of the EXACT products the fp32
# GEMMs approximate (ranges differ from the layered GPU route's by its round-off, as the layered GPU route's differ from
# the reference's CPU GEMMs); everything else -- estimators, state machine, exchanges of a sharded calibration -- is the
# layered code.  Follows INT8_LINEAR: off where that is off (and under autograd / training mode / forward hooks).
INT8_CALIBRATION = True
# ... for GEMMs of at least this many multiply-accumulates (M x K x N; 2^33 = 16 384 tokens through a 768 x 768 Linear, 4 096
# through BERT's feed-forward Linears).  Below, the ~45 us of extra host work + one more launch per layer (the input's
# indices) cost an EAGER calibrating forward more than the fp32 GEMM they replace (profiles/r06/calib_int8_ab.txt: with
# every Linear on the integer path [8,128] went 7.8 -> 12.2 ms eager while its hipGraph went 4.2 -> 3.2 ms; [128,128]:
# 33.1 -> 19.1 ms either way).  The rule depends on the shapes only, so a recorded forward takes the route the eager one took.
INT8_CALIBRATION_MIN_MACS = 1 << 33

# Integer Linears with a GELU: evaluate activation + output quantizer through a staircase table built on the device from
# the quantizer's range (csrc/tq_stair.hip, one extra launch per range state) instead of the erf fit + exact quotient in
# the epilogue.  The table is the correctly rounded GELU followed by the reference quantizer, exact by construction; the
# arithmetic epilogue stays in place for grids the table cannot hold (decided on the device).
# Reproducibility note: the table evaluates the CORRECTLY ROUNDED GELU, the arithmetic epilogue a degree-7 erfc fit; they
# agree on all but <= 2e-5 of the outputs, where the index differs by ONE grid step.  Which of the two a launch uses depends
# on the tile kernel (call shape: M, N), on the room for the table and on the builder's verdict -- so the same layer with
# the same ranges can differ in those few indices between batch sizes.  Every launch is deterministic; set
# INT8_ACT_STAIR = False for one definition (the fit) at every shape.
INT8_ACT_STAIR = True

# BERT's head on the integer route: the pooler (Linear + Tanh on the first token, M = batch rows) and the classifier
# (N = num_labels output features) have shapes no tile of the integer Linear covers, so by default they run layered -- fp32
# GEMMs through hipBLASLt, whose bits depend on the BLAS build: the logits are the one output of the default route that is
# not reproducible across platforms.  With this switch a Linear whose input lies on a fixed per-tensor asymmetric <= 8-bit
# grid and has at most 256 rows (in_features a multiple of 16, <= 16384) runs tq_linear_i8_skinny_fwd instead: the same
# exact integer contraction on the vector ALU, Tanh / GELU evaluated in float64 and narrowed once, the reference
# quantizer's own arithmetic -- one definition at every shape, bit-equal to a CPU evaluation (tests/test_bert_head_route.py).
# The harness model reads the first token's indices in place (quantization/fused.py first_token_linear).  Inference only;
# hooks, unsigned weight grids, estimating quantizers and learnable ranges keep the layered route as for the other plans.
# Off by default: the whole-model tests fix the default route's launches.  Measured (profiles/r09/int8_head.txt,
# tools/tuning/head_time.py; BERT-base default-route forward as hipGraph replays, the two arms interleaved): [8,128] 670.3 us
# with the switch on against 682.6 us off, [128,128] 4002.6 against 4009.9 us (inside the spread); the two launches alone take
# 5.4 us (pooler, batch 8) and 3.6 us (classifier).  Flipping the default is left to a change that also moves those tests.
# The switch also covers the 16-bit head sites and packed batches, through tq_linear_i16x8_skinny_fwd (the 8-bit entry is this one
# without planes and without a row table: planes are the two bytes of a <= 16-bit index, the table is a device tensor of rows):
#  * a pooler whose output quantizer has 9..16 bits (site 'P': 16 of the STS-B recipe) writes y AND the byte planes of its
#    indices, which travel in y's provenance record (`planes`); the classifier reads them -- no tq_quantize_hilo_fwd launch
#    in between -- with a 16-bit ('C': 16), 8-bit or no output quantizer.  Without such a record a 16-bit classifier input
#    stays layered: the head is one route.
#  * `forward_packed` runs the pooler with seq_start[:-1] as the row table on the hidden state's indices (no gather, no
#    host read: capturable, a replay is valid for other lengths of the captured B and M).
# tests/test_bert_mp16_head_route.py, tests/test_bert_packed_head_route.py: logits torch.equal to the CPU twin.  Measured
# (profiles/r13/mp16_head.txt, tools/tuning/mp16_head_time.py; medians of interleaved hipGraph replays, against the same build
# with the backend method hidden = the previous route): STS-B recipe [8,128] 810.8 against 829.7 us, [128,128] 5409.9 against
# 5427.0 us; packed W8A8 at B = 8 636.2 against 649.7 us, B = 128 2610.2 against 2624.4 us.
INT8_HEAD = False

# Integer route for any sequence length.  Evaluation batches padded only to their longest sequence (the reference's
# `--no-pad-to-max-length`) have an arbitrary T; the attention core takes T % 64 == 0 and the tiled integer Linears M % 32 == 0
# rows, so by default such a batch runs the encoder layered -- fp32 GEMMs through hipBLASLt, outside
# the bit-for-bit GPU == CPU statement of tests/test_bert_exact_route.py.  With this switch, for the per-tensor <= 8-bit
# plan: the attention core runs tq_attention_i8_ragged_fwd for 1 <= T <= 512 (bit-identical to the core on the batch padded
# to 64 * ceil(T / 64) with -inf on the pad keys; nothing outside the B * T rows is read or written) and every tiled integer
# Linear is launched over 64 * ceil(M / 64) rows of buffers the backend allocates with that room (rows are independent: exact
# on the first M; HipBackend.PADS_ROWS; the roomy allocation is made only while this switch is on).  With INT8_HEAD on too, a
# Linear that may take either plan keeps the skinny one.  The fused tails and the embedding block take any row count already.  PEG and W8A16
# plans (without INT8_RAGGED_RECIPES, below), skinny plans, MobileBERT's chains, calibration and training keep today's shape rules.  Inference only.
# Off by default: existing tests fix what happens at such shapes today.  Measured (profiles/r10/ragged_route.txt,
# tools/tuning/ragged_time.py; BERT-base forward as hipGraph replays, arms interleaved): [8,100] 712.6 us on against 2083.0 us
# off, [128,100] 3394.9 against 7437.6 us; the same batches padded by the caller to T = 128: 715.8 / 3988.4 us.
INT8_RAGGED = False


def int8_ragged(be):
    """INT8_RAGGED with a backend that has the ragged attention core and pads row tails itself"""
    return bool(INT8_RAGGED) and hasattr(be, 'attention_i8_ragged') and bool(getattr(be, 'PADS_ROWS', False))


# The W8A16 and PEG recipes on the integer route at any sequence length.  INT8_RAGGED keeps the per-tensor <= 8-bit plan on the
# route at any token count, but FFN1 under {'x': 16, 'h': 16, 'y': 16} (tq_linear_i16x8_fwd on the byte planes of site x) and
# under {'x', 'h', 'y': 'ng6'} / 'ngp6' (tq_linear_i8_cls_fwd on x's class-ordered indices) took whole 64-row tiles only: at
# B * T % 64 != 0 it ran layered -- a requantize, an fp32 hipBLASLt GEMM, a [M, 3072] fp32 activation, GELU and a fake-quant --,
# the hidden states were no longer bit-equal to a CPU evaluation, and INT8_PLANE_TAILS, INT8_PLANE_RESIDUALS and
# INT8_PEG_INDEX_RESIDUALS declined for the whole layer.  With this switch the MP16 and PEG plans accept any M >= 1 where the
# caller asks with ragged=True (the fused feed-forward block and the three site-x routes): the backend launches the same two
# kernels over 64 * ceil(M / 64) rows of buffers with that room (HipBackend.PADS_RECIPE_ROWS; `_rows_empty`, `_rows_operand`),
# exactly as it does for tq_linear_i8_stair_fwd.  No kernel and no C entry changed.  The pad rows hold whatever the memory held:
# the operands are integers (any byte is a valid index; there is no NaN or trap value to meet) and the rows of a Linear are
# independent, so the first M rows are exact and nobody reads the rest.  K % 128, N % 64 and inference only stay.
# Needs all three: this switch, INT8_RAGGED (the ragged attention core, row tails and the roomy allocations are its) and a
# backend that declares PADS_RECIPE_ROWS.  It cannot ride on INT8_RAGGED alone: tests/test_peg_index_residuals_host.py and
# tests/test_bert_peg_index_residuals_route.py pin today's decline under that switch.  Off by default: the existing whole-model
# tests fix today's launches.  `forward` and `forward_packed` of harness.bert stay on the integer route under both recipes, with
# and without INT8_HEAD (tests/test_ragged_recipes_host.py, tests/test_bert_ragged_recipes_route.py: hidden states and logits
# torch.equal to the CPU twin, and to the batch padded by the caller to whole tiles).
# Measured (profiles/r19/ragged_recipes.txt, tools/tuning/ragged_recipes_time.py; BERT-base forward as hipGraph replays, 60
# interleaved rounds, medians, against the same build with this switch off, INT8_RAGGED on in both arms): W8A16 [8,100] 865.5 us
# on against 1339.1 us off, packed B = 8 (M = 567) 723.0 against 1063.7 us, packed B = 128 (M = 9135) 4054.4 against 7978.6 us;
# PEG [8,100] 808.7 against 1356.2 us, packed B = 8 752.8 against 1105.3 us, packed B = 128 3700.9 against 8012.9 us.  [128,100]
# is M = 12800 = 200 whole tiles: the switch changes no launch there and the arms came out level (4336.5 / 4334.3 us, 3794.6 /
# 3803.8 us).  The logits of the two arms differ by FFN1's fp32 round-off amplified through the layers: 1.5 % of max |off| on
# 3-layer models (inside the 5 % default-against-layered bar of tests/test_bert_mp16_route.py, which is a 3-layer statement),
# 7.7-13.9 % on the 12-layer models that were timed (outside it).
INT8_RAGGED_RECIPES = False


def int8_ragged_recipes(be):
    """INT8_RAGGED_RECIPES on top of `int8_ragged`, with a backend that pads the row tails of the MP16 and PEG Linears too"""
    return bool(INT8_RAGGED_RECIPES) and int8_ragged(be) and bool(getattr(be, 'PADS_RECIPE_ROWS', False))

# Residuals as int8 indices in the residual + LayerNorm tails.  Every hidden state between launches of the integer route is a
# value on an 8-bit grid whose producer already emitted its int8 indices, yet both tails of a BERT layer read their residual
# as fp32 and write an fp32 `y` beside `y_idx`: 26 B per element and layer over the two tails.  With this switch the per-tensor
# fp32 LayerNorm tails run tq_residual_layernorm_quant_ires_fwd: the residual goes in as the producer's indices (dequantized
# in registers: the producer's own bits) with one NaN flag per row beside them (an index cannot say NaN; the flag keeps "a row
# with a NaN input is NaN as a whole" intact from launch to launch: provenance.row_nan_of), and the attention-output tail,
# whose fp32 output only the feed-forward block reads (FFN1 as indices, the FFN tail as residual), writes indices and flags
# alone (quantization/fused.py quantized_bert_attention_output_ffn) -- 16 B per element and layer, bit-identical results, NaN
# rows included.  The first tail of a forward reads the embedding block's fp32 output (no flags known yet) and starts the
# chain.  The layer's output keeps its fp32 `y`.  PEG (per-column) tails, tails with a grid of more than 8 bits (W8A16),
# NoNorm, hooks or save targets on site x and backends without the entry keep today's launches.  Inference only.
# Off by default: the whole-model tests fix the default route's launches.  Measured (profiles/r12/index_residuals.txt,
# tools/tuning/ires_time.py; BERT-base default-route forward as hipGraph replays, the two arms interleaved): [128,128] 3921.6 us
# with the switch on against 4028.8 us off, [8,128] 680.5 against 680.7 us (inside the spread: that forward is bound by its
# launches); the tail alone at [131072,768] 232.6 -> 182.7 us with y, 127.0 us index-only.
INT8_INDEX_RESIDUALS = False

# LayerNorm tails write the byte planes of 16-bit outputs (W8A16).  Under a mixed-precision recipe such as {'x': 16, 'h': 16,
# 'y': 16} the output of the attention-output tail (site x) lies on a 16-bit per-tensor grid and feeds the 16-bit integer Linear
# (tq_linear_i16x8_fwd), which reads the index as two int8 byte planes: by default one tq_quantize_hilo_fwd launch per layer
# reads the fp32 x back and re-derives the index the tail held in registers.  With this switch a per-tensor fp32 LayerNorm
# tail whose output grid is fixed, asymmetric, linear and 9..16 bits wide runs tq_residual_layernorm_quant_planes_fwd: the
# same y, bit for bit, and the two planes from the same launch (2 B per element beside 12), which travel in y's provenance
# record (`planes`).  FFN1 reads them (autoquant_utils._int8_operands) and so does, under INT8_HEAD, the pooler behind a
# 16-bit last hidden state (site z of the last layer; fused.first_token_linear reads the first-token rows of the planes in
# place, strided or through the row table of a packed batch) -- the head of such a recipe leaves the layered route.  A record
# is valid only for the unchanged tensor object on an unchanged grid; anything else (hooks, save targets, estimating
# quantizers, grad mode, per-column or NoNorm tails, bf16, <= 8-bit grids) keeps today's launches.  Inference only.
# Off by default: tests/test_bert_mp16_route.py fixes one tq_quantize_hilo_fwd launch per layer on the default route.
# Measured (profiles/r15/plane_tails.txt, tools/tuning/plane_tails_time.py; BERT-base forward under {'x': 16, 'h': 16, 'y': 16} as
# hipGraph replays, the two arms interleaved): [8,128] 788.6 us with the switch on against 823.3 us off, [128,128] 5297.5 against
# 5431.1 us; the tail alone at [1024,768] 7.94 us (existing tail + quantize_hilo) -> 4.46 us, at [131072,768] 320.9 -> 254.2 us
# (DESIGN.md section 5).
INT8_PLANE_TAILS = False

# Residuals as byte planes in the LayerNorm tails for W8A16.  INT8_INDEX_RESIDUALS does nothing under {'x': 16, 'h': 16, 'y': 16}
# (a 16-bit index does not fit its int8 residual), and INT8_PLANE_TAILS still writes site x -- the attention-output tail's
# result, FFN1's input and the feed-forward tail's residual -- as fp32 beside its planes and reads it back as fp32.  With this
# switch a BERT layer whose site x lies on a fixed asymmetric linear per-tensor grid of 9..16 bits runs both tails through
# tq_residual_layernorm_quant_pres_fwd (quantization/fused.py quantized_bert_attention_output_ffn): the attention-output tail
# reads its residual h as the producer's int8 indices + row flags (fp32 in layer 0) and writes the two byte planes of x and one
# NaN flag per row, nothing else; FFN1 (tq_linear_i16x8_fwd) reads the planes; the feed-forward tail dequantizes them in
# registers -- scale * (index - zero_point), the bits the plane tail writes as y -- and writes y, its int8 indices and flags.
# 18 B per element and layer over the two tails against 27 with INT8_PLANE_TAILS; bit-identical hidden states and logits, NaN
# rows included (tests/test_bert_plane_residuals_route.py).  Declines, before the first launch, to today's launches (the plane
# tail and the index-residual route included): a feed-forward tail whose output has more than 8 bits (site z of the STS-B head
# recipe's last layer), a token count that is no multiple of 64 (FFN1's MP16 plan; not with INT8_RAGGED_RECIPES), unsigned weight grids, hooks or save
# targets on site x, estimating quantizers, grad mode, per-column or NoNorm tails, bf16, a backend without the entry.
# Inference only.  Off by default: tests/test_bert_plane_tails_route.py fixes the plane-tail launches of that recipe.
# Measured (profiles/r17/plane_residuals.txt, tools/tuning/plane_residuals_time.py; BERT-base forward under {'x': 16, 'h': 16,
# 'y': 16} as hipGraph replays, interleaved with the same build with this switch off and INT8_PLANE_TAILS on): [8,128] 776.0 us
# against 798.3 us, [128,128] 5313.6 against 5472.8 us (both 0.97x).  The launches alone beside the ones they replace: the
# attention-output tail at [1024,768] 4.58 us (plane tail) -> 4.35 us (4.10 us with an fp32 residual), at [131072,768] 222.7 ->
# 143.8 us (181.3 us); the feed-forward tail at [131072,768] 224.9 -> 196.3 us, but at [1024,768] it is SLOWER than the existing
# tail, 4.71 against 4.56 us: it is the y form of the index-residual body, which was 0.18 us behind that tail at this size
# already (INT8_INDEX_RESIDUALS above); not profiled further.
INT8_PLANE_RESIDUALS = False

# Residuals as int8 indices in the per-column (PEG) LayerNorm tails.  INT8_INDEX_RESIDUALS does nothing where a tail has a
# per-column quantizer, so under {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'} (and 'ngp6') both tails of every layer run
# tq_residual_layernorm_quant_axis_fwd: fp32 in, fp32 out, 26 B per element and layer.  With this switch a BERT layer one of whose
# tails has a per-column quantizer runs both through tq_residual_layernorm_quant_axis_ires_fwd (quantization/fused.py
# quantized_bert_attention_output_ffn): the attention-output tail reads its residual h as the producer's int8 indices + row
# flags (fp32 in layer 0, or behind a layer that declined) and writes the int8 indices of x (natural column order) and one NaN
# flag per row, nothing else; FFN1 (tq_linear_i8_cls_fwd) reads the indices; the feed-forward tail dequantizes them in registers
# on x's per-column grid -- max(delta_c, eps) * (index - clamp(round(zero_float_c))), the bits the axis tail writes as y -- and
# writes y, its int8 indices and flags.  16 B per element and layer; bit-identical hidden states and logits, NaN rows included
# (tests/test_bert_peg_index_residuals_route.py).  Declines, before the first launch, to today's launches: a token count that is
# no multiple of 64 (FFN1's PEG plan; not with INT8_RAGGED_RECIPES), d = 1024 (the residual's per-column grid does not fit in LDS beside the axis tail's
# tables), bf16, a site x or site y that is symmetric, in the log domain or wider than 8 bits, unsigned weight grids, hooks or
# save targets on site x, estimating quantizers, grad mode, NoNorm, a backend without the entry.  Inference only.  Off by
# default: tests/test_bert_peg_route.py fixes the axis-tail launches of the recipe.
# Measured (profiles/r18/peg_index_residuals.txt, tools/tuning/peg_ires_time.py; BERT-base forward under {'x': 'ng6', 'h': 'ng6',
# 'y': 'ng6'} as hipGraph replays, interleaved with the same build with this switch off): [128,128] 4418.3 us against 4474.5 us
# (0.987x), but [8,128] 786.2 against 778.7 us: 1 % SLOWER.  The launches alone beside tq_residual_layernorm_quant_axis_fwd: the
# attention-output tail at [1024,768] 6.03 -> 5.92 us (5.66 us with an fp32 residual), at [131072,768] 221.3 -> 192.0 us; the
# feed-forward tail at [131072,768] 232.7 -> 225.7 us, at [1024,768] 6.05 -> 6.55 us: slower; not profiled further (DESIGN.md
# section 5).
INT8_PEG_INDEX_RESIDUALS = False

# The attention half of a BERT layer on the integer route under `--per-groups N` (per-embedding-group grids on every [B, T, d]
# activation; harness.bert.apply_activation_granularity(model, per_groups=N)).  The feed-forward half of that recipe already runs
# integer (tq_linear_i8_cls_fwd, per-column LayerNorm tails), the attention half layered: Q, K, V and the context carry
# per-column output grids, which `QuantLinear._int8_plan_from`, `fused.quantized_self_attention` and the core refused.  Without
# permutation a group is a run of d / N columns -- whole heads and whole output tiles where d / N is a multiple of 64 and of
# head_dim --, so with this switch `quantized_self_attention` runs ONE index-only tq_linear_i8_cls_grouped_fwd for the stacked
# Q | K | V (class-ordered input, block-constant per-column output grids) and ONE attention core with a grid per head
# (tq_attention_i8*_fwd with wide quantizers); the context leaves with its natural-order int8 indices for the attention-output
# Linear's PEG plan.  An input grid whose classes are no multiple of 128 columns (per_groups 12, 4 at d = 768) goes in with its
# classes padded to whole K slabs (peg.PaddedClassLayout).  Exact: tests/_peg_attention_twin.py is its CPU twin.  Declines, before the first launch, to today's
# launches: permuted groups or per-embedding grids (not constant over a head and over blocks of 64 columns), symmetric or
# log-domain grids, grids above 8 bits, hooks, save targets, estimating quantizers, grad mode, packed batches, MobileBERT's
# separate inputs, bf16, a ragged T or B * T without INT8_RAGGED + INT8_RAGGED_RECIPES, a backend without the entry, a layer
# without any per-column grid (the per-tensor recipe keeps its own launches).  Inference
# only.  Off by default: tests/test_bert_peg_route.py fixes today's launches of the recipe.
INT8_PEG_ATTENTION = False


def int8_peg_attention(be):
    """INT8_PEG_ATTENTION with a backend that has the grouped class-ordered Linear"""
    return bool(INT8_PEG_ATTENTION) and hasattr(be, 'linear_i8_cls_grouped')


# BERT's embedding block as ONE launch under `--per-embd`, `--per-groups N` and `--per-groups-permute`, where its three
# activation sites (sum_input_token_type_embd_act_quantizer, sum_pos_embd_act_quantizer, embeddings.LayerNorm) are per-column
# quantizers (harness.bert.apply_activation_granularity).  tq_embeddings_layernorm_quant_fwd takes per-tensor quantizers only,
# so under these recipes `fused.embeddings_layernorm_quant` declined and the block ran layered: three look-ups, two adds,
# three fake-quant launches and torch's LayerNorm, 13 launches that read and write [B, T, d] nine times.  With this switch it
# is one tq_embeddings_layernorm_quant_axis_fwd (each site absent, per-tensor or per-column; d in 64 .. 1024), whose output
# leaves with its int8 indices under the rule of the per-tensor block.  Exact against the CPU chain
# (tests/_exact_backend.embeddings_chain), which torch's LayerNorm on the GPU is not: with it the PEG recipe's GPU forward
# equals its CPU twin from the input ids on (tests/test_bert_peg_embeddings_route.py).  Declines, before the first launch, to
# the layered modules: hooks, save targets, estimating quantizers, training modules, grad mode, a row length without an
# instantiation, log-domain or per-channel grids, a backend without the entry.  A block without any per-column site keeps the
# per-tensor launch whatever this switch says.  Off by default: the layered block is what tests/test_bert_peg_route.py fixes.
# Packed batches: with this switch AND INT8_PEG_ATTENTION on, `fused._peg_self_attention` also takes a PackedSequences (grouped
# class-ordered Linear over the packed rows, tq_attention_i8_varlen_fwd with a grid per head), so `forward_packed` equals the CPU
# twin from the ids on as well; INT8_PEG_ATTENTION alone keeps declining packed batches (tests/test_peg_attention_host.py).
# Measured (profiles/r21/peg_embeddings.txt, tools/tuning/peg_embeddings_time.py; BERT-base forward under per_groups=6 as hipGraph
# replays, interleaved with the same build with this switch off, INT8_PEG_ATTENTION on): [8,128] 870.9 us against 899.4 us,
# [128,128] 5056.4 against 5185.5 us.  The launch alone: 6.21 us at [1024,768] and 30.7 us at [16384,768], level with
# tq_residual_layernorm_quant_axis_fwd on dense rows (6.02 and 30.4 us); the per-tensor block takes 4.84 and 24.9 us.
INT8_PEG_EMBEDDINGS = False


def int8_peg_embeddings(be):
    """INT8_PEG_EMBEDDINGS with a backend that has the per-column embedding launch"""
    return bool(INT8_PEG_EMBEDDINGS) and hasattr(be, 'embeddings_layernorm_quant_axis')


# README recipe (MSE / golden-section weight ranges, reference README.md:149-157): run the searches of ALL weight tensors in
# lock step before the first calibrating forward (autoquant_utils.precalibrate_weights -> range_estimators.
# golden_section_lockstep): every search is scipy's bounded Brent restated as a resumable generator (pinned against scipy,
# tests/test_lockstep.py), each round evaluates the pending candidate of every live search with prepared launches queued
# back to back and ONE device->host copy.  Bit-identical ranges; BERT-base (102 tensors, 2 096 evaluations in 26 rounds):
# 148-156 ms layer by layer (71-75 us per evaluation: 11 us of kernels, 17 us of synchronisation, ~25 us of Python) ->
# 64.5 ms (2.3x; the kernels alone are ~38 ms).  (A first version with one scipy instance per search in its own THREAD was
# slower than layer by layer -- 250-290 ms: 102 thread wake-ups per round -- and is gone.)
LOCKSTEP_WEIGHT_SEARCH = True

# Estimator state (current_xmin / current_xmax) and quantizer parameters (_delta / _zero_float / _signed)
# are rebound to FRESH tensors on every calibrating forward, like the reference does.  With this switch
# the fused calibration step updates the existing buffers IN PLACE once they exist (same values, same
# shapes), which makes a calibrating forward replayable as a hipGraph: capture one forward after the
# first (eager) batch, then copy each new batch into the static input and replay -- no Python, no
# allocation, no host synchronisation between the 161 + 102 quantizers of a BERT-base.  Off by
# default because code that keeps references to earlier state tensors would see them change.
INPLACE_CALIBRATION_STATE = False

# AdaRound: after three eager iterations the loop body (sample gather, soft-quantized weight, layer forward, gradient
# GEMM, fused backward + regulariser + Adam) is recorded once as a hipGraph and replayed for the remaining iterations,
# with the per-iteration sample indices and schedule scalars read from device tables.  Same kernels in the same order
# on the same data: the learned rounding is bit-identical to the eager loop (tests/test_adaround_inits.py).  Applies to
# the fused step of plain Linear layers (closed-form gradient, no folded activation function) on one GPU with the
# relaxation loss; anything else runs the eager loop.
GRAPH_ADAROUND = True

# Bumped by anything that rewrites parameters or range buffers behind autograd's back -- a hipGraph replay of a training
# step updates weights and learnable ranges in place WITHOUT touching tensor._version -- so that every derived cache
# (int8 weight indices, NoNorm parameters, stacked QKV operands, provenance records) sees a new key:
# QuantizerBase.range_state_key() includes it.
CACHE_EPOCH = 0


def int8_active():
    """Is the integer / fused fixed-range route on for the call being made right now?  (see INT8_LINEAR)"""
    m = INT8_LINEAR
    if not m:
        return False
    # torch.inference_mode(): tensors created there carry no version counter, so an in-place change of an activation between
    # the quantizer that produced it and the integer Linear that consumes its indices could not be noticed (provenance.py):
    # the layered route runs there, whatever the switch says.  torch.no_grad() keeps the counters and is what 'auto' is for.
    if torch.is_inference_mode_enabled():
        return False
    if m is True:
        return True
    return not torch.is_grad_enabled()


def fuse_on(flag, module=None, probe=None):
    """Tri-state `fuse` switches of the harness models: True / False force it, None (default) follows INT8_LINEAR for
    modules in eval mode whose ranges are fixed.  probe: a QuantizedActivation / quantized layer of the block whose
    manager's state stands for the block's (a calibrating forward then skips the fused helpers' eligibility checks
    altogether instead of failing them one by one: ~1 ms of host time per BERT-base forward)."""
    if flag is None:
        if not int8_active() or (module is not None and module.training):
            return False
        if probe is not None:
            mgr = probe._modules.get('activation_quantizer')
            state = getattr(mgr, 'state', None)
            return state is None or state.name == 'fix_ranges'
        return True
    return bool(flag)


def invalidate_derived_caches():
    global CACHE_EPOCH
    CACHE_EPOCH += 1
