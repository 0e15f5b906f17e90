"""Fused fixed-range layer tails -- new, no counterpart module upstream.

``residual_layernorm_quant`` runs the tail of BertSelfOutput / BertOutput
(reference models/quantized_bert.py:238-248, 264-280)

    Q_ln( LayerNorm( Q_res( Q_dense(dense_out) + residual ) ) )

as ONE kernel (``tq_residual_layernorm_quant_fwd``: 2 reads + 1 write of [B*T, d]) when every
quantizer involved has a fixed per-tensor range -- or, for LayerNorm rows of up to 1024 columns, a fixed range per
column (per-embedding / per-embedding-group quantizers: ``tq_residual_layernorm_quant_axis_fwd``); otherwise it runs the
layered modules (the same HIP kernels, one launch per stage), so calibration / QAT keep their exact
semantics.  ``scores_softmax_quant`` does the same for the attention probabilities
(``tq_scores_softmax_quant_fwd``: quantizer -> 1/sqrt(d) -> mask -> softmax -> quantizer, 1 read + 1 write).
"""
from collections import namedtuple

import torch

from quantization import _hip
from quantization import options
from quantization import peg as peg_layout
from quantization import provenance
from quantization.autoquant_utils import (INT8_STATS, QuantEmbedding, QuantLayerNorm, QuantLinear, QuantNoNorm,
                                          _fixed_per_tensor_manager, _hooked)
from quantization.base_quantized_classes import FP32Acts
from quantization.int8_route import MP16, PEG, SKINNY, TILED, QSpec, XGrid, emits_int8, emits_planes, tagged
from quantization.quantization_manager import QuantizationManager, Qstates

NOT_FUSABLE = object()      # what the helpers below answer for a quantizer no fused launch can take (compared with `is`)


def _fixed_along_last(enabled, mgr, d=None):
    """-> (None | NOT_FUSABLE | QSpec): disabled quantizer, not fusable, or kernel arguments of a fixed per-tensor quantizer.
    Given the row length d it also accepts a fixed quantizer whose parameters run along the LAST dimension of its input,
    one per column of a row of length d (per-embedding / per-embedding-group quantizers hold `_delta[d]` and
    `_zero_float[d]` in natural column order, permuted groups included): the per-column tail kernel
    (tq_residual_layernorm_quant_axis_fwd) takes those buffers as they are.  Linear scale domain only."""
    if not enabled or isinstance(mgr, FP32Acts):
        return None
    if not isinstance(mgr, QuantizationManager) or mgr.state != Qstates.fix_ranges:
        return NOT_FUSABLE
    q = mgr.quantizer
    if mgr._forward_hooks or mgr._forward_pre_hooks or q._forward_hooks or q._forward_pre_hooks:
        return NOT_FUSABLE               # an observer on a stage the fused launch would skip: layered route
    if not q.is_initialized:
        return NOT_FUSABLE
    delta = q._delta
    if delta.numel() == 1:
        return QSpec.of(q)
    if (d is None or d <= 1 or delta.numel() != d or delta.shape[-1] != d
            or delta.requires_grad or delta.dtype != torch.float32 or getattr(q, 'per_channel', False)
            or q.scale_domain != 'linear'):
        return NOT_FUSABLE
    zf = getattr(q, '_zero_float', None)
    if not q.symmetric and (zf is None or zf.numel() != d or zf.shape[-1] != d or zf.dtype != torch.float32):
        return NOT_FUSABLE
    return QSpec.of(q)._replace(delta=delta.reshape(-1), zero_float=None if zf is None else zf.reshape(-1))


_fixed_per_tensor = _fixed_along_last      # (enabled, mgr): without a row length, per-tensor quantizers only


def _refused(*specs):
    for s in specs:                      # (plain loops here and in _hooked: a generator costs a call per element on a path
        if s is NOT_FUSABLE:             #  that runs some ten times per encoder layer of an eager forward)
            return True
    return False


def _per_column(*specs):
    for s in specs:
        if isinstance(s, QSpec) and s.delta.numel() != 1:
            return True
    return False


def _tail_specs(dense, res_quantizer, layer_norm, d_out=None):
    """(q_dense, q_sum, q_out) of the tail `layer_norm(res_quantizer(dense(.) + residual))`: per-tensor quantizers only, or,
    given the row length d_out, per-column ones too (_fixed_along_last).  (res_quantizer may be an FP32Acts: site switched off.)"""
    return (_fixed_along_last(dense._quant_a and dense.activation_function is None, dense.activation_quantizer, d_out),
            _fixed_along_last(getattr(res_quantizer, '_quant_a', False),
                              getattr(res_quantizer, 'activation_quantizer', res_quantizer), d_out),
            _fixed_along_last(layer_norm._quant_a and layer_norm.activation_function is None, layer_norm.activation_quantizer,
                              d_out))


def _core_args(scores_quantizer, probs_quantizer, context_quantizer, mask, B, T):
    """What both attention helpers hand the integer core besides Q, K, V: (q_scores, q_probs, q_ctx, mask [B,T]), or None --
    a quantizer that is not fixed per-tensor, probabilities off an asymmetric linear <= 8-bit grid, a mask of another shape."""
    qs = _fixed_per_tensor(scores_quantizer._quant_a, scores_quantizer.activation_quantizer)
    qp = _fixed_per_tensor(probs_quantizer._quant_a, probs_quantizer.activation_quantizer)
    qc = _fixed_per_tensor(context_quantizer._quant_a, context_quantizer.activation_quantizer)
    if _refused(qs, qp, qc) or qp is None or not qp.fits_int8:
        return None
    if mask is not None:                 # additive [B,1,1,T] -> fp32 [B,T] for the cores; any other shape: not theirs
        if not (mask.dim() == 4 and mask.shape[0] == B and mask.shape[1] == 1 and mask.shape[2] == 1 and mask.shape[3] == T):
            return None
        mask = mask.reshape(B, T).float().contiguous()
    return qs, qp, qc, mask


class PackedSequences:
    """A batch of B sequences packed row after row, without pad tokens, into [1, M, d] tensors; passed to the attention helpers
    (and to harness.bert's layers) where the additive mask goes.

        seq_start   int32 tensor [B + 1] on the tensors' device, non-decreasing: sequence b owns rows seq_start[b] ..
                    seq_start[b + 1] - 1, seq_start[B] <= M (rows past it belong to nobody)
        max_len     host int, a bound on every length (1..512)

    Every key of a sequence is visible to every query of the same sequence and to no other: there is no additive mask.
    `quantized_self_attention` / `quantized_attention` run such a batch with the variable-length integer core
    (HipBackend.attention_i8_varlen) under options.INT8_RAGGED; `padded` / `unpadded` are the index maps of the layered
    fall-back (plain torch index ops of static shapes: no host synchronisation, safe inside a captured graph)."""

    def __init__(self, seq_start, max_len):
        if not (torch.is_tensor(seq_start) and seq_start.dtype == torch.int32 and seq_start.dim() == 1 and seq_start.numel() >= 2):
            raise ValueError('PackedSequences: seq_start must be an int32 tensor [B + 1]')
        self.seq_start, self.max_len = seq_start, int(max_len)
        self._maps = None

    @property
    def batch(self):
        return self.seq_start.numel() - 1

    def _index_maps(self, M):
        if self._maps is None or self._maps[0] != M:
            B, T = self.batch, self.max_len
            s = self.seq_start.long()
            t = torch.arange(T, device=s.device)
            valid = t[None, :] < (s[1:] - s[:-1])[:, None]                              # [B, T]
            src = (s[:-1, None] + t[None, :]).clamp_(max=M - 1)                         # packed row of (b, t)
            i = torch.arange(M, device=s.device)
            b = torch.bucketize(i, s[1:].contiguous(), right=True).clamp_(max=B - 1)    # owner of packed row i
            dst = b * T + (i - s[b]).clamp_(0, T - 1)                                   # its row of the [B * T] batch
            self._maps = (M, valid, src.reshape(-1), dst)
        return self._maps[1:]

    def padded(self, h):
        """h [1, M, d] -> ([B, max_len, d] with zeros in the pad rows, additive mask [B, 1, 1, max_len]: (1 - valid) * -10000)"""
        valid, src, _ = self._index_maps(h.shape[1])
        x = h[0].index_select(0, src).view(self.batch, self.max_len, h.shape[-1])
        x = torch.where(valid[:, :, None], x, torch.zeros((), dtype=h.dtype, device=h.device))
        return x, ((1.0 - valid.float()) * -10000.0)[:, None, None, :]

    def unpadded(self, y, M):
        """y [B, max_len, d] -> [1, M, d]: the valid rows back in their packed places"""
        _, _, dst = self._index_maps(M)
        return y.reshape(self.batch * self.max_len, y.shape[-1]).index_select(0, dst).unsqueeze(0)


def _varlen_core(be, packed):
    """`attention_i8_varlen` bound to a PackedSequences, with the call signature of the other two cores"""
    def core(q_idx, k_idx, v_idx, num_heads, mask, *rest, **kw):
        return be.attention_i8_varlen(q_idx, k_idx, v_idx, num_heads, packed.seq_start, packed.max_len, mask, *rest, **kw)
    return core


def _packed_ok(packed, B):
    """options.INT8_RAGGED on a backend with the variable-length core, inference only, one packed row of sequences"""
    be = _hip.backend()
    return (options.int8_ragged(be) and hasattr(be, 'attention_i8_varlen') and not torch.is_grad_enabled() and B == 1
            and 1 <= packed.max_len <= 512)


def _attention_core(core, idx, grids, num_heads, head_dim, args, context_quantizer):
    """the integer core on the int8 indices `idx` of Q, K, V and their `grids`; the context leaves with its record"""
    qs, qp, qc, mask = args
    cq = context_quantizer.activation_quantizer.quantizer if qc is not None else None
    want_idx = emits_int8(cq)
    out = core(*idx, num_heads, mask, float(head_dim) ** 0.5, *grids, qs, qp, qc, want_idx=want_idx)
    return tagged(out, cq, want_idx)


def _axis_tail_ok(d, dtype):
    """Row lengths tq_residual_layernorm_quant_axis_fwd is built for: the vector counts of _LN_VECTORS whose per-column
    tables fit in LDS (d <= 1024)."""
    vec = 4 if dtype == torch.float32 else 8
    return (hasattr(_hip.backend(), 'residual_layernorm_quant_axis') and dtype in (torch.float32, torch.bfloat16, torch.float16)
            and d <= _AXIS_MAX_D and d % vec == 0 and d // vec in _LN_VECTORS)


hooked = _hooked      # public name for the harness models (containers they bypass when they take a merged launch)


def residual_layernorm_quant(dense, res_quantizer, layer_norm, x, residual, _gemm=None):
    """dense: QuantLinear, res_quantizer: QuantizedActivation, layer_norm: QuantLayerNorm or MobileBERT's
    QuantNoNorm (tq_residual_nonorm_quant_fwd).  Equivalent to ``layer_norm(res_quantizer(dense(x) + residual))``.
    (_gemm: the pre-quantizer output of `dense`, already computed by quantized_bert_ffn from int8 indices.)"""
    if _gemm is not None:
        x = _gemm
    d_out = dense.out_features if hasattr(dense, 'out_features') else x.shape[-1]
    q1, q2, q3 = _tail_specs(dense, res_quantizer, layer_norm, d_out)
    is_nonorm = isinstance(layer_norm, QuantNoNorm)
    # per-column parameters (per-embedding / PEG quantizers): LayerNorm only, through the per-column kernel, where the
    # backend has it and the row length fits (the GEMM output has x's dtype); everything else keeps the layered modules
    axis = _per_column(q1, q2, q3)
    if axis and (is_nonorm or not _axis_tail_ok(d_out, x.dtype)
                 or tuple(getattr(layer_norm, 'normalized_shape', ())) != (d_out,)):
        q1 = NOT_FUSABLE
    fusable = (not _refused(q1, q2, q3) and dense.activation_function is None
               and layer_norm.activation_function is None and _hip.on_device(x) and x.dtype != torch.float64
               and not (torch.is_grad_enabled() and (x.requires_grad or residual.requires_grad))
               and (is_nonorm or len(layer_norm.normalized_shape) == 1)
               and dense.activation_save_target is None and layer_norm.activation_save_target is None
               and not _hooked(dense, res_quantizer, layer_norm))
    if not fusable:
        if _gemm is not None:
            raise RuntimeError('residual_layernorm_quant: pre-computed GEMM handed to a tail that is not fusable')
        return layer_norm(res_quantizer(dense(x) + residual))
    if is_nonorm and _gemm is None:
        y = _linear_nonorm_i8(dense, layer_norm, x, residual, q1, q2, q3)      # GEMM + whole tail as ONE integer launch
        if y is not None:
            return y
    gemm = _gemm
    if gemm is None and options.int8_active() and hasattr(dense, '_int8_forward'):
        gemm = dense._int8_forward(x, with_output_quantizer=False)     # exact integer GEMM (MFMA i8)
    if gemm is None:
        w, b = dense.get_params()
        gemm = dense.run_forward(x, w, b)                   # hipBLASLt through torch (fp32 simulation)
    if is_nonorm:
        # one weight quantizer serves weight and bias, in this order (upstream quirk, autoquant_utils.QuantNoNorm)
        ln_w, ln_b = layer_norm.quantized_params()          # cached with fixed ranges in inference
    else:
        ln_w, ln_b = layer_norm.get_params()                # fake-quantized (cached in eval) affine
    oq = layer_norm.activation_quantizer.quantizer if q3 is not None else None
    want_idx = options.int8_active() and emits_int8(oq) and gemm.dtype == torch.float32
    if (want_idx and residual.dtype == torch.float32 and _route_on(_hip.backend(), _INDEX_ROUTE)
            and _route_tail_ok(_INDEX_ROUTE, layer_norm, d_out, q1, q2, q3)):
        # options.INT8_INDEX_RESIDUALS: the residual as its producer's indices + row flags where its record holds both, else
        # as fp32 (the embedding block's output, once per forward); the output leaves with indices and flags
        res = _index_residual(residual)
        if res is not None:
            y, idx, row_nan = _hip.backend().residual_layernorm_quant_ires(gemm, *res, q1, q2, ln_w, ln_b, layer_norm.eps, q3)
            return provenance.tag(y, oq, idx, row_nan=row_nan)
    if _planes_tail_ok(layer_norm, d_out, gemm, residual, q1, q2, q3, oq):
        # options.INT8_PLANE_TAILS: y and the byte planes of its 9..16-bit indices from one launch; the 16-bit integer Linear
        # (and the pooler's first-token rows) read the planes from y's record
        y, planes = _hip.backend().residual_layernorm_quant_planes(gemm, residual, q1, q2, ln_w, ln_b, layer_norm.eps, q3)
        return provenance.tag(y, oq, planes=planes)
    tail = _hip.backend().residual_layernorm_quant_axis if axis else _hip.backend().residual_layernorm_quant
    out = tail(gemm, residual, q1, q2, ln_w, ln_b, None if is_nonorm else layer_norm.eps, q3, want_idx=want_idx)
    return tagged(out, oq, want_idx)


_LN_VECTORS = (16, 32, 64, 96, 128, 192, 256, 384, 512, 768)      # 16-byte vectors per row the tail kernels are built for
_AXIS_MAX_D = 1024          # widest row of the per-column tail (its quantizer tables live in LDS)
_AXIS_IRES_D = (64, 128, 256, 384, 512, 768)      # row lengths tq_residual_layernorm_quant_axis_ires_fwd is built for

# The three opt-in switches under which site x (the attention-output tail's result) is never written as fp32, each as one
# record for `quantized_bert_attention_output_ffn`:
#   option, method   the switch in `options` and the backend's tail entry (`_switch_on`)
#   per_column       the tails and the residual grids may be per-column (per-embedding / PEG): tails of the row lengths in
#                    _AXIS_IRES_D, FFN1 planned with peg=True -> a PEG plan (a TILED one where x happens to be per-tensor)
#   planes           site x lies on a 9..16-bit grid and travels as the two byte planes of its index, FFN1 planned with
#                    mp16=True -> an MP16 plan; else as int8 indices of a <= 8-bit grid.  Every plan is asked with ragged=True:
#                    any token count under options.INT8_RAGGED (TILED) / options.INT8_RAGGED_RECIPES (MP16, PEG), else whole tiles
#   wide_h_fp32      a layer input recorded on a grid of more than 8 bits goes into the first tail as fp32 (False: declines)
_XRoute = namedtuple('_XRoute', 'option method per_column planes wide_h_fp32')
_INDEX_ROUTE = _XRoute('INT8_INDEX_RESIDUALS', 'residual_layernorm_quant_ires', False, False, False)
_PLANE_ROUTE = _XRoute('INT8_PLANE_RESIDUALS', 'residual_layernorm_quant_pres', False, True, True)
_PEG_ROUTE = _XRoute('INT8_PEG_INDEX_RESIDUALS', 'residual_layernorm_quant_axis_ires', True, False, True)


def _switch_on(be, option, method):
    """the switch `option` on the integer route of a backend that has the entry `method`; inference only"""
    return bool(getattr(options, option)) and options.int8_active() and not torch.is_grad_enabled() and hasattr(be, method)


def _route_on(be, route):
    return _switch_on(be, route.option, route.method)


def _ln_tail_ok(layer_norm, d_out, q3):
    """What every index / plane form of the (fusable) tail needs: a LayerNorm (not NoNorm) over the last dimension with an
    output quantizer, of a row length the fp32 tail kernels are built for."""
    return (not isinstance(layer_norm, QuantNoNorm) and q3 is not None
            and tuple(getattr(layer_norm, 'normalized_shape', ())) == (d_out,) and d_out % 4 == 0 and d_out // 4 in _LN_VECTORS)


def _route_tail_ok(route, layer_norm, d_out, q1, q2, q3, int8_out=True):
    """Is this (fusable) fp32 tail one for `route`'s entry?  `_ln_tail_ok`; per-tensor quantizers alone -- or, on a per-column
    route, a row length of _AXIS_IRES_D behind `_axis_tail_ok` --; int8_out: the output lies on an asymmetric linear <= 8-bit
    grid (the next tail reads its indices as a residual).  NoNorm and the other tails keep their launches."""
    if not _ln_tail_ok(layer_norm, d_out, q3) or (int8_out and not q3.fits_int8):
        return False
    if route.per_column:
        return _axis_tail_ok(d_out, torch.float32) and d_out in _AXIS_IRES_D
    return not _per_column(q1, q2, q3)


def _planes_tail_ok(layer_norm, d_out, gemm, residual, q1, q2, q3, oq):
    """Is this (fusable) tail one for tq_residual_layernorm_quant_planes_fwd?  options.INT8_PLANE_TAILS on the integer route,
    inference only: the per-tensor fp32 LayerNorm tail of a row length the kernel is built for whose output lies on a fixed
    asymmetric linear grid of 9..16 bits (`emits_planes`: its consumer reads byte planes).  Per-column (PEG) tails, NoNorm,
    bf16 / fp16 and outputs of <= 8 bits keep their launches."""
    return (_switch_on(_hip.backend(), 'INT8_PLANE_TAILS', 'residual_layernorm_quant_planes')
            and _ln_tail_ok(layer_norm, d_out, q3) and not _per_column(q1, q2, q3)
            and gemm.dtype == torch.float32 and residual.dtype == torch.float32 and emits_planes(oq))


def _axis_index_grid(q):
    """`QSpec.index_grid` of a per-tensor or per-column quantizer, its buffers flat as the backend takes them"""
    spec = QSpec.index_grid(q)
    return spec if spec.delta.numel() == 1 else spec._replace(delta=spec.delta.reshape(-1), zero_float=spec.zero_float.reshape(-1))


def _index_residual(residual, d=None):
    """How a residual goes into an index-residual entry, as its arguments (residual, res_idx, q_res, res_row_nan): as indices +
    flags when its record holds contiguous int8 indices of its shape on a fixed asymmetric linear <= 8-bit grid AND row flags;
    as fp32 otherwise (the embedding block's output, or the output of a layer that kept today's launches).  The grid is
    per-tensor; given the row length d (the per-column entry) it may also hold one parameter per column.
    None: a recorded grid of more than 8 bits (W8A16's hidden states) -- the caller declines or passes fp32."""
    rec = provenance.of(residual)
    if rec is None:
        return residual, None, None, None
    q, idx = rec
    if getattr(q, 'n_bits', 8) > 8:
        return None
    flags = provenance.row_nan_of(residual)
    if (idx is not None and flags is not None and idx.dtype == torch.int8 and idx.shape == residual.shape and idx.is_contiguous()
            and emits_int8(q) and q.scale_domain == 'linear' and not q._delta.requires_grad):
        n = q._delta.numel()
        if d is None:
            if n == 1:
                return None, idx, QSpec.index_grid(q), flags
        else:
            zf = getattr(q, '_zero_float', None)
            if (n in (1, d) and zf is not None and zf.numel() == n
                    and (n == 1 or (q._delta.shape[-1] == d and zf.shape[-1] == d))):
                return None, idx, _axis_index_grid(q), flags
    return residual, None, None, None


def _tail_modules_ok(dense, res_quantizer, layer_norm):
    """the module-side conditions of residual_layernorm_quant's fused launch"""
    return (dense.activation_function is None and layer_norm.activation_function is None
            and len(getattr(layer_norm, 'normalized_shape', ())) == 1 and dense.activation_save_target is None
            and layer_norm.activation_save_target is None and not _hooked(dense, res_quantizer, layer_norm))


def quantized_bert_attention_output_ffn(attention_output, intermediate, output, ctx, h):
    """The second half of a BERT layer from the attention context `ctx` and the layer input `h`, with site x -- the
    attention-output tail's result, which the first feed-forward Linear reads and the feed-forward tail reads as its residual --
    never written as fp32.  attention_output / output: the two dense -> (+ residual) -> quantize -> LayerNorm blocks,
    intermediate: the QuantLinear + GELU between them.  One sequence of five launches (`_attention_output_ffn`):

        attention-output Linear (integer GEMM, pre-quantizer output)
        tail, x alone: int8 indices or byte planes + row flags           (residual h: indices + flags, or fp32 in layer 0)
        FFN1, index-only, on x
        FFN2 on FFN1's indices
        FFN tail with x and its flags as residual -> y (fp32), its indices and flags

    under one of three switches, each an `_XRoute` record, picked in this order:

        a tail has a per-column (per-embedding / PEG) quantizer: _PEG_ROUTE (options.INT8_PEG_INDEX_RESIDUALS) or nothing --
            both tails through tq_residual_layernorm_quant_axis_ires_fwd, FFN1 the class-ordered Linear (tq_linear_i8_cls_fwd)
            on x's indices in natural column order; the feed-forward tail dequantizes them on x's per-column grid
        x on a fixed asymmetric linear per-tensor grid of 9..16 bits (W8A16): _PLANE_ROUTE (options.INT8_PLANE_RESIDUALS) --
            x as the two byte planes of its index (tq_residual_layernorm_quant_pres_fwd), FFN1 tq_linear_i16x8_fwd on them
        otherwise: _INDEX_ROUTE (options.INT8_INDEX_RESIDUALS) -- x as int8 indices (tq_residual_layernorm_quant_ires_fwd)

    Bit-identical to `residual_layernorm_quant` + `quantized_bert_ffn`.  Everything is decided before the first launch: both
    tails qualify (`_route_tail_ok` and every condition of the tail helper; the layer's output grid has at most 8 bits on every
    route, a 16-bit site z declines), the three Linears have the route's plans and signed weight grids, nothing observes site x
    (hooks, save targets).  None otherwise, with nothing launched: the caller runs those two calls."""
    be = _hip.backend()
    ao, out = attention_output, output
    ires, pres, peg = _route_on(be, _INDEX_ROUTE), _route_on(be, _PLANE_ROUTE), _route_on(be, _PEG_ROUTE)
    if (not (ires or pres or peg) or not hasattr(intermediate, '_int8_plan_from') or not hasattr(ao.dense, '_int8_plan')
            or not hasattr(out.dense, '_int8_plan_from') or not _hip.on_device(ctx) or ctx.dtype != torch.float32
            or h.dtype != torch.float32 or h.shape[:-1] != ctx.shape[:-1]
            or not _tail_modules_ok(ao.dense, ao.res_act_quantizer, ao.LayerNorm)
            or not _tail_modules_ok(out.dense, out.res_act_quantizer, out.LayerNorm)
            or intermediate.activation_save_target is not None or _hooked(intermediate)):
        return None
    d = ao.dense.out_features
    if out.dense.out_features != d or intermediate.in_features != d or h.shape[-1] != d:
        return None
    qa, qf = _tail_specs(ao.dense, ao.res_act_quantizer, ao.LayerNorm, d), _tail_specs(out.dense, out.res_act_quantizer, out.LayerNorm, d)
    if _refused(*qa) or _refused(*qf):
        return None
    if _per_column(*qa) or _per_column(*qf):
        route = _PEG_ROUTE if peg else None      # the other two switches do nothing where a tail has a per-column quantizer
    elif pres and emits_planes(ao.LayerNorm.activation_quantizer.quantizer if qa[2] is not None else None):
        route = _PLANE_ROUTE
    else:
        route = _INDEX_ROUTE if ires else None
    return None if route is None else _attention_output_ffn(route, be, ao, intermediate, out, ctx, h, d, qa, qf)


def _attention_output_ffn(route, be, ao, intermediate, out, ctx, h, d, qa, qf):
    """The plan checks and the five launches of `quantized_bert_attention_output_ffn` for one `_XRoute`, behind that helper's
    common conditions; qa / qf: the (fusable) quantizer specs of the two tails.  None before the first launch, or the layer's
    output with its indices and row flags."""
    if (not _route_tail_ok(route, ao.LayerNorm, d, *qa, int8_out=not route.planes)
            or not _route_tail_ok(route, out.LayerNorm, d, *qf)):
        return None
    res = _index_residual(h, d if route.per_column else None)
    if res is None:
        if not route.wide_h_fp32:
            return None
        res = (h, None, None, None)
    x_q = ao.LayerNorm.activation_quantizer.quantizer                 # site x: grid of FFN1's input and of the FFN tail's residual
    M = ctx.numel() // ao.dense.in_features
    plan0 = ao.dense._int8_plan(ctx, with_output_quantizer=False, ragged=True)
    # ragged=True on every route: the TILED plan takes any M under options.INT8_RAGGED, the MP16 and PEG plans under
    # options.INT8_RAGGED_RECIPES on top of it; without them a token count that is no multiple of 64 declines here
    plan1 = intermediate._int8_plan_from(x_q, M, with_output_quantizer=True, peg=route.per_column, mp16=route.planes, ragged=True)
    kind1 = MP16 if route.planes else TILED if qa[2].delta.numel() == 1 else PEG
    if (plan0 is None or plan0.kind is not TILED or plan1 is None or plan1.kind is not kind1 or plan1.q_out is None
            or not plan1.q_out.fits_int8):
        return None
    plan2 = out.dense._int8_plan_from(intermediate.activation_quantizer.quantizer, M, with_output_quantizer=False, ragged=True)
    if (plan2 is None or plan2.kind is not TILED
            or not (ao.dense._int8_weights()[2] and intermediate._int8_weights()[2] and out.dense._int8_weights()[2])):
        return None
    tail = getattr(be, route.method)
    gemm = ao.dense._int8_compute(ctx, plan0)
    ln_w, ln_b = ao.LayerNorm.get_params()
    if route.planes:
        _, _, x, x_nan = tail(gemm, res[0], res[1], None, res[2], res[3], qa[0], qa[1], ln_w, ln_b, ao.LayerNorm.eps, qa[2],
                              want_y=False, want_planes=True)
    else:
        _, x, x_nan = tail(gemm, *res, qa[0], qa[1], ln_w, ln_b, ao.LayerNorm.eps, qa[2], want_y=False, want_idx=True)
    mid_idx = intermediate._int8_compute(None, plan1, x_idx=x, index_only=True)
    gemm = out.dense._int8_compute(None, plan2, x_idx=mid_idx)
    ln_w, ln_b = out.LayerNorm.get_params()
    if route.planes:
        y, idx, _, row_nan = tail(gemm, None, None, x, _axis_index_grid(x_q), x_nan, qf[0], qf[1], ln_w, ln_b, out.LayerNorm.eps,
                                  qf[2], want_y=True, want_idx=True)
    else:
        y, idx, row_nan = tail(gemm, None, x, _axis_index_grid(x_q), x_nan, qf[0], qf[1], ln_w, ln_b, out.LayerNorm.eps, qf[2])
    return provenance.tag(y, out.LayerNorm.activation_quantizer.quantizer, idx, row_nan=row_nan)


def embeddings_layernorm_quant(word_emb, type_emb, pos_emb, sum1, sum2, layer_norm, input_ids, type_ids, pos_ids):
    """BERT's embedding block (reference models/quantized_bert.py:75-111):

        layer_norm( sum2( sum1( word_emb(input_ids) + type_emb(type_ids) ) + pos_emb(pos_ids) ) )

    with three QuantEmbeddings (no output quantizer), two QuantizedActivations and a QuantLayerNorm, as ONE launch
    (tq_embeddings_layernorm_quant_fwd: the 13 launches of the layered modules read and write [B, T, d] nine times) when
    every range involved is fixed and per-tensor -- or, under options.INT8_PEG_EMBEDDINGS, per-column along d
    (tq_embeddings_layernorm_quant_axis_fwd).  Returns None otherwise: the caller runs the layered modules."""
    be = _hip.backend()
    embs = (word_emb, type_emb, pos_emb)
    if (not hasattr(be, 'embeddings_layernorm_quant') or not _hip.on_device(input_ids) or input_ids.dim() != 2
            or input_ids.dtype != torch.int64 or type(layer_norm) is not QuantLayerNorm
            or layer_norm.activation_function is not None or len(layer_norm.normalized_shape) != 1
            or layer_norm.activation_save_target is not None or layer_norm.training
            or _needs_autograd(word_emb, type_emb, pos_emb, layer_norm) or _hooked(*embs, sum1, sum2, layer_norm)):
        return None
    for e in embs:
        if (type(e) is not QuantEmbedding or e.training or e.max_norm is not None or e.activation_save_target is not None
                or not isinstance(e.activation_quantizer, FP32Acts) or _hooked(e._modules.get('weight_quantizer'))):
            return None
    d = word_emb.embedding_dim
    q1 = _fixed_along_last(getattr(sum1, '_quant_a', False), getattr(sum1, 'activation_quantizer', sum1), d)
    q2 = _fixed_along_last(getattr(sum2, '_quant_a', False), getattr(sum2, 'activation_quantizer', sum2), d)
    q3 = _fixed_along_last(layer_norm._quant_a, layer_norm.activation_quantizer, d)
    if _refused(q1, q2, q3):
        return None
    # per-column sites (per-embedding / PEG quantizers): the per-column launch, under options.INT8_PEG_EMBEDDINGS and at the
    # row lengths it is built for; otherwise the layered modules, as before there was one
    axis = _per_column(q1, q2, q3)
    if axis and not (options.int8_peg_embeddings(be) and _axis_tail_ok(d, torch.float32)
                     and tuple(layer_norm.normalized_shape) == (d,)):
        return None
    tables = [e.get_params()[0] for e in embs]                  # fake-quantized (cached in eval mode) fp32 tables
    if (any(t.dtype != torch.float32 or t.shape[-1] != d or not _hip.on_device(t) for t in tables) or d % 4
            or d // 4 not in _LN_VECTORS):
        return None
    B, T = input_ids.shape
    if pos_ids.shape[-1] != T or type_ids.shape != input_ids.shape:
        return None
    pos_full = pos_ids.expand(B, T) if pos_ids.shape[0] != B else pos_ids
    ln_w, ln_b = layer_norm.get_params()
    oq = layer_norm.activation_quantizer.quantizer if q3 is not None else None
    want_idx = options.int8_active() and emits_int8(oq)
    block = be.embeddings_layernorm_quant_axis if axis else be.embeddings_layernorm_quant
    out = block(tables[0], input_ids, tables[1], type_ids, tables[2], pos_full, q1, q2, ln_w, ln_b, layer_norm.eps, q3,
                want_idx=want_idx)
    return tagged(tuple(t.view(B, T, d) for t in out) if want_idx else out.view(B, T, d), oq, want_idx)


def quantized_bert_ffn(intermediate, dense, res_quantizer, layer_norm, x, residual):
    """BERT feed-forward block (reference models/quantized_bert.py:252-280 behind hijacker.py:66-116):

        layer_norm(res_quantizer(dense(intermediate(x)) + residual))

    with `intermediate` a QuantLinear + GELU whose 8-bit output ONLY feeds `dense`.  With options.INT8_LINEAR and fixed
    ranges everywhere (per-tensor; the tail's three quantizers and the input's may also be per-column, the PEG recipe; the
    input's and the tail's per-tensor ones may have up to 16 bits, the W8A16 recipe), the intermediate Linear runs index-only (tq_linear_i8_fwd with y = NULL: the
    [tokens, 3072] fp32 activation -- 12.6 MB per layer at B = 8, 4/5 of that kernel's HBM writes -- is never stored),
    `dense` consumes the int8 indices, and the residual + LayerNorm tail follows as one kernel.  Same integer
    contractions and element arithmetic as the separate calls: bit-identical result.  Anything else: the layered
    modules / the tail helper."""
    def separate():
        return residual_layernorm_quant(dense, res_quantizer, layer_norm, intermediate(x), residual)

    if (not options.int8_active() or not hasattr(intermediate, '_int8_plan') or not hasattr(dense, '_int8_plan_from')
            or not _hip.on_device(x) or x.dtype != torch.float32 or dense.activation_function is not None
            or _needs_autograd(intermediate, dense, layer_norm, x, residual)
            or _hooked(intermediate, dense, res_quantizer, layer_norm)):
        return separate()
    d_out = dense.out_features
    q1, q2, q3 = _tail_specs(dense, res_quantizer, layer_norm, d_out)
    if (_refused(q1, q2, q3) or isinstance(layer_norm, QuantNoNorm) or layer_norm.activation_function is not None
            or len(layer_norm.normalized_shape) != 1 or dense.activation_save_target is not None
            or layer_norm.activation_save_target is not None or intermediate.activation_save_target is not None
            or residual.dtype != torch.float32
            or (_per_column(q1, q2, q3) and (not _axis_tail_ok(d_out, torch.float32)
                                             or tuple(layer_norm.normalized_shape) != (d_out,)))):
        return separate()                                  # (the same conditions the tail helper checks)
    # peg=True: an input on a per-embedding-group grid (site x of the PEG recipe) takes the class-ordered integer Linear;
    # mp16=True: one on a 16-bit per-tensor grid (site x of the W8A16 recipe) its byte planes and tq_linear_i16x8_fwd
    plan1 = intermediate._int8_plan(x, with_output_quantizer=True, peg=True, mp16=True, ragged=True)
    if plan1 is None or plan1.q_out is None or not plan1.q_out.fits_int8:
        return separate()                                  # intermediate quantizer: asymmetric, linear domain, <= 8 bit
    mid_q = intermediate.activation_quantizer.quantizer
    M = x.numel() // intermediate.in_features
    plan2 = dense._int8_plan_from(mid_q, M, with_output_quantizer=False, ragged=True)
    if plan2 is None or not dense._int8_weights()[2]:
        return separate()
    mid_idx = intermediate._int8_compute(x, plan1, index_only=True)
    if mid_idx is None:
        return separate()
    gemm = dense._int8_compute(None, plan2, x_idx=mid_idx)
    if gemm is None:
        return separate()
    return residual_layernorm_quant(dense, res_quantizer, layer_norm, None, residual, _gemm=gemm)


def first_token_linear(dense, h, seq_start=None):
    """`dense(h[:, 0])` for h [B, T, d] on a fixed per-tensor asymmetric <= 8-bit grid (BERT's pooler; options.INT8_HEAD):
    the slice is a new tensor object without a provenance record, so the record of `h` is used instead -- its quantizer, and
    the first token of every sequence of its int8 indices as a strided view [B, d] (row stride T * d) that the skinny integer
    Linear reads in place.  Without emitted indices the [B, d] slice alone is quantized.  The result carries dense's output
    quantizer and indices like any integer Linear's -- or, for an output grid of 9..16 bits, the byte planes of its indices,
    which the launch writes beside y (tq_linear_i16x8_skinny_fwd) and the next skinny Linear reads.
    Packed form, seq_start int32 [B + 1] on h's device: h is the [1, M, d] hidden state of a packed batch and the first token
    of sequence b is its row seq_start[b] -- the launch takes `seq_start[:-1]` (a view) as its row table, on h's emitted
    indices; without them the gathered [B, d] rows are quantized.  No host read: capturable, and a replay is valid for other
    lengths of the captured B and M.
    None: not applicable (the plan's conditions), the caller runs the layered modules."""
    packed = seq_start is not None
    if (not options.int8_active() or not options.INT8_HEAD or not hasattr(dense, '_int8_plan_from') or h.dim() != 3
            or not _hip.on_device(h) or h.dtype != torch.float32 or h.shape[2] != dense.in_features
            or _needs_autograd(dense, h) or _hooked(dense)):
        return None
    be = _hip.backend()
    if packed and (h.shape[0] != 1 or seq_start.dim() != 1 or seq_start.dtype != torch.int32 or seq_start.numel() < 2
                   or seq_start.device != h.device or not hasattr(be, 'linear_i16x8_skinny')):
        return None
    src, idx = provenance.of(h) or (None, None)
    B = seq_start.numel() - 1 if packed else h.shape[0]
    plan = dense._int8_plan_from(src, B, with_output_quantizer=True, skinny='always')
    if plan is None or plan.kind is not SKINNY:
        return None                      # (no record, more rows than the skinny kernel takes, another input grid: layered route)
    rows = None
    if src.n_bits > 8:
        # a 16-bit hidden state: the byte planes its producer wrote (a LayerNorm tail under options.INT8_PLANE_TAILS), the
        # first-token rows read in place like the indices below; without them the head stays one layered route
        planes = provenance.planes_like(h)
        if planes is None:
            return None
        x_idx = tuple(p[0] if packed else p[:, 0] for p in planes)
        rows = seq_start[:-1] if packed else None
    elif idx is not None and idx.shape == h.shape and idx.is_contiguous():
        x_idx = idx[0] if packed else idx[:, 0]
        rows = seq_start[:-1] if packed else None
    else:
        first = h[0].index_select(0, seq_start[:-1]) if packed else h[:, 0]
        x_idx = be.quantize_to_int8(first.detach(), *QSpec.index_grid(src), 1, 1, minus_128=True)
    return dense._int8_compute(None, plan, x_idx=x_idx, want_planes=True, rows=rows)


def _needs_autograd(*modules_and_tensors):
    """True when a result must carry a grad_fn: grad mode is on and an input tensor or a parameter of one of the given
    modules requires grad.  The fused integer kernels are inference-only; checking the input alone would silently drop
    the gradients of Linear / NoNorm weights behind a frozen input (frozen embeddings, first layer)."""
    if not torch.is_grad_enabled():
        return False
    for m in modules_and_tensors:
        if m is None:
            continue
        if torch.is_tensor(m):
            if m.requires_grad:
                return True
        elif any(p.requires_grad for p in m.parameters()):
            return True
    return False


def _linear_nonorm_i8(dense, layer_norm, x, residual, q1, q2, q3):
    """Integer Linear -> (+ residual -> Q_sum) -> NoNorm -> Q_out in one launch (tq_linear_i8_nonorm_fwd), or None when
    the integer path does not apply to `dense` / `x` (then the caller runs GEMM and tail separately).  Bit-identical to
    that two-launch form: same integer contraction, same element arithmetic."""
    if not options.int8_active() or not hasattr(dense, '_int8_plan') or (residual is not None and (
            residual.dtype != torch.float32 or not _hip.on_device(residual))) or _needs_autograd(dense, layer_norm, x, residual):
        return None
    plan = dense._int8_plan(x, with_output_quantizer=False)
    if plan is None or plan.act != _hip.ACT_NONE:
        return None
    ops = dense._int8_operands(x, plan)
    if ops is None:
        return None
    ln_w, ln_b = layer_norm.quantized_params()
    oq = layer_norm.activation_quantizer.quantizer if q3 is not None else None
    want_idx = emits_int8(oq)
    INT8_STATS['kernel_calls'] += 1
    out = _hip.backend().linear_i8_nonorm(ops.x_idx, ops.w_idx, ops.rowsum, ops.bias, residual, ln_w, ln_b, ops.x_q,
                                          ops.w_delta, ops.w_eps, q1, q2, q3, torch.float32, want_idx=want_idx)
    return tagged(out, oq, want_idx)


def linear_nonorm_quant(dense, layer_norm, x):
    """MobileBERT bottleneck: ``layer_norm(dense(x))`` with a QuantLinear and a QuantNoNorm, fixed per-tensor ranges:
    one integer launch when options.INT8_LINEAR applies, the layered modules otherwise."""
    if (isinstance(layer_norm, QuantNoNorm) and _hip.on_device(x) and x.dtype == torch.float32
            and dense.activation_function is None and layer_norm.activation_function is None
            and dense.activation_save_target is None and layer_norm.activation_save_target is None
            and not _needs_autograd(dense, layer_norm, x) and not _hooked(dense, layer_norm)):
        q1 = _fixed_per_tensor(dense._quant_a, dense.activation_quantizer)
        q3 = _fixed_per_tensor(layer_norm._quant_a, layer_norm.activation_quantizer)
        if not _refused(q1, q3):
            y = _linear_nonorm_i8(dense, layer_norm, x, None, q1, None, q3)
            if y is not None:
                return y
    return layer_norm(dense(x))


def linear_nonorm_quant_pair(dense_a, layer_norm_a, dense_b, layer_norm_b, x, value=None):
    """MobileBERT's two input bottlenecks (reference models/quantized_mobilebert.py:404-417, built at :483-488):

        layer_norm_a(dense_a(x)), layer_norm_b(dense_b(x))        [, value(x)]

    -- two QuantLinear -> QuantNoNorm chains reading the SAME tensor -- as ONE integer launch
    (tq_linear_i8_nonorm_grouped_fwd) when options.INT8_LINEAR applies and every range involved is fixed and per-tensor;
    each result is a contiguous tensor of its own, tagged with its quantizer and int8 indices.  `value`: the attention's
    value QuantLinear, which reads x too (:216-226 called at :507-513): it rides along as a third group -- a chain with the
    identity affine map whose two quantizers are the Linear's own output quantizer (idempotent on its grid: the group's
    output IS value(x), bit for bit) -- when it has the bottlenecks' width and an asymmetric <= 8-bit fixed output
    quantizer; a third result is returned then.  None when the pair itself is not eligible (the caller runs the chains
    separately).  Bit-identical to the separate launches."""
    be = _hip.backend()
    pairs = ((dense_a, layer_norm_a), (dense_b, layer_norm_b))
    if (not options.int8_active() or not hasattr(be, 'linear_i8_nonorm_grouped') or not _hip.on_device(x)
            or x.dtype != torch.float32 or _needs_autograd(dense_a, layer_norm_a, dense_b, layer_norm_b, x)
            or _hooked(dense_a, layer_norm_a, dense_b, layer_norm_b)):
        return None
    K = x.shape[-1]
    M = x.numel() // K
    N = dense_a.out_features
    if M % 64 or K % 128 or K > 16384 or N % 64 or dense_b.out_features != N:
        return None
    q_dense, q_out, plans = [], [], []
    for d, ln in pairs:
        if (type(d) is not QuantLinear or type(ln) is not QuantNoNorm or d.training or ln.training or d.in_features != K
                or d.activation_function is not None or ln.activation_function is not None
                or d.activation_save_target is not None or ln.activation_save_target is not None
                or not hasattr(d, '_int8_plan') or _hooked(getattr(d, 'weight_quantizer', None))):
            return None
        q1 = _fixed_per_tensor(d._quant_a, d.activation_quantizer)
        q3 = _fixed_per_tensor(ln._quant_a, ln.activation_quantizer)
        if _refused(q1, q3):
            return None
        plan = d._int8_plan(x, with_output_quantizer=False)
        if plan is None or plan.act != _hip.ACT_NONE:
            return None
        q_dense.append(q1)
        q_out.append(q3)
        plans.append(plan)
    if ((q_dense[0] is None) != (q_dense[1] is None) or (q_out[0] is None) != (q_out[1] is None)
            or dense_a.weight_quantizer.quantizer.eps != dense_b.weight_quantizer.quantizer.eps):
        return None
    oqs = [ln.activation_quantizer.quantizer if q is not None else None for (_, ln), q in zip(pairs, q_out)]
    layers = [dense_a, dense_b]
    # the value Linear as a third chain: needs the same structure of quantizers as the bottlenecks (both present)
    if (value is not None and q_dense[0] is not None and q_out[0] is not None and type(value) is QuantLinear and not value.training
            and value.in_features == K and value.out_features == N and value.activation_function is None
            and value.activation_save_target is None and hasattr(value, '_int8_plan') and value._quant_a
            and _fixed_per_tensor_manager(value.activation_quantizer) and not _needs_autograd(value)
            and not _hooked(value, getattr(value, 'weight_quantizer', None))
            and value.weight_quantizer.quantizer.eps == dense_a.weight_quantizer.quantizer.eps):
        vq = value.activation_quantizer.quantizer
        vplan = value._int8_plan(x, with_output_quantizer=False)
        if vplan is not None and vplan.act == _hip.ACT_NONE and emits_int8(vq) and vq.scale_domain == 'linear':
            layers.append(value)
            q_dense.append(QSpec.index_grid(vq))
            q_out.append(q_dense[-1])
            oqs.append(vq)
    G = len(layers)
    want_idx = all(emits_int8(oq) for oq in oqs)
    packed = _stacked_qkv(tuple(layers))
    if packed is None and G == 3:
        layers, q_dense, q_out, oqs, G = layers[:2], q_dense[:2], q_out[:2], oqs[:2], 2
        packed = _stacked_qkv(tuple(layers))
    if packed is None:
        return None
    w_idx, rowsum, bias, scales = packed
    ops = dense_a._int8_operands(x, plans[0])              # the shared input's indices and quantizer
    if ops is None:
        return None
    affine = [ln.quantized_params() for _, ln in pairs]    # cached with fixed ranges in inference
    # quantized pairs: fresh tensors per (parameter versions, range state) from quantized_params' own cache; with
    # _quant_w = False they ARE the raw Parameters, which an optimizer step / load_state_dict rewrites in place behind the
    # same pointers: versions and CACHE_EPOCH (hipGraph replays of a training step) are part of the key
    key = tuple((w.data_ptr(), w._version, b.data_ptr(), b._version) for w, b in affine) + (G, options.CACHE_EPOCH)
    hit = getattr(layer_norm_a, '_stacked_affine_cache', None)
    if hit is None or hit[0] != key:
        ws = [w.detach().float().reshape(-1) for w, _ in affine]
        bs = [b.detach().float().reshape(-1) for _, b in affine]
        if G == 3:                                         # identity affine map of the value group
            ws.append(torch.ones(N, dtype=torch.float32, device=x.device))
            bs.append(torch.zeros(N, dtype=torch.float32, device=x.device))
        hit = (key, torch.cat(ws).contiguous(), torch.cat(bs).contiguous(), affine)   # (keeps the parts alive)
        layer_norm_a._stacked_affine_cache = hit
    INT8_STATS['kernel_calls'] += G
    out = be.linear_i8_nonorm_grouped(ops.x_idx, w_idx, rowsum, bias, hit[1], hit[2], ops.x_q, scales, ops.w_eps,
                                      None if q_dense[0] is None else q_dense, None if q_out[0] is None else q_out,
                                      torch.float32, want_idx=want_idx, n_groups=G)
    ys, idxs = out if want_idx else (out, [None] * G)
    res = []
    for y, idx, oq in zip(ys, idxs, oqs):
        y = y.view(x.shape[:-1] + (N,))
        if oq is not None:
            provenance.tag(y, oq, None if idx is None else idx.view(y.shape))
        res.append(y)
    return res


def _ffn_block_plan(be, block, x, src=None, M=None):
    """Preconditions of ONE MobileBERT feed-forward block (intermediate, dense, res_quantizer, layer_norm) shared by the
    merged launches quantized_ffn and quantized_ffn_chain: -> (plan of `intermediate`, (q_dense, q_sum, q_out)) or None.
    The block reads `x` or, with src, the int8 indices the quantizer `src` emitted for M rows (the inner blocks of a chain)."""
    intermediate, dense, res_quantizer, layer_norm = block
    # (a save target on either Linear: dense's _int8_weight_side_ok and, through its plan, intermediate's refuse it)
    if (not isinstance(layer_norm, QuantNoNorm) or not hasattr(intermediate, '_int8_plan')
            or not hasattr(dense, '_int8_weight_side_ok') or _needs_autograd(intermediate, dense, layer_norm, x)
            or dense.activation_function is not None or layer_norm.activation_function is not None
            or layer_norm.activation_save_target is not None or not dense._int8_weight_side_ok()
            or _hooked(intermediate, dense, res_quantizer, layer_norm)
            or (intermediate.in_features, intermediate.out_features, dense.out_features) not in be.FFN_SHAPES
            or dense.in_features != intermediate.out_features):
        return None
    plan = (intermediate._int8_plan(x, with_output_quantizer=True) if src is None
            else intermediate._int8_plan_from(src, M, with_output_quantizer=True))
    specs = _tail_specs(dense, res_quantizer, layer_norm)
    if plan is None or plan.act != _hip.ACT_RELU or plan.q_out is None or _refused(*specs) or not plan.q_out.fits_int8:
        return None                                          # intermediate quantizer: asymmetric, linear, <= 8 bit
    return plan, specs


# one feed-forward block as the merged kernels take it (ffn_chain_i8_nonorm: a list of these as dicts)
_FfnStage = namedtuple('_FfnStage', 'w1_idx w1_rowsum bias1 w1_delta w1_eps q_mid w2_idx w2_rowsum bias2 w2_delta w2_eps '
                                    'nn_w nn_b q_dense q_sum q_out')


def _ffn_block_stage(block, plan, specs, x, x_idx=None):
    """-> (operands of `intermediate`, _FfnStage) or None (an unsigned weight grid).
    x_idx given: `x` is not touched (weight side only)."""
    intermediate, dense, _, layer_norm = block
    ops = intermediate._int8_operands(x, plan, x_idx=x_idx)
    if ops is None:
        return None
    w2_idx, rs2, w2_signed = dense._int8_weights()
    if not w2_signed:
        return None
    ln_w, ln_b = layer_norm.quantized_params()
    wq2 = dense.weight_quantizer.quantizer
    return ops, _FfnStage(ops.w_idx, ops.rowsum, ops.bias, ops.w_delta, ops.w_eps, plan.q_out,
                          w2_idx, rs2, None if dense.bias is None else dense.bias.detach(), wq2._delta.reshape(-1), wq2.eps,
                          ln_w, ln_b, *specs)


def quantized_ffn(intermediate, dense, res_quantizer, layer_norm, x):
    """MobileBERT feed-forward block (reference models/quantized_mobilebert.py:330-352):

        layer_norm(res_quantizer(dense(intermediate(x)) + x))

    with `intermediate` a QuantLinear + ReLU, `dense` a QuantLinear, `layer_norm` a QuantNoNorm -- as ONE integer launch
    (tq_ffn_i8_nonorm_fwd: the [tokens, 512] intermediate stays in LDS) when options.INT8_LINEAR applies to both Linears,
    every range involved is fixed and per-tensor and the shape is one the kernel is built for; otherwise the two
    Linears run on their own (integer or layered) and the tail through residual_layernorm_quant."""
    def separate():
        return residual_layernorm_quant(dense, res_quantizer, layer_norm, intermediate(x), x)

    be = _hip.backend()
    block = (intermediate, dense, res_quantizer, layer_norm)
    if not options.int8_active() or not hasattr(be, 'ffn_i8_nonorm') or not _hip.on_device(x) or x.dtype != torch.float32:
        return separate()
    planned = _ffn_block_plan(be, block, x)
    if planned is None or (x.numel() // intermediate.in_features) % 32:
        return separate()
    staged = _ffn_block_stage(block, *planned, x)
    if staged is None:
        return separate()
    ops, s = staged
    oq = layer_norm.activation_quantizer.quantizer if s.q_out is not None else None
    want_idx = emits_int8(oq)
    INT8_STATS['kernel_calls'] += 2                          # two Linears' worth of integer GEMM
    out = be.ffn_i8_nonorm(ops.x_idx, ops.x_q, s.w1_idx, s.w1_rowsum, s.bias1, s.w1_delta, s.w1_eps, s.q_mid,
                           s.w2_idx, s.w2_rowsum, s.bias2, s.w2_delta, s.w2_eps, x, s.nn_w, s.nn_b,
                           s.q_dense, s.q_sum, s.q_out, torch.float32, want_idx=want_idx)
    return tagged(out, oq, want_idx)


def quantized_ffn_chain(blocks, x):
    """Consecutive MobileBERT feed-forward blocks, each the input of the next (reference
    models/quantized_mobilebert.py:523-529: three FFN layers, then intermediate + output), as ONE integer launch
    (tq_ffn_chain_i8_nonorm_fwd: a workgroup takes its 16 token rows through all blocks; only the last output is
    written).  blocks: [(intermediate, dense, res_quantizer, layer_norm), ...] as for `quantized_ffn`.  Same
    preconditions as `quantized_ffn` for every block, and every block's output quantizer must be asymmetric, linear,
    <= 8 bit (its grid is the next block's input grid).  None when not eligible (the caller runs the blocks one by one);
    bit-identical to that."""
    be = _hip.backend()
    if (not options.int8_active() or not hasattr(be, 'ffn_chain_i8_nonorm') or not 2 <= len(blocks) <= 4
            or not _hip.on_device(x) or x.dtype != torch.float32):
        return None
    M = x.numel() // x.shape[-1]
    if M % 32:
        return None
    stages, src, x_ops = [], None, None
    for block in blocks:
        planned = _ffn_block_plan(be, block, x, src, M)
        if planned is None:
            return None
        plan, specs = planned
        oq = block[3].activation_quantizer.quantizer if specs[2] is not None else None
        if not emits_int8(oq) or oq.scale_domain != 'linear':    # (the chain alone: its grid is the next block's input grid)
            return None
        staged = _ffn_block_stage(block, plan, specs, None if x_ops else x, x_ops.x_idx if x_ops else None)
        if staged is None:
            return None
        x_ops = x_ops or staged[0]
        stages.append(staged[1]._asdict())
        src = oq
    INT8_STATS['kernel_calls'] += 2 * len(blocks)
    y, idx = be.ffn_chain_i8_nonorm(x_ops.x_idx, x_ops.x_q, x, stages, torch.float32, want_idx=True)
    provenance.tag(y, oq, idx)
    return y


def scores_softmax_quant(scores_quantizer, probs_quantizer, scores, mask, denom):
    """Equivalent to ``probs_quantizer(softmax(scores_quantizer(scores) / denom + mask, dim=-1))``
    (reference models/quantized_bert.py:153-198) as one kernel when both quantizers are fixed and
    per-tensor.  scores: fp32 [B, H, Tq, Tk]; mask: additive, broadcastable [B, 1, 1, Tk] or None."""
    q1 = _fixed_per_tensor(scores_quantizer._quant_a, scores_quantizer.activation_quantizer)
    q2 = _fixed_per_tensor(probs_quantizer._quant_a, probs_quantizer.activation_quantizer)
    Tk = scores.shape[-1]
    ok_mask = mask is None or (mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == 1
                               and mask.shape[0] == scores.shape[0] and mask.shape[3] == Tk)
    if (_refused(q1, q2) or not _hip.on_device(scores) or scores.dtype != torch.float32 or scores.dim() != 4
            or not ok_mask or Tk not in (32, 64, 128, 256, 512, 1024)
            or (torch.is_grad_enabled() and scores.requires_grad) or _hooked(scores_quantizer, probs_quantizer)):
        s = scores_quantizer(scores) / denom
        if mask is not None:
            s = s + mask
        return probs_quantizer(torch.softmax(s, dim=-1))
    m = None if mask is None else mask.reshape(mask.shape[0], Tk).float().contiguous()
    return _hip.backend().scores_softmax_quant(scores, m, scores.shape[1] * scores.shape[2], denom, q1, q2)


def _int8_source(t):
    """(int8 indices, QSpec) of a tensor produced by a fixed per-tensor asymmetric <= 8-bit quantizer
    that emitted its indices (provenance records of QuantizationManager / the integer Linear)."""
    q, idx = provenance.of(t) or (None, None)
    if (idx is None or idx.shape != t.shape or not emits_int8(q) or q.scale_domain != 'linear' or q._delta.numel() != 1):
        return None
    return idx, QSpec.index_grid(q)


def quantized_attention(query, key, value, mask, num_heads, scores_quantizer, probs_quantizer,
                        context_quantizer):
    """Attention core of a quantized BERT layer (reference models/quantized_bert.py:135-213) on the
    OUTPUTS of the quantized query / key / value Linears, each [B, T, H * d]:

        ctx = context_quantizer(merge_heads(probs_quantizer(softmax(
                  scores_quantizer(Q K^T) / sqrt(d) + mask)) V))

    Runs as one integer kernel (tq_attention_i8_fwd) when options.INT8_LINEAR is on, the three inputs
    carry their int8 grid indices, every quantizer involved is fixed, per-tensor (asymmetric <= 8 bit
    for Q, K, V and the probabilities), T a multiple of 64 up to 512 and d in (32, 64).  Returns None otherwise: the
    caller then runs the layered modules."""
    if (not options.int8_active() or query.dim() != 3 or not _hip.on_device(query)
            or _hooked(scores_quantizer, probs_quantizer, context_quantizer)):
        return None
    if torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad):
        return None
    B, T, D = query.shape
    packed = mask if isinstance(mask, PackedSequences) else None          # [1, M, D] rows of B' packed sequences, no mask
    if packed is not None:
        if not _packed_ok(packed, B) or D % num_heads or D // num_heads not in (32, 64):
            return None
        mask = None
    ragged = T % 64 != 0 and options.int8_ragged(_hip.backend())         # any 1 <= T <= 512 (options.INT8_RAGGED)
    if packed is None and (D % num_heads or D // num_heads not in (32, 64) or (T % 64 and not ragged) or not 1 <= T <= 512):
        return None
    srcs = [_int8_source(t) for t in (query, key, value)]
    args = None if None in srcs else _core_args(scores_quantizer, probs_quantizer, context_quantizer, mask, B, T)
    if args is None:
        return None
    core = _hip.backend().attention_i8_ragged if ragged else _hip.backend().attention_i8
    if packed is not None:
        core = _varlen_core(_hip.backend(), packed)
    return _attention_core(core, [s[0] for s in srcs], [s[1] for s in srcs], num_heads, D // num_heads, args, context_quantizer)


def _stacked_qkv(layers):
    """int8 weights / row sums / biases / per-row weight scales of several QuantLinears stacked along the
    output dimension, cached on the first layer until any weight or weight range changes."""
    key = tuple((l.weight.data_ptr(), l.weight._version, l.weight_quantizer.quantizer.range_state_key(),
                 None if l.bias is None else (l.bias.data_ptr(), l.bias._version)) for l in layers)
    cache = getattr(layers[0], '_stacked_i8_cache', None)
    if cache is not None and cache[0] == key:
        return cache[1]
    parts = [l._int8_weights() for l in layers]              # (w_idx, rowsum, signed) per layer
    if not all(p[2] for p in parts):
        return None
    dev = layers[0].weight.device
    w_idx = torch.cat([p[0] for p in parts], dim=0).contiguous()
    rowsum = torch.cat([p[1] for p in parts], dim=0).contiguous()
    if all(l.bias is None for l in layers):
        bias = None
    else:
        bias = torch.cat([l.bias.detach().float() if l.bias is not None else
                          torch.zeros(l.out_features, device=dev) for l in layers]).contiguous()
    scales = torch.cat([l.weight_quantizer.quantizer._delta.detach().reshape(-1).float().expand(l.out_features)
                        if l.weight_quantizer.quantizer._delta.numel() == 1
                        else l.weight_quantizer.quantizer._delta.detach().reshape(-1).float() for l in layers]).contiguous()
    packed = (w_idx, rowsum, bias, scales)
    layers[0]._stacked_i8_cache = (key, packed)
    return packed


def _stacked_qkv_cls(layers, layout):
    """`_stacked_qkv` for a class-ordered input: (w_idx with its columns in the class order of `layout`, per-class row sums
    [C, N], bias, per-row weight scales, the order as a device tensor), cached on the first layer per (stacked key, layout)."""
    packed = _stacked_qkv(layers)
    if packed is None:
        return None
    key = (layers[0]._stacked_i8_cache[0], layout.key)
    cache = getattr(layers[0], '_stacked_cls_cache', None)
    if cache is not None and cache[0] == key and cache[2] is layout:
        return cache[1]
    be = _hip.backend()
    w_idx, _, bias, scales = packed
    order = layout.order_on(w_idx.device)
    w_c = w_idx if layout.identity else w_idx.index_select(1, order).contiguous()
    if getattr(layout, 'pad', None) is not None:         # classes padded to whole K slabs: zero weights in the pad columns
        w_c[:, layout.pad_on(w_idx.device)] = 0
    starts = (0,) + layout.ends[:-1]
    rs = torch.stack([be.rowsum_i8(w_c[:, s:e].contiguous()) for s, e in zip(starts, layout.ends)]).contiguous()
    out = (w_c, rs, bias, scales, order)
    layers[0]._stacked_cls_cache = (key, out, layout)
    return out


def _one_class_layout(q, K):
    """the class layout of a per-tensor input grid: one class over the K columns in their own order (cached on `q`)"""
    import numpy as np
    key = peg_layout.layout_key(q)
    cached = q.__dict__.get('_peg_one_class')
    if cached is None or cached[0] != (key, K):
        cached = q.__dict__['_peg_one_class'] = ((key, K), peg_layout.ClassLayout(key, np.arange(K, dtype=np.int64), [K], [0]))
    return cached[1]


def _head_grid(enabled, mgr, D, head_dim):
    """A Q / K / V / context site for the per-head attention route: -> (QSpec | None, block width | None) or NOT_FUSABLE.
    QSpec: fixed, asymmetric, linear domain, <= 8 bits; per-tensor (block None), or per-column over the D columns and constant
    over every head and over every aligned block of `block` >= 64 columns (quantization/peg.py).  None: the site is off."""
    spec = _fixed_along_last(enabled, mgr, D)
    if spec is None or spec is NOT_FUSABLE:
        return spec if spec is NOT_FUSABLE else (None, None)
    if not spec.fits_int8 or spec.delta.requires_grad:
        return NOT_FUSABLE
    spec = QSpec.index_grid(mgr.quantizer)._replace(delta=spec.delta, zero_float=spec.zero_float)
    if spec.delta.numel() == 1:
        return spec, None
    blocks = peg_layout.block_layout(mgr.quantizer, D)
    if blocks is None or blocks.block is None or not blocks.constant_over(head_dim):
        return NOT_FUSABLE               # permuted groups, per-embedding grids: not whole heads / whole tiles
    return spec, blocks.block


def _peg_self_attention(x, layers, mask, num_heads, scores_quantizer, probs_quantizer, context_quantizer):
    """options.INT8_PEG_ATTENTION: the attention half of a BERT layer whose Q / K / V / context sites carry per-embedding-group
    grids (a group = a run of whole heads and whole 64-column tiles) as two integer launches -- one index-only
    tq_linear_i8_cls_grouped_fwd for the stacked Q | K | V on x's indices in class order, one attention core with a grid per
    head.  Everything is decided before the first launch; None: the caller goes on with today's path."""
    be = _hip.backend()
    query = layers[0]
    if (x.dim() != 3 or not _hip.on_device(x) or x.dtype != torch.float32 or torch.is_grad_enabled()
            or not hasattr(be, 'linear_i8_cls_grouped')
            or _hooked(*layers, scores_quantizer, probs_quantizer, context_quantizer,
                       *(getattr(l, 'weight_quantizer', None) for l in layers))):
        return None
    B, T, K = x.shape
    # A PackedSequences in the mask's place ([1, M, K] rows of packed sequences): declined under INT8_PEG_ATTENTION alone, as
    # before; with options.INT8_PEG_EMBEDDINGS also on -- the recipe exact from the input ids on -- the grouped launch runs over
    # the M rows and the variable-length core takes the per-head grids (it accepts them like the other two cores).
    pseq = mask if isinstance(mask, PackedSequences) else None
    if pseq is not None:
        if not (options.int8_peg_embeddings(be) and _packed_ok(pseq, B)):
            return None
        mask = None
    D = query.out_features
    if (D % num_heads or D // num_heads not in (32, 64) or D % 64 or K % 128 or K > 16384
            or (pseq is None and not 1 <= T <= 512)):
        return None
    head_dim = D // num_heads
    ragged = bool(T % 64 or (B * T) % 64)
    if ragged and not options.int8_ragged_recipes(be):
        return None
    # the input: a fixed asymmetric linear-domain grid of <= 8 bits, per-tensor or PEG with a class layout
    src = provenance.quantizer_of(x)
    if (src is None or src.symmetric or src.n_bits > 8 or src._delta is None or src.scale_domain != 'linear'
            or src._delta.requires_grad or getattr(src, '_zero_float', None) is None):
        return None
    if src._delta.numel() == 1:
        layout = _one_class_layout(src, K)
    else:
        # (classes of 64 or 192 columns -- per_groups 12, 4 at d = 768 -- padded to whole 128-column K slabs: peg.PaddedClassLayout)
        layout = peg_layout.padded_class_layout(src, K)
        if layout is None or layout.ends[-1] > 16384:
            return None
    outs, blocks = [], []
    for l in layers:
        if (type(l) is not QuantLinear or l.training or not l._quant_w or not l._quant_a
                or l.activation_function is not None or l.activation_save_target is not None
                or l.in_features != K or l.out_features != D
                or not isinstance(l.weight_quantizer, QuantizationManager) or l.weight_quantizer.state != Qstates.fix_ranges):
            return None
        wq = l.weight_quantizer.quantizer
        if (not wq.symmetric or wq.n_bits > 8 or wq.scale_domain != 'linear' or wq._delta.numel() not in (1, D)
                or wq.eps != query.weight_quantizer.quantizer.eps):
            return None
        grid = _head_grid(True, l.activation_quantizer, D, head_dim)
        if grid is NOT_FUSABLE or grid[0] is None:
            return None
        outs.append(grid[0])
        blocks.append(grid[1])
    qs = _fixed_per_tensor(scores_quantizer._quant_a, scores_quantizer.activation_quantizer)
    qp = _fixed_per_tensor(probs_quantizer._quant_a, probs_quantizer.activation_quantizer)
    ctx_grid = _head_grid(context_quantizer._quant_a, context_quantizer.activation_quantizer, D, head_dim)
    if _refused(qs, qp, ctx_grid) or qp is None or not qp.fits_int8 or _per_column(qs, qp):
        return None
    qc = ctx_grid[0]
    if src._delta.numel() == 1 and not _per_column(*outs, qc):
        return None                      # no per-column grid anywhere: the per-tensor recipe, which has its own launches
    if mask is not None:
        if not (mask.dim() == 4 and mask.shape[0] == B and mask.shape[1] == 1 and mask.shape[2] == 1 and mask.shape[3] == T):
            return None
        mask = mask.reshape(B, T).float().contiguous()
    packed = _stacked_qkv_cls(tuple(layers), layout)
    if packed is None:
        return None
    w_c, cls_rs, bias, scales, order = packed
    # one block width for the launch: the narrowest any per-column output grid needs (128 keeps the launcher's tile plan)
    q_block = min([b for b in blocks if b is not None] + [128 if D % 128 == 0 else 64])
    # ---- launches -----------------------------------------------------------------------------------------------------
    x_idx = provenance.indices_of(x)                     # natural column order (quantization/peg.py), or one launch over x
    if x_idx is None or x_idx.shape != x.shape:
        x_idx = be.quantize_to_int8(x.detach(), *QSpec.index_grid(src), src._delta.numel(), 1, minus_128=True)
    if not layout.identity:
        roomy = getattr(be, '_rows_empty', None) if (B * T) % 64 else None
        if roomy is None:
            x_idx = x_idx.index_select(-1, order)
        else:
            x_idx = torch.index_select(x_idx, -1, order, out=roomy(tuple(x_idx.shape[:-1]) + (order.numel(),), torch.int8,
                                                                   x_idx.device, force=True))
    INT8_STATS['kernel_calls'] += 3                      # counted in Linears, like the other fused launches
    _, buf = be.linear_i8_cls_grouped(x_idx.contiguous(), w_c, cls_rs, bias, XGrid.of(src), layout.table(be), scales,
                                      query.weight_quantizer.quantizer.eps, 0, outs, q_block, want_y=False, want_idx=True)
    cols = [buf[..., j * D:(j + 1) * D] for j in range(3)]
    core = _varlen_core(be, pseq) if pseq is not None else (be.attention_i8_ragged if T % 64 else be.attention_i8)
    return _attention_core(core, cols, outs, num_heads, head_dim, (qs, qp, qc, mask), context_quantizer)


def quantized_self_attention(x, query, key, value, mask, num_heads, scores_quantizer, probs_quantizer,
                             context_quantizer, value_out=None):
    """Self-attention of a quantized BERT / MobileBERT layer from the inputs of its query / key / value Linears: Linears
    that share their input run as ONE grouped integer GEMM that only emits int8 indices (tq_linear_i8_grouped_fwd:
    no fp32 output is written), which the integer attention core consumes in place (column blocks of the stacked
    buffers).  `x`: the one layer input (BERT: one launch for Q | K | V), or a (query_in, key_in, value_in) tuple
    (MobileBERT, reference models/quantized_mobilebert.py:214-226 called at :507-513: query and key read the bottlenecked
    shared input -> Q | K in one launch, V in another).  Same preconditions as `quantized_attention` plus: the three
    Linears are plain eval-mode QuantLinears without activation function whose weight and output quantizers are fixed,
    and the inputs carry their int8 indices.  value_out: value(value_in) already computed by another launch
    (linear_nonorm_quant_pair), tagged with the value Linear's output quantizer and its indices -- the value Linear is not
    launched then.  Returns None when any of that does not hold (run the layered modules then).
    options.INT8_PEG_ATTENTION: one shared input whose Q / K / V / context sites carry per-embedding-group grids made of whole
    heads goes through `_peg_self_attention` first (class-ordered grouped Linear + the core with a grid per head)."""
    layers = (query, key, value)
    if (options.INT8_PEG_ATTENTION and options.int8_active() and torch.is_tensor(x)
            and options.int8_peg_attention(_hip.backend())):
        out = _peg_self_attention(x, layers, mask, num_heads, scores_quantizer, probs_quantizer, context_quantizer)
        if out is not None:
            return out
    xs = tuple(x) if isinstance(x, (tuple, list)) else (x, x, x)
    if (not options.int8_active() or len(xs) != 3
            or any(t.dim() != 3 or not _hip.on_device(t) or t.dtype != torch.float32 for t in xs)
            or _hooked(query, key, value, scores_quantizer, probs_quantizer, context_quantizer,
                       *(getattr(l, 'weight_quantizer', None) for l in layers))):
        return None
    if torch.is_grad_enabled() and (any(t.requires_grad for t in xs) or any(l.weight.requires_grad for l in layers)):
        return None
    B, T, _ = xs[0].shape
    D = query.out_features
    # PackedSequences in the mask's place: [1, M, K] rows of packed sequences -- the grouped launch over the M rows, then the
    # variable-length core (no additive mask: a sequence's keys are its own rows, all visible)
    pseq = mask if isinstance(mask, PackedSequences) else None
    if pseq is not None:
        if not _packed_ok(pseq, B):
            return None
        mask = None
    # options.INT8_RAGGED: any 1 <= T <= 512 and any B * T (ragged core, grouped launches over padded rows)
    ragged_ok = options.int8_ragged(_hip.backend()) and not torch.is_grad_enabled()
    if (any(t.shape[:2] != (B, T) for t in xs) or D % num_heads or D // num_heads not in (32, 64)
            or (pseq is None and not 1 <= T <= 512) or ((T % 64 or (B * T) % 64) and not ragged_ok) or D % 64):
        return None
    outs = []
    for l, t in zip(layers, xs):
        K = t.shape[-1]
        if (type(l) is not QuantLinear or l.training or not l._quant_w or not l._quant_a
                or l.activation_function is not None or l.activation_save_target is not None
                or l.in_features != K or l.out_features != D or K % 128 or K > 16384
                or not _fixed_per_tensor_manager(l.activation_quantizer)
                or not isinstance(l.weight_quantizer, QuantizationManager)      # e.g. replaced by FP32Acts
                or l.weight_quantizer.state != Qstates.fix_ranges):
            return None
        wq, oq = l.weight_quantizer.quantizer, l.activation_quantizer.quantizer
        if (not wq.symmetric or wq.n_bits > 8 or wq.scale_domain != 'linear' or wq._delta.numel() not in (1, D)
                or not emits_int8(oq) or oq.scale_domain != 'linear'
                or wq.eps != query.weight_quantizer.quantizer.eps):     # one eps argument serves the stacked weights
            return None
        outs.append(QSpec.index_grid(oq))
    args = _core_args(scores_quantizer, probs_quantizer, context_quantizer, mask, B, T)
    if args is None:
        return None
    # consecutive Linears reading the SAME tensor object form one launch: (Q, K, V) | (Q, K), (V) | (Q), (K), (V)
    groups = [[0]]
    for i in (1, 2):
        if xs[i] is xs[groups[-1][0]]:
            groups[-1].append(i)
        else:
            groups.append([i])
    v_src = None
    if value_out is not None:
        rec = provenance.of(value_out)
        v_src = _int8_source(value_out)
        if (rec is None or rec[0] is not value.activation_quantizer.quantizer or v_src is None
                or value_out.shape != (B, T, D) or not value_out.is_contiguous()):
            return None
        groups = [g for g in ([i for i in grp if i != 2] for grp in groups) if g]
    srcs = {}
    for g in groups:
        src = _int8_source(xs[g[0]])
        if src is None:
            return None
        srcs[g[0]] = src
    be = _hip.backend()
    cols = [None, None, None]
    packs = [_stacked_qkv(tuple(layers[i] for i in g)) for g in groups]
    if any(p is None for p in packs):
        return None
    for g, packed in zip(groups, packs):
        INT8_STATS['kernel_calls'] += len(g)                  # counted in Linears, like the other fused launches
        w_idx, rowsum, bias, scales = packed
        x_idx, xq = srcs[g[0]]
        _, buf = be.linear_i8_grouped(x_idx, w_idx, rowsum, bias, XGrid.of_spec(xq), scales,
                                      layers[g[0]].weight_quantizer.quantizer.eps, 0, [outs[i] for i in g], want_y=False,
                                      want_idx=True)
        for j, i in enumerate(g):
            cols[i] = buf[..., j * D:(j + 1) * D]
    if v_src is not None:
        cols[2] = v_src[0]
    core = _varlen_core(be, pseq) if pseq is not None else be.attention_i8_ragged if T % 64 else be.attention_i8
    return _attention_core(core, cols, outs, num_heads, D // num_heads, args, context_quantizer)
