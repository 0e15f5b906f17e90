"""Quantized drop-ins for nn.Linear / nn.LayerNorm / nn.Embedding and the recursive
``quantize_model`` rewriter (counterpart of the reference's quantization/autoquant_utils.py).

``run_forward`` stays the per-op hook of the reference (:20-21, :59-66, :76-85); it is also where a
fused GEMM + fake-quant epilogue would plug in.
"""
import copy
import warnings

import torch
from torch import nn
from torch.nn import functional as F
from torch.nn.modules.pooling import _AdaptiveAvgPoolNd, _AvgPoolNd

from quantization import _hip
from quantization import options
from quantization import peg as peg_layout
from quantization import provenance
from quantization.base_quantized_classes import FP32Acts, QuantizedActivation, QuantizedModule
from quantization.hijacker import QuantizationHijacker, activations_list
from quantization.int8_route import (MP16, PEG, SKINNY, TILED, IntOperands, IntPlan, QSpec, XGrid, emits_int8,  # noqa: F401
                                     emits_planes, tagged)

_new_tuple = tuple.__new__     # IntPlan / IntOperands are built once per Linear call: past the generated __new__ (see int8_route)
from quantization.quantization_manager import QuantizationManager, _GLOBAL_FWD_HOOKS, _GLOBAL_FWD_PRE_HOOKS


# The integer path is switched on with quantization.options.INT8_LINEAR (see there).
# how often the MFMA Linear ran (plain / under autograd) and how often an unsigned weight grid sent a layer back to
# the layered path
INT8_STATS = {'kernel_calls': 0, 'autograd_calls': 0, 'unsigned_weight_fallbacks': 0}
_ACT_CODES = {type(None): _hip.ACT_NONE, nn.ReLU: _hip.ACT_RELU, nn.GELU: _hip.ACT_GELU, nn.Tanh: _hip.ACT_TANH}


def _hooked(*modules):
    """Does any of these modules carry forward (pre-)hooks?  The integer / fused routes evaluate whole module chains in
    one launch without calling the modules, so a hook on any of them would silently stop firing -- leaf modules AND the
    containers whose __call__ a merged launch bypasses (the harness models pass those: QResidualBlock, QFFN, the Sequential
    around an intermediate Linear, ...) -- as would global module hooks (torch.nn.modules.module.
    register_module_forward_hook), which every bypassed __call__ would have fired."""
    if _GLOBAL_FWD_HOOKS or _GLOBAL_FWD_PRE_HOOKS:
        return True
    for m in modules:
        if m is not None and isinstance(m, nn.Module) and (m._forward_hooks or m._forward_pre_hooks):
            return True
    return False


def _rows_covered(rows):
    """the rows an MP16 / PEG launch covers for `rows` input rows: whole 64-row tiles (the backend pads the tail,
    options.INT8_RAGGED_RECIPES); the staircase bin count is asked for with these"""
    return -(-rows // 64) * 64


def _fixed_per_tensor_manager(mgr):
    from quantization.quantization_manager import Qstates
    return (isinstance(mgr, QuantizationManager) and mgr.state == Qstates.fix_ranges
            and mgr.quantizer.is_initialized and mgr.quantizer._delta.numel() == 1)


def prequantize_weights(model):
    """Fill the eval-mode parameter cache of every quantized layer below `model` whose weight range is FIXED with ONE
    multi-tensor launch per 40 tensors (`tq_fake_quant_multi_fwd`) instead of one launch per layer on its first eval
    forward.  The reference quantizes and caches the weights layer by layer (hijacker.py:52-64 `get_params`: 102 weight
    tensors in a BERT-base); this is the same computation on the same inputs -- `cached_params` ends up bit-identical
    -- batched over independent sites.  Layers that do not qualify (training mode, caching off, a cache already
    present, weights not quantized, ranges not fixed / learnable / not initialised, rows that are not whole 16-byte
    vectors, float64) are left to the lazy path.  -> number of layers served."""
    from quantization.quantization_manager import Qstates
    from quantization.quantizers import AsymmetricUniformQuantizer, SymmetricUniformQuantizer, param_layout
    be = _hip.backend()
    if not hasattr(be, 'fake_quant_multi'):
        return 0
    groups = {}                     # (device, dtype) -> [(module, weight, bias, item)]
    for m in model.modules():
        if not isinstance(m, QuantizationHijacker) or m.training or not m._caching or m.cached_params or not m._quant_w:
            continue
        mgr = m._modules.get('weight_quantizer')
        if not isinstance(mgr, QuantizationManager) or mgr.state != Qstates.fix_ranges:
            continue
        if mgr._forward_hooks or mgr._forward_pre_hooks:
            continue
        q = mgr.quantizer
        if type(q) not in (AsymmetricUniformQuantizer, SymmetricUniformQuantizer) or not q.is_initialized:
            continue
        if q._forward_hooks or q._forward_pre_hooks:
            continue
        weight, bias = m.get_weight_bias()
        delta = q._delta
        if (not weight.is_cuda or weight.dtype not in (torch.float32, torch.bfloat16, torch.float16)
                or delta.requires_grad or delta.device != weight.device or not weight.is_contiguous()
                or weight.data_ptr() % 16):
            continue
        try:
            n_params, inner = param_layout(weight, delta.numel(), q.axis, q.per_channel, tuple(delta.shape))
        except (ValueError, RuntimeError):
            continue                # the lazy path raises the reference's error
        vec = 4 if weight.dtype == torch.float32 else 8
        if n_params > 1 and inner % vec:
            continue
        item = (weight.detach(), delta, None if q.symmetric else q._zero_float, getattr(q, '_signed', None), q.n_bits,
                q.symmetric, q.scale_domain == 'log', q.eps, n_params, inner)
        groups.setdefault((weight.device, weight.dtype), []).append((m, bias, item))
    served = 0
    for (device, _), entries in groups.items():
        with torch.cuda.device(device):
            ys = be.fake_quant_multi([e[2] for e in entries])
        for (m, bias, _), y in zip(entries, ys):
            # exactly what get_params caches: detached fp32 copies resident in HBM
            m.cached_params = (y.detach().to(torch.float32), None if bias is None else bias.detach().to(torch.float32))
            served += 1
    return served


def precalibrate_weights(model):
    """Golden-section weight ranges of every layer below `model` in ONE lock-step search
    (`range_estimators.golden_section_lockstep`) instead of one scipy search -- with a host round trip per loss
    evaluation -- per layer on its first calibrating forward.  The README's standard recipe (reference README.md:149-157:
    `--weight-quant-method MSE --weight-opt-method golden_section`) runs 102 such searches of ~35 evaluations each on a
    BERT-base; the weights do not depend on the data, so the searches are independent and advance together: ~35 rounds of
    102 queued launches and one device->host copy each.  Every estimator keeps the thresholds and a memo of the tensor they
    were found for; the calibrating forward that follows (`pass_data_for_range_estimation`) finds them there and
    launches nothing for the search.  Same scipy calls on the same fp32 loss values: `_delta` is bit-identical
    (tests/test_bert_e2e.py::test_bert_base_readme_recipe_*).  Layers that do not qualify (other estimators, per-channel
    ranges, weights not quantized, not in an estimating state, sharded calibration) keep the lazy path.
    -> {'searches', 'rounds', 'evaluations'}"""
    from quantization.range_estimators import golden_section_lockstep, lockstep_eligible
    jobs, devices = [], set()
    for m in model.modules():
        if not isinstance(m, QuantizationHijacker) or not m._quant_w:
            continue
        mgr = m._modules.get('weight_quantizer')
        if not isinstance(mgr, QuantizationManager) or not mgr._estimating() or _hooked(mgr, mgr.range_estimator):
            continue
        weight, _ = m.get_weight_bias()
        if torch.is_tensor(weight) and lockstep_eligible(mgr.range_estimator, weight):
            jobs.append((mgr.range_estimator, weight))
            devices.add(weight.device)
    if len(jobs) < 2 or len(devices) != 1:
        return {'searches': 0, 'rounds': 0, 'evaluations': 0}
    with torch.cuda.device(next(iter(devices))) if next(iter(devices)).type == 'cuda' else _null():
        return golden_section_lockstep(jobs)


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def int8_stair_status(model):
    """{QuantLinear name: {n_bins: table accepted by its builder?}} for every integer Linear below `model` that has built a
    GELU staircase table so far.  Reads the tables' headers (a host synchronisation): diagnostics, not the data path."""
    report = {}
    for name, m in model.named_modules():
        tables = getattr(m, '_int8_stair', None)
        if isinstance(m, QuantLinear) and tables:
            report[name] = {n_bins: bool(entry[1][0][:16].view(torch.float32)[3].item() == 1.0)
                            for n_bins, entry in tables.items() if torch.is_tensor(entry[1][0])}
    return report


class QuantLinear(QuantizationHijacker, nn.Linear):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._int8_cache = None
        self._int8_signed = None
        self._int8_stair = None
        self._int8_cls_cache = None

    def run_forward(self, x, weight, bias, offsets=None):
        return F.linear(x.contiguous(), weight.contiguous(), bias=bias)

    def forward(self, x, offsets=None):
        if options.int8_active() and (options.INT8_LINEAR is True or not self.training):
            amgr = self._modules.get('activation_quantizer')
            calibrating = self._quant_a and type(amgr) is QuantizationManager and amgr._estimating()
            y = self._int8_calibrating_forward(x) if calibrating else self._int8_forward(x)
            if y is not None:
                return y
        return super().forward(x, offsets)

    def _int8_calibrating_forward(self, x):
        """options.INT8_CALIBRATION: this layer's output quantizer is still ESTIMATING its range, but the input lies on
        the grid its producer just set (provenance: the estimating quantizer tags what it returns) and the weight grid
        is known -- so the GEMM is the same exact integer contraction as in a fixed-range forward (the fp32 simulation
        of the layered route approximates this very value), with bias and activation function in the epilogue and the
        un-quantized fp32 result handed to the estimator as usual.  None: not applicable, the layered modules run."""
        amgr = self._modules.get('activation_quantizer')
        if (not options.INT8_CALIBRATION or self.training or not self._quant_a or type(amgr) is not QuantizationManager
                or not amgr._estimating() or torch.is_grad_enabled()):
            return None
        # small GEMMs stay with torch's fp32 GEMM: the integer path costs one more launch (the input's indices) and ~60 us
        # more host time per layer than F.linear -- at [8,128] tokens an eager calibrating forward was 12.2 instead of 7.8 ms
        if x.is_cuda and x.numel() // self.in_features * self.in_features * self.out_features < options.INT8_CALIBRATION_MIN_MACS:
            return None
        pre = self._int8_forward(x, with_output_quantizer=False, peg=False)   # bias + activation applied, no quantizer
        if pre is None:
            return None
        self._save('', pre)
        out = amgr.quantize(pre)
        self._save('_Q', out)
        return out

    # ---- integer path ---------------------------------------------------------------------------
    def _int8_weights(self):
        """(int8 indices [N, K], int32 row sums [N], signed grid?) of the fake-quantized weight.  The indices are
        cached per (weight version, range state); the `signed` flag -- the one host read of this path -- per range
        state only, so that a training step (weights change every iteration, ranges fixed or learnable) re-quantizes
        its weights without a host synchronisation and stays hipGraph-capturable.  While a TRAINING step is being
        captured the weights are always re-quantized: the recorded launches must not depend on a cache hit."""
        wq = self.weight_quantizer.quantizer
        rkey = wq.range_state_key()
        if self._int8_signed is None or self._int8_signed[0] != rkey:
            self._int8_signed = (rkey, bool(wq.signed))          # host sync, once per range state
        key = (self.weight.data_ptr(), self.weight._version, rkey)
        recording = (torch.is_grad_enabled() and self.weight.requires_grad and torch.cuda.is_available()
                     and torch.cuda.is_current_stream_capturing())
        if self._int8_cache is None or self._int8_cache[0] != key or recording:
            be = _hip.backend()
            n_par = wq._delta.numel()
            w_idx = be.quantize_to_int8(self.weight.detach(), wq._delta, None, wq._signed, wq.n_bits, True,
                                        False, wq.eps, n_par, self.in_features if n_par > 1 else 1,
                                        minus_128=False)
            self._int8_cache = (key, w_idx, be.rowsum_i8(w_idx))
        return self._int8_cache[1], self._int8_cache[2], self._int8_signed[1]

    def _int8_weight_side_ok(self):
        """The weight half of the integer path's preconditions: fixed symmetric <= 8-bit linear-domain weight ranges
        (per-tensor or per-output-channel), weights quantized, nothing recording this layer's activations."""
        from quantization.quantization_manager import Qstates
        wmgr = self.weight_quantizer
        if _hooked(wmgr, getattr(wmgr, 'quantizer', None), self._modules.get('activation_quantizer'),
                   getattr(self._modules.get('activation_quantizer'), 'quantizer', None), self.activation_function):
            return False                 # somebody observes a stage the fused launch would skip: layered route
        if not (self._quant_w and self.activation_save_target is None and isinstance(wmgr, QuantizationManager)):
            return False
        if wmgr.state != Qstates.fix_ranges:
            # calibrating forward (options.INT8_CALIBRATION): the weight range is whatever the layered route's first step
            # -- get_params(): estimate, fake-quantize, cache in eval mode -- leaves behind; run exactly that step
            if not (options.INT8_CALIBRATION and not self.training and wmgr._estimating() and not torch.is_grad_enabled()):
                return False
            self.get_params()
        return bool(wmgr.quantizer.is_initialized
                    and wmgr.quantizer.symmetric and wmgr.quantizer.n_bits <= 8
                    and wmgr.quantizer.scale_domain == 'linear'
                    and wmgr.quantizer._delta.numel() in (1, self.out_features)
                    and not wmgr.quantizer._delta.requires_grad)

    def _int8_plan(self, x, with_output_quantizer=True, peg=False, mp16=False, skinny=False, ragged=False):
        """Arguments of the integer evaluation of this layer for input `x`, or None when the configuration does not
        allow it (no fixed per-tensor asymmetric <= 8-bit input quantizer known for x, unsupported weight / output
        quantizer, shapes the MFMA kernel does not tile, ...).  peg=True also accepts an input on a per-embedding-group
        grid (quantization/peg.py), mp16=True one on a per-tensor grid of 9..16 bits (mixed precision W8A16), skinny=True
        a shape no tile covers (options.INT8_HEAD; 'always': any shape the skinny kernel takes), ragged=True any row count
        for the per-tensor <= 8-bit plan (options.INT8_RAGGED: the backend launches over padded rows) and, with
        options.INT8_RAGGED_RECIPES on top, for the MP16 and PEG plans: only callers that hand the plan to `_int8_compute` may
        ask for them."""
        src = provenance.quantizer_of(x)                 # the quantizer that produced x (fixed range)
        if not _hip.on_device(x) or x.dtype != torch.float32:
            return None
        plan = self._int8_plan_from(src, x.numel() // self.in_features, with_output_quantizer, peg=peg, mp16=mp16,
                                    skinny=skinny, ragged=ragged)
        if plan is not None and plan.kind is SKINNY and src.n_bits > 8 and (x.dim() != 2 or provenance.planes_of(x) is None):
            # a wide skinny input is the [rows, K] output of a skinny launch with its producer's byte planes, or the Linear stays
            # layered (a [B, T, d] hidden state with planes, options.INT8_PLANE_TAILS, is for the MP16 plan and the first-token
            # helper: a 16-bit Linear input at a ragged M keeps its layered route)
            return None
        return plan

    def _int8_plan_from(self, src, M, with_output_quantizer=True, peg=False, mp16=False, skinny=False, ragged=False):
        """_int8_plan for an input that is known only by the quantizer `src` that produced it and its row count `M`
        (index-only producers: the fp32 tensor never exists).  -> IntPlan; its kind: PEG for an input on a per-embedding-group
        grid (with its class layout), MP16 for one on a 9..16-bit per-tensor grid, SKINNY for a shape the tiled kernels do not
        take with options.INT8_HEAD and skinny=True -- also behind a 9..16-bit per-tensor grid, whose byte planes the caller
        then owes (`_int8_plan` asks the input's record for them) --, else TILED."""
        act_code = _ACT_CODES.get(type(self.activation_function))
        if (src is None or act_code is None or not self._int8_weight_side_ok()
                or src.symmetric or src.n_bits > 16 or src._delta is None
                or src.scale_domain != 'linear' or src._delta.requires_grad):
            return None
        kind, layout = TILED, None
        # options.INT8_RAGGED_RECIPES: the backend launches the 16-bit and the class-ordered kernel over 64 * ceil(M / 64) rows too
        rows_ok = M % 64 == 0 or (ragged and M >= 1 and options.int8_ragged_recipes(_hip.backend()))
        if src.n_bits > 8:
            # 16-bit input: per-tensor (a 16-bit PEG input stays layered), shapes of tq_linear_i16x8_fwd
            be = _hip.backend()
            if (mp16 and src._delta.numel() == 1 and hasattr(be, 'linear_i16x8') and hasattr(be, 'quantize_hilo')
                    and not (self.in_features % 128 or self.out_features % 64) and rows_ok and self._int8_inference()):
                kind = MP16
            elif (skinny and src._delta.numel() == 1 and options.INT8_HEAD and hasattr(be, 'linear_i16x8_skinny')
                    and self._skinny_shape_ok(be, M) and self._int8_inference()):
                kind = SKINNY            # the head behind a 16-bit pooler: the input's byte planes, tq_linear_i16x8_skinny_fwd
            else:
                return None
        elif src._delta.numel() != 1:
            # PEG input: shapes of the class-ordered kernel
            if (not peg or not hasattr(_hip.backend(), 'linear_i8_cls') or self.in_features % 128 or self.out_features % 64
                    or not rows_ok or not self._int8_inference()):
                return None
            kind, layout = PEG, peg_layout.class_layout(src, self.in_features)
            if layout is None:
                return None
        # (the row count of an MP16 / PEG plan was settled above: whole 64-row tiles, or `rows_ok` under INT8_RAGGED_RECIPES)
        tiled = not (self.in_features % 64 or self.out_features % 32 or (M % 32 and kind is TILED) or self.in_features > 16384)
        if kind is not SKINNY and (not tiled or (skinny == 'always' and kind is TILED)):
            # no tile covers the shape (BERT's pooler: M = batch, classifier: N = num_labels).  options.INT8_HEAD: the skinny
            # kernel takes few rows and any N for an 8-bit per-tensor input grid.
            # skinny='always' (the first-token helper): also where a tile would fit (batch 32, 64, ...), so that the pooler has
            # ONE definition -- float64 Tanh, first-token rows read in place -- at every batch size the kernel takes
            be = _hip.backend()
            if (skinny and kind is TILED and options.INT8_HEAD and hasattr(be, 'linear_i8_skinny')
                    and self._skinny_shape_ok(be, M) and self._int8_inference()):
                kind = SKINNY
            elif not tiled:
                # options.INT8_RAGGED: the backend launches the tiled kernel over 64 * ceil(M / 64) rows.
                # Behind the skinny plan: where both options apply (a ragged M <= 256 with skinny=True) the Linear keeps the
                # kernel it has under INT8_HEAD alone -- one definition of its Tanh / GELU whatever INT8_RAGGED says.
                if not (ragged and kind is TILED and M >= 1 and options.int8_ragged(be) and self._int8_inference()
                        and not (self.in_features % 64 or self.out_features % 32 or self.in_features > 16384)):
                    return None
        q_out = None
        amgr = self.activation_quantizer
        if with_output_quantizer and self._quant_a and not isinstance(amgr, FP32Acts):
            if not _fixed_per_tensor_manager(amgr) or amgr.quantizer._delta.requires_grad:
                return None
            q_out = QSpec.of(amgr.quantizer)
        return _new_tuple(IntPlan, (src, act_code, q_out, kind, layout))

    def _skinny_shape_ok(self, be, M):
        """the shape limits both skinny entries share (include/tq_hip.h)"""
        return (1 <= M <= getattr(be, 'SKINNY_MAX_ROWS', 256) and self.in_features % 16 == 0
                and self.in_features <= getattr(be, 'SKINNY_MAX_K', 16384))

    def _int8_inference(self):
        """The gate of every plan but the whole-tile TILED one: no parameter of this layer needs a gradient from this call."""
        return not (torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in (self.weight, self.bias)))

    def _int8_cls_weights(self, layout):
        """(int8 weight indices with their columns in the class order of `layout`, int32 per-class row sums [C, N], the
        order as a device tensor), cached per (weight version, weight range state, class layout)."""
        w_idx, _, _ = self._int8_weights()
        key = (self._int8_cache[0], layout.key)
        c = self._int8_cls_cache
        if c is None or c[0] != key or c[3] is not layout:
            be = _hip.backend()
            order = layout.order_on(w_idx.device)
            w_c = w_idx if layout.identity else w_idx.index_select(1, order).contiguous()
            starts = (0,) + layout.ends[:-1]
            rs = torch.stack([be.rowsum_i8(w_c[:, s:e].contiguous()) for s, e in zip(starts, layout.ends)]).contiguous()
            # (the order tensor rides along: a recorded graph's gather reads it, graphs.derived_cache_tensors keeps it)
            c = self._int8_cls_cache = (key, w_c, rs, layout, order)
        return c[1], c[2], c[4]

    def _int8_operands(self, x, plan, x_idx=None):
        """Kernel operands of the integer evaluation (IntOperands), or None when the weight grid is unsigned (indices do not
        fit int8: the layered path runs, counted in INT8_STATS).  A 16-bit plan gets the two int8 byte planes of its input's
        indices: x_idx the high one, x_lo the low one.  x_idx given (index-only producer): `x` is not touched."""
        src = plan.src
        be = _hip.backend()
        w_idx, rowsum, w_signed = self._int8_weights()
        if not w_signed:
            INT8_STATS['unsigned_weight_fallbacks'] += 1
            return None
        if plan.kind is PEG:
            return self._int8_cls_operands(x, plan, x_idx)
        x_q, x_lo = XGrid.of(src), None
        if plan.kind is MP16:
            # the two byte planes of the 16-bit indices: the ones its producer wrote (a LayerNorm tail under
            # options.INT8_PLANE_TAILS; the record holds for this unchanged tensor on an unchanged grid only), else one
            # launch over x
            if x_idx is None:
                x_idx = provenance.planes_like(x)
            x_idx, x_lo = be.quantize_hilo(x.detach(), x_q) if x_idx is None else x_idx
        elif plan.kind is SKINNY and src.n_bits > 8:
            # the byte planes its producer wrote (the skinny pooler): no launch between the two (`_int8_plan` saw the record)
            x_idx, x_lo = provenance.planes_of(x) if x_idx is None else x_idx
        else:
            x_idx = self._int8_input_indices(x, src, x_idx, 1)
        wq = self.weight_quantizer.quantizer
        bias = None if self.bias is None else self.bias.detach()
        return _new_tuple(IntOperands, (x_idx, x_lo, w_idx, rowsum, bias, x_q, wq._delta.reshape(-1), wq.eps, None))

    def _int8_input_indices(self, x, src, x_idx, n_params):
        """the input's int8 indices, natural column order: handed in, the producer's (provenance), or one launch over x"""
        if x_idx is None:
            x_idx = provenance.indices_of(x)
        if x_idx is None or (x is not None and x_idx.shape != x.shape):
            x_idx = _hip.backend().quantize_to_int8(x.detach(), *QSpec.index_grid(src), n_params, 1, minus_128=True)
        return x_idx

    def _int8_cls_operands(self, x, plan, x_idx=None):
        """_int8_operands for an input on a per-embedding-group grid: per-class row sums and the class layout, with the columns
        of x_idx and w_idx in class order.  Indices recorded by provenance.py are
        in natural column order (every producer writes them so); they are reordered here into a tensor that never leaves
        this call.  Without them the input is quantized per column first.  At a row count that is no multiple of 64
        (options.INT8_RAGGED_RECIPES) the gather writes straight into a buffer with room for the rows the launch covers."""
        src, layout = plan.src, plan.layout
        w_c, cls_rs, order = self._int8_cls_weights(layout)
        x_idx = self._int8_input_indices(x, src, x_idx, self.in_features)
        if not layout.identity:
            roomy = getattr(_hip.backend(), '_rows_empty', None) if (x_idx.numel() // self.in_features) % 64 else None
            if roomy is None:
                x_idx = x_idx.index_select(-1, order)
            else:
                x_idx = torch.index_select(x_idx, -1, order, out=roomy(tuple(x_idx.shape), torch.int8, x_idx.device, force=True))
        wq = self.weight_quantizer.quantizer
        bias = None if self.bias is None else self.bias.detach()
        return _new_tuple(IntOperands, (x_idx.contiguous(), None, w_c, cls_rs, bias, XGrid.of(src), wq._delta.reshape(-1), wq.eps,
                                        layout))

    def _int8_act_stair(self, act_code, q_out, rows, n_bins=None):
        """(table, n_bins) of GELU + this layer's output quantizer for the integer epilogue of a call with `rows` input
        rows, cached per range state of that quantizer and bin count (built by one launch, no host read), or None (no
        GELU, no output quantizer, > 8 bits, switched off).  Unlike the int8 weights it is NOT rebuilt while a training
        step is being recorded: the integer path requires FIXED output ranges (`_int8_plan_from`), so the table a recorded
        launch reads stays valid for every replay, and `GraphedForward` / `GraphedTrainStep` keep the tensors of all
        derived caches they recorded alive (`quantization.graphs.derived_cache_tensors`)."""
        be = _hip.backend()
        if (act_code != _hip.ACT_GELU or q_out is None or q_out.n_bits > 8 or not options.INT8_ACT_STAIR
                or not hasattr(be, 'act_stair')):
            return None
        if n_bins is None:
            n_bins = be.stair_bins_for(rows, self.out_features) if hasattr(be, 'stair_bins_for') else None
        oq = self.activation_quantizer.quantizer
        # the table bakes in delta, zero_float, the grid ends and eps: every one of them is part of the key (an in-place
        # `zero_float.fill_()` moves neither `_range_gen` nor `_delta._version`)
        zf, sg = oq._buffers.get('_zero_float'), oq._buffers.get('_signed')
        key = (oq.range_state_key(), None if zf is None else zf._version, None if sg is None else sg._version, oq.eps,
               oq.symmetric)
        if self._int8_stair is None:
            self._int8_stair = {}
        cached = self._int8_stair.get(n_bins)           # one table per bin count (two call shapes may alternate)
        if (cached is None or cached[0] != key
                or getattr(cached[1][0], 'device', q_out.delta.device) != q_out.delta.device):
            cached = self._int8_stair[n_bins] = (key, be.act_stair(act_code, q_out, n_bins))
        return cached[1]

    def _int8_compute(self, x, plan, x_idx=None, index_only=False, want_planes=False, rows=None):
        """The fused integer Linear itself (no autograd): y [, its int8 indices] or None (unsigned weight grid).
        index_only: only the int8 indices of the output are produced and returned (the consumer is another integer
        Linear; needs an asymmetric <= 8-bit output quantizer in the plan).  SKINNY plans only -- want_planes: where the
        output quantizer's grid has 9..16 bits (`emits_planes`) the launch also writes the byte planes of the indices and y
        leaves with them in its record; rows: int32 device row numbers into x_idx, one per output row (a packed batch's
        first tokens)."""
        act_code, q_out = plan.act, plan.q_out
        ops = self._int8_operands(x, plan, x_idx)
        if ops is None:
            return None
        oq = self.activation_quantizer.quantizer if q_out is not None else None
        want_idx = emits_int8(oq)
        want_planes = bool(want_planes and plan.kind is SKINNY and not index_only and emits_planes(oq)
                           and hasattr(_hip.backend(), 'linear_i16x8_skinny'))
        INT8_STATS['kernel_calls'] += 1
        be = _hip.backend()
        if index_only:
            assert want_idx, 'index-only output needs an asymmetric <= 8-bit output quantizer'
        kind, want_y, N, K = plan.kind, not index_only, self.out_features, self.in_features
        # every kernel takes the weight side, the input grid, the epilogue and the output form alike, behind its own input
        # operands; the three tiled ones a staircase table for GELU, sized by the kernel's own rule (None: no table)
        if kind is TILED:
            stair = self._int8_act_stair(act_code, q_out, ops.rows)
            out = be.linear_i8(ops.x_idx, ops.w_idx, ops.rowsum, ops.bias, ops.x_q, ops.w_delta, ops.w_eps, act_code, q_out,
                               torch.float32, want_idx=want_idx, want_y=want_y, stair=stair)
        elif kind is SKINNY:
            # few rows / any N: no staircase (the kernel evaluates the correctly rounded activation itself); a strided 2-D view
            # of the indices (the first token of every sequence) goes to the kernel as it is
            flat = ops.x_idx.dim() == 2
            xi = ops.x_idx if flat else ops.x_idx.reshape(-1, K)
            if ops.x_lo is not None or want_planes or rows is not None:
                # a 16-bit input's planes, index planes out or a row table: the entry that takes them (the 8-bit recipes of a
                # padded batch call tq_linear_i8_skinny_fwd, which is this entry without planes and without a row table)
                assert flat or rows is None
                xin = xi if ops.x_lo is None else (xi, ops.x_lo if flat else ops.x_lo.reshape(-1, K))
                out = be.linear_i16x8_skinny(xin, ops.w_idx, ops.rowsum, ops.bias, ops.x_q, ops.w_delta, ops.w_eps, act_code,
                                             q_out, torch.float32, want_idx=want_idx, want_planes=want_planes, want_y=want_y,
                                             rows=rows)
            else:
                out = be.linear_i8_skinny(xi, ops.w_idx, ops.rowsum, ops.bias, ops.x_q, ops.w_delta, ops.w_eps, act_code, q_out,
                                          torch.float32, want_idx=want_idx, want_y=want_y)
            if not flat:
                shape = tuple(ops.x_idx.shape[:-1]) + (N,)
                rs = lambda t: None if t is None else (tuple(u.reshape(shape) for u in t) if isinstance(t, tuple) else t.reshape(shape))
                out = tuple(rs(t) for t in out) if (want_idx or want_planes) else out.reshape(shape)
        elif kind is MP16:              # 16-bit input: the two byte planes
            rows = _rows_covered(ops.rows)
            bins = be.i16x8_stair_bins_for(rows, N, K) if hasattr(be, 'i16x8_stair_bins_for') else None
            stair = None if bins is None else self._int8_act_stair(act_code, q_out, rows, n_bins=bins)
            out = be.linear_i16x8(ops.x_idx, ops.x_lo, ops.w_idx, ops.rowsum, ops.bias, ops.x_q, ops.w_delta, ops.w_eps, act_code,
                                  q_out, torch.float32, want_idx=want_idx, want_y=want_y, stair=stair)
        else:                           # per-embedding-group input: the class-ordered kernel
            rows = _rows_covered(ops.rows)      # the bin count follows the tile plan of the rows the launch covers
            bins = be.cls_stair_bins_for(rows, N, K, ops.layout.n_classes)
            stair = None if bins is None else self._int8_act_stair(act_code, q_out, rows, n_bins=bins)
            out = be.linear_i8_cls(ops.x_idx, ops.w_idx, ops.rowsum, ops.bias, ops.x_q, ops.layout.table(be), ops.w_delta,
                                   ops.w_eps, act_code, q_out, torch.float32, want_idx=want_idx, want_y=want_y, stair=stair)
        if index_only:
            return out[1]
        return tagged(out, oq, want_idx, want_planes)   # (the indices / planes: the next integer Linear consumes these)

    def _int8_forward(self, x, with_output_quantizer=True, peg=True):
        """Integer-GEMM evaluation of this layer, or None when the configuration does not allow it.
        with_output_quantizer=False returns the pre-quantizer output (for fused layer tails).

        Inference: the fused kernel alone.  Training / autograd (QAT with fixed ranges): the same integer forward on
        the matrix cores, wrapped in `_Int8LinearSTE` whose backward is the straight-through estimator of the layered
        modules (reference hijacker.py:66-116, quantizers.py:12-33)."""
        plan = self._int8_plan(x, with_output_quantizer, peg=peg, skinny=True, ragged=True)   # (16-bit inputs: the fused feed-forward block alone opts in)
        if plan is None:
            return None
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad or
                                                   (self.bias is not None and self.bias.requires_grad))
        if needs_grad and plan.kind is not TILED:
            return None                      # per-embedding-group, 16-bit and skinny plans: inference only
        if not needs_grad:
            return self._int8_compute(x, plan)
        if not with_output_quantizer:
            return None                      # fused tails are inference-only
        y = _Int8LinearSTE.apply(x, self.weight, self.bias, self, plan)
        if y is not None and plan.q_out is not None:
            provenance.tag(y, self.activation_quantizer.quantizer, provenance.indices_of(y))
        return y


class _Int8LinearSTE(torch.autograd.Function):
    """y = Q_out(act(F.linear(x, Q_w(W), b))) evaluated exactly on the integer grids by the MFMA kernel; gradients of
    the layered modules.  The backward re-runs the layered forward of this ONE layer under autograd (fp32 GEMM, STE
    fake-quant kernels) and differentiates it: by construction the gradients w.r.t. x, W and b are those of the
    reference's module chain, at the cost of one recomputed GEMM (activation-checkpoint style); the pre-activation
    tensor never has to be written by the forward."""

    @staticmethod
    def forward(ctx, x, weight, bias, layer, plan):
        INT8_STATS['autograd_calls'] += 1
        y = layer._int8_compute(x, plan)
        if y is None:
            raise _hip.TQError('integer Linear: unsigned weight grid under autograd (disable options.INT8_LINEAR)')
        ctx.layer = layer
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        (x,) = ctx.saved_tensors
        layer = ctx.layer
        with torch.enable_grad():
            xr = x.detach().requires_grad_(True)
            y = QuantizationHijacker.forward(layer, xr)                 # layered path, straight-through estimators
            params = [p for p in (layer.weight, layer.bias) if p is not None and p.requires_grad]
            grads = torch.autograd.grad(y, [xr] + params, grad_y, allow_unused=True)
        gx = grads[0] if ctx.needs_input_grad[0] else None
        it = iter(grads[1:])
        gw = next(it) if layer.weight.requires_grad else None
        gb = next(it) if (layer.bias is not None and layer.bias.requires_grad) else None
        return gx, gw, gb, None, None


class QuantLayerNorm(QuantizationHijacker, nn.LayerNorm):
    def __init__(self, *args, activation=None, **kwargs):
        super().__init__(*args, activation=activation, **kwargs)

    def run_forward(self, x, weight, bias, offsets=None):
        return F.layer_norm(input=x.contiguous(), normalized_shape=self.normalized_shape,
                            weight=weight.contiguous(), bias=bias.contiguous(), eps=self.eps)


class QuantEmbedding(QuantizationHijacker, nn.Embedding):
    def __init__(self, *args, activation=None, **kwargs):
        super().__init__(*args, activation=activation, **kwargs)
        # a lookup in an already-quantized table needs no output quantizer
        self.activation_quantizer = FP32Acts()

    def run_forward(self, x, weight, bias, offsets=None):
        return F.embedding(input=x.contiguous(), weight=weight.contiguous(),
                           padding_idx=self.padding_idx, max_norm=self.max_norm,
                           norm_type=self.norm_type, scale_grad_by_freq=self.scale_grad_by_freq,
                           sparse=self.sparse)


class QuantNoNorm(QuantizationHijacker):
    """MobileBERT's element-wise affine "LayerNorm" with quantized parameters and output
    (counterpart of the reference's models/quantized_mobilebert.py:58-72).

    One weight quantizer is applied to the weight and then to the bias; while it is estimating,
    the bias call therefore overwrites the range found for the weight (upstream quirk, kept).
    With fixed ranges the whole layer -- x * Q(w) + Q(b) followed by the output quantizer -- is one
    fused launch (``tq_affine_fake_quant_fwd``) instead of ~8 element-wise kernels."""

    def __init__(self, org_model, *args, activation=None, **kwargs):
        super().__init__(*args, activation=activation, **kwargs)
        self.weight = org_model.weight
        self.bias = org_model.bias

    def _fusable(self, x):
        from quantization.quantization_manager import Qstates
        mgr = self.activation_quantizer
        return (self._quant_a and self.activation_function is None
                and self.activation_save_target is None
                and isinstance(mgr, QuantizationManager) and mgr.state == Qstates.fix_ranges
                and mgr.quantizer.is_initialized and mgr.quantizer._delta.numel() == 1
                and not torch.is_grad_enabled() and x.dim() >= 1
                and x.shape[-1] == self.weight.numel() and x.shape[-1] % 8 == 0)

    def quantized_params(self):
        """(Q(weight), Q(bias)) through the ONE weight quantizer, weight first (upstream order).  With fixed ranges in
        inference the pair is constant: cached per (parameter versions, range state) -- the reference re-quantizes both
        vectors on every forward (2 launches per NoNorm, 7 NoNorms per MobileBERT layer)."""
        if not self._quant_w:
            return self.weight, self.bias
        from quantization.quantization_manager import Qstates
        mgr = self.weight_quantizer
        cacheable = (not self.training and not torch.is_grad_enabled() and isinstance(mgr, QuantizationManager)
                     and mgr.state == Qstates.fix_ranges and mgr.quantizer.is_initialized)
        key = None
        if cacheable:
            key = (self.weight.data_ptr(), self.weight._version, self.bias.data_ptr(), self.bias._version,
                   mgr.quantizer.range_state_key())
            hit = getattr(self, '_qparam_cache', None)
            if hit is not None and hit[0] == key:
                return hit[1], hit[2]
        weight = mgr(self.weight)
        bias = mgr(self.bias)
        if cacheable:
            self._qparam_cache = (key, weight.detach(), bias.detach())
        return weight, bias

    def forward(self, x, offsets=None):
        weight, bias = self.quantized_params()
        if self._fusable(x):
            q = self.activation_quantizer.quantizer
            # feeding integer Linears (MobileBERT's bottlenecks -> query / key): emit the int8 indices in the same launch
            want_idx = (options.int8_active() and emits_int8(q) and q.scale_domain == 'linear'
                        and _hip.on_device(x) and x.dtype == torch.float32)
            out = _hip.backend().affine_fake_quant(x, weight, bias, *QSpec.of(q), **({'want_idx': True} if want_idx else {}))
            if want_idx:
                return provenance.tag(out[0], q, out[1])
            return out
        return self.quantize_activations(x * weight + bias)


class QuantizedActivationWrapper(QuantizedActivation):
    """Runs `layer` and quantizes its output; can share ("tie") the quantizer of the layer
    before it, in which case the range is not updated here (useful for average pooling)."""

    def __init__(self, layer, tie_activation_quantizers=False,
                 input_quantizer: QuantizationManager = None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.tie_activation_quantizers = tie_activation_quantizers
        if input_quantizer:
            assert isinstance(input_quantizer, QuantizationManager)
            self.activation_quantizer = input_quantizer
        self.layer = layer

    def quantize_activations_no_range_update(self, x):
        return self.activation_quantizer.quantizer(x) if self._quant_a else x

    def forward(self, x):
        x = self.layer(x)
        if self.tie_activation_quantizers:
            return self.quantize_activations_no_range_update(x)
        return self.quantize_activations(x)


module_map = {nn.Linear: QuantLinear, nn.LayerNorm: QuantLayerNorm, nn.Embedding: QuantEmbedding}

non_param_modules = (_AdaptiveAvgPoolNd, _AvgPoolNd)


def get_act(module, i):
    """First activation function after position i of a Sequential, and its index."""
    for j in range(i + 1, len(module)):
        if isinstance(module[j], tuple(activations_list)):
            return module[j], j
    return None, None


def get_linear_args(module):
    return dict(in_features=module.in_features, out_features=module.out_features,
                bias=module.bias is not None)


def get_layernorm_args(module):
    return dict(normalized_shape=module.normalized_shape, eps=module.eps)


def get_embedding_args(module):
    return {k: getattr(module, k) for k in (
        'num_embeddings', 'embedding_dim', 'padding_idx', 'max_norm', 'norm_type',
        'scale_grad_by_freq', 'sparse')}


def get_module_args(mod, act):
    if isinstance(mod, nn.Linear):
        kwargs = get_linear_args(mod)
    elif isinstance(mod, nn.LayerNorm):
        kwargs = get_layernorm_args(mod)
    elif isinstance(mod, nn.Embedding):
        kwargs = get_embedding_args(mod)
    else:
        raise ValueError
    kwargs['activation'] = act
    return kwargs


def quant_module(module, i, **quant_params):
    """Quantized copy of module[i], folding a following activation function into it."""
    act, _ = get_act(module, i)
    src = module[i]
    new_module = module_map[type(src)](**get_module_args(src, act), **quant_params)
    new_module.weight.data = src.weight.data.clone()
    if src.bias is not None:
        new_module.bias.data = src.bias.data.clone()
    return new_module, i + int(bool(act)) + 1


def quantize_sequence(model, specials=None, tie_activation_quantizers=False, **quant_params):
    specials = specials or dict()
    out = []
    i = 0
    while i < len(model):
        m = model[i]
        if isinstance(m, QuantizedModule):
            out.append(m)
        elif type(m) in module_map:
            new_module, i = quant_module(model, i, **quant_params)
            out.append(new_module)
            continue
        elif type(m) in specials:
            out.append(specials[type(m)](m, **quant_params))
        elif isinstance(m, non_param_modules):
            input_quantizer = None
            if out and isinstance(out[-1], QuantizedModule) and tie_activation_quantizers:
                input_quantizer = out[-1].activation_quantizer
                warnings.warn(f'Tying input quantizer {i}^th layer of type {type(out[-1])} to the '
                              f'quantized {type(m)} following it')
            out.append(QuantizedActivationWrapper(
                m, tie_activation_quantizers=tie_activation_quantizers,
                input_quantizer=input_quantizer, **quant_params))
        else:
            out.append(quantize_model(m, specials=specials, **quant_params))
        i += 1
    return out


def quantize_sequential(model, specials=None, tie_activation_quantizers=False, **quant_params):
    return nn.Sequential(*quantize_sequence(model, specials, tie_activation_quantizers,
                                            **quant_params))


def quantize_module_list(model, specials=None, tie_activation_quantizers=False, **quant_params):
    return nn.ModuleList(quantize_sequence(model, specials, tie_activation_quantizers,
                                           **quant_params))


def quantize_model(model, specials=None, tie_activation_quantizers=False, **quant_params):
    """Recursively replace Linear / LayerNorm / Embedding (and `specials`) by quantized versions."""
    specials = specials or dict()

    if isinstance(model, nn.Sequential):
        return quantize_sequential(model, specials, tie_activation_quantizers, **quant_params)
    if type(model) in specials:
        return specials[type(model)](model, **quant_params)
    if isinstance(model, non_param_modules):
        return QuantizedActivationWrapper(model, **quant_params)
    if type(model) in module_map:
        # exact type match on purpose: subclasses of these layers are treated as containers
        quant_model = module_map[type(model)](**get_module_args(model, None), **quant_params)
        quant_model.weight.data = model.weight.data
        if getattr(model, 'bias', None) is not None:
            quant_model.bias.data = model.bias.data
        return quant_model

    quant_model = copy.deepcopy(model)
    for name, child in quant_model._modules.items():
        new_child = quantize_model(child, specials=specials, **quant_params)
        if new_child is not None:
            setattr(quant_model, name, new_child)
    return quant_model
