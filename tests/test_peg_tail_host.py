"""Host logic of the per-column residual + LayerNorm tail, replayed on the CPU: BERT with the README's PEG recipe
({'x', 'h', 'y'}: 'ng6') runs both tails of every layer as ONE backend call each (`residual_layernorm_quant_axis`), the
first feed-forward Linear index-only through the class-ordered integer Linear and the second one through the plain integer
Linear on its int8 indices -- the [tokens, 3072] fp32 activation is never produced.  Calibration, autograd, hooks, a backend
without the new method and the per-tensor recipe keep what they did before.  The double's tail uses F.layer_norm on both
routes, so the routes differ by the exact-vs-fp32 GEMMs alone."""
import pytest
import torch

from oracle import tq_oracle as O
from tests.test_peg_route_host import _ClsOracle

# launch counts of the product's default route: run once, with the harness models' fuse switches following the option
pytestmark = pytest.mark.default_route


class _NoAxis(_ClsOracle):
    """the parent commit's double (class-ordered Linear, no per-column tail), with its integer launches recorded"""

    def __init__(self):
        super().__init__()
        self.cls_want_y, self.lin_calls, self.axis_calls = [], [], []

    def linear_i8_cls(self, *a, want_y=True, **k):
        self.cls_want_y.append(want_y)
        return super().linear_i8_cls(*a, want_y=want_y, **k)

    def linear_i8(self, x_idx, *a, **k):
        self.lin_calls.append(tuple(x_idx.shape))
        return super().linear_i8(x_idx, *a, **k)


class _AxisOracle(_NoAxis):
    """+ the per-column tail: the parent's double with `_quant(v, *a, d, 1)` for [d] parameters"""

    def residual_layernorm_quant_axis(self, dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out,
                                      want_idx=False):
        d = dense_out.shape[-1]

        def q(v, a):
            if a is None:
                return None, v
            assert a[0].numel() in (1, d) and a[0].dim() <= 1
            return self._quant(v, *a, a[0].numel(), 1)
        self.axis_calls.append(tuple(None if a is None else a[0].numel() for a in (q_dense, q_sum, q_out)))
        u = q(q(dense_out.float(), q_dense)[1] + residual.float(), q_sum)[1]
        v = torch.nn.functional.layer_norm(u, (d,), ln_weight.float(), ln_bias.float(), ln_eps)
        idx, y = q(v, q_out)
        return (y.to(dense_out.dtype), (idx - 128).to(torch.int8)) if want_idx else y.to(dense_out.dtype)


def _model(num_layers, quant_dict, calib):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from harness.bert import estimate_permutation_ranges
    from tests.harness_bert import apply_quant_dict, build_bert_base
    from utils.utils import pass_data_for_range_estimation
    permuted = any(isinstance(v, str) and v.startswith('ngp') for v in quant_dict.values())
    # (range-sorted groups are collected by the current-min-max estimator only, as in the reference)
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax,
              act_range_method=RangeEstimators.current_minmax if permuted else RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=num_layers, **qp)
    apply_quant_dict(model, quant_dict)
    model = model.eval()
    with torch.no_grad():
        if permuted:
            estimate_permutation_ranges(model, [(calib,)])
        pass_data_for_range_estimation([(calib,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
    return model


def _ids():
    g = torch.Generator().manual_seed(0)
    return torch.randint(1000, 30000, (2, 64), generator=g), torch.randint(1000, 30000, (2, 64), generator=g)


def _first(t):
    return t[0] if isinstance(t, (tuple, list)) else t


def _with_layer_outputs(model, ids):
    """logits + the output of every encoder layer (instance-level wrappers: no module hooks, which would send the hooked
    blocks down the layered route)"""
    outs = []
    for L in model.layers:
        L.forward = (lambda h, m, _f=type(L).forward, _L=L: (outs.append(_f(_L, h, m)), outs[-1])[1])
    try:
        y = _first(model(ids))
    finally:
        for L in model.layers:
            del L.forward
    return y, outs


def _run_recipe(quant_dict, layers=2):
    from quantization import _hip, options
    from quantization.autoquant_utils import INT8_STATS
    be = _AxisOracle()
    prev = _hip.set_backend(be)
    saved = options.INT8_LINEAR
    try:
        calib, ids = _ids()
        model = _model(layers, quant_dict, calib)
        assert be.axis_calls == [] and be.cls_calls == []          # calibrating forwards: layered modules only
        be.lin_calls.clear()                                        # (they may take per-tensor integer Linears)
        with torch.no_grad():
            model.fix_ranges()
            options.INT8_LINEAR = False
            layered = _first(model(ids))
            assert be.axis_calls == [] and be.cls_calls == [] and be.lin_calls == []
            options.INT8_LINEAR = 'auto'                            # the product default
            k0 = INT8_STATS['kernel_calls']
            fast, outs = _with_layer_outputs(model, ids)
            kernel_calls = INT8_STATS['kernel_calls'] - k0
        return be, model, ids, layered, fast, outs, kernel_calls
    finally:
        options.INT8_LINEAR = saved
        _hip.set_backend(prev)


def _check_route(be, model, layered, fast, outs, kernel_calls, layers=2):
    d = 768
    # two per-column tails per layer: attention output (only site x per-column), feed-forward (h and y per-column)
    assert be.axis_calls == [(1, 1, d), (d, d, 1)] * layers
    # FFN1: class-ordered, index-only -- its [tokens, 3072] fp32 output is never produced
    assert len(be.cls_calls) == layers and be.cls_want_y == [False] * layers
    assert all(shape == (2, 64, d) and len(ends) == 6 and ends[-1] == d for shape, ends in be.cls_calls)
    # FFN2 consumes FFN1's indices through the plain integer Linear
    assert sum(1 for s in be.lin_calls if s[-1] == 3072) == layers
    # every integer Linear launch is one of the double's recorded calls
    assert kernel_calls >= len(be.lin_calls) + len(be.cls_calls) and len(be.lin_calls) >= 2 * layers
    # every encoder output lies on the grid of its quantizer (site z: per-tensor under this recipe)
    for L, h in zip(model.layers, outs):
        q = L.output.LayerNorm.activation_quantizer.quantizer
        assert torch.equal(O.fake_quant(h, q._delta, q._zero_float, 8, False)[1], h)
    diff = (fast.float() - layered.float()).abs()
    assert float(diff.max()) <= 0.05 * float(layered.abs().max()) + 1e-6, float(diff.max())


def test_peg_recipe_takes_both_tails_and_ffn2_on_the_integer_route_cpu():
    be, model, ids, layered, fast, outs, kc = _run_recipe({'x': 'ng6', 'h': 'ng6', 'y': 'ng6'})
    _check_route(be, model, layered, fast, outs, kc)


def test_permuted_groups_take_the_same_launches_cpu():
    be, model, ids, layered, fast, outs, kc = _run_recipe({'x': 'ngp6', 'h': 'ngp6', 'y': 'ngp6'})
    _check_route(be, model, layered, fast, outs, kc)
    # the groups really are scattered over the columns
    q = model.layers[0].output.dense.activation_quantizer.quantizer
    dl = q._delta.reshape(-1)
    assert dl.numel() == 768 and int((dl[1:] != dl[:-1]).sum()) > 5


def test_layered_route_is_kept_where_it_was_cpu():
    from quantization import _hip, options
    from quantization.autoquant_utils import INT8_STATS
    be, model, ids, layered, fast, outs, kc = _run_recipe({'x': 'ng6', 'h': 'ng6', 'y': 'ng6'})
    saved = options.INT8_LINEAR
    prev = _hip.set_backend(be)
    try:
        n_axis = len(be.axis_calls)
        # autograd (parameters require grad, grad mode on): layered
        options.INT8_LINEAR = True
        model(ids)
        assert len(be.axis_calls) == n_axis
        options.INT8_LINEAR = 'auto'
        with torch.no_grad():
            # an observer on a stage the fused launch would skip: that block stays layered, the others do not
            hook = model.layers[0].output.res_act_quantizer.register_forward_hook(lambda m, a, o: None)
            try:
                hooked = _first(model(ids))
            finally:
                hook.remove()
            assert be.axis_calls[n_axis:] == [(1, 1, 768), (1, 1, 768), (768, 768, 1)]
            # a backend without the new method keeps the parent's route: class-ordered FFN1 WITH its fp32 output, the tails
            # and FFN2 as layered modules
            old = _NoAxis()
            _hip.set_backend(old)
            k0 = INT8_STATS['kernel_calls']
            parent = _first(model(ids))
            assert old.cls_want_y == [True, True] and not any(s[-1] == 3072 for s in old.lin_calls)
            assert INT8_STATS['kernel_calls'] - k0 >= len(old.lin_calls) + len(old.cls_calls)
            _hip.set_backend(be)
            bound = 0.05 * float(layered.abs().max()) + 1e-6
            assert float((parent.float() - layered.float()).abs().max()) <= bound
            assert float((hooked.float() - layered.float()).abs().max()) <= bound
            # calibrating forwards: layered
            n_axis = len(be.axis_calls)
            model.estimate_ranges()
            model(ids)
            assert len(be.axis_calls) == n_axis
    finally:
        options.INT8_LINEAR = saved
        _hip.set_backend(prev)


def test_per_tensor_recipe_makes_no_axis_tail_calls_cpu():
    be, model, ids, layered, fast, outs, kc = _run_recipe({})
    assert be.axis_calls == [] and be.cls_calls == []
    assert sum(1 for s in be.lin_calls if s[-1] == 3072) == 2          # the per-tensor FFN hand-over is what it was
