"""options.FUSED_LN_AXIS_TRAINING: `fused.residual_layernorm_quant` under autograd with per-column quantizers = the axis forward
launch + the one-launch backward, against the float64 reference of tests/test_ln_axis_quant_bwd.py (T) within its bounds and
against the layered modules' autograd within TWICE those bounds; the gradients of x and of dense's parameters through the
linear-map argument of tests/test_ln_training_route.py (R), whose tail block this file gives per-column parameters: K's ranges
times (0.85 + 0.06 g) for six groups of columns."""
import copy

import pytest
import torch

from tests import test_ln_axis_quant_bwd as T
from tests import test_ln_training_route as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def switch():
    from quantization import options
    options.FUSED_LN_AXIS_TRAINING = False
    yield lambda on: setattr(options, 'FUSED_LN_AXIS_TRAINING', on)
    options.FUSED_LN_AXIS_TRAINING = False


def _block(learn, per_column=True, **kw):
    blk, x, r, gy = R._block(learn, **kw)
    d = x.shape[-1]
    for q in R._acts(blk) if per_column else ():
        f = (0.85 + 0.06 * (torch.arange(d, device=x.device) * 6 // d)).float()
        new = [q._delta.detach().reshape(1) * f, q._zero_float.detach().expand(d).clone()]
        q._delta, q._zero_float = (torch.nn.Parameter(t) for t in new) if learn else new
    return blk, x, r, gy


def _grads(blk, x, r, gy):
    """R._grads with range gradients [2, d]"""
    from quantization.fused import residual_layernorm_quant
    x, r = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    blk.zero_grad()
    y = residual_layernorm_quant(blk.dense, blk.res_act_quantizer, blk.LayerNorm, x, r)
    y.backward(gy)
    out = {'y': y.detach(), 'x': x.grad, 'residual': r.grad, 'dense.weight': blk.dense.weight.grad, 'dense.bias': blk.dense.bias.grad,
           'ln_weight': blk.LayerNorm.weight.grad, 'ln_bias': blk.LayerNorm.bias.grad}
    for name, q in zip(('q_dense', 'q_sum', 'q_out'), R._acts(blk)):
        if q._delta.requires_grad:
            out[name] = torch.stack([q._delta.grad.reshape(-1), q._zero_float.grad.reshape(-1)])
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize('learn', [False, True])
def test_gradients_match_reference_and_layered_autograd(learn, switch, monkeypatch):
    from quantization import _hip
    from quantization.int8_route import QSpec
    blk, x, r, gy = _block(learn)
    off = _grads(blk, x, r, gy)
    switch(True)
    cls, calls = type(_hip.backend()), []
    bwd = cls.residual_layernorm_quant_axis_bwd
    monkeypatch.setattr(cls, 'residual_layernorm_quant_axis_bwd', lambda *a, **kw: calls.append(1) or bwd(*a, **kw))
    on = _grads(blk, x, r, gy)
    assert set(on) == set(off) and len(on) == (10 if learn else 7) and len(calls) == 1
    with torch.no_grad():
        wq, bq = blk.dense.get_params()
        gemm = blk.dense.run_forward(x, wq, bq)
        ln_w, ln_b = blk.LayerNorm.get_params()
        blk.eval()
        assert torch.equal(on['y'], blk(x, r))                                  # the value is the fused (axis) forward's
    c = lambda t: t.detach().cpu().reshape(-1, t.shape[-1])
    qs = [QSpec.of(q)._replace(delta=c(q._delta)[0], zero_float=c(q._zero_float)[0]) for q in R._acts(blk)]
    ref = T._reference(c(gemm), c(r), c(gy), c(ln_w)[0], c(ln_b)[0], qs, c(on['y']), 1)
    g, B = ref['dense']
    W, X, n = c(wq).double(), c(x).double(), T.U * (R.D + 2)
    ref['x'] = (g @ W, B @ W.abs() + n * (g.abs() @ W.abs()))
    ref['dense.weight'] = (g.t() @ X, B.t() @ X.abs() + 44 * T.U * (g.abs().t() @ X.abs()))
    ref['dense.bias'] = (g.sum(0), B.sum(0) + 44 * T.U * g.abs().sum(0))
    for name in set(on) - {'y'}:
        (val, bound), (a, b) = ref[name], (c(t).double().reshape(ref[name][0].shape) for t in (on[name], off[name]))
        assert bool(((a - b).abs() <= 2 * bound).all()), name
        assert bool((((b == 0) & (name == 'dense.weight')) | ((a - val).abs() <= bound)).all()), name


@pytest.mark.parametrize('decline', ['off', 'hook', 'save_target', 'estimating', 'd48', 'nonorm', 'per_tensor_only'])
def test_declines_are_bit_equal_to_today(decline, switch, monkeypatch):
    from quantization import _hip
    blk, x, r, gy = _block(decline != 'estimating', per_column=decline != 'per_tensor_only', d=48 if decline == 'd48' else R.D,
                           nonorm=decline == 'nonorm')
    if decline == 'hook':
        blk.res_act_quantizer.activation_quantizer.register_forward_hook(lambda *a: None)
    if decline == 'save_target':
        blk.dense.activation_save_target = {}
        blk.dense.activation_save_name = 'site'
    if decline == 'estimating':
        blk.res_act_quantizer.estimate_ranges_train()
    ref = _grads(copy.deepcopy(blk), x, r, gy)          # today's: the option is off (copies: an estimating forward moves ranges)
    switch(decline != 'off')

    def no_launch(*a, **kw):
        raise AssertionError('the route was taken')
    monkeypatch.setattr(type(_hip.backend()), 'residual_layernorm_quant_axis_bwd', no_launch)
    now = _grads(copy.deepcopy(blk), x, r, gy)
    assert set(ref) == set(now) and all(torch.equal(ref[k], now[k]) for k in ref)


def test_whole_model_step_eager_and_graphed(switch, monkeypatch):
    """a 2-layer harness BERT (d = 384) under per_groups=6 with learnable ranges: one training step with the switch on, eager ==
    GraphedTrainStep bit for bit, loss == off's; the tails take the route: 2 layers x 2 backward launches in the eager step"""
    from transformers import BertConfig, BertForSequenceClassification
    from harness.bert import apply_activation_granularity
    from quantization import _hip
    from quantization.quantizers import QMethods
    from tests.harness_bert import QBertForSequenceClassification
    from tests.test_softmax_training_route import _step_arms
    torch.manual_seed(0)
    cfg = BertConfig(hidden_size=384, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, num_labels=2,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base = QBertForSequenceClassification(BertForSequenceClassification(cfg).eval(), method=QMethods.symmetric_uniform,
                                          act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8)
    assert apply_activation_granularity(base, per_groups=6) > 0
    base = base.cuda()
    g = torch.Generator().manual_seed(0)
    ids, labels = torch.randint(1000, 30000, (2, 64), generator=g).cuda(), torch.randint(0, 2, (2,), generator=g).cuda()
    with torch.no_grad():
        base.set_quant_state(True, True)
        base.estimate_ranges()
        base(ids)
    base.learn_ranges()
    cls, calls = type(_hip.backend()), []
    bwd = cls.residual_layernorm_quant_axis_bwd
    monkeypatch.setattr(cls, 'residual_layernorm_quant_axis_bwd', lambda *a, **kw: calls.append(torch.cuda.is_current_stream_capturing()) or bwd(*a, **kw))
    _step_arms(base.train(), (ids,), (labels,), torch.nn.functional.cross_entropy, switch)
    assert calls.count(False) >= 4 and len(calls) >= 8
