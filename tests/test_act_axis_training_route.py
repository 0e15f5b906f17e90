"""options.FUSED_ACT_AXIS_TRAINING: QuantLinear.forward under autograd with a per-column output quantizer = F.linear without bias
+ tq_bias_act_quant_axis_fwd + the one-launch backward, against the float64 reference of tests/test_act_axis_quant_bwd.py (A)
within its bounds and against the layered modules' autograd within TWICE them (the rule of tests/test_act_training_route.py;
x's and the weight's bounds through |W| and |X| as there).  The site: a QuantLinear(64 -> 96), with and without GELU, whose
output quantizer is set per column by set_act_quant_axis_and_groups(axis=2, n_groups=6) on [2, 21, 64] (96 columns: six groups
need a width they divide), its estimated ranges shrunk so that every group's clamp cuts data on both sides."""
import copy

import pytest
import torch
from torch import nn

from tests import test_act_axis_quant_bwd as A
from tests import test_act_quant_bwd as K

pytestmark = pytest.mark.gpu
N_OUT = 96


@pytest.fixture
def switch():
    from quantization import options
    options.FUSED_ACT_AXIS_TRAINING = options.FUSED_ACT_TRAINING = False
    yield lambda on, name='FUSED_ACT_AXIS_TRAINING': setattr(options, name, on)
    options.FUSED_ACT_AXIS_TRAINING = options.FUSED_ACT_TRAINING = False


def _site(gelu, learn, dev='cuda', act=None, per_column=True, per_channel=False):
    """-> (model, its QuantLinear, x [2, 21, 64], grad_y); `act`: another activation module"""
    from quantization.autoquant_utils import quantize_model
    from quantization.quantizers import QMethods
    from utils.per_embd_quant_utils import set_act_quant_axis_and_groups
    torch.manual_seed(0)
    fp = nn.Sequential(nn.Linear(64, N_OUT), act or nn.GELU()) if gelu else nn.Linear(64, N_OUT)
    model = quantize_model(fp, method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8)
    layer = model[0] if gelu else model
    layer.to(dev).quantized()
    if per_column:
        set_act_quant_axis_and_groups(layer, axis=2, n_groups=6)
    x, _, gy = K._inputs(42, N_OUT, 4)
    x, gy = x[:, :64].reshape(2, 21, 64).to(dev), gy.reshape(2, 21, N_OUT).to(dev)
    with torch.no_grad():
        layer.estimate_ranges()
        layer(x)
        layer.activation_quantizer.quantizer._delta.mul_(0.6)
    layer.learn_ranges() if learn else layer.fix_ranges()
    layer.activation_quantizer.quantizer.per_channel = per_channel
    return model.train(), layer, x, gy


def _grads(layer, x, gy):
    """-> {name: gradient} of x, the weight, the bias and the learnable range parameters (in their own shapes), + y"""
    x = x.clone().requires_grad_(True)
    layer.zero_grad()
    y = layer(x)
    y.backward(gy)
    q = layer.activation_quantizer.quantizer
    out = {'y': y.detach(), 'x': x.grad, 'weight': layer.weight.grad, 'bias': layer.bias.grad}
    if q._delta.requires_grad:
        assert q._delta.grad.shape == q._delta.shape and q._zero_float.grad.shape == q._zero_float.shape
        out['q_out'] = torch.stack([q._delta.grad.reshape(-1), q._zero_float.grad.reshape(-1)])
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize('learn', [False, True])
@pytest.mark.parametrize('gelu', [True, False])
def test_gradients_match_reference_and_layered_autograd(gelu, learn, switch):
    from quantization.fused import linear_act_quant_training
    from quantization.int8_route import QSpec
    _, layer, x, gy = _site(gelu, learn)
    switch(False)                                       # (a second pass of this body starts where the first one ended)
    off = _grads(layer, x, gy)
    with torch.no_grad():                               # off is today's line, bit for bit, and so is on under no_grad
        wq, bias = layer.get_params()
        assert torch.equal(off['y'], layer.quantize_activations(layer.run_forward(x, wq, bias)))
        switch(True)
        assert torch.equal(off['y'], layer(x))
        gemm = layer.run_forward(x, wq, None)
    switch(False)
    switch(True, 'FUSED_ACT_TRAINING')                  # the per-tensor switch alone: today's line as well
    assert linear_act_quant_training(layer, x.clone().requires_grad_(True)) is None
    alone = _grads(layer, x, gy)
    assert all(torch.equal(alone[k], off[k]) for k in off)
    switch(False, 'FUSED_ACT_TRAINING')
    switch(True)
    on = _grads(layer, x, gy)
    assert linear_act_quant_training(layer, x.clone().requires_grad_(True)) is not None         # the route is taken
    assert set(on) == set(off) and len(on) == (5 if learn else 4)
    c = lambda t: t.detach().cpu().reshape(-1, t.shape[-1])
    q = layer.activation_quantizer.quantizer
    spec = QSpec.of(q)._replace(delta=c(q._delta)[0], zero_float=c(q._zero_float)[0])
    ref = A._reference(c(gemm), c(bias)[0], c(gy), K.GELU if gelu else K.NONE, spec, c(on['y']), 1)
    g, B = ref['gemm']
    W, X = c(wq).double(), c(x).double()
    ref['x'] = (g @ W, B @ W.abs() + (W.shape[0] + 2) * K.U * (g.abs() @ W.abs()))
    ref['weight'] = (g.t() @ X, B.t() @ X.abs() + 44 * K.U * (g.abs().t() @ X.abs()))
    for k in set(on) - {'y'}:
        (val, bound), (a, b) = ref[k], (c(t).double().reshape(ref[k][0].shape) for t in (on[k], off[k]))
        assert bool(((a - b).abs() <= 2 * bound).all()), k
        assert bool(((a - val).abs() <= bound).all()), k


def test_graphed_step_equals_eager(switch):
    """a training step of the Linear + GELU model with the switch on: GraphedTrainStep == eager, bit for bit"""
    from quantization.data_parallel import GradientBuckets, train_step
    from quantization.graphs import GraphedTrainStep
    base, _, x, w = _site(True, True)
    loss_fn, out = (lambda y: (y * w).sum()), {}
    switch(True)
    for arm in ('eager', 'graphed'):
        model = copy.deepcopy(base)
        opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3)
        if arm == 'graphed':
            loss = GraphedTrainStep(model, loss_fn, opt, (x,), ())((x,), ()).clone()
        else:
            loss = train_step(model, loss_fn, opt, GradientBuckets(model.parameters()), (x,), ())
        out[arm] = [loss] + [p.detach().clone() for p in model.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(out['eager'], out['graphed']))


def test_whole_model_step_eager_and_graphed(switch, monkeypatch):
    """a 2-layer harness BERT (d = 384) under per_groups=6 with learnable ranges in training mode: one step with the switch on,
    eager == GraphedTrainStep bit for bit, loss == off's; Q, K and V of both layers take the route: at least 6 backward launches
    in the eager step (the dense Linears of the two tails carry per-column quantizers too and take it while the tail's own
    switch is off)"""
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
    bwd = cls.bias_act_quant_axis_bwd
    monkeypatch.setattr(cls, 'bias_act_quant_axis_bwd', lambda *a, **kw: calls.append(torch.cuda.is_current_stream_capturing()) or bwd(*a, **kw))
    _step_arms(base.train(), (ids,), (labels,), torch.nn.functional.cross_entropy, switch)
    assert calls.count(False) >= 6 and len(calls) >= 12
