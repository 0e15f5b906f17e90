"""options.FUSED_ACT_TRAINING: QuantLinear.forward under autograd = F.linear without bias + tq_bias_act_quant_fwd + the one-launch
backward, against the layered modules' autograd within TWICE the bounds of tests/test_act_quant_bwd.py (K): the layered side
carries fp32 round-off of its own, and torch's GELU in the place of the library's fit.  K's reference gives the bounds of the
GEMM output's gradient (B), the bias and the range parameters; x's and the weight's gradients are linear maps M of the first, so
their bound is |M| applied to B plus (n + 2) u |M| |ref| for the n-term fp32 dot products."""
import copy

import pytest
import torch
from torch import nn

from tests import test_act_quant_bwd as K

pytestmark = pytest.mark.gpu
SITES = {'gelu': (K.GELU, 256, K.RANGE), 'plain': (K.NONE, 64, (-1.0, 1.2))}      # act code, out_features, output range


@pytest.fixture
def switch():
    from quantization import options
    options.FUSED_ACT_TRAINING = False
    yield lambda on: setattr(options, 'FUSED_ACT_TRAINING', on)
    options.FUSED_ACT_TRAINING = False


def _site(name, learn, dev='cuda', act=None):
    """-> (model, its QuantLinear with the site's output range, x [2, 21, 64], grad_y); `act`: another activation module"""
    from quantization.autoquant_utils import quantize_model
    from quantization.quantizers import QMethods
    torch.manual_seed(0)
    _, n_out, (lo, hi) = SITES[name]
    fp = nn.Sequential(nn.Linear(64, n_out), act or nn.GELU()) if name == 'gelu' else nn.Linear(64, n_out)
    model = quantize_model(fp, method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8)
    layer = model[0] if name == 'gelu' else model
    layer.to(dev).quantized()
    x, _, gy = K._inputs(42, max(64, n_out), 4)
    x, gy = x[:, :64].reshape(2, 21, 64).to(dev), gy[:, :n_out].reshape(2, 21, n_out).to(dev)
    with torch.no_grad():
        layer.estimate_ranges()
        layer(x)
    layer.activation_quantizer.set_quant_range(torch.tensor(lo, device=dev), torch.tensor(hi, device=dev))
    layer.learn_ranges() if learn else layer.fix_ranges()
    return model.train(), layer, x, gy


def _grads(layer, x, gy):
    """-> {name: gradient} of x, the weight, the bias and the learnable range parameters of the output quantizer, + y"""
    x = x.clone().requires_grad_(True)
    layer.zero_grad()
    y = layer(x)
    y.backward(gy)
    q = layer.activation_quantizer.quantizer
    out = {'y': y.detach(), 'x': x.grad, 'weight': layer.weight.grad, 'bias': layer.bias.grad}
    if q._delta.requires_grad:
        out['q_out'] = torch.stack([q._delta.grad.reshape(()), q._zero_float.grad.reshape(())])
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize('learn', [False, True])
@pytest.mark.parametrize('name', sorted(SITES))
def test_gradients_match_layered_autograd(name, learn, switch):
    from quantization.fused import linear_act_quant_training
    from quantization.int8_route import QSpec
    _, layer, x, gy = _site(name, learn)
    off = _grads(layer, x, gy)
    with torch.no_grad():                               # off is today's line, bit for bit, and so is on under no_grad
        wq, bias = layer.get_params()
        assert torch.equal(off['y'], layer.quantize_activations(layer.run_forward(x, wq, bias)))
        switch(True)
        assert torch.equal(off['y'], layer(x))
        gemm = layer.run_forward(x, wq, None)
    on = _grads(layer, x, gy)
    assert linear_act_quant_training(layer, x.clone().requires_grad_(True)) is not None         # the route is taken
    assert set(on) == set(off) and len(on) == (5 if learn else 4)
    c = lambda t: t.detach().cpu().reshape(-1, t.shape[-1])
    ref = K._reference(c(gemm), c(bias)[0], c(gy), SITES[name][0], QSpec.of(layer.activation_quantizer.quantizer), c(on['y']), 1)
    g, B = ref['gemm']
    W, X = c(wq).double(), c(x).double()
    ref['x'] = (g @ W, B @ W.abs() + (W.shape[0] + 2) * K.U * (g.abs() @ W.abs()))
    ref['weight'] = (g.t() @ X, B.t() @ X.abs() + 44 * K.U * (g.abs().t() @ X.abs()))
    for k in set(on) - {'y'}:
        a, b = (c(t).double().reshape(ref[k][0].shape) for t in (on[k], off[k]))
        assert bool(((a - b).abs() <= 2 * ref[k][1]).all()), k


def test_graphed_step_equals_eager(switch):
    """a training step of the Linear + GELU model with the switch on: GraphedTrainStep == eager, bit for bit"""
    from quantization.data_parallel import GradientBuckets, train_step
    from quantization.graphs import GraphedTrainStep
    base, _, x, w = _site('gelu', True)
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
