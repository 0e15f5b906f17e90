"""options.FUSED_LN_TRAINING: `fused.residual_layernorm_quant` under autograd = the forward launch + the one-launch backward,
against the float64 reference of tests/test_ln_quant_bwd.py (K) within its bounds and against the layered modules' autograd
within TWICE those bounds (the layered side carries fp32 round-off of its own).  The reference gives the gradients of the GEMM
output, the residual, the fake-quantized affine and the six range parameters; the gradients of x and of dense's parameters
are linear maps M of the GEMM output's gradient, so their bound is |M| applied to K's bound B plus (n + 2) u |M| |ref| for
the n-term fp32 dot products.  dense.weight alone passes a weight quantizer's STE, which passes or zeroes an entry: where
layered autograd has an exact 0 there the reference (of the fake-quantized weight's gradient) does not apply."""
import copy

import pytest
import torch

from tests import test_ln_quant_bwd as K

pytestmark = pytest.mark.gpu
D = 128


@pytest.fixture
def switch():
    from quantization import options
    options.FUSED_LN_TRAINING = False
    yield lambda on: setattr(options, 'FUSED_LN_TRAINING', on)
    options.FUSED_LN_TRAINING = False


def _block(learn, d=D, dev='cuda', nonorm=False):
    """a harness tail block (dense d -> d; `nonorm`: MobileBERT's element-wise affine in the LayerNorm's place) with K's ranges
    on its three activation quantizers, x, residual, grad_y"""
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertSelfOutput
    from harness.bert import QResidualBlock
    from quantization.autoquant_utils import QuantNoNorm
    from quantization.quantizers import QMethods
    torch.manual_seed(0)
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8)
    hf = BertSelfOutput(BertConfig(hidden_size=d, hidden_dropout_prob=0.0)).eval()
    blk = QResidualBlock(hf, **qp)
    if nonorm:
        blk.LayerNorm = QuantNoNorm(hf.LayerNorm, **qp)
    blk.to(dev).set_quant_state(True, True)
    x, r, gy = (t.to(dev).view(2, 21, d) for t in K._inputs(2 * 21, d, 4)[:3])
    with torch.no_grad():
        blk.estimate_ranges()
        blk(x, r)
    for m, (lo, hi) in zip((blk.dense, blk.res_act_quantizer, blk.LayerNorm), K.RANGES):
        m.activation_quantizer.set_quant_range(torch.tensor(lo, device=dev), torch.tensor(hi, device=dev))
    blk.learn_ranges() if learn else blk.fix_ranges()
    return blk.train(), x, r, gy


_acts = lambda blk: [m.activation_quantizer.quantizer for m in (blk.dense, blk.res_act_quantizer, blk.LayerNorm)]


def _grads(blk, x, r, gy):
    """-> {name: gradient} of x, residual, dense's and the LayerNorm's weight / bias and the learnable range parameters, + y"""
    from quantization.fused import residual_layernorm_quant
    x, r = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    blk.zero_grad()
    y = residual_layernorm_quant(blk.dense, blk.res_act_quantizer, blk.LayerNorm, x, r)
    y.backward(gy)
    out = {'y': y.detach(), 'x': x.grad, 'residual': r.grad, 'dense.weight': blk.dense.weight.grad, 'dense.bias': blk.dense.bias.grad,
           'ln_weight': blk.LayerNorm.weight.grad, 'ln_bias': blk.LayerNorm.bias.grad}
    for name, q in zip(('q_dense', 'q_sum', 'q_out'), _acts(blk)):
        if q._delta.requires_grad:
            out[name] = torch.stack([q._delta.grad.reshape(()), q._zero_float.grad.reshape(())])
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize('learn', [False, True])
def test_gradients_match_reference_and_layered_autograd(learn, switch):
    from quantization.int8_route import QSpec
    blk, x, r, gy = _block(learn)
    off = _grads(blk, x, r, gy)
    switch(True)
    on = _grads(blk, x, r, gy)
    assert set(on) == set(off) and len(on) == (10 if learn else 7)
    with torch.no_grad():
        wq, bq = blk.dense.get_params()
        gemm = blk.dense.run_forward(x, wq, bq)
        ln_w, ln_b = blk.LayerNorm.get_params()
        blk.eval()
        assert torch.equal(on['y'], blk(x, r))                                  # the value is the fused forward's
    c = lambda t: t.detach().cpu().reshape(-1, t.shape[-1])
    ref = K._reference(c(gemm), c(r), c(gy), c(ln_w)[0], c(ln_b)[0], [QSpec.of(q) for q in _acts(blk)], c(on['y']), 1)
    g, B = ref['dense']
    W, X, n = c(wq).double(), c(x).double(), K.U * (D + 2)
    ref['x'] = (g @ W, B @ W.abs() + n * (g.abs() @ W.abs()))
    ref['dense.weight'] = (g.t() @ X, B.t() @ X.abs() + 44 * K.U * (g.abs().t() @ X.abs()))
    ref['dense.bias'] = (g.sum(0), B.sum(0) + 44 * K.U * g.abs().sum(0))
    for name in set(on) - {'y'}:
        (val, bound), (a, b) = ref[name], (c(t).double().reshape(ref[name][0].shape) for t in (on[name], off[name]))
        assert bool(((a - b).abs() <= 2 * bound).all()), name
        assert bool((((b == 0) & (name == 'dense.weight')) | ((a - val).abs() <= bound)).all()), name


@pytest.mark.parametrize('decline', ['off', 'hook', 'save_target', 'estimating', 'd48', 'per_column', 'nonorm', 'bfloat16', 'float16', 'gemm'])
def test_declines_are_bit_equal_to_today(decline, switch):
    from quantization.fused import residual_layernorm_quant
    learn = decline not in ('estimating', 'per_column')                 # (those two: fixed ranges)
    blk, x, r, gy = _block(learn, d=48 if decline == 'd48' else D, nonorm=decline == 'nonorm')
    if decline == 'per_column':                         # one (equal) parameter per column, as a per-embedding quantizer holds them
        q = blk.res_act_quantizer.activation_quantizer.quantizer
        q._delta, q._zero_float = q._delta.expand(D).clone(), q._zero_float.expand(D).clone()
    if decline == 'hook':
        blk.res_act_quantizer.activation_quantizer.register_forward_hook(lambda *a: None)
    if decline == 'save_target':
        blk.dense.activation_save_target = {}
        blk.dense.activation_save_name = 'site'
    if decline == 'estimating':
        blk.res_act_quantizer.estimate_ranges_train()
    if decline in ('bfloat16', 'float16'):
        # 16-bit storage: the route's own answer (None falls straight into the unchanged line), because the layered 16-bit line
        # is not reproducible on the GPU whatever the option says: repeated runs in one process differed in the forward's y
        # already (and in ln_bias and range gradients), so not through a GEMM backward.  Cause not found
        from quantization.fused import _ln_training_tail
        dt = getattr(torch, decline)
        switch(True)
        assert _ln_training_tail(blk.dense, blk.res_act_quantizer, blk.LayerNorm, x.requires_grad_(True), r) is not None
        x16 = x.detach().to(dt).requires_grad_(True)
        assert _ln_training_tail(blk.to(dt).dense, blk.res_act_quantizer, blk.LayerNorm, x16, r.to(dt)) is None
        return
    if decline == 'gemm':                               # a pre-computed GEMM is the inference helpers' business: never this route
        blk.fix_ranges(), blk.eval()
        with torch.no_grad():
            gemm = blk.dense.run_forward(x, *blk.dense.get_params())
            off, on = (switch(on) or residual_layernorm_quant(blk.dense, blk.res_act_quantizer, blk.LayerNorm, x, r, _gemm=gemm)
                       for on in (False, True))
        assert torch.equal(off, on)
        return
    ref = _grads(copy.deepcopy(blk), x, r, gy)          # today's: the option is off (copies: an estimating forward moves ranges)
    switch(decline != 'off')
    now = _grads(copy.deepcopy(blk), x, r, gy)
    assert set(ref) == set(now) and all(torch.equal(ref[k], now[k]) for k in ref)


def test_whole_model_step_eager_and_graphed(switch, monkeypatch):
    """the softmax route's 2-layer harness BERT step with THIS switch: on eager == GraphedTrainStep bit for bit, loss == off's;
    and the harness tails take the route: 2 layers x 2 backward launches in the eager step, at least as many under capture"""
    from quantization import _hip
    from tests.test_softmax_training_route import test_whole_model_step_eager_and_graphed as step_arms
    cls, calls = type(_hip.backend()), []
    bwd = cls.residual_layernorm_quant_bwd
    monkeypatch.setattr(cls, 'residual_layernorm_quant_bwd', lambda *a, **kw: calls.append(1) or bwd(*a, **kw))
    step_arms(switch)
    assert len(calls) >= 8
