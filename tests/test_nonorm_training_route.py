"""options.FUSED_NONORM_TRAINING: `fused.residual_layernorm_quant` on a NoNorm tail under autograd = the forward launch + the
one-launch backward, against the float64 reference of tests/test_nonorm_quant_bwd.py (K) within its bounds and against the
layered modules' autograd within TWICE those bounds (the layered side carries fp32 round-off of its own).  The gradients of x
and of dense's parameters are linear maps M of the GEMM output's gradient: their bound is |M| applied to K's bound plus
(n + 2) u |M| |ref| for the n-term fp32 dot products, as tests/test_ln_training_route.py (R) extends them.  dense.weight and the
NoNorm's weight / bias pass a weight quantizer's STE, which passes or zeroes an entry: where layered autograd has an exact 0
there the reference (of the fake-quantized tensor's gradient) does not apply."""
import copy

import pytest
import torch

from tests import test_ln_training_route as R
from tests import test_nonorm_quant_bwd as K

pytestmark = pytest.mark.gpu
D = R.D


@pytest.fixture
def switch():
    from quantization import options
    assert options.FUSED_NONORM_TRAINING is False
    yield lambda on: setattr(options, 'FUSED_NONORM_TRAINING', on)
    options.FUSED_NONORM_TRAINING = False


@pytest.mark.parametrize('learn', [False, True])
def test_gradients_match_reference_and_layered_autograd(learn, switch):
    from quantization.int8_route import QSpec
    blk, x, r, gy = R._block(learn, nonorm=True)
    off = R._grads(blk, x, r, gy)
    switch(True)
    on = R._grads(blk, x, r, gy)
    assert set(on) == set(off) and len(on) == (10 if learn else 7)
    with torch.no_grad():
        wq, bq = blk.dense.get_params()
        gemm = blk.dense.run_forward(x, wq, bq)
        nn_w, nn_b = blk.LayerNorm.quantized_params()
        blk.eval()
        assert torch.equal(on['y'], blk(x, r))                                  # the value is the fused forward's
    c = lambda t: t.detach().cpu().reshape(-1, t.shape[-1])
    ref, _ = K._reference(c(gemm), c(r), c(gy), c(nn_w)[0], c(nn_b)[0], [QSpec.of(q) for q in R._acts(blk)], 1)
    (g, B), W, X, n = ref['dense'], c(wq).double(), c(x).double(), K.U * (D + 2)
    ref['x'] = (g @ W, B @ W.abs() + n * (g.abs() @ W.abs()))
    ref['dense.weight'] = (g.t() @ X, B.t() @ X.abs() + 44 * K.U * (g.abs().t() @ X.abs()))
    ref['dense.bias'] = (g.sum(0), B.sum(0) + 44 * K.U * g.abs().sum(0))
    for name in set(on) - {'y'}:
        (val, bound), (a, b) = ref[name], (c(t).double().reshape(ref[name][0].shape) for t in (on[name], off[name]))
        ste = (b == 0) & (name in ('dense.weight', 'ln_weight', 'ln_bias'))
        if name in ('ln_weight', 'ln_bias'):            # (g s) / s of the NoNorm's weight quantizer: two more roundings
            bound = bound + 2 * K.U * val.abs()
        assert bool(((a - b).abs() <= 2 * bound).all()), name
        assert bool((ste | ((a - val).abs() <= bound)).all()), name


@pytest.mark.parametrize('decline', ['off', 'hook', 'save_target', 'estimating', 'per_column', 'd48', 'gemm'])
def test_declines_are_bit_equal_to_today(decline, switch):
    from quantization.fused import residual_layernorm_quant
    learn = decline not in ('estimating', 'per_column')                 # (those two: fixed ranges)
    blk, x, r, gy = R._block(learn, d=48 if decline == 'd48' else D, nonorm=True)
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
    if decline == 'gemm':                               # a pre-computed GEMM is the inference helpers' business: never this route
        blk.fix_ranges(), blk.eval()
        with torch.no_grad():
            gemm = blk.dense.run_forward(x, *blk.dense.get_params())
            off, on = (switch(on) or residual_layernorm_quant(blk.dense, blk.res_act_quantizer, blk.LayerNorm, x, r, _gemm=gemm)
                       for on in (False, True))
        assert torch.equal(off, on)
        return
    ref = R._grads(copy.deepcopy(blk), x, r, gy)        # today's: the option is off (copies: an estimating forward moves ranges)
    switch(decline != 'off')
    now = R._grads(copy.deepcopy(blk), x, r, gy)
    assert set(ref) == set(now) and all(torch.equal(ref[k], now[k]) for k in ref)


def test_whole_model_step_eager_and_graphed(switch, monkeypatch):
    """a 2-layer W4A4 harness MobileBERT with learnable ranges: one QAT step with the switch on, eager == GraphedTrainStep bit for
    bit, loss == off's; the six tails of a layer take the route: 2 x 6 backward launches in the eager step, as many under capture"""
    from harness.mobilebert import build_mobilebert
    from quantization import _hip
    from quantization.quantizers import QMethods
    from tests.test_softmax_training_route import _step_arms
    cls, calls = type(_hip.backend()), []
    bwd = cls.residual_nonorm_quant_bwd
    monkeypatch.setattr(cls, 'residual_nonorm_quant_bwd', lambda *a, **kw: calls.append(1) or bwd(*a, **kw))
    model, _ = build_mobilebert(seed=1000, num_layers=2, method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform,
                                n_bits=4, n_bits_act=4, quant_dict={'attn_probs_n_bits_act': 8})
    model = model.cuda()
    g = torch.Generator().manual_seed(0)
    ids, labels = torch.randint(1000, 30000, (2, 64), generator=g).cuda(), torch.randint(0, 2, (2,), generator=g).cuda()
    with torch.no_grad():
        model.set_quant_state(True, True)
        model.estimate_ranges()
        model(ids)
    model.learn_ranges()
    _step_arms(model.train(), (ids,), (labels,), torch.nn.functional.cross_entropy, switch)
    assert len(calls) >= 2 * 2 * 6 and len(calls) % 12 == 0
