"""BERT's head on the integer route (options.INT8_HEAD): pooler and classifier as skinny integer Linears, so that the LOGITS --
what a user reads -- are bit-equal between the GPU and the exact CPU twin, like every hidden state before them
(tests/test_bert_exact_route.py, whose models, calibration, inputs and twin this file imports).

CPU: the host logic against tests/_skinny_twin.SkinnyTwin -- which launches the head makes, with which operands, and when it
stays layered.  GPU: logits, pooled tensor and its int8 indices `torch.equal` to the twin's, eager and as a hipGraph replay, at
[3, 64] and [8, 128] with one padded sample, and under the W8A16 recipe (sites 'P' and 'C' stay 8-bit there); the default route
is unchanged by a process that switched the option on and off again."""
import copy

import pytest
import torch

from oracle import tq_oracle as O
from tests.test_bert_exact_route import _calibrate, _expected_census, _ids, _model, _twin_of

pytestmark = pytest.mark.default_route        # statements about the product's default route with one more switch on

SKINNY = 'linear_i8_skinny'


def _forward(model, be, ids, am=None):
    """one no-grad forward with backend `be` installed (None: the HIP backend) -> (logits, pooled, pooled indices,
    launches of `be`, integer Linears counted)"""
    from quantization import _hip, provenance
    from quantization.autoquant_utils import INT8_STATS
    seen = {}
    clf, fwd = model.classifier, type(model.classifier).forward

    def wrapped(x, *a, **k):                   # instance-level wrapper: a module hook would be an observer of the head
        seen['pooled'], seen['idx'] = x, provenance.indices_of(x)
        return fwd(clf, x, *a, **k)
    clf.forward = wrapped
    prev = _hip.set_backend(be) if be is not None else None
    try:
        if be is not None:
            del be.census[:]
        k0 = INT8_STATS['kernel_calls']
        with torch.no_grad():
            logits = model(ids) if am is None else model(ids, am)
        calls = INT8_STATS['kernel_calls'] - k0
    finally:
        del clf.forward
        if be is not None:
            _hip.set_backend(prev)
    cp = lambda t: None if t is None else t.detach().cpu().clone()
    return cp(logits), cp(seen['pooled']), cp(seen['idx']), [] if be is None else list(be.census), calls


# ---- CPU: host logic ------------------------------------------------------------------------------------------------------------
_CPU = {}


def _cpu_model(quant_setup):
    """2-layer BERT-base W8A8 calibrated on the CPU twin with the option off (the product default); built once per setup"""
    from quantization import _hip, options
    from quantization.base_quantized_classes import FP32Acts
    from tests._skinny_twin import SkinnyTwin
    if quant_setup not in _CPU:
        assert options.INT8_HEAD is False
        prev = _hip.set_backend(SkinnyTwin())
        try:
            model = _model('w8a8', 2, 'cpu')
            if quant_setup == 'FP_logits':
                model.classifier.activation_quantizer = FP32Acts()      # what QBertForSequenceClassification(quant_setup=...) does
            _CPU[quant_setup] = _calibrate(model, 'w8a8', [_ids(10, 2, 64)])
        finally:
            _hip.set_backend(prev)
    return copy.deepcopy(_CPU[quant_setup])


def _split(census):
    return [e for e in census if e[0] == SKINNY], [e for e in census if e[0] != SKINNY]


def test_head_takes_two_skinny_launches_cpu(monkeypatch):
    from quantization import options
    from tests._skinny_twin import SkinnyTwin
    B, T = 2, 64
    ids = _ids(3, B, T)
    _, _, _, census, calls = _forward(_cpu_model('all'), SkinnyTwin(), ids)
    assert _split(census) == ([], _expected_census('w8a8', 2, B, T)) and calls == 12
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    model = _cpu_model('all')
    logits, pooled, pooled_idx, census, calls = _forward(model, SkinnyTwin(), ids)
    skinny, encoder = _split(census)
    assert encoder == _expected_census('w8a8', 2, B, T)
    assert calls == 12 + 2
    # (name, M, N, K, activation, strides of x_idx, output quantizer?, want_y): Tanh on the first-token VIEW, then the classifier
    assert skinny == [(SKINNY, B, 768, 768, 3, (T * 768, 1), True, True), (SKINNY, B, 2, 768, 0, (768, 1), True, True)], skinny
    assert census[-2:] == skinny                                            # after the encoder, in this order
    q = model.classifier.activation_quantizer.quantizer
    i, y = O.fake_quant(logits, q._delta, q._zero_float, 8, False)
    assert torch.equal(y, logits), 'the logits do not lie on the classifier quantizer\'s grid'
    q = model.pooler[0].activation_quantizer.quantizer
    i, y = O.fake_quant(pooled, q._delta, q._zero_float, 8, False)
    assert torch.equal(y, pooled) and pooled_idx is not None and torch.equal(pooled_idx.float() + 128, i)


def test_fp_logits_classifier_has_no_output_quantizer_cpu(monkeypatch):
    from quantization import options
    from tests._skinny_twin import SkinnyTwin
    B, T = 2, 64
    model = _cpu_model('FP_logits')                           # (calibrated under the default, before the switch)
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    logits, _, _, census, calls = _forward(model, SkinnyTwin(), _ids(3, B, T))
    skinny, encoder = _split(census)
    assert encoder == _expected_census('w8a8', 2, B, T) and calls == 14
    assert skinny == [(SKINNY, B, 768, 768, 3, (T * 768, 1), True, True), (SKINNY, B, 2, 768, 0, (768, 1), False, True)], skinny
    assert torch.isfinite(logits).all()


@pytest.mark.parametrize('why', ['option off', 'hook on the pooler', 'pooler ranges not fixed', 'fuse_head = False'])
def test_head_stays_layered_cpu(why, monkeypatch):
    """no skinny launch, and the logits of the parent's route (the same model with the option off) bit for bit"""
    from quantization import options
    from tests._skinny_twin import SkinnyTwin
    B, T = 2, 64
    ids = _ids(3, B, T)

    def prepared():
        model = _cpu_model('all')
        if why == 'hook on the pooler':
            model.pooler.register_forward_hook(lambda m, a, o: None)
        if why == 'pooler ranges not fixed':
            model.pooler[0].activation_quantizer.estimate_ranges()
        if why == 'fuse_head = False':
            model.fuse_head = False
        return model
    want, _, _, census, calls = _forward(prepared(), SkinnyTwin(), ids)
    assert _split(census)[0] == [] and calls == 12
    if why != 'option off':
        monkeypatch.setattr(options, 'INT8_HEAD', True)
    got, _, _, census, calls = _forward(prepared(), SkinnyTwin(), ids)
    skinny, encoder = _split(census)
    assert skinny == [] and calls == 12 and encoder == _expected_census('w8a8', 2, B, T)
    assert torch.equal(got, want)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
_GPU = {}


def _gpu_model(recipe, B, T):
    if (recipe, B, T) not in _GPU:
        _GPU[(recipe, B, T)] = _calibrate(_model(recipe, 2, 'cuda'), recipe, [_ids(10, B, T).cuda(), _ids(11, B, T).cuda()])
    return _GPU[(recipe, B, T)]


def _mask(B, T):
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return am


def _head_case(recipe, B, T, monkeypatch, graph):
    from quantization import _hip, options
    from quantization.graphs import GraphedForward
    from tests._skinny_twin import SkinnyTwin
    assert options.INT8_LINEAR == 'auto' and options.INT8_HEAD is False
    model = _gpu_model(recipe, B, T)
    ids, am = _ids(3, B, T), _mask(B, T)
    before = _forward(model, None, ids.cuda(), am.cuda())[0]             # the default route, option never touched
    log = []
    orig = _hip.HipBackend.linear_i8_skinny

    def counted(self, *a, **k):
        log.append((SKINNY, a[0].shape[0], a[1].shape[0], a[0].shape[1], int(a[7]), tuple(a[0].stride()), a[8] is not None,
                    k.get('want_y', True)))
        return orig(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, 'linear_i8_skinny', counted)
    twin = _twin_of(model)
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    logits, pooled, pooled_idx, _, calls = _forward(model, None, ids.cuda(), am.cuda())
    torch.cuda.synchronize()
    t_logits, t_pooled, t_idx, t_census, t_calls = _forward(twin, SkinnyTwin(rules=_hip.backend()), ids, am)
    assert log == _split(t_census)[0] and len(log) == 2 and calls == t_calls == 12 + 2, (log, t_census[-2:], calls, t_calls)
    assert log[0][1:6] == (B, 768, 768, 3, (T * 768, 1)) and log[1][1:6] == (B, 2, 768, 0, (768, 1))
    assert pooled_idx is not None and torch.equal(pooled_idx, t_idx), 'pooled indices differ from the twin'
    assert torch.equal(pooled, t_pooled), 'pooled tensor differs from the twin'
    assert torch.equal(logits, t_logits), f'logits differ from the twin: {(logits - t_logits).abs().max()}'
    assert torch.isfinite(logits).all()
    if graph:
        with torch.no_grad():
            g = GraphedForward(model, ids.cuda(), am.cuda())
            replay = g(ids.cuda(), am.cuda())
            torch.cuda.synchronize()
            assert torch.equal(replay.cpu(), t_logits), 'hipGraph replay differs from the twin'
    monkeypatch.setattr(options, 'INT8_HEAD', False)
    n = len(log)
    after = _forward(model, None, ids.cuda(), am.cuda())[0]
    assert len(log) == n and torch.equal(after, before), 'the default route changed after the option was switched on and off'


@pytest.mark.gpu
@pytest.mark.parametrize('B,T', [(3, 64), (8, 128)])
def test_logits_equal_the_twin_w8a8(B, T, monkeypatch):
    _head_case('w8a8', B, T, monkeypatch, graph=True)


@pytest.mark.gpu
def test_logits_equal_the_twin_mixed_precision_recipe(monkeypatch):
    """{'x': 16, 'h': 16, 'y': 16}: the encoder's last LayerNorm (site z) and the head's sites 'P', 'C' stay 8-bit"""
    _head_case('mp16', 3, 64, monkeypatch, graph=False)
