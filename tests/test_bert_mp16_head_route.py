"""BERT's head on the integer route under the mixed-precision recipes (options.INT8_HEAD with sites 'P' and / or 'C' at 16 bits):
the STS-B recipe {'x': 16, 'h': 16, 'y': 16, 'P': 16, 'C': 16} puts the pooler's output -- the classifier's input -- and the
logits on 16-bit grids.  The pooler then runs on tq_linear_i16x8_skinny_fwd (8-bit input read in place, Tanh, y and both byte
planes of its 16-bit indices out) and the classifier on the same entry from those planes, with no tq_quantize_hilo_fwd launch
between the two; the logits are bit-equal between the GPU and the exact CPU twin.

CPU: the host logic against tests/_skinny16_twin.Skinny16Twin -- which launches the head makes, with which operands, and when it
stays layered.  GPU: logits and pooled tensor `torch.equal` to the twin's, eager and as a hipGraph replay, at [3, 64] and
[8, 128] with one padded sample; the default route is unchanged by a process that switched the option on and off again."""
import copy

import pytest
import torch

from oracle import tq_oracle as O
from tests.test_bert_exact_route import _calibrate, _expected_census, _ids, _twin_of

pytestmark = pytest.mark.default_route        # statements about the product's default route with one more switch on

OLD, NEW = 'linear_i8_skinny', 'linear_i16x8_skinny'
ENCODER = {'x': 16, 'h': 16, 'y': 16}
RECIPES = {
    'sts-b': dict(ENCODER, P=16, C=16),
    'P alone': dict(ENCODER, P=16),
    'C alone': dict(ENCODER, C=16),
    'w8a8': {},
}
ACT_NONE, ACT_TANH = 0, 3


def _model(recipe, device, quant_setup='all'):
    from quantization.base_quantized_classes import FP32Acts
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=2, **qp)
    apply_quant_dict(model, RECIPES[recipe])
    if quant_setup == 'FP_logits':
        model.classifier.activation_quantizer = FP32Acts()      # what QBertForSequenceClassification(quant_setup=...) does
    return model.to(device).eval()


def _forward(model, be, ids, am=None):
    """one no-grad forward with backend `be` installed (None: the HIP backend) -> (logits, pooled, planes the pooled tensor
    carries, launches of `be`, integer Linears counted)"""
    from quantization import _hip, provenance
    from quantization.autoquant_utils import INT8_STATS
    seen = {}
    clf, fwd = model.classifier, type(model.classifier).forward

    def wrapped(x, *a, **k):                   # instance-level wrapper: a module hook would be an observer of the head
        seen['pooled'], seen['planes'], seen['idx'] = x, provenance.planes_of(x), provenance.indices_of(x)
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
    planes = None if seen['planes'] is None else tuple(cp(t) for t in seen['planes'])
    assert seen['idx'] is None or planes is None
    return cp(logits), cp(seen['pooled']), planes, [] if be is None else list(be.census), calls


def _split(census):
    return [e for e in census if e[0] in (OLD, NEW)], [e for e in census if e[0] not in (OLD, NEW)]


def _enc(recipe, B, T):
    return _expected_census('w8a8' if recipe == 'w8a8' else 'mp16', 2, B, T)


def _new(M, N, K, act, strides, planes_in, q_out, form):
    """a census entry of Skinny16Twin / of the counted HIP method (no row table, y wanted)"""
    return (NEW, M, N, K, act, strides, planes_in, False, q_out, form, True)


def _head(recipe, B, T, fp_logits=False):
    """the head's launches per recipe, in call order"""
    first = (T * 768, 1)
    q = not fp_logits
    return {
        'sts-b': [_new(B, 768, 768, ACT_TANH, first, False, True, 'planes'), _new(B, 2, 768, ACT_NONE, (768, 1), True, q, 'y')],
        'P alone': [_new(B, 768, 768, ACT_TANH, first, False, True, 'planes'),
                    _new(B, 2, 768, ACT_NONE, (768, 1), True, q, 'idx' if q else 'y')],
        'C alone': [(OLD, B, 768, 768, ACT_TANH, first, True, True), (OLD, B, 2, 768, ACT_NONE, (768, 1), q, True)],
        'w8a8': [(OLD, B, 768, 768, ACT_TANH, first, True, True), (OLD, B, 2, 768, ACT_NONE, (768, 1), q, True)],
    }[recipe]


# ---- CPU: host logic ------------------------------------------------------------------------------------------------------------
_CPU = {}


def _cpu_model(recipe, quant_setup='all'):
    """calibrated on the CPU twin with the option off (the product default); built once per recipe and setup"""
    from quantization import _hip, options
    from tests._skinny16_twin import Skinny16Twin
    if (recipe, quant_setup) not in _CPU:
        assert options.INT8_HEAD is False
        prev = _hip.set_backend(Skinny16Twin())
        try:
            _CPU[(recipe, quant_setup)] = _calibrate(_model(recipe, 'cpu', quant_setup), 'mp16', [_ids(10, 2, 64)])
        finally:
            _hip.set_backend(prev)
    return copy.deepcopy(_CPU[(recipe, quant_setup)])


def _on_grid(t, q, n_bits):
    i, y = O.fake_quant(t, q._delta, q._zero_float, n_bits, False)
    return torch.equal(y, t), i


def test_sts_b_head_takes_two_launches_of_the_new_entry_cpu(monkeypatch):
    from quantization import options
    from tests._skinny16_twin import Skinny16Twin, index_of
    B, T = 2, 64
    ids = _ids(3, B, T)
    off_logits, _, planes, census, calls = _forward(_cpu_model('sts-b'), Skinny16Twin(), ids)
    assert _split(census) == ([], _enc('sts-b', B, T)) and planes is None         # option off: the layered head
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    model = _cpu_model('sts-b')
    logits, pooled, planes, census, calls_on = _forward(model, Skinny16Twin(), ids)
    skinny, encoder = _split(census)
    assert encoder == _enc('sts-b', B, T), 'the encoder census moved with the option'
    assert calls_on == calls + 2
    assert skinny == _head('sts-b', B, T), skinny
    assert census[-2:] == skinny                                    # after the encoder: no quantize_hilo between or behind
    assert [e[0] for e in census].count('quantize_hilo') == 2       # the encoder's, one per layer
    ok, i = _on_grid(logits, model.classifier.activation_quantizer.quantizer, 16)
    assert ok, 'the logits do not lie on the classifier quantizer\'s 16-bit grid'
    ok, i = _on_grid(pooled, model.pooler[0].activation_quantizer.quantizer, 16)
    assert ok and planes is not None and torch.equal(torch.from_numpy(index_of(*planes)).float(), i)
    assert i.max() > 255                                            # a 16-bit index: no int8 tensor holds it
    assert torch.isfinite(logits).all() and torch.isfinite(off_logits).all()


@pytest.mark.parametrize('recipe,quant_setup', [('P alone', 'all'), ('C alone', 'all'), ('sts-b', 'FP_logits'),
                                                ('P alone', 'FP_logits'), ('w8a8', 'all')])
def test_the_other_mixes_cpu(recipe, quant_setup, monkeypatch):
    """'P' alone: planes out of the pooler, the classifier reads them and emits int8 indices; 'C' alone and the 8-bit recipe:
    the old entry twice (a 16-bit q_out needs no planes: nobody reads them); FP_logits: no output quantizer"""
    from quantization import options
    from tests._skinny16_twin import Skinny16Twin
    B, T = 2, 64
    model = _cpu_model(recipe, quant_setup)
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    logits, pooled, planes, census, calls = _forward(model, Skinny16Twin(), _ids(3, B, T))
    skinny, encoder = _split(census)
    assert encoder == _enc(recipe, B, T)
    assert skinny == _head(recipe, B, T, fp_logits=quant_setup == 'FP_logits'), skinny
    assert (planes is not None) == (recipe != 'C alone' and recipe != 'w8a8')
    assert torch.isfinite(logits).all()
    if quant_setup == 'all':
        assert _on_grid(logits, model.classifier.activation_quantizer.quantizer, 16 if recipe == 'C alone' else 8)[0]


@pytest.mark.parametrize('why', ['hook on the pooler', 'pooler ranges not fixed', 'fuse_head = False'])
def test_head_stays_layered_cpu(why, monkeypatch):
    """no skinny launch, and the logits of the same model with the option off bit for bit"""
    from quantization import options
    from tests._skinny16_twin import Skinny16Twin
    B, T = 2, 64
    ids = _ids(3, B, T)

    def prepared():
        model = _cpu_model('sts-b')
        if why == 'hook on the pooler':
            model.pooler.register_forward_hook(lambda m, a, o: None)
        if why == 'pooler ranges not fixed':
            model.pooler[0].activation_quantizer.estimate_ranges()
        if why == 'fuse_head = False':
            model.fuse_head = False
        return model
    want, _, _, census, calls = _forward(prepared(), Skinny16Twin(), ids)
    assert _split(census)[0] == []
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    got, _, planes, census, calls_on = _forward(prepared(), Skinny16Twin(), ids)
    skinny, encoder = _split(census)
    assert skinny == [] and calls_on == calls and encoder == _enc('sts-b', B, T) and planes is None
    assert torch.equal(got, want)


def test_a_wide_classifier_input_without_planes_stays_layered_cpu(monkeypatch):
    """the pooler through the old entry (a backend without the new method: the parent's route): its 16-bit output carries no
    planes, and the classifier is the layered fp32 GEMM"""
    from quantization import options
    from tests._skinny_twin import SkinnyTwin
    B, T = 2, 64
    model = _cpu_model('sts-b')
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    _, _, planes, census, _ = _forward(model, SkinnyTwin(), _ids(3, B, T))
    assert _split(census)[0] == [(OLD, B, 768, 768, ACT_TANH, (T * 768, 1), True, True)] and planes is None


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
_GPU = {}


def _gpu_model(B, T):
    if (B, T) not in _GPU:
        _GPU[(B, T)] = _calibrate(_model('sts-b', 'cuda'), 'mp16', [_ids(10, B, T).cuda(), _ids(11, B, T).cuda()])
    return _GPU[(B, T)]


def _mask(B, T):
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return am


@pytest.mark.gpu
@pytest.mark.parametrize('B,T', [(3, 64), (8, 128)])
def test_logits_equal_the_twin_sts_b(B, T, monkeypatch):
    from quantization import _hip, options
    from quantization.graphs import GraphedForward
    from tests._skinny16_twin import Skinny16Twin, count_hip_launches
    assert options.INT8_LINEAR == 'auto' and options.INT8_HEAD is False
    model = _gpu_model(B, T)
    ids, am = _ids(3, B, T), _mask(B, T)
    before = _forward(model, None, ids.cuda(), am.cuda())[0]             # the default route, option never touched
    log = count_hip_launches(monkeypatch)
    twin = _twin_of(model)
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    logits, pooled, planes, _, calls = _forward(model, None, ids.cuda(), am.cuda())
    torch.cuda.synchronize()
    t_logits, t_pooled, t_planes, t_census, t_calls = _forward(twin, Skinny16Twin(rules=_hip.backend()), ids, am)
    assert log == _split(t_census)[0] == _head('sts-b', B, T) and calls == t_calls, (log, t_census[-2:], calls, t_calls)
    assert planes is not None and all(torch.equal(a, b) for a, b in zip(planes, t_planes)), 'pooled planes differ from the twin'
    assert torch.equal(pooled, t_pooled), 'pooled tensor differs from the twin'
    assert torch.equal(logits, t_logits), f'logits differ from the twin: {(logits - t_logits).abs().max()}'
    assert torch.isfinite(logits).all()
    with torch.no_grad():
        g = GraphedForward(model, ids.cuda(), am.cuda())
        replay = g(ids.cuda(), am.cuda())
        torch.cuda.synchronize()
        assert torch.equal(replay.cpu(), t_logits), 'hipGraph replay differs from the twin'
    monkeypatch.setattr(options, 'INT8_HEAD', False)
    n = len(log)
    after = _forward(model, None, ids.cuda(), am.cuda())[0]
    assert len(log) == n and torch.equal(after, before), 'the default route changed after the option was switched on and off'
