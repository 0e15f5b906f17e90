"""BERT on the integer route at ANY sequence length (options.INT8_RAGGED): the ragged attention core plus row tails for the
tiled integer Linears, so that a batch padded only to its longest sequence keeps the launches -- and the bit-for-bit GPU == CPU
statement -- of tests/test_bert_exact_route.py, whose models, calibration, capture, census and comparison this file imports.

CPU (tests/_ragged_twin.RaggedTwin): which launches the route makes at [3,50] with the option on and off, and that [3,64] does
not notice the option.  GPU: embedding output and, after every layer, both hidden states with their int8 indices `torch.equal`
to the twin's at [3,50], [2,37] and [8,72] with padded samples, eager and as a hipGraph replay; and, without any twin, the
[3,50] forward equals on [:, :50] the existing route's forward of the same batch padded by the caller to [3,64]."""
import copy

import pytest
import torch

from tests.test_bert_exact_route import (_Capture, _calibrate, _compare, _expected_census, _hip_census, _host, _ids, _model,
                                         _twin_chained, _twin_of)

pytestmark = pytest.mark.default_route        # statements about the product's default route with one more switch on

RAGGED = 'attention_i8_ragged'


def _mask(B, T):
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return am


def _ragged_census(layers, B, T, stair=True):
    """the default route's launches with the ragged core in place of the whole-tile one"""
    return [((RAGGED,) + e[1:]) if e[0] == 'attention_i8' else e for e in _expected_census('w8a8', layers, B, T, stair=stair)]


# ---- CPU: host logic ------------------------------------------------------------------------------------------------------------
_CPU = []


def _cpu_model():
    """2-layer BERT-base W8A8 calibrated on the CPU twin with the option off (the product default); built once"""
    from quantization import _hip, options
    from tests._ragged_twin import RaggedTwin
    if not _CPU:
        assert options.INT8_RAGGED is False
        prev = _hip.set_backend(RaggedTwin())
        try:
            _CPU.append(_calibrate(_model('w8a8', 2, 'cpu'), 'w8a8', [_ids(10, 2, 64)]))
        finally:
            _hip.set_backend(prev)
    return copy.deepcopy(_CPU[0])


def _encoder_launches(census):
    return [e for e in census if e[0].startswith(('linear_i8', 'attention_i8'))]


def test_option_on_puts_the_whole_encoder_on_the_integer_entry_points_cpu(monkeypatch):
    from quantization import options
    from quantization.autoquant_utils import INT8_STATS
    from tests._ragged_twin import RaggedTwin
    B, T = 3, 50
    model = _cpu_model()                                      # (calibrated under the default, before the switch)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    fb0 = INT8_STATS['unsigned_weight_fallbacks']
    rec, calls, census, _ = _twin_chained(model, RaggedTwin(), _ids(3, B, T), _mask(B, T))
    assert census == _ragged_census(2, B, T), census
    assert calls == 2 * 6 and INT8_STATS['unsigned_weight_fallbacks'] == fb0     # Q, K, V, attention output, FFN1, FFN2: none layered
    assert all(i is not None and torch.isfinite(h).all() for h, i in rec['h'] + rec['attn'] + rec['emb'])
    assert rec['h'][-1][0].shape == (B, T, 768)


def test_option_off_keeps_the_parents_launches_cpu(monkeypatch):
    """off (the default): what a backend without the capability gives with the option on -- the parent's route: embedding
    block and tails fused (they take any row count), every encoder Linear and the attention core layered"""
    from quantization import options
    from tests._exact_backend import ExactBackend
    from tests._ragged_twin import RaggedTwin
    B, T = 3, 50
    ids, am = _ids(3, B, T), _mask(B, T)
    assert options.INT8_RAGGED is False
    off, calls_off, census_off, _ = _twin_chained(_cpu_model(), RaggedTwin(), ids, am)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    assert not hasattr(ExactBackend, RAGGED) and not getattr(ExactBackend, 'PADS_ROWS', False)
    parent, calls_parent, census_parent, _ = _twin_chained(_cpu_model(), ExactBackend(), ids, am)
    assert census_off == census_parent and calls_off == calls_parent == 0
    assert _encoder_launches(census_off) == []
    assert [e[0] for e in census_off] == ['embeddings_layernorm_quant'] + ['residual_layernorm_quant'] * 4
    assert torch.equal(off['h'][-1][0], parent['h'][-1][0])


def test_whole_tile_shapes_do_not_notice_the_option_cpu(monkeypatch):
    from quantization import options
    from tests._ragged_twin import RaggedTwin
    B, T = 3, 64
    ids, am = _ids(3, B, T), _mask(B, T)
    off, calls_off, census_off, _ = _twin_chained(_cpu_model(), RaggedTwin(), ids, am)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    on, calls_on, census_on, _ = _twin_chained(_cpu_model(), RaggedTwin(), ids, am)
    assert census_on == census_off == _expected_census('w8a8', 2, B, T) and calls_on == calls_off == 12
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(on['h'], off['h']))


def test_ragged_forward_equals_the_callers_padding_cpu(monkeypatch):
    """the twin's [3,50] forward equals, on [:, :50], the existing route on the batch padded by the caller to [3,64] with
    attention_mask = 0 on the pads (HF's -10000 there: the pad keys' exponentials are exactly 0 as well)"""
    from quantization import options
    from tests._ragged_twin import RaggedTwin
    B, T = 3, 50
    ids, am = _ids(3, B, T), _mask(B, T)
    ids_p = torch.cat([ids, torch.full((B, 14), 1000)], 1)
    am_p = torch.cat([am, torch.zeros(B, 14, dtype=torch.long)], 1)
    padded, _, census, _ = _twin_chained(_cpu_model(), RaggedTwin(), ids_p, am_p)
    assert census == _expected_census('w8a8', 2, B, 64)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    ragged, _, _, _ = _twin_chained(_cpu_model(), RaggedTwin(), ids, am)
    for where in ('emb', 'attn', 'h'):
        for l, (r, p) in enumerate(zip(ragged[where], padded[where])):
            assert torch.equal(r[0], p[0][:, :T]) and torch.equal(r[1], p[1][:, :T]), f'{where} {l}'


def test_skinny_plan_keeps_precedence_where_both_options_apply_cpu(monkeypatch):
    """INT8_HEAD and INT8_RAGGED both on: a Linear that asks for both at a ragged M <= 256 keeps the skinny plan it has under
    INT8_HEAD alone (one definition of its Tanh / GELU); without INT8_HEAD the same call gets the padded tiled plan"""
    from quantization import _hip, options
    from quantization.autoquant_utils import SKINNY
    from quantization.int8_route import TILED
    from tests._ragged_twin import RaggedTwin
    from tests._skinny_twin import SkinnyTwin

    class Both(RaggedTwin, SkinnyTwin):
        pass
    model = _cpu_model()
    dense = model.layers[0].attention_output.dense
    src = model.embeddings.LayerNorm.activation_quantizer.quantizer
    prev = _hip.set_backend(Both())
    try:
        with torch.no_grad():
            assert dense._int8_plan_from(src, 50, skinny=True, ragged=True) is None          # both off: no tile, no plan
            monkeypatch.setattr(options, 'INT8_RAGGED', True)
            plan = dense._int8_plan_from(src, 50, skinny=True, ragged=True)
            assert plan is not None and plan.kind is TILED and plan.layout is None           # padded tiled launch
            assert dense._int8_plan_from(src, 50, skinny=True) is None                       # ... only for callers that ask
            monkeypatch.setattr(options, 'INT8_HEAD', True)
            plan = dense._int8_plan_from(src, 50, skinny=True, ragged=True)
            assert plan.kind is SKINNY and plan.layout is None
            plan = dense._int8_plan_from(src, 300, skinny=True, ragged=True)                 # more rows than the skinny kernel takes
            assert plan is not None and plan.kind is TILED and plan.layout is None
    finally:
        _hip.set_backend(prev)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
LAYERS = 3
_GPU = []


def _gpu_model():
    """3 layers of BERT-base W8A8, calibrated once on the default route at a whole-tile shape"""
    from quantization import options
    if not _GPU:
        assert options.INT8_RAGGED is False
        _GPU.append(_calibrate(_model('w8a8', LAYERS, 'cuda'), 'w8a8', [_ids(10, 4, 64).cuda(), _ids(11, 4, 64).cuda()]))
    return _GPU[0]


def _census_with_ragged(monkeypatch):
    from quantization import _hip
    log = _hip_census(monkeypatch)
    orig = _hip.HipBackend.attention_i8_ragged

    def counted(self, *a, **k):
        log.append((RAGGED, tuple(a[0].shape)))
        return orig(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, RAGGED, counted)
    return log


@pytest.mark.gpu
@pytest.mark.parametrize('B,T', [(3, 50), (2, 37), (8, 72)])
def test_ragged_route_equals_the_twin(B, T, monkeypatch):
    from quantization import _hip, options
    from quantization.autoquant_utils import INT8_STATS
    from quantization.graphs import GraphedForward
    from tests._ragged_twin import RaggedTwin
    assert options.INT8_LINEAR == 'auto'
    model = _gpu_model()
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    ids, am = _ids(3, B, T), _mask(B, T)
    args = (ids.cuda(), am.cuda())
    twin = _twin_of(model)
    log = _census_with_ragged(monkeypatch)
    with torch.no_grad(), _Capture(model) as cap:
        k0, fb0 = INT8_STATS['kernel_calls'], INT8_STATS['unsigned_weight_fallbacks']
        model(*args)
        torch.cuda.synchronize()
        calls = INT8_STATS['kernel_calls'] - k0
        assert INT8_STATS['unsigned_weight_fallbacks'] == fb0
        census = list(log)
        gpu = _host(cap.runs[-1])
        g = GraphedForward(model, *args)
        static = cap.runs[-1]                                   # the capture pass: the graph's own tensors
        g(*args)
        torch.cuda.synchronize()
        replay = _host(static)
    be = RaggedTwin(rules=_hip.backend())
    chained, twin_calls, twin_census, seconds = _twin_chained(twin, be, ids, am)
    print(f'[{B},{T}] {len(census)} launches ({calls} integer Linears), twin forward {seconds:.1f} s on the CPU')
    assert calls == twin_calls == LAYERS * 6, (calls, twin_calls)
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    stair = [e[-1] for e in census if e[0] == 'linear_i8' and e[2] == 3072]
    assert len(stair) == LAYERS and len(set(stair)) == 1 and census == _ragged_census(LAYERS, B, T, stair=stair[0])
    for where in ('emb', 'attn', 'h'):
        for l, (r, e) in enumerate(zip(replay[where], gpu[where])):
            assert torch.equal(r[0], e[0]) and r[1] is not None and e[1] is not None and torch.equal(r[1], e[1]), \
                f'hipGraph replay differs from the eager forward: {where} {l}'
    for name, rec in (('eager', gpu), ('replay', replay)):
        out = _compare(f'ragged {name} [{B},{T}]', model, twin, be, rec, chained, am, LAYERS)
        assert all(torch.isfinite(h).all() for h, _ in rec['h'])
        print(name, out)


@pytest.mark.gpu
def test_ragged_route_equals_the_existing_route_on_the_callers_padding(monkeypatch):
    """no twin: [3,50] with the option on == [:, :50] of the parent's route on the same batch padded to [3,64] with
    attention_mask = 0 on the pads -- the hidden states (and their indices) of every layer"""
    from quantization import options
    B, T = 3, 50
    model = _gpu_model()
    ids, am = _ids(3, B, T), _mask(B, T)
    ids_p = torch.cat([ids, torch.full((B, 14), 1000)], 1)
    am_p = torch.cat([am, torch.zeros(B, 14, dtype=torch.long)], 1)
    assert options.INT8_RAGGED is False
    log = _census_with_ragged(monkeypatch)
    with torch.no_grad(), _Capture(model) as cap:
        model(ids_p.cuda(), am_p.cuda())
        padded = _host(cap.runs[-1])
        assert [e[0] for e in log].count('attention_i8') == LAYERS and RAGGED not in [e[0] for e in log]
        monkeypatch.setattr(options, 'INT8_RAGGED', True)
        model(ids.cuda(), am.cuda())
        ragged = _host(cap.runs[-1])
        assert [e[0] for e in log].count(RAGGED) == LAYERS
    for where in ('emb', 'attn', 'h'):
        for l, (r, p) in enumerate(zip(ragged[where], padded[where])):
            assert r[0].shape == (B, T, 768) and torch.equal(r[0], p[0][:, :T]), f'{where} {l}: values differ'
            assert r[1] is not None and torch.equal(r[1], p[1][:, :T]), f'{where} {l}: indices differ'
