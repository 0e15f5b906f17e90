"""options.INT8_PEG_INDEX_RESIDUALS on the GPU: a 3-layer BERT under the PEG recipes ({'x', 'h', 'y'}: 'ng6' and 'ngp6') whose
site x travels as int8 indices and row flags alone (tq_residual_layernorm_quant_axis_ires_fwd) equals the same model with the
switch off -- every hidden state and the logits, eager and as a hipGraph replay -- and the exact CPU twin
(tests/_peg_ires_twin.PegIresTwin) at zero tolerance with the same launches on both sides; with options.INT8_HEAD the logits
equal the twin's; at a ragged token count the helper declines; a hidden state with a NaN row goes through a layer as today."""
import pytest
import torch

from tests.test_bert_exact_route import _calibrate, _expected_census, _ids, _model, _twin_of
from tests.test_bert_plane_tails_route import _assert_tables_accepted, _hip_log, _host, _mask, _on_twin, _Sites

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]

NEW, AXIS = 'residual_layernorm_quant_axis_ires', 'residual_layernorm_quant_axis'
SKINNY = ('linear_i16x8_skinny', 'linear_i8_skinny')
LAYERS, B, T, D = 3, 3, 64, 768
_GPU = {}


def _gpu_model(recipe):
    from quantization import options
    if recipe not in _GPU:
        assert not (options.INT8_PEG_INDEX_RESIDUALS or options.INT8_HEAD or options.INT8_RAGGED or options.INT8_INDEX_RESIDUALS)
        _GPU[recipe] = _calibrate(_model(recipe, LAYERS, 'cuda'), recipe, [_ids(10, B, T).cuda(), _ids(11, B, T).cuda()])
    return _GPU[recipe]


def _log(monkeypatch):
    """launches of the HIP backend in the form the twin records its own, the new entry included"""
    from quantization import _hip
    log = _hip_log(monkeypatch)
    orig = _hip.HipBackend.residual_layernorm_quant_axis_ires

    def counted(self, *a, **k):
        log.append((NEW, tuple(a[0].shape), tuple(None if q is None else q[0].numel() for q in (a[5], a[6], a[10])),
                    'f32' if a[1] is not None else 'idx', None if a[3] is None else a[3][0].numel(), a[4] is not None,
                    k.get('want_y', True), k.get('want_idx', True)))
        return orig(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, 'residual_layernorm_quant_axis_ires', counted)
    return log


def _twin_backend(rules):
    from tests._packed_twin import PackedTwin
    from tests._peg_ires_twin import PegIresTwin
    from tests._skinny_twin import SkinnyTwin

    class PackedPegIresTwin(PackedTwin, SkinnyTwin, PegIresTwin):
        name = 'exact-twin-packed-peg-index-residuals'
    return PackedPegIresTwin(rules=rules)


def _census_on(recipe, stair):
    """the switch-on launches of the encoder: per layer both tails through the new entry"""
    s = (B, T, D)
    out, l = [], -1
    for c in _expected_census(recipe, LAYERS, B, T, stair=stair):
        if c[0] == 'linear_i8_grouped':
            l += 1
        if c[0] == AXIS and c[2] == (1, 1, D):
            c = (NEW, s, c[2], 'f32', None, False, False, True) if l == 0 else (NEW, s, c[2], 'idx', 1, True, False, True)
        elif c[0] == AXIS:
            c = (NEW, s, c[2], 'idx', D, True, True, True)
        out.append(c)
    return out


def _equal_sites(got, want, what):
    """the embedding block's output and every layer's hidden state, as bit patterns, with their int8 index records"""
    for where in ('emb', 'h'):
        assert len(got[where]) == len(want[where]) == (1 if where == 'emb' else LAYERS), what
        for l, (g, w) in enumerate(zip(got[where], want[where])):
            at = f'{what}: {where} {l}'
            assert torch.equal(g[0].view(torch.int32), w[0].view(torch.int32)), f'{at}: values differ ({int((g[0] != w[0]).sum())} elements)'
            assert g[1] is not None and w[1] is not None and torch.equal(g[1], w[1]), f'{at}: int8 index records differ'


@pytest.mark.parametrize('head', [False, True], ids=['layered_head', 'int8_head'])
@pytest.mark.parametrize('recipe', ['peg', 'peg_permuted'])
def test_encoder_equals_the_switch_off_and_the_twin_eager_and_replayed(recipe, head, monkeypatch):
    from quantization import _hip, options
    from quantization.graphs import GraphedForward
    assert options.INT8_LINEAR == 'auto' and options.INT8_PEG_INDEX_RESIDUALS is False
    model = _gpu_model(recipe)
    ids, am = _ids(3, B, T), _mask(B, T)
    args = (ids.cuda(), am.cuda())
    twin = _twin_of(model)
    log = _log(monkeypatch)
    monkeypatch.setattr(options, 'INT8_HEAD', head)
    with torch.no_grad(), _Sites(model) as cap:
        off_logits = model(*args).clone()
        torch.cuda.synchronize()
        off, off_census = _host(cap.runs[-1]), list(log)
        del log[:]
        monkeypatch.setattr(options, 'INT8_PEG_INDEX_RESIDUALS', True)
        on_logits = model(*args).clone()
        torch.cuda.synchronize()
        on, census = _host(cap.runs[-1]), list(log)
        del log[:]
        g = GraphedForward(model, *args)
        static = cap.runs[-1]                                   # the capture pass: the graph's own tensors
        graph_census = list(log)
        replay_logits = g(*args).clone()
        torch.cuda.synchronize()
        replay = _host(static)
    _assert_tables_accepted(model)                               # the staircase premise of a zero-tolerance comparison
    stair = [c[-1] for c in census if c[0] == 'linear_i8_cls']
    assert len(stair) == LAYERS and len(set(stair)) == 1
    enc = lambda cs: [c for c in cs if c[0] not in SKINNY]
    assert enc(off_census) == _expected_census(recipe, LAYERS, B, T, stair=stair[0]), off_census
    assert enc(census) == _census_on(recipe, stair[0]), census
    names = [c[0] for c in census]
    assert names.count(NEW) == 2 * LAYERS and AXIS not in names
    assert 'x' not in on and len(off['x']) == LAYERS             # site x is not produced as a tensor any more
    assert len(graph_census) % len(census) == 0 and graph_census == census * (len(graph_census) // len(census)), \
        'the launches of the graph\'s warm-up / capture passes differ from the eager forward\'s'
    # switch on == switch off on the GPU, eager and replayed
    assert torch.equal(on_logits, off_logits) and torch.isfinite(on_logits).all()
    _equal_sites(on, off, 'switch on against switch off')
    _equal_sites(replay, off, 'hipGraph replay against switch off')
    assert torch.equal(replay_logits, off_logits)
    # GPU == twin, with both sides' censuses agreeing
    be = _twin_backend(_hip.backend())
    prev = options.INT8_PEG_INDEX_RESIDUALS
    twin_logits, chained, twin_census = _on_twin(twin, be, lambda m: m(ids, am))
    assert options.INT8_PEG_INDEX_RESIDUALS is prev is True
    assert twin_census == census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    _equal_sites(on, chained, f'[{B},{T}] eager against the twin')
    assert all(torch.isfinite(y).all() for y, _, _ in on['h'])
    if head:                                                     # the skinny pooler and classifier: exact on both sides
        assert [c[0] for c in census[-2:]] == ['linear_i8_skinny'] * 2
        assert torch.equal(on_logits.cpu(), twin_logits), f'logits differ from the twin\'s: {(on_logits.cpu() - twin_logits).abs().max()}'


def test_a_ragged_token_count_declines(monkeypatch):
    """[3,50] under INT8_RAGGED: M = 150 rows are no whole 64-row tiles for FFN1's PEG plan: bits and tail launches equal the
    switch-off run"""
    from quantization import options
    model = _gpu_model('peg')
    Tr = 50
    args = (_ids(3, B, Tr).cuda(), _mask(B, Tr).cuda())
    log = _log(monkeypatch)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    with torch.no_grad(), _Sites(model) as cap:
        off_logits = model(*args).clone()
        torch.cuda.synchronize()
        off, off_census = _host(cap.runs[-1]), list(log)
        del log[:]
        monkeypatch.setattr(options, 'INT8_PEG_INDEX_RESIDUALS', True)
        on_logits = model(*args).clone()
        torch.cuda.synchronize()
        on, census = _host(cap.runs[-1]), list(log)
    assert NEW not in [c[0] for c in census] and census == off_census
    assert [c[0] for c in census].count(AXIS) == 2 * LAYERS
    assert torch.equal(on_logits, off_logits) and torch.isfinite(on_logits).all()
    _equal_sites(on, off, 'ragged')
    assert all(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) for a, b in zip(on['x'], off['x']))


def test_a_nan_row_goes_through_a_layer_as_it_does_today(monkeypatch):
    """one QLayer on a tagged hidden state (values, int8 indices, row flags) whose row (0, 5) is NaN: the same output bits, the
    row NaN as a whole and flagged"""
    from quantization import options, provenance
    model = _gpu_model('peg')
    ids, am = _ids(3, B, T).cuda(), _mask(B, T).cuda()
    mask = (1.0 - am[:, None, None, :].float()) * -10000.0
    layer = model.layers[1]
    outs = {}
    log = _log(monkeypatch)
    with torch.no_grad():
        h0 = model.layers[0](model.embeddings(ids), mask)
        q, idx = provenance.of(h0)
        assert idx is not None
        h = h0.clone()
        h[0, 5] = float('nan')
        flags = torch.zeros(h.shape[:-1], dtype=torch.uint8, device='cuda')
        flags[0, 5] = 1
        provenance.tag(h, q, idx.clone(), row_nan=flags)      # (the index bytes of a NaN row mean nothing)
        del log[:]
        for on in (False, True):
            monkeypatch.setattr(options, 'INT8_PEG_INDEX_RESIDUALS', on)
            y = layer(h, mask)
            outs[on] = (y.clone(), provenance.indices_of(y), provenance.row_nan_of(y))
            assert provenance.row_nan_of(h) is flags          # the record is still valid
    s = (B, T, D)
    assert [c for c in log if c[0] == NEW] == [(NEW, s, (1, 1, D), 'idx', 1, True, False, True),
                                               (NEW, s, (D, D, 1), 'idx', D, True, True, True)]
    y_off, y_on = outs[False][0], outs[True][0]
    nan_rows = torch.isnan(y_off).any(-1)
    assert torch.isnan(y_off[0, 5]).all() and bool(nan_rows[0, 5])
    assert torch.equal(y_on.view(torch.int32), y_off.view(torch.int32))
    keep = ~nan_rows
    assert torch.equal(outs[True][1][keep], outs[False][1][keep])
    assert torch.equal(outs[True][2].bool(), nan_rows)
