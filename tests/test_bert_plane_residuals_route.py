"""options.INT8_PLANE_RESIDUALS on the GPU: a 3-layer BERT under the mixed-precision recipe {'x': 16, 'h': 16, 'y': 16} whose
site x travels as byte planes and row flags alone (tq_residual_layernorm_quant_pres_fwd, both forms) equals the exact CPU twin
(tests/_plane_residuals_twin.PlaneResidualsTwin) at zero tolerance -- the embedding block's output and the hidden state of
every layer with their int8 index records, and with options.INT8_HEAD the logits -- eager and as a hipGraph replay, with the
same launches on both sides; and it equals the same model with the switch off, also with each of INT8_INDEX_RESIDUALS,
INT8_PLANE_TAILS and INT8_HEAD on beside it, through `forward_packed`, and for a hidden state with a NaN row."""
import pytest
import torch

from tests.test_bert_exact_route import _expected_census, _ids, _twin_of
from tests.test_bert_plane_tails_route import (LAYERS, LENGTHS, _assert_tables_accepted, _gpu_model, _hip_log, _host, _mask, _on_twin,
                                               _Sites)

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]

NEW, PLANES, HILO, TAIL = ('residual_layernorm_quant_pres', 'residual_layernorm_quant_planes', 'quantize_hilo',
                           'residual_layernorm_quant')
SKINNY = ('linear_i16x8_skinny', 'linear_i8_skinny')
B, T, D = 3, 64, 768


def _log(monkeypatch):
    """launches of the HIP backend in the form the twin records its own, the new entry included"""
    from quantization import _hip
    log = _hip_log(monkeypatch)
    orig = _hip.HipBackend.residual_layernorm_quant_pres

    def counted(self, *a, **k):
        kind = 'f32' if a[1] is not None else 'idx' if a[2] is not None else 'planes'
        log.append((NEW, tuple(a[0].shape), kind, a[5] is not None, k.get('want_y', True), k.get('want_idx', False),
                    k.get('want_planes', False)))
        return orig(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, 'residual_layernorm_quant_pres', counted)
    return log


def _twin_backend(rules):
    from tests._packed_twin import PackedTwin
    from tests._plane_residuals_twin import PlaneResidualsTwin

    class PackedPlaneResidualsTwin(PackedTwin, PlaneResidualsTwin):
        name = 'exact-twin-packed-plane-residuals'
    return PackedPlaneResidualsTwin(rules=rules)


def _census_on(shape, stair):
    """the switch-on launches of the encoder: per layer both tails through the new entry, FFN1 on the planes"""
    s = tuple(shape) + (D,)
    out = []
    l = -1
    for c in _expected_census('mp16', LAYERS, shape[0], shape[1], stair=stair):
        if c[0] == 'linear_i8_grouped':
            l += 1
        if c[0] == HILO:
            continue
        if c[0] == TAIL and c[2] is False:
            c = (NEW, s, 'f32', False, False, False, True) if l == 0 else (NEW, s, 'idx', True, False, False, True)
        elif c[0] == TAIL:
            c = (NEW, s, 'planes', True, True, True, False)
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
def test_encoder_equals_the_twin_eager_and_replayed(head, monkeypatch):
    from quantization import _hip, options
    from quantization.graphs import GraphedForward
    assert options.INT8_LINEAR == 'auto' and options.INT8_PLANE_RESIDUALS is False
    model = _gpu_model('mp16', B, T)
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
        monkeypatch.setattr(options, 'INT8_PLANE_RESIDUALS', True)
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
    stair = [c[-1] for c in census if c[0] == 'linear_i16x8']
    assert len(stair) == LAYERS and len(set(stair)) == 1
    enc = lambda cs: [c for c in cs if c[0] not in SKINNY]
    assert enc(off_census) == _expected_census('mp16', LAYERS, B, T, stair=stair[0]), off_census
    assert enc(census) == _census_on((B, T), stair[0]), census
    names = [c[0] for c in census]
    assert names.count(NEW) == 2 * LAYERS and names.count('linear_i16x8') == LAYERS
    assert HILO not in names and PLANES not in names and TAIL not in names
    assert 'x' not in on and len(off['x']) == LAYERS             # site x is not produced as a tensor any more
    assert len(graph_census) % len(census) == 0 and graph_census == census * (len(graph_census) // len(census)), \
        'the launches of the graph\'s warm-up / capture passes differ from the eager forward\'s'
    # switch on == switch off on the GPU
    assert torch.equal(on_logits, off_logits) and torch.isfinite(on_logits).all()
    _equal_sites(on, off, 'switch on against switch off')
    # GPU == twin, eager and replayed
    be = _twin_backend(_hip.backend())
    twin_logits, chained, twin_census = _on_twin(twin, be, lambda m: m(ids, am))
    assert twin_census == census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    _equal_sites(on, chained, f'[{B},{T}] eager')
    _equal_sites(replay, chained, f'[{B},{T}] hipGraph replay')
    assert torch.equal(replay_logits, on_logits)
    assert all(torch.isfinite(y).all() for y, _, _ in on['h'])
    if head:                                                     # the skinny pooler and classifier: exact on both sides
        assert [c[0] for c in census[-2:]] == ['linear_i8_skinny'] * 2
        assert torch.equal(on_logits.cpu(), twin_logits), f'logits differ from the twin\'s: {(on_logits.cpu() - twin_logits).abs().max()}'


@pytest.mark.parametrize('also', ['INT8_INDEX_RESIDUALS', 'INT8_PLANE_TAILS', 'INT8_HEAD'])
def test_with_another_switch_on_as_well_equals_the_switch_off(also, monkeypatch):
    from quantization import options
    model = _gpu_model('mp16', B, T)
    args = (_ids(3, B, T).cuda(), _mask(B, T).cuda())
    log = _log(monkeypatch)
    with torch.no_grad(), _Sites(model) as cap:
        plain_logits = model(*args).clone()
        plain = _host(cap.runs[-1])
        monkeypatch.setattr(options, also, True)
        ref_logits = model(*args).clone()
        ref = _host(cap.runs[-1])
        del log[:]
        monkeypatch.setattr(options, 'INT8_PLANE_RESIDUALS', True)
        logits = model(*args).clone()
        torch.cuda.synchronize()
        got = _host(cap.runs[-1])
    names = [c[0] for c in log]
    assert names.count(NEW) == 2 * LAYERS and HILO not in names and PLANES not in names and TAIL not in names
    assert torch.equal(logits, ref_logits)
    if also != 'INT8_HEAD':                                       # (the integer head's logits are not the layered head's)
        assert torch.equal(logits, plain_logits)
    _equal_sites(got, ref, f'with {also}')
    _equal_sites(got, plain, f'with {also}, against every switch off')


def test_through_forward_packed(monkeypatch):
    """lengths (64, 40, 24): 128 packed rows, whole tiles for FFN1's MP16 plan"""
    from harness.bert import pack_batch
    from quantization import options
    from tests.test_bert_packed_route import _batch
    model = _gpu_model('mp16', B, T)
    ids, am = _batch(LENGTHS)
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    p_args = tuple(t.cuda() for t in (p_ids, p_pos, seq_start))
    M = sum(LENGTHS)
    assert M == 128
    log = _log(monkeypatch)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    with torch.no_grad(), _Sites(model) as cap:
        padded_logits = model(ids.cuda(), am.cuda()).clone()
        cap.runs.append({})                                     # (`forward_packed` is not the wrapped `forward`: open its record here)
        off_logits = model.forward_packed(*p_args, max_len).clone()
        off = _host(cap.runs[-1])
        assert NEW not in [c[0] for c in log]
        del log[:]
        monkeypatch.setattr(options, 'INT8_PLANE_RESIDUALS', True)
        cap.runs.append({})
        on_logits = model.forward_packed(*p_args, max_len).clone()
        torch.cuda.synchronize()
        on = _host(cap.runs[-1])
    new = [c for c in log if c[0] == NEW]
    s = (1, M, D)
    assert new == [(NEW, s, 'f32', False, False, False, True), (NEW, s, 'planes', True, True, True, False)] + \
                  [(NEW, s, 'idx', True, False, False, True), (NEW, s, 'planes', True, True, True, False)] * (LAYERS - 1), new
    assert HILO not in [c[0] for c in log]
    assert torch.equal(on_logits, off_logits) and torch.isfinite(on_logits).all()
    _equal_sites(on, off, 'packed')
    assert on['h'][-1][0].shape == s and padded_logits.shape == on_logits.shape


def test_a_nan_row_goes_through_a_layer_as_it_does_today(monkeypatch):
    """one QLayer on a tagged hidden state (values, int8 indices, row flags) whose row (0, 5) is NaN: the same output bits, the
    row NaN as a whole and flagged"""
    from quantization import options, provenance
    model = _gpu_model('mp16', B, T)
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
            monkeypatch.setattr(options, 'INT8_PLANE_RESIDUALS', on)
            y = layer(h, mask)
            outs[on] = (y.clone(), provenance.indices_of(y), provenance.row_nan_of(y))
            assert provenance.row_nan_of(h) is flags          # the record is still valid
    s = (B, T, D)
    assert [c for c in log if c[0] == NEW] == [(NEW, s, 'idx', True, False, False, True), (NEW, s, 'planes', True, True, True, False)]
    y_off, y_on = outs[False][0], outs[True][0]
    assert torch.isnan(y_off[0, 5]).all() and int(torch.isnan(y_off).any(-1).sum()) == 1
    assert torch.equal(y_on.view(torch.int32), y_off.view(torch.int32))
    keep = ~torch.isnan(y_off).any(-1)
    assert torch.equal(outs[True][1][keep], outs[False][1][keep])
    assert torch.equal(outs[True][2].bool(), ~keep)
