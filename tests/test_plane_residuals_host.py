"""Host logic of options.INT8_PLANE_RESIDUALS, replayed on the CPU with the exact twin
(tests/_plane_residuals_twin.PlaneResidualsTwin): which layers of a BERT under {'x': 16, 'h': 16, 'y': 16} run both tails
through `residual_layernorm_quant_pres`, what those launches are handed, and where the route keeps today's launches.  The twin
answers the new method with the tail chain the existing methods are answered with, on the residual dequantized from its indices
or planes, so the route with the switch on must give `torch.equal` hidden states and logits to the route with it off."""
import pytest
import torch

from tests.test_bert_exact_route import _expected_census, _ids
from tests.test_plane_tails_host import B, D, LAYERS, S, T, _bert, _inputs, _names, _same

pytestmark = pytest.mark.default_route

NEW, PLANES, HILO, TAIL = ('residual_layernorm_quant_pres', 'residual_layernorm_quant_planes', 'quantize_hilo',
                           'residual_layernorm_quant')
# census entries of the two forms: (name, shape, residual kind, flags given, want_y, want_idx, want_planes)
F1_FIRST = (NEW, S, 'f32', False, False, False, True)       # layer 0: the embedding block's fp32 output, no flags yet
F1 = (NEW, S, 'idx', True, False, False, True)
F2 = (NEW, S, 'planes', True, True, True, False)
PER_LAYER = ['linear_i8_grouped', 'attention_i8', 'linear_i8', NEW, 'linear_i16x8', 'linear_i8', NEW]


def _run(model, on, be=None, plane_tails=True, inputs=None, **switches):
    """-> (the double, logits, hidden state after every layer, (indices, row flags) each hidden state carried)"""
    from quantization import _hip, options, provenance
    from tests._plane_residuals_twin import PlaneResidualsTwin
    be = be or PlaneResidualsTwin()
    prev = _hip.set_backend(be)
    want = dict(INT8_PLANE_RESIDUALS=on, INT8_PLANE_TAILS=plane_tails, **switches)
    saved = {k: getattr(options, k) for k in want}
    for k, v in want.items():
        setattr(options, k, v)
    try:
        ids, am = inputs or _inputs()
        outs, recs = [], []

        def wrap(L):
            f = type(L).forward

            def forward(h, m):
                y = f(L, h, m)
                outs.append(y)
                recs.append((provenance.indices_of(y), provenance.row_nan_of(y)))
                return y
            return forward
        for L in model.layers:
            L.forward = wrap(L)
        try:
            with torch.no_grad():
                y = model(ids, am)
        finally:
            for L in model.layers:
                del L.forward
    finally:
        for k, v in saved.items():
            setattr(options, k, v)
        _hip.set_backend(prev)
    return be, y.detach(), [o.detach() for o in outs], recs


def _layers(census):
    """a census cut at every layer's first launch: [embedding block, layer 0, layer 1, ...]"""
    cuts = [i for i, c in enumerate(census) if c[0] == 'linear_i8_grouped'] + [len(census)]
    return [census[:cuts[0]]] + [census[a:b] for a, b in zip(cuts, cuts[1:])]


def test_switch_is_off_by_default_cpu():
    from quantization import options
    assert options.INT8_PLANE_RESIDUALS is False


def test_switch_off_nothing_moves_cpu():
    """the new double under today's switches: today's census, the new method never called"""
    model = _bert()
    off = _run(model, False, plane_tails=False)
    assert off[0].census == _expected_census('mp16', LAYERS, B, T), off[0].census
    tails = _run(model, False, plane_tails=True)
    assert NEW not in _names(tails[0]) and _names(tails[0]).count(PLANES) == LAYERS
    _same(tails, off)


def test_three_layers_carry_x_as_planes_cpu():
    model = _bert()
    off = _run(model, False, plane_tails=False)
    tails = _run(model, False, plane_tails=True)
    on = _run(model, True)
    names = _names(on[0])
    assert names == ['embeddings_layernorm_quant'] + PER_LAYER * LAYERS, names
    # no plane tail, no quantize_hilo, no tail that writes x as fp32: site x exists as planes and flags alone
    assert PLANES not in names and HILO not in names and TAIL not in names
    new = [c for c in on[0].census if c[0] == NEW]
    assert new == [F1_FIRST, F2] + [F1, F2] * (LAYERS - 1), new
    # FFN1: the 16-bit Linear, index-only, on the planes; every other launch as with the switch off, in the same order
    ffn1 = [c for c in on[0].census if c[0] == 'linear_i16x8']
    assert len(ffn1) == LAYERS and all(c[1] == S and c[2] == 4 * D and c[3] is False for c in ffn1)
    other = lambda census: [c for c in census if c[0] not in (NEW, PLANES, TAIL, HILO)]
    assert other(on[0].census) == other(tails[0].census) == other(off[0].census)
    _same(on, off)
    _same(on, tails)
    # the layer outputs carry indices and flags: the next layer's first tail reads them
    assert all(i is not None and f is not None and not bool(f.any()) for i, f in on[3])
    assert all(torch.equal(i, j) for (i, _), (j, _) in zip(on[3], off[3]))
    # every tail still got ITS three quantizers in order
    ptr = lambda m: getattr(m, 'activation_quantizer', m).quantizer._delta.data_ptr()
    assert on[0].tail_bindings == [(ptr(b.dense.activation_quantizer), ptr(b.res_act_quantizer.activation_quantizer),
                                    ptr(b.LayerNorm.activation_quantizer)) for L in model.layers for b in (L.attention_output, L.output)]
    # without INT8_PLANE_TAILS beside it the switch gives the same launches: it does not ride on that one
    alone = _run(model, True, plane_tails=False)
    assert alone[0].census == on[0].census
    _same(alone, off)


def test_one_layer_cpu():
    """one layer called on its own, behind the embedding block: the seven launches, and the layer's output equal to today's"""
    from quantization import _hip, options, provenance
    from tests._plane_residuals_twin import PlaneResidualsTwin
    model = _bert()
    L = model.layers[0]
    out = {}
    for on in (False, True):
        be = PlaneResidualsTwin()
        prev, saved = _hip.set_backend(be), options.INT8_PLANE_RESIDUALS
        options.INT8_PLANE_RESIDUALS = on
        try:
            with torch.no_grad():
                h = model.embeddings(_inputs()[0])
                n = len(be.census)
                y = L(h, None)
                out[on] = (y, provenance.indices_of(y), provenance.row_nan_of(y), be.census[n:])
        finally:
            options.INT8_PLANE_RESIDUALS = saved
            _hip.set_backend(prev)
    assert [c[0] for c in out[True][3]] == PER_LAYER and [c for c in out[True][3] if c[0] == NEW] == [F1_FIRST, F2]
    assert out[False][3] == _layers(_expected_census('mp16', 1, B, T))[1]
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert out[True][2] is not None and out[False][2] is None


@pytest.mark.parametrize('also', ['INT8_INDEX_RESIDUALS', 'INT8_HEAD'])
def test_other_switches_beside_it_cpu(also):
    model = _bert()
    off = _run(model, False, plane_tails=False)
    on = _run(model, True, **{also: True})
    assert [c for c in on[0].census if c[0] == NEW] == [F1_FIRST, F2] + [F1, F2] * (LAYERS - 1)
    assert all(torch.equal(a, b) for a, b in zip(on[2], off[2]))
    if also == 'INT8_INDEX_RESIDUALS':
        _same(on, off)


def test_backend_without_the_entry_keeps_todays_calls_cpu():
    from tests._plane_residuals_twin import NoPlaneResidualsTwin
    model = _bert()
    off = _run(model, False, NoPlaneResidualsTwin())
    on = _run(model, True, NoPlaneResidualsTwin())
    assert on[0].census == off[0].census and _names(on[0]).count(PLANES) == LAYERS
    _same(on, off)


def _hook(model):
    model.layers[0].attention_output.LayerNorm.register_forward_hook(lambda m, a, o: None)
    return model


def _save_target(model):
    ln = model.layers[0].attention_output.LayerNorm
    ln.activation_save_target, ln.activation_save_name = {}, 'x'
    return model


def _estimating(model):
    model.layers[0].attention_output.LayerNorm.activation_quantizer.estimate_ranges()
    return model


@pytest.mark.parametrize('plane_tails', [True, False], ids=['plane_tails', 'default'])
@pytest.mark.parametrize('prepare', [_hook, _save_target, _estimating], ids=['hook', 'save_target', 'estimating'])
def test_an_observed_or_estimating_site_x_keeps_todays_launches_cpu(prepare, plane_tails):
    """layer 0's site x is observed, or its quantizer estimates: that layer runs exactly what it runs with the switch off (the
    plane tail and quantize_hilo included); the layers behind it carry x as planes"""
    off = _run(prepare(_bert()), False, plane_tails=plane_tails)
    on = _run(prepare(_bert()), True, plane_tails=plane_tails)
    l_on, l_off = _layers(on[0].census), _layers(off[0].census)
    assert l_on[:2] == l_off[:2], (l_on[1], l_off[1])
    assert NEW not in [c[0] for c in l_on[1]]
    # layer 1 reads layer 0's output as fp32 (no flags in its record), layer 2 as indices
    assert [[c for c in l if c[0] == NEW] for l in l_on[2:]] == [[F1_FIRST, F2], [F1, F2]]
    _same(on, off)


def test_a_16_bit_z_declines_for_that_layer_cpu():
    """the STS-B head recipe: site z of the last layer has 16 bits, so that layer keeps today's launches; the others do not"""
    off = _run(_bert('head'), False)
    on = _run(_bert('head'), True)
    l_on, l_off = _layers(on[0].census), _layers(off[0].census)
    assert l_on[-1] == l_off[-1] and NEW not in [c[0] for c in l_on[-1]] and PLANES in [c[0] for c in l_on[-1]]
    assert [[c for c in l if c[0] == NEW] for l in l_on[1:-1]] == [[F1_FIRST, F2]] + [[F1, F2]] * (LAYERS - 2)
    _same(on, off)


def test_a_ragged_token_count_declines_cpu():
    """M = 3 * 32 = 96 rows: no whole 64-row tiles for FFN1's MP16 plan -- today's launches at that shape, whatever they are"""
    ids = _ids(5, 3, 32)
    inputs = (ids, torch.ones_like(ids))
    off = _run(_bert(), False, inputs=inputs)
    on = _run(_bert(), True, inputs=inputs)
    assert NEW not in _names(on[0]) and on[0].census == off[0].census
    _same(on, off)


def test_fused_helper_declines_before_its_first_launch_cpu():
    """an unsigned weight grid on FFN2 is found after the plans: the helper must not have launched anything by then"""
    from quantization import _hip, fused, options
    from tests._plane_residuals_twin import PlaneResidualsTwin
    model = _bert()
    L = model.layers[0]
    be = PlaneResidualsTwin()
    prev, saved = _hip.set_backend(be), options.INT8_PLANE_RESIDUALS
    options.INT8_PLANE_RESIDUALS = True
    try:
        with torch.no_grad():
            h = model.embeddings(_inputs()[0])
            ctx = L.attention_self(h, None)
            n = len(be.census)
            args = (L.attention_output, L.intermediate[0], L.output, ctx, h)
            y = fused.quantized_bert_attention_output_ffn(*args)
            assert y is not None and [c[0] for c in be.census[n:]] == PER_LAYER[2:]
            wq = L.output.dense.weight_quantizer.quantizer
            wq._signed = torch.zeros_like(wq._signed)
            L.output.dense.cached_params = None
            L.output.dense._int8_cache = None
            n = len(be.census)
            assert fused.quantized_bert_attention_output_ffn(*args) is None
            assert len(be.census) == n
    finally:
        options.INT8_PLANE_RESIDUALS = saved
        _hip.set_backend(prev)


def test_twin_dequantizes_planes_to_the_plane_tails_y_cpu():
    """the premise of the route on the twin: scale * (index - zero_point) from the planes IS the y the plane tail wrote"""
    from tests._plane_residuals_twin import PlaneResidualsTwin, dequantized_residual
    g = torch.Generator().manual_seed(7)
    a, r = torch.randn(37, 64, generator=g) * 3, torch.randn(37, 64, generator=g)
    w, b = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    for n_bits, lo, hi in ((16, -6.0, 7.0), (12, -2.0, 9.0), (9, -5.0, 1.0)):
        delta = torch.tensor((hi - lo) / (2 ** n_bits - 1))
        q = (delta, torch.tensor(-lo) / delta, None, n_bits, False, False, 1e-8)
        y, planes = PlaneResidualsTwin().residual_layernorm_quant_planes(a, r, None, None, w, b, 1e-12, q)
        assert torch.equal(dequantized_residual(q, res_planes=planes), y)
