"""Host logic of options.INT8_PEG_INDEX_RESIDUALS, replayed on the CPU with the exact twin (tests/_peg_ires_twin.PegIresTwin):
which layers of a BERT under the PEG recipes run both tails through `residual_layernorm_quant_axis_ires`, what those launches
are handed, and where the route keeps today's launches.  The twin answers the new method with the tail chain the existing
methods are answered with, on the residual dequantized from its indices, so the route with the switch on must give
`torch.equal` hidden states and logits to the route with it off."""
import pytest
import torch

from tests.test_bert_exact_route import _expected_census, _ids
from tests.test_index_residuals_host import B, D, T, _bert, _inputs, _same

pytestmark = pytest.mark.default_route

NEW, AXIS = 'residual_layernorm_quant_axis_ires', 'residual_layernorm_quant_axis'
S = (B, T, D)
# census entries: (name, shape, (q_dense, q_sum, q_out) parameters, residual kind, residual grid parameters, flags, want_y, want_idx)
A_FIRST = (NEW, S, (1, 1, D), 'f32', None, False, False, True)      # layer 0: the embedding block's fp32 output, no flags yet
A = (NEW, S, (1, 1, D), 'idx', 1, True, False, True)               # attention-output tail: h on its per-tensor grid
F = (NEW, S, (D, D, 1), 'idx', D, True, True, True)                # feed-forward tail: x on its per-column grid
PER_LAYER = ['linear_i8_grouped', 'attention_i8', 'linear_i8', NEW, 'linear_i8_cls', 'linear_i8', NEW]


def _run(model, on, be=None, inputs=None, **switches):
    """-> (the double, logits, hidden state after every layer, (indices, row flags) each hidden state carried)"""
    from quantization import _hip, options, provenance
    from tests._peg_ires_twin import PegIresTwin
    be = be or PegIresTwin()
    prev = _hip.set_backend(be)
    want = dict(INT8_PEG_INDEX_RESIDUALS=on, **switches)
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


def _names(be):
    return [c[0] for c in be.census]


def _layers(census):
    """a census cut at every layer's first launch: [embedding block, layer 0, layer 1, ...]"""
    cuts = [i for i, c in enumerate(census) if c[0] == 'linear_i8_grouped'] + [len(census)]
    return [census[:cuts[0]]] + [census[a:b] for a, b in zip(cuts, cuts[1:])]


def test_switch_is_off_by_default_cpu():
    from quantization import options
    assert options.INT8_PEG_INDEX_RESIDUALS is False


@pytest.mark.parametrize('layers', [1, 3])
@pytest.mark.parametrize('recipe', ['peg', 'peg_permuted'])
def test_layers_carry_x_as_indices_cpu(recipe, layers):
    model = _bert(recipe, layers)
    off = _run(model, False)
    on = _run(model, True)
    assert off[0].census == _expected_census(recipe, layers, B, T), off[0].census      # switch off: today's launches
    names = _names(on[0])
    assert names == ['embeddings_layernorm_quant'] + PER_LAYER * layers, names
    assert AXIS not in names                                                       # no tail writes x as fp32
    # layer 0's first tail takes an fp32 residual without flags, every later tail indices + flags; the attention-output tails
    # ask for no y, the feed-forward tails keep theirs
    new = [c for c in on[0].census if c[0] == NEW]
    assert new == [A_FIRST, F] + [A, F] * (layers - 1), new
    # FFN1: the class-ordered Linear, index-only, on the tail's indices; every other launch as with the switch off, in order
    ffn1 = [c for c in on[0].census if c[0] == 'linear_i8_cls']
    assert len(ffn1) == layers and all(c[1] == S and c[2] == 4 * D and c[3] is False for c in ffn1)
    other = lambda census: [c for c in census if c[0] not in (NEW, AXIS)]
    assert other(on[0].census) == other(off[0].census)
    _same(on, off)
    # the layer outputs carry indices and flags: the next layer's first tail reads them
    assert all(i is not None and f is not None and not bool(f.any()) for i, f in on[3])
    assert all(torch.equal(i, j) for (i, _), (j, _) in zip(on[3], off[3]))
    assert all(f is None for _, f in off[3])
    # every tail still got ITS three quantizers in order
    ptr = lambda m: getattr(m, 'activation_quantizer', m).quantizer._delta.data_ptr()
    assert on[0].tail_bindings == [(ptr(b.dense.activation_quantizer), ptr(b.res_act_quantizer.activation_quantizer),
                                    ptr(b.LayerNorm.activation_quantizer)) for L in model.layers for b in (L.attention_output, L.output)]


@pytest.mark.parametrize('recipe', ['w8a8', 'mp16'])
def test_per_tensor_recipes_keep_todays_launches_cpu(recipe):
    model = _bert(recipe, 2)
    off = _run(model, False)
    on = _run(model, True)
    assert NEW not in _names(on[0]) and on[0].census == off[0].census
    _same(on, off)


def test_index_residuals_switch_beside_it_cpu():
    """INT8_INDEX_RESIDUALS goes on doing nothing under PEG, with or without the new switch"""
    model = _bert('peg', 2)
    off = _run(model, False)
    both = _run(model, True, INT8_INDEX_RESIDUALS=True)
    assert [c for c in both[0].census if c[0] == NEW] == [A_FIRST, F, A, F]
    _same(both, off)
    old = _run(model, False, INT8_INDEX_RESIDUALS=True)
    assert old[0].census == off[0].census


def test_backend_without_the_entry_keeps_todays_calls_cpu():
    from tests._peg_ires_twin import NoPegIresTwin
    model = _bert('peg', 1)
    off = _run(model, False, NoPegIresTwin())
    on = _run(model, True, NoPegIresTwin())
    assert on[0].census == off[0].census and _names(on[0]).count(AXIS) == 2
    _same(on, off)


def _hook(model):
    model.layers[0].attention_output.LayerNorm.register_forward_hook(lambda m, a, o: None)
    return model


def _save_target(model):
    ln = model.layers[0].attention_output.LayerNorm
    ln.activation_save_target, ln.activation_save_name = {}, 'x'
    return model


@pytest.mark.parametrize('prepare', [_hook, _save_target], ids=['hook', 'save_target'])
def test_an_observed_site_x_keeps_todays_launches_cpu(prepare):
    """layer 0's site x is observed: that layer runs exactly what it runs with the switch off; the layer behind it reads its
    output as fp32 (no flags in its record: the chain-start rule of the embedding block) and carries x as indices"""
    off = _run(prepare(_bert('peg', 2)), False)
    on = _run(prepare(_bert('peg', 2)), True)
    l_on, l_off = _layers(on[0].census), _layers(off[0].census)
    assert l_on[:2] == l_off[:2], (l_on[1], l_off[1])
    assert NEW not in [c[0] for c in l_on[1]]
    assert [c for c in l_on[2] if c[0] == NEW] == [A_FIRST, F]
    _same(on, off)


def test_unsigned_ffn2_weight_grid_declines_before_the_first_launch_cpu():
    """an unsigned weight grid on FFN2 is found after the plans: the helper must not have launched anything by then"""
    from quantization import _hip, fused, options
    from tests._peg_ires_twin import PegIresTwin
    model = _bert('peg', 1)
    L = model.layers[0]
    be = PegIresTwin()
    prev, saved = _hip.set_backend(be), options.INT8_PEG_INDEX_RESIDUALS
    options.INT8_PEG_INDEX_RESIDUALS = True
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
        options.INT8_PEG_INDEX_RESIDUALS = saved
        _hip.set_backend(prev)


def test_a_ragged_token_count_declines_cpu():
    """[2,50] under INT8_RAGGED: M = 100 rows are no whole 64-row tiles for FFN1's PEG plan -- today's launches at that shape"""
    from tests._peg_ires_twin import PegIresTwin
    from tests._ragged_twin import RaggedTwin

    class _RaggedPeg(PegIresTwin, RaggedTwin):
        pass
    ids = _ids(5, 2, 50)
    inputs = (ids, torch.ones_like(ids))
    off = _run(_bert('peg', 1), False, _RaggedPeg(), inputs=inputs, INT8_RAGGED=True)
    on = _run(_bert('peg', 1), True, _RaggedPeg(), inputs=inputs, INT8_RAGGED=True)
    assert NEW not in _names(on[0]) and on[0].census == off[0].census
    _same(on, off)


def test_d_1024_declines_cpu():
    """rows of 1024 columns: the axis tail takes them, the new entry does not (its tables would need 69.6 KB of LDS) -- the tail
    conditions, which the helper checks before its first launch, say no"""
    from quantization import _hip, fused
    from quantization.int8_route import QSpec
    from tests._peg_ires_twin import PegIresTwin
    prev = _hip.set_backend(PegIresTwin())
    try:
        q = QSpec(torch.full((1024,), 0.1), torch.full((1024,), 3.0), None, 8, False, False, 1e-8)

        class _LN:
            normalized_shape = (1024,)
        assert fused._axis_tail_ok(1024, torch.float32)
        assert not fused._route_tail_ok(fused._PEG_ROUTE, _LN(), 1024, None, None, q)
        _LN.normalized_shape = (768,)
        assert fused._route_tail_ok(fused._PEG_ROUTE, _LN(), 768, None, None, q._replace(delta=q.delta[:768], zero_float=q.zero_float[:768]))
        assert not fused._route_tail_ok(fused._PEG_ROUTE, _LN(), 768, None, None, q._replace(n_bits=9))
    finally:
        _hip.set_backend(prev)


def test_twin_dequantizes_indices_to_the_axis_tails_y_cpu():
    """the premise of the route on the twin: max(delta_c, eps) * (index - clamp(round(zero_float_c))) IS the y the per-column
    tail wrote, -0.0 inputs and tiny negatives included"""
    from tests._peg_ires_twin import PegIresTwin, dequantized_axis_residual
    g = torch.Generator().manual_seed(7)
    d = 768
    a, r = torch.randn(37, d, generator=g) * 3, torch.randn(37, d, generator=g)
    a[0, :8] = torch.tensor([-0.0, 0.0, -1e-9, 1e-9, -0.0, 0.0, -1e-9, 1e-9])
    r[0, :8] = 0.0
    w, b = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g) * 0.1
    b[:8] = torch.tensor([-0.0, 0.0, -1e-9, 1e-9, 0.0, -0.0, 1e-9, -1e-9])
    lo = -(torch.rand(6, generator=g) * 4 + 0.5)
    hi = torch.rand(6, generator=g) * 4 + 0.5
    perm = torch.randperm(d, generator=g)
    for n_bits in (8, 4, 1):
        delta6 = (hi - lo) / (2 ** n_bits - 1)
        group = torch.arange(d) // (d // 6)
        for cols in (group, group[perm]):
            delta, zf = delta6[cols].contiguous(), (-lo / delta6)[cols].contiguous()
            q = (delta, zf, None, n_bits, False, False, 1e-8)
            y, idx = PegIresTwin().residual_layernorm_quant_axis(a, r, None, None, w, b, 1e-12, q, want_idx=True)
            back = dequantized_axis_residual(q, idx)
            assert torch.equal(back.view(torch.int32), y.view(torch.int32))
