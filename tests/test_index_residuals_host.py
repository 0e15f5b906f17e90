"""Host logic of options.INT8_INDEX_RESIDUALS, replayed on the CPU with a recording double: which tails take the new entry
(`residual_layernorm_quant_ires`), what they are handed as residual, and where the route keeps today's calls.

The double is the exact twin (tests/_exact_backend.ExactBackend) plus the new method, answered by the twin's own tail chain
on the dequantized residual -- scale * ((index + 128) - zero_point), flagged rows NaN -- so the route with the option on
must give `torch.equal` hidden states and logits to the route with it off."""
import pytest
import torch

from tests._exact_backend import ExactBackend

pytestmark = pytest.mark.default_route

B, T, D = 2, 64, 768


class _IresTwin(ExactBackend):
    """+ the index-residual tail; every call is recorded in `self.ires`"""

    def __init__(self):
        super().__init__()
        self.ires = []

    def residual_layernorm_quant_ires(self, dense_out, residual, res_idx, q_res, res_row_nan, q_dense, q_sum, ln_weight, ln_bias,
                                      ln_eps, q_out, want_y=True, want_idx=True):
        assert (residual is None) != (res_idx is None) and (res_row_nan is None or res_idx is not None)
        assert q_out is not None and not q_out[4] and q_out[3] <= 8
        self.ires.append(dict(shape=tuple(dense_out.shape), indices=res_idx is not None, flags=res_row_nan is not None,
                              want_y=want_y, want_idx=want_idx))
        self._count('residual_layernorm_quant_ires', tuple(dense_out.shape), want_y, want_idx)
        if res_idx is not None:
            delta, zf, _, n_bits, symmetric, log_domain, eps = q_res
            assert not symmetric and not log_domain and n_bits <= 8 and delta.numel() == 1
            assert res_idx.dtype == torch.int8 and res_idx.shape == dense_out.shape and res_idx.is_contiguous()
            scale = torch.maximum(delta.detach().float().reshape(()), torch.tensor(eps, dtype=torch.float32))
            zp = torch.clamp(torch.round(zf.detach().float().reshape(())), 0, 2 ** n_bits - 1)
            residual = scale * ((res_idx.float() + 128.0) - zp)
            if res_row_nan is not None:
                assert res_row_nan.dtype == torch.uint8 and res_row_nan.shape == dense_out.shape[:-1]
                residual[res_row_nan.bool()] = float('nan')
        y, idx = self._tail(dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out, True)
        return (y if want_y else None), (idx if want_idx else None), torch.isnan(y).any(-1).to(torch.uint8)


class _NoIres(ExactBackend):
    """the parent commit's double: no index-residual tail"""


_MEMO = {}


def _bert(recipe, layers=2):
    import copy
    from quantization import _hip
    from tests.test_bert_exact_route import _calibrate, _ids, _model
    key = (recipe, layers)
    if key not in _MEMO:
        prev = _hip.set_backend(ExactBackend())
        try:
            _MEMO[key] = _calibrate(_model(recipe, layers, 'cpu'), recipe, [_ids(10, B, T)])
        finally:
            _hip.set_backend(prev)
    return copy.deepcopy(_MEMO[key])


def _inputs():
    ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(3))
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return ids, am


def _run(model, on, be=None):
    """-> (the double, logits, hidden state after every layer)"""
    from quantization import _hip, options
    be = be or _IresTwin()
    prev = _hip.set_backend(be)
    saved = options.INT8_INDEX_RESIDUALS
    options.INT8_INDEX_RESIDUALS = on
    try:
        ids, am = _inputs()
        outs = []
        for L in model.layers:
            L.forward = (lambda h, m, _f=type(L).forward, _L=L: (outs.append(_f(_L, h, m)), outs[-1])[1])
        try:
            with torch.no_grad():
                y = model(ids, am)
        finally:
            for L in model.layers:
                del L.forward
    finally:
        options.INT8_INDEX_RESIDUALS = saved
        _hip.set_backend(prev)
    return be, y, outs


def _kinds(census):
    """the launches with both tail entries under one name (the new one through `want_y`, as the old one always writes y)"""
    out = []
    for c in census:
        if c[0] == 'residual_layernorm_quant':
            out.append(('tail', c[1], True, c[2]))
        elif c[0] == 'residual_layernorm_quant_ires':
            out.append(('tail',) + tuple(c[1:]))
        else:
            out.append(c)
    return out


def _same(on, off):
    assert torch.equal(on[1], off[1])
    assert len(on[2]) == len(off[2]) and all(torch.equal(a, b) for a, b in zip(on[2], off[2]))


def test_option_on_residuals_travel_as_indices_cpu():
    layers = 2
    model = _bert('w8a8', layers)
    off = _run(model, False)
    on = _run(model, True)
    s = (B, T, D)
    assert off[0].ires == []                                             # option off: the new method is never called
    assert [c[0] for c in off[0].census].count('residual_layernorm_quant') == 2 * layers
    # option on: layer 0's attention-output tail gets the embedding block's fp32 output, every later tail indices and flags;
    # the attention-output tails ask for no y, the feed-forward tails keep theirs
    first = dict(shape=s, indices=False, flags=False, want_y=False, want_idx=True)
    attn = dict(shape=s, indices=True, flags=True, want_y=False, want_idx=True)
    ffn = dict(shape=s, indices=True, flags=True, want_y=True, want_idx=True)
    assert on[0].ires == [first, ffn] + [attn, ffn] * (layers - 1)
    names = [c[0] for c in on[0].census]
    assert 'residual_layernorm_quant' not in names
    # the same launches otherwise, in the same order: per layer QKV, core, attention-output Linear, tail, FFN1 index-only, FFN2, tail
    assert [c for c in on[0].census if not c[0].startswith('residual')] == [c for c in off[0].census if not c[0].startswith('residual')]
    per_layer = ['linear_i8_grouped', 'attention_i8', 'linear_i8', 'residual_layernorm_quant_ires', 'linear_i8', 'linear_i8',
                 'residual_layernorm_quant_ires']
    assert names == ['embeddings_layernorm_quant'] + per_layer * layers
    ffn1 = [c for c in on[0].census if c[0] == 'linear_i8' and c[2] == 4 * D]
    assert len(ffn1) == layers and all(c[3] is False for c in ffn1)       # index-only on the tail's indices
    _same(on, off)
    # the layer outputs carry their flags, the chain's link to the next layer
    from quantization import provenance
    assert all(provenance.row_nan_of(h) is not None and provenance.indices_of(h) is not None for h in on[2])
    assert all(provenance.row_nan_of(h) is None for h in off[2])


def test_backend_without_the_entry_keeps_todays_calls_cpu():
    model = _bert('w8a8', 1)
    off = _run(model, False, _NoIres())
    on = _run(model, True, _NoIres())
    assert on[0].census == off[0].census
    _same(on, off)


def _hook_site_x(model):
    fired = []
    h = model.layers[0].attention_output.LayerNorm.register_forward_hook(lambda m, a, o: fired.append(tuple(o.shape)))
    return fired, h.remove


def _save_site_x(model):
    ln = model.layers[0].attention_output.LayerNorm
    ln.activation_save_target, ln.activation_save_name = {}, 'x'
    return ln.activation_save_target, (lambda: None)


def _drain(seen):
    """how many observations were made since the last call"""
    n = len(seen)
    seen.clear()
    return n


@pytest.mark.parametrize('observe', [_hook_site_x, _save_site_x], ids=['hook', 'save_target'])
def test_an_observer_of_site_x_gets_todays_call_sequence_cpu(observe):
    """the layer whose site x is observed runs today's two calls (site x is produced as fp32, where the observer sees it): the
    same launches in the same order as with the option off; the layers behind it go back to the index form"""
    layers = 2
    model = _bert('w8a8', layers)
    seen, undo = observe(model)
    try:
        off = _run(model, False)
        n_off = _drain(seen)
        on = _run(model, True)
        n_on = _drain(seen)
    finally:
        undo()
    assert n_off >= 1 and n_on == n_off                                  # the observer saw site x in both runs
    k_on, k_off = _kinds(on[0].census), _kinds(off[0].census)
    # layer 0: no launch differs in kind, order or output form (its feed-forward tail takes the new entry with an fp32
    # residual and writes y); layer 1: the index form
    cut = next(i for i, c in enumerate(k_on) if c[0] == 'tail' and c[2] is False)
    assert k_on[:cut] == k_off[:cut] and [c for c in k_on if c[0] != 'tail'] == [c for c in k_off if c[0] != 'tail']
    assert all(not c['indices'] and c['want_y'] for c in on[0].ires[:-2])
    assert on[0].ires[-2:] == [dict(shape=(B, T, D), indices=True, flags=True, want_y=False, want_idx=True),
                               dict(shape=(B, T, D), indices=True, flags=True, want_y=True, want_idx=True)]
    _same(on, off)


@pytest.mark.parametrize('recipe', ['peg', 'mp16'])
def test_peg_and_w8a16_recipes_keep_todays_launches_cpu(recipe):
    model = _bert(recipe, 2)
    off = _run(model, False)
    on = _run(model, True)
    assert on[0].ires == [] and on[0].census == off[0].census
    _same(on, off)


def test_fused_helper_declines_before_its_first_launch_cpu():
    """an unsigned weight grid on FFN2 is found after the plans: the helper must not have launched anything by then"""
    from quantization import _hip, fused, options
    model = _bert('w8a8', 1)
    L = model.layers[0]
    wq = L.output.dense.weight_quantizer.quantizer
    wq._signed = torch.zeros_like(wq._signed)
    L.output.dense.cached_params = None
    be = _IresTwin()
    prev, saved = _hip.set_backend(be), options.INT8_INDEX_RESIDUALS
    options.INT8_INDEX_RESIDUALS = True
    try:
        with torch.no_grad():
            h = model.embeddings(_inputs()[0])
            ctx = L.attention_self(h, None)
            n = len(be.census)
            assert fused.quantized_bert_attention_output_ffn(L.attention_output, L.intermediate[0], L.output, ctx, h) is None
            assert len(be.census) == n and be.ires == []
    finally:
        options.INT8_INDEX_RESIDUALS = saved
        _hip.set_backend(prev)


def test_provenance_row_flags_cpu():
    from quantization import provenance

    class _Q:
        def range_state_key(self):
            return 1
    q, t, idx, flags = _Q(), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int8), torch.zeros(2, dtype=torch.uint8)
    provenance.tag(t, q, idx)
    assert provenance.of(t) == (q, idx) and provenance.row_nan_of(t) is None          # no flags known
    provenance.tag(t, q, idx, row_nan=flags)
    assert provenance.of(t) == (q, idx) and provenance.row_nan_of(t) is flags
    t.add_(1)                                                                          # a stale record has no flags either
    assert provenance.of(t) is None and provenance.row_nan_of(t) is None
    assert provenance.row_nan_of(torch.zeros(1)) is None
