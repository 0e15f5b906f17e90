"""Host logic of options.INT8_RAGGED_RECIPES, replayed on the CPU with the exact twin (tests/_ragged_recipes_twin): under the W8A16
recipe {'x': 16, 'h': 16, 'y': 16} and the PEG recipes {'x', 'h', 'y'}: 'ng6' / 'ngp6' the first feed-forward Linear of a BERT
layer stays on the integer route at a token count that is no multiple of 64 -- `linear_i16x8` / `linear_i8_cls`, index-only --
only with the switch, INT8_RAGGED and a backend that declares PADS_RECIPE_ROWS; the three opt-in routes built on FFN1
(INT8_PLANE_TAILS, INT8_PLANE_RESIDUALS, INT8_PEG_INDEX_RESIDUALS) then take their entries at that shape; whole-tile shapes do not
notice the switch; and the [3,50] forward equals, on [:, :50], the forward of the batch padded by the caller to [3,64].

The twin's Linears are the row-by-row formulas the kernel tests use as reference, so nothing here says anything about the
backend's padded launches: tests/test_recipe_row_tails.py and tests/test_bert_ragged_recipes_route.py do, on the GPU."""
import pytest
import torch

from tests.test_bert_exact_route import _expected_census, _ids, _twin_chained
from tests.test_index_residuals_host import _bert

pytestmark = pytest.mark.default_route

B, T, D = 3, 50, 768
S = (B, T, D)
RECIPES = ['mp16', 'peg', 'peg_permuted']
FFN1 = {'mp16': 'linear_i16x8', 'peg': 'linear_i8_cls', 'peg_permuted': 'linear_i8_cls'}
RAGGED, VARLEN, HILO = 'attention_i8_ragged', 'attention_i8_varlen', 'quantize_hilo'
# (switch, recipe, the entry of its tails): the three opt-in routes built on FFN1
ROUTES = [('INT8_PLANE_TAILS', 'mp16', 'residual_layernorm_quant_planes'),
          ('INT8_PLANE_RESIDUALS', 'mp16', 'residual_layernorm_quant_pres'),
          ('INT8_PEG_INDEX_RESIDUALS', 'peg', 'residual_layernorm_quant_axis_ires'),
          ('INT8_PEG_INDEX_RESIDUALS', 'peg_permuted', 'residual_layernorm_quant_axis_ires')]


def _inputs(b=B, t=T):
    am = torch.ones(b, t, dtype=torch.long)
    am[1, t - t // 4:] = 0                                    # one padded sample
    return _ids(3, b, t), am


def _ragged_census(recipe, layers, b, t):
    """the default route's launches of the recipe with the ragged core in place of the whole-tile one"""
    return [((RAGGED,) + e[1:]) if e[0] == 'attention_i8' else e for e in _expected_census(recipe, layers, b, t)]


def _switches(**want):
    """options set for the duration of a `with`"""
    import contextlib
    from quantization import options

    @contextlib.contextmanager
    def ctx():
        saved = {k: getattr(options, k) for k in want}
        for k, v in want.items():
            setattr(options, k, v)
        try:
            yield
        finally:
            for k, v in saved.items():
                setattr(options, k, v)
    return ctx()


def _run(model, be=None, inputs=None, recipes=True, ragged=True, packed=False, **switches):
    """one forward on the twin -> dict(be, logits, emb, h = [(values, indices, row flags)] per layer, calls, census)"""
    from quantization import _hip, provenance
    from quantization.autoquant_utils import INT8_STATS
    from tests._ragged_recipes_twin import RaggedRecipesTwin
    be = be or RaggedRecipesTwin()
    ids, am = inputs or _inputs()
    out = dict(be=be, h=[])
    rec = lambda y: (y.detach(), provenance.indices_of(y), provenance.row_nan_of(y))

    def wrap(L):
        f = type(L).forward

        def forward(h, m):
            y = f(L, h, m)
            out['h'].append(rec(y))
            return y
        return forward
    prev = _hip.set_backend(be)
    try:
        with _switches(INT8_RAGGED=ragged, INT8_RAGGED_RECIPES=recipes, **switches), torch.no_grad():
            for L in model.layers:
                L.forward = wrap(L)
            try:
                k0, fb0 = INT8_STATS['kernel_calls'], INT8_STATS['unsigned_weight_fallbacks']
                if packed:
                    from harness.bert import pack_batch
                    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
                    out['seq_start'] = seq_start
                    y = model.forward_packed(p_ids, p_pos, seq_start, max_len)
                else:
                    y = model(ids, am)
                out['calls'] = INT8_STATS['kernel_calls'] - k0
                assert INT8_STATS['unsigned_weight_fallbacks'] == fb0
            finally:
                for L in model.layers:
                    del L.forward
    finally:
        _hip.set_backend(prev)
    out.update(logits=y.detach(), census=list(be.census))
    return out


def _names(run):
    return [c[0] for c in run['census']]


def _same(a, b):
    assert torch.equal(a['logits'], b['logits']), 'logits differ'
    assert len(a['h']) == len(b['h'])
    for l, (x, y) in enumerate(zip(a['h'], b['h'])):
        assert torch.equal(x[0], y[0]), f'hidden state {l} differs'
        assert x[1] is not None and y[1] is not None and torch.equal(x[1], y[1]), f'indices of hidden state {l} differ'


def test_the_switch_needs_all_three_cpu():
    from quantization import options
    from tests._exact_backend import ExactBackend
    from tests._ragged_recipes_twin import NoRecipeRowsTwin, RaggedRecipesTwin
    assert options.INT8_RAGGED_RECIPES is False and options.INT8_RAGGED is False
    full, none = RaggedRecipesTwin(), NoRecipeRowsTwin()
    assert not options.int8_ragged_recipes(full)
    with _switches(INT8_RAGGED_RECIPES=True):
        assert not options.int8_ragged_recipes(full)                     # INT8_RAGGED is off
    with _switches(INT8_RAGGED=True):
        assert options.int8_ragged(full) and not options.int8_ragged_recipes(full)       # cannot ride on INT8_RAGGED alone
    with _switches(INT8_RAGGED=True, INT8_RAGGED_RECIPES=True):
        assert options.int8_ragged_recipes(full)
        assert options.int8_ragged(none) and not options.int8_ragged_recipes(none)       # no PADS_RECIPE_ROWS
        assert not options.int8_ragged_recipes(ExactBackend())            # no ragged core, no row tails at all
    from quantization import _hip
    assert _hip.HipBackend.PADS_RECIPE_ROWS is True and _hip.HipBackend.PADS_ROWS is True


@pytest.mark.parametrize('recipe', RECIPES)
def test_switch_on_ffn1_stays_on_the_integer_route_cpu(recipe):
    layers = 2
    on = _run(_bert(recipe, layers))
    assert on['census'] == _ragged_census(recipe, layers, B, T), on['census']
    ffn1 = [c for c in on['census'] if c[0] == FFN1[recipe]]
    assert ffn1 == [(FFN1[recipe], S, 4 * D, False, True)] * layers          # index-only, staircase, on (3, 50, 768)
    assert on['calls'] == layers * 6                                          # Q, K, V, attention output, FFN1, FFN2: none layered
    assert all(i is not None and torch.isfinite(y).all() and y.shape == S for y, i, _ in on['h'])


@pytest.mark.parametrize('recipe', RECIPES)
def test_switch_off_or_a_backend_without_the_rows_keeps_the_parents_route_cpu(recipe):
    from tests._ragged_recipes_twin import NoRecipeRowsTwin
    layers = 2
    off = _run(_bert(recipe, layers), recipes=False)
    parent = _run(_bert(recipe, layers), NoRecipeRowsTwin())
    assert off['census'] == parent['census'] and off['calls'] == parent['calls'] == layers * 5
    assert FFN1[recipe] not in _names(off) and HILO not in _names(off)      # FFN1 layered: fp32 GEMM, GELU, fake-quant
    assert _names(off).count(RAGGED) == layers
    _same(off, parent)
    # without INT8_RAGGED the new switch does nothing at all: the encoder is layered at this shape, as ever
    alone = _run(_bert(recipe, layers), ragged=False)
    nothing = _run(_bert(recipe, layers), ragged=False, recipes=False)
    assert alone['census'] == nothing['census'] and alone['calls'] == nothing['calls'] == 0
    _same(alone, nothing)


@pytest.mark.parametrize('recipe', RECIPES)
def test_whole_tiles_do_not_notice_the_switch_cpu(recipe):
    layers = 1
    inputs = _inputs(3, 64)
    off = _run(_bert(recipe, layers), inputs=inputs, recipes=False)
    on = _run(_bert(recipe, layers), inputs=inputs)
    assert on['census'] == off['census'] == _expected_census(recipe, layers, 3, 64) and on['calls'] == off['calls'] == 6
    _same(on, off)


@pytest.mark.parametrize('recipe', RECIPES)
def test_ragged_forward_equals_the_callers_padding_cpu(recipe):
    """[3,50] with the switches on equals, on [:, :50], the default route on the batch padded by the caller to [3,64] with
    attention_mask = 0 on the pads: the embedding block, site x and the hidden state of every layer, with their indices"""
    from tests._ragged_recipes_twin import RaggedRecipesTwin
    layers = 2
    ids, am = _inputs()
    ids_p = torch.cat([ids, torch.full((B, 64 - T), 1000)], 1)
    am_p = torch.cat([am, torch.zeros(B, 64 - T, dtype=torch.long)], 1)
    padded, calls_p, census, _ = _twin_chained(_bert(recipe, layers), RaggedRecipesTwin(), ids_p, am_p)
    assert census == _expected_census(recipe, layers, B, 64) and calls_p == layers * 6
    with _switches(INT8_RAGGED=True, INT8_RAGGED_RECIPES=True):
        ragged, calls, census, _ = _twin_chained(_bert(recipe, layers), RaggedRecipesTwin(), ids, am)
    assert census == _ragged_census(recipe, layers, B, T) and calls == layers * 6
    for where in ('emb', 'attn', 'h'):
        for l, (r, p) in enumerate(zip(ragged[where], padded[where])):
            assert r[0].shape == S and torch.equal(r[0], p[0][:, :T]), f'{where} {l}: values differ'
            assert (r[1] is None) == (p[1] is None) and (r[1] is None or torch.equal(r[1], p[1][:, :T])), f'{where} {l}: indices'
    assert all(i is not None for _, i in ragged['h'])


@pytest.mark.parametrize('switch,recipe,entry', ROUTES)
def test_each_route_built_on_ffn1_takes_its_entry_at_the_ragged_shape_cpu(switch, recipe, entry):
    layers = 2
    off = _run(_bert(recipe, layers))
    on = _run(_bert(recipe, layers), **{switch: True})
    new = [c for c in on['census'] if c[0] == entry]
    assert entry not in _names(off)
    assert len(new) == (layers if switch == 'INT8_PLANE_TAILS' else 2 * layers) and all(c[1] == S for c in new), new
    ffn1 = [c for c in on['census'] if c[0] == FFN1[recipe]]
    assert ffn1 == [(FFN1[recipe], S, 4 * D, False, True)] * layers and on['calls'] == layers * 6
    assert HILO not in _names(on)                                # W8A16: the planes the tail wrote are read, nothing re-derives them
    _same(on, off)
    if switch != 'INT8_PLANE_TAILS':
        # site x never exists as fp32; the layer outputs carry flags, and layer 1's first tail read layer 0's indices
        assert all(f is not None and not bool(f.any()) for _, _, f in on['h'])
        assert [c[-5 if entry.endswith('pres') else 3] for c in new] == ['f32', 'planes' if entry.endswith('pres') else 'idx',
                                                                       'idx', 'planes' if entry.endswith('pres') else 'idx']
    # without INT8_RAGGED_RECIPES the route declines for the whole layer, as the parent does
    declined = _run(_bert(recipe, layers), recipes=False, **{switch: True})
    base = _run(_bert(recipe, layers), recipes=False)
    if switch == 'INT8_PLANE_TAILS':
        assert FFN1[recipe] not in _names(declined)               # (the tail takes any row count: its planes are never read)
    else:
        assert entry not in _names(declined) and declined['census'] == base['census']
    _same(declined, base)


@pytest.mark.parametrize('switch,recipe,entry', ROUTES)
def test_a_nan_row_goes_through_a_layer_as_it_does_today_cpu(switch, recipe, entry):
    """one QLayer on a tagged hidden state (values, int8 indices, row flags) whose row (0, 5) is NaN, at [3,50]: with the route's
    switch on the same output as with it off -- the row NaN as a whole, every other row bit-equal"""
    from quantization import _hip, provenance
    from tests._ragged_recipes_twin import RaggedRecipesTwin
    model = _bert(recipe, 2)
    ids, am = _inputs()
    mask = (1.0 - am[:, None, None, :].float()) * -10000.0
    be = RaggedRecipesTwin()
    prev = _hip.set_backend(be)
    outs = {}
    try:
        with _switches(INT8_RAGGED=True, INT8_RAGGED_RECIPES=True), torch.no_grad():
            h0 = model.layers[0](model.embeddings(ids), mask)
            q, idx = provenance.of(h0)
            assert idx is not None
            h = h0.clone()
            h[0, 5] = float('nan')
            flags = torch.zeros(h.shape[:-1], dtype=torch.uint8)
            flags[0, 5] = 1
            provenance.tag(h, q, idx.clone(), row_nan=flags)      # (the index bytes of a NaN row mean nothing)
            for on in (False, True):
                del be.census[:]
                with _switches(**{switch: on}):
                    y = model.layers[1](h, mask)
                outs[on] = (y.clone(), provenance.indices_of(y), provenance.row_nan_of(y), list(be.census))
    finally:
        _hip.set_backend(prev)
    assert entry in [c[0] for c in outs[True][3]] and entry not in [c[0] for c in outs[False][3]]
    assert all(c[1] == S for c in outs[True][3] if c[0] == entry)
    y_off, y_on = outs[False][0], outs[True][0]
    nan_rows = torch.isnan(y_off).any(-1)
    assert torch.isnan(y_off[0, 5]).all() and bool(nan_rows[0, 5])
    assert torch.equal(torch.isnan(y_on), torch.isnan(y_off))
    keep = ~nan_rows
    assert torch.equal(y_on[keep], y_off[keep]) and torch.equal(outs[True][1][keep], outs[False][1][keep])
    if outs[True][2] is not None:
        assert torch.equal(outs[True][2].bool(), nan_rows)


@pytest.mark.parametrize('head', [False, True], ids=['layered_head', 'int8_head'])
@pytest.mark.parametrize('recipe', RECIPES)
def test_packed_forward_equals_the_padded_one_on_owned_rows_cpu(recipe, head):
    from tests.test_bert_packed_route import _batch
    layers = 2
    lengths = (50, 37, 12)                                    # 99 packed rows against [3,50]
    inputs = _batch(lengths)
    padded = _run(_bert(recipe, layers), inputs=inputs, INT8_HEAD=head)
    packed = _run(_bert(recipe, layers), inputs=inputs, packed=True, INT8_HEAD=head)
    M = sum(lengths)
    ffn1 = [c for c in packed['census'] if c[0] == FFN1[recipe]]
    assert ffn1 == [(FFN1[recipe], (1, M, D), 4 * D, False, True)] * layers and packed['calls'] - 2 * head == layers * 6
    assert _names(packed).count(VARLEN) == layers and _names(padded).count(RAGGED) == layers
    s = packed['seq_start'].tolist()
    for l, (pk, pd) in enumerate(zip(packed['h'], padded['h'])):
        assert pk[0].shape == (1, M, D)
        for b, n in enumerate(lengths):
            assert torch.equal(pk[0][0, s[b]:s[b + 1]], pd[0][b, :n]), f'layer {l}, sequence {b}: values differ'
            assert torch.equal(pk[1][0, s[b]:s[b + 1]], pd[1][b, :n]), f'layer {l}, sequence {b}: indices differ'
    assert torch.equal(packed['logits'], padded['logits'])
    if head:
        # pooler (through the row table of the packed batch) and classifier: the skinny integer Linears, none layered
        assert all(c[0].endswith('_skinny') for c in packed['census'][-2:] + padded['census'][-2:])
