"""options.INT8_RAGGED_RECIPES on the GPU: a 2-layer BERT-base under the W8A16 recipe {'x': 16, 'h': 16, 'y': 16} and the PEG
recipes {'x', 'h', 'y'}: 'ng6' / 'ngp6' stays on the integer route at token counts that are no multiple of 64 ([3,50]: M = 150,
[2,37]: M = 74) -- FFN1 as tq_linear_i16x8_fwd / tq_linear_i8_cls_fwd over 64 * ceil(M / 64) rows -- and

* the embedding block's output and both hidden states of every layer (site x and the layer's output), with the int8 indices
  they carry, are `torch.equal` to the exact CPU twin (tests/_ragged_recipes_twin.RaggedRecipesTwin), eager and as a hipGraph
  replay, with the same launches on both sides and every row operand of a padded launch read in place;
* the [3,50] forward equals, on [:, :50], the default route on the batch padded by the caller to [3,64];
* `forward_packed` equals the padded forward on the rows its sequences own, also replayed with other lengths;
* with options.INT8_HEAD the logits equal the twin's, the STS-B head recipe (16-bit site z, 'P', 'C') included.

Models, calibration, capture, census and comparison are those of tests/test_bert_exact_route.py and its followers."""
import pytest
import torch

from tests.test_bert_exact_route import (RECIPES as EXACT_RECIPES, _Capture, _calibrate, _expected_census, _hip_census, _host, _ids,
                                         _twin_of)
from tests.test_bert_packed_route import _PackedCapture, _assert_valid_rows_equal, _batch

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]

LAYERS, D = 2, 768
ENCODER16 = {'x': 16, 'h': 16, 'y': 16}
RECIPES = dict({k: EXACT_RECIPES[k] for k in ('mp16', 'peg', 'peg_permuted')},
               head=dict(ENCODER16, **{'z%d' % (LAYERS - 1): 16, 'P': 16, 'C': 16}))      # the STS-B head recipe
ENCODER_RECIPES = ['mp16', 'peg', 'peg_permuted']
FFN1 = {'mp16': 'linear_i16x8', 'head': 'linear_i16x8', 'peg': 'linear_i8_cls', 'peg_permuted': 'linear_i8_cls'}
RAGGED, VARLEN = 'attention_i8_ragged', 'attention_i8_varlen'
SHAPES = [(3, 50), (2, 37)]
_GPU = {}


def _gpu_model(recipe):
    """2 layers of BERT-base, calibrated once per recipe on the default route at a whole-tile shape"""
    from quantization import options
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    if recipe not in _GPU:
        assert not (options.INT8_RAGGED or options.INT8_RAGGED_RECIPES or options.INT8_HEAD or options.INT8_PLANE_TAILS)
        permuted = recipe == 'peg_permuted'
        qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
                  weight_range_method=RangeEstimators.current_minmax,
                  act_range_method=RangeEstimators.current_minmax if permuted else RangeEstimators.running_minmax)
        model, _ = build_bert_base(seed=1000, num_layers=LAYERS, **qp)
        apply_quant_dict(model, RECIPES[recipe])
        _GPU[recipe] = _calibrate(model.to('cuda').eval(), recipe, [_ids(10, 4, 64).cuda(), _ids(11, 4, 64).cuda()])
    return _GPU[recipe]


def _mask(B, T):
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return am


def _switch_on(monkeypatch, **more):
    from quantization import options
    for k, v in dict(INT8_RAGGED=True, INT8_RAGGED_RECIPES=True, **more).items():
        monkeypatch.setattr(options, k, v)


def _log(monkeypatch):
    """launches of the HIP backend in the form the twin records its own (both ragged cores included), and what
    `_rows_operand` did on the way: True per operand it handed back in place"""
    from quantization import _hip
    log = _hip_census(monkeypatch)
    for name in (RAGGED, VARLEN):
        orig = getattr(_hip.HipBackend, name)

        def counted(self, *a, _o=orig, _n=name, **k):
            log.append((_n, tuple(a[0].shape)))
            return _o(self, *a, **k)
        monkeypatch.setattr(_hip.HipBackend, name, counted)
    in_place = []
    orig_op = _hip.HipBackend._rows_operand

    def operand(self, x, M_pad):
        out = orig_op(self, x, M_pad)
        in_place.append(out is x)
        return out
    monkeypatch.setattr(_hip.HipBackend, '_rows_operand', operand)
    return log, in_place


def _ragged_census(recipe, B, T, stair, core=RAGGED):
    r = 'mp16' if recipe == 'head' else recipe
    return [((core,) + e[1:]) if e[0] == 'attention_i8' else e for e in _expected_census(r, LAYERS, B, T, stair=stair)]


def _twin_backend():
    from quantization import _hip
    from tests._ragged_recipes_twin import RaggedRecipesTwin
    return RaggedRecipesTwin(rules=_hip.backend())


def _twin_run(twin, be, call, capture=_Capture):
    """call(twin) under the CPU backend `be` -> (capture record on the host, integer Linears launched, census, logits)"""
    from quantization import _hip
    from quantization.autoquant_utils import INT8_STATS
    prev = _hip.set_backend(be)
    try:
        del be.census[:]
        k0 = INT8_STATS['kernel_calls']
        with torch.no_grad(), capture(twin) as cap:
            logits = call(twin)
        return _host(cap.runs[-1]), INT8_STATS['kernel_calls'] - k0, list(be.census), logits.detach().cpu().clone()
    finally:
        _hip.set_backend(prev)


def _assert_tables_accepted(model):
    """premise of a zero-tolerance comparison behind a GELU launch (tests/test_bert_exact_route.py): every feed-forward launch
    evaluates the correctly rounded GELU through an accepted staircase table"""
    from quantization.autoquant_utils import int8_stair_status
    status = int8_stair_status(model)
    for l in range(LAYERS):
        tables = status.get(f'layers.{l}.intermediate.0', {})
        assert tables and all(tables.values()), f'layer {l}: GELU table declined or absent ({tables}): no exact statement possible'


def _equal_records(got, want, what, rows=None):
    """'emb', 'attn' (site x), 'h' of two capture records: values as bit patterns and the int8 indices they carry (site x of the
    W8A16 recipe carries none: its index has 16 bits); rows: compare [:, :rows] of `want`"""
    cut = (lambda t: t) if rows is None else (lambda t: t[:, :rows])
    for where in ('emb', 'attn', 'h'):
        assert len(got[where]) == len(want[where]) == (1 if where == 'emb' else LAYERS), (what, where)
        for l, (g, w) in enumerate(zip(got[where], want[where])):
            at = f'{what}: {where} {l}'
            assert g[0].shape == cut(w[0]).shape, at
            assert torch.equal(g[0].view(torch.int32), cut(w[0]).contiguous().view(torch.int32)), \
                f'{at}: values differ ({int((g[0] != cut(w[0])).sum())} elements)'
            assert (g[1] is None) == (w[1] is None), f'{at}: one side carries no int8 indices'
            assert g[1] is None or torch.equal(g[1], cut(w[1])), f'{at}: int8 index records differ'
    assert all(i is not None for _, i in got['h'] + got['emb'])


@pytest.mark.parametrize('B,T', SHAPES)
@pytest.mark.parametrize('recipe', ENCODER_RECIPES)
def test_route_equals_the_twin_eager_and_replayed(recipe, B, T, monkeypatch):
    from quantization import options
    from quantization.autoquant_utils import INT8_STATS
    from quantization.graphs import GraphedForward
    assert options.INT8_LINEAR == 'auto' and options.INT8_RAGGED_RECIPES is False
    model = _gpu_model(recipe)
    _switch_on(monkeypatch)
    ids, am = _ids(3, B, T), _mask(B, T)
    args = (ids.cuda(), am.cuda())
    twin = _twin_of(model)
    log, in_place = _log(monkeypatch)
    with torch.no_grad(), _Capture(model) as cap:
        k0, fb0 = INT8_STATS['kernel_calls'], INT8_STATS['unsigned_weight_fallbacks']
        model(*args)
        torch.cuda.synchronize()
        calls = INT8_STATS['kernel_calls'] - k0
        assert INT8_STATS['unsigned_weight_fallbacks'] == fb0
        census, gpu = list(log), _host(cap.runs[-1])
        g = GraphedForward(model, *args)
        static = cap.runs[-1]                                   # the capture pass: the graph's own tensors
        g(*args)
        torch.cuda.synchronize()
        replay = _host(static)
    _assert_tables_accepted(model)
    be = _twin_backend()
    chained, twin_calls, twin_census, _ = _twin_run(twin, be, lambda m: m(ids, am))
    assert calls == twin_calls == LAYERS * 6, (calls, twin_calls)             # no Linear is layered
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    stair = [e[-1] for e in census if e[0] == FFN1[recipe]]
    assert len(stair) == LAYERS and len(set(stair)) == 1 and census == _ragged_census(recipe, B, T, stair[0]), census
    assert [e for e in census if e[0] == FFN1[recipe]] == [(FFN1[recipe], (B, T, D), 4 * D, False, stair[0])] * LAYERS
    # every row operand of a padded launch came from the backend's own allocator: none was copied (the class-order gather of
    # 'ngp6' writes straight into such a buffer)
    assert in_place and all(in_place), f'{in_place.count(False)} of {len(in_place)} row operands were copied'
    _equal_records(gpu, chained, f'{recipe} [{B},{T}] eager against the twin')
    _equal_records(replay, chained, f'{recipe} [{B},{T}] hipGraph replay against the twin')
    assert all(torch.isfinite(h).all() for h, _ in gpu['h'])


@pytest.mark.parametrize('recipe', ENCODER_RECIPES)
def test_ragged_forward_equals_the_default_route_on_the_callers_padding(recipe, monkeypatch):
    """no twin: [3,50] with the switches on == [:, :50] of the default route on the same batch padded to [3,64] with
    attention_mask = 0 on the pads"""
    from quantization import options
    B, T = 3, 50
    model = _gpu_model(recipe)
    ids, am = _ids(3, B, T), _mask(B, T)
    ids_p = torch.cat([ids, torch.full((B, 64 - T), 1000)], 1)
    am_p = torch.cat([am, torch.zeros(B, 64 - T, dtype=torch.long)], 1)
    assert not (options.INT8_RAGGED or options.INT8_RAGGED_RECIPES)
    log, _ = _log(monkeypatch)
    with torch.no_grad(), _Capture(model) as cap:
        model(ids_p.cuda(), am_p.cuda())
        torch.cuda.synchronize()
        padded, p_census = _host(cap.runs[-1]), list(log)
        del log[:]
        _switch_on(monkeypatch)
        model(ids.cuda(), am.cuda())
        torch.cuda.synchronize()
        ragged, census = _host(cap.runs[-1]), list(log)
    stair = [e[-1] for e in census if e[0] == FFN1[recipe]]
    assert len(stair) == LAYERS and census == _ragged_census(recipe, B, T, stair[0])
    assert [e[0] for e in p_census] == [e[0] if e[0] != RAGGED else 'attention_i8' for e in census]
    _equal_records(ragged, padded, f'{recipe}: [3,50] against [3,64][:, :50]', rows=T)


PACKED = ((50, 37, 12), (40, 49, 10))        # lengths, and other lengths of the same B, the same M = 99 and no longer sequence


@pytest.mark.parametrize('recipe', ENCODER_RECIPES)
def test_packed_forward_equals_the_padded_one_on_valid_rows_replayed_with_other_lengths(recipe, monkeypatch):
    from harness.bert import PackedForward, pack_batch
    from quantization.autoquant_utils import INT8_STATS
    from quantization.graphs import GraphedForward
    lengths, other = PACKED
    model = _gpu_model(recipe)
    _switch_on(monkeypatch)
    (ids, am), (o_ids_b, o_am) = _batch(lengths), _batch(other, seed=4)
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    o_ids, o_pos, o_start, o_max = pack_batch(o_ids_b, o_am)
    M = p_ids.shape[1]
    assert o_ids.shape == p_ids.shape and o_max <= max_len and M % 64 != 0
    args, o_args = tuple(t.cuda() for t in (p_ids, p_pos, seq_start)), tuple(t.cuda() for t in (o_ids, o_pos, o_start))
    log, in_place = _log(monkeypatch)
    with torch.no_grad(), _PackedCapture(model) as cap:
        model(ids.cuda(), am.cuda())
        padded = _host(cap.runs[-1])
        model(o_ids_b.cuda(), o_am.cuda())
        o_padded = _host(cap.runs[-1])
        del log[:], in_place[:]
        k0 = INT8_STATS['kernel_calls']
        logits = model.forward_packed(*args, max_len).clone()
        torch.cuda.synchronize()
        calls, census, packed = INT8_STATS['kernel_calls'] - k0, list(log), _host(cap.runs[-1])
        g = GraphedForward(PackedForward(model, max_len), *args)
        static = cap.runs[-1]                                   # the capture pass: the graph's own tensors
        r_logits = g(*args).clone()
        torch.cuda.synchronize()
        replay = _host(static)
        ro_logits = g(*o_args).clone()                          # other lengths copied into the static inputs
        torch.cuda.synchronize()
        o_replay = _host(static)
    stair = [e[-1] for e in census if e[0] == FFN1[recipe]]
    assert calls == LAYERS * 6 and len(stair) == LAYERS and census == _ragged_census(recipe, 1, M, stair[0], core=VARLEN), census
    assert in_place and all(in_place)
    _assert_valid_rows_equal(packed, padded, seq_start, 'eager: ')
    _assert_valid_rows_equal(replay, padded, seq_start, 'hipGraph replay: ')
    _assert_valid_rows_equal(o_replay, o_padded, o_start, 'hipGraph replay with other lengths: ')
    # (the head is layered here: its logits are outside the exact statement; with options.INT8_HEAD they are in it, below)
    assert torch.equal(r_logits, logits) and logits.shape == (len(lengths), 2) and torch.isfinite(logits).all()
    assert torch.isfinite(ro_logits).all() and not torch.equal(ro_logits, logits)


@pytest.mark.parametrize('recipe', ENCODER_RECIPES + ['head'])
def test_with_the_integer_head_the_logits_equal_the_twin(recipe, monkeypatch):
    """options.INT8_HEAD: pooler and classifier are the skinny integer Linears, so the logits are exact too -- through `forward`
    at [3,50] and through `forward_packed`.  'head': site z of the last layer, 'P' and 'C' at 16 bits (the STS-B recipe), with
    options.INT8_PLANE_TAILS: the last feed-forward tail writes the planes of the hidden state at M = 150 / 99 rows, the pooler
    reads their first-token rows."""
    from harness.bert import pack_batch
    from quantization.autoquant_utils import INT8_STATS
    B, T = 3, 50
    model = _gpu_model(recipe)
    _switch_on(monkeypatch, INT8_HEAD=True, INT8_PLANE_TAILS=recipe == 'head')
    ids, am = _batch((50, 37, 12))
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    twin = _twin_of(model)
    log, _ = _log(monkeypatch)
    with torch.no_grad():
        k0, fb0 = INT8_STATS['kernel_calls'], INT8_STATS['unsigned_weight_fallbacks']
        logits = model(ids.cuda(), am.cuda()).cpu().clone()
        torch.cuda.synchronize()
        calls, census = INT8_STATS['kernel_calls'] - k0, list(log)
        k0 = INT8_STATS['kernel_calls']
        packed = model.forward_packed(p_ids.cuda(), p_pos.cuda(), seq_start.cuda(), max_len).cpu().clone()
        torch.cuda.synchronize()
        p_calls = INT8_STATS['kernel_calls'] - k0
        assert INT8_STATS['unsigned_weight_fallbacks'] == fb0
    _assert_tables_accepted(model)
    assert calls == p_calls == LAYERS * 6 + 2                                # the encoder's Linears, pooler, classifier: none layered
    assert [e for e in census if e[0] == FFN1[recipe]] and (B, T) == tuple(ids.shape)
    be = _twin_backend()
    _, t_calls, _, t_logits = _twin_run(twin, be, lambda m: m(ids, am))
    _, tp_calls, _, tp_logits = _twin_run(twin, be, lambda m: m.forward_packed(p_ids, p_pos, seq_start, max_len), capture=_PackedCapture)
    assert t_calls == tp_calls == calls
    assert torch.equal(logits, t_logits), f'logits differ from the twin\'s: {(logits - t_logits).abs().max()}'
    assert torch.equal(packed, tp_logits), f'packed logits differ from the twin\'s: {(packed - tp_logits).abs().max()}'
    assert torch.equal(packed, logits) and logits.shape == (B, 2) and torch.isfinite(logits).all()
