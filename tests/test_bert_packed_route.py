"""BERT on the integer route over PACKED variable-length batches (no pad tokens): `harness.bert.pack_batch`,
`QBertForSequenceClassification.forward_packed`, `fused.PackedSequences` and the variable-length attention core.

The statement: Linears and LayerNorm tails are row by row, and a pad key contributes exactly nothing to the attention core --
so the packed forward equals, on the valid rows and with `torch.equal`, the forward of the same batch padded to its longest
sequence with its attention mask (options.INT8_RAGGED, the parent's best).

CPU (tests/_packed_twin.PackedTwin): that equality at lengths (50, 37, 12) for the embedding output, every attention block, every
hidden state with its int8 indices and the logits; the launches the packed forward makes; the scatter / gather fall-back where
the option is off or the backend has no variable-length core; `pack_batch`'s refusals.  GPU: the packed forward equals the
PackedTwin's under the comparison rule of tests/test_bert_exact_route.py (`_compare`, declined-staircase clause included), eager
and as a hipGraph replay, and a replay with OTHER lengths of the same B and M equals the eager forward of that batch."""
import pytest
import torch

from tests import test_bert_exact_route as exact
from tests.test_bert_exact_route import _Capture, _compare, _hip_census, _host, _ids, _twin_of
from tests.test_bert_ragged_route import LAYERS, _cpu_model, _gpu_model, _ragged_census

pytestmark = pytest.mark.default_route        # statements about the product's default route with one more switch on

VARLEN, RAGGED = 'attention_i8_varlen', 'attention_i8_ragged'


def _batch(lengths, seed=3):
    """[B, max(lengths)] ids with pad id 1000 behind every sequence, and the attention mask"""
    B, T = len(lengths), max(lengths)
    ids = _ids(seed, B, T)
    am = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lengths):
        am[b, :n] = 1
        ids[b, n:] = 1000
    return ids, am


def _packed_census(layers, M, stair=True):
    """the ragged route's launches over [1, M] with the variable-length core in place of the ragged one"""
    return [((VARLEN,) + e[1:]) if e[0] == RAGGED else e for e in _ragged_census(layers, 1, M, stair=stair)]


class _PackedCapture(_Capture):
    """_Capture whose records also start at `forward_packed`"""

    def __enter__(self):
        super().__enter__()
        m, fp = self.model, type(self.model).forward_packed

        def whole(*a, _m=m, **k):
            self.runs.append({})
            return fp(_m, *a, **k)
        m.forward_packed = whole
        return self

    def __exit__(self, *exc):
        del self.model.forward_packed
        return super().__exit__(*exc)


def _twin_run(twin, be, call):
    """call(twin) under backend `be` -> (capture record on the host, integer Linears launched, census, logits)"""
    from quantization import _hip
    from quantization.autoquant_utils import INT8_STATS
    prev = _hip.set_backend(be)
    try:
        del be.census[:]
        k0 = INT8_STATS['kernel_calls']
        with torch.no_grad(), _PackedCapture(twin) as cap:
            logits = call(twin)
        return _host(cap.runs[-1]), INT8_STATS['kernel_calls'] - k0, list(be.census), logits.detach().cpu().clone()
    finally:
        _hip.set_backend(prev)


def _assert_valid_rows_equal(packed, padded, seq_start, what=''):
    """capture records: packed [1, M, d] against padded [B, T, d], sequence by sequence, values and int8 indices"""
    s = [int(v) for v in seq_start]
    for where in ('emb', 'attn', 'h'):
        assert len(packed[where]) == len(padded[where]) > 0
        for l, (p, q) in enumerate(zip(packed[where], padded[where])):
            assert (p[1] is None) == (q[1] is None), f'{what}{where} {l}: one side carries no int8 indices'
            for b in range(len(s) - 1):
                n = s[b + 1] - s[b]
                assert torch.equal(p[0][0, s[b]:s[b + 1]], q[0][b, :n]), f'{what}{where} {l}, sequence {b}: values differ'
                assert p[1] is None or torch.equal(p[1][0, s[b]:s[b + 1]], q[1][b, :n]), f'{what}{where} {l}, sequence {b}: indices differ'


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
LENGTHS = (50, 37, 12)


def test_pack_batch_cpu():
    from harness.bert import pack_batch
    ids, am = _batch(LENGTHS)
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    assert p_ids.shape == p_pos.shape == (1, 99) and p_ids.dtype == p_pos.dtype == torch.int64
    assert seq_start.dtype == torch.int32 and seq_start.tolist() == [0, 50, 87, 99] and max_len == 50
    assert torch.equal(p_ids[0, 50:87], ids[1, :37]) and p_pos[0].tolist() == list(range(50)) + list(range(37)) + list(range(12))
    hole = am.clone()
    hole[0, 10] = 0                                            # not ones followed by zeros
    with pytest.raises(ValueError):
        pack_batch(ids, hole)
    front = am.clone()
    front[1] = torch.cat([torch.zeros(13, dtype=torch.long), torch.ones(37, dtype=torch.long)])     # left padding
    with pytest.raises(ValueError):
        pack_batch(ids, front)
    empty = am.clone()
    empty[2] = 0
    with pytest.raises(ValueError):
        pack_batch(ids, empty)
    with pytest.raises(ValueError):
        pack_batch(torch.zeros(1, 513, dtype=torch.long), torch.ones(1, 513, dtype=torch.long))
    assert pack_batch(torch.zeros(1, 512, dtype=torch.long), torch.ones(1, 512, dtype=torch.long))[3] == 512


def test_packed_forward_equals_the_padded_forward_cpu(monkeypatch):
    """option on, PackedTwin: every captured tensor and the logits, on the valid rows; the launches are the ragged route's with
    the variable-length core over M = 99 rows"""
    from harness.bert import pack_batch
    from quantization import options
    from quantization.autoquant_utils import INT8_STATS
    from tests._packed_twin import PackedTwin
    ids, am = _batch(LENGTHS)
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    _cpu_model()                                              # (calibrated under the default, before the switch)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    fb0 = INT8_STATS['unsigned_weight_fallbacks']
    padded, calls_p, census_p, logits_p = _twin_run(_cpu_model(), PackedTwin(), lambda m: m(ids, am))
    assert census_p == _ragged_census(2, 3, 50), census_p
    packed, calls, census, logits = _twin_run(_cpu_model(), PackedTwin(), lambda m: m.forward_packed(p_ids, p_pos, seq_start, max_len))
    assert census == _packed_census(2, 99), census
    assert calls == calls_p == 2 * 6 and INT8_STATS['unsigned_weight_fallbacks'] == fb0
    assert packed['h'][-1][0].shape == (1, 99, 768) and all(i is not None for _, i in packed['emb'] + packed['attn'] + packed['h'])
    _assert_valid_rows_equal(packed, padded, seq_start)
    assert logits.shape == (3, 2) and torch.equal(logits, logits_p)


@pytest.mark.parametrize('config', ['option-off', 'backend-without-the-core'])
def test_packed_forward_falls_back_to_scatter_and_gather_cpu(config, monkeypatch):
    """where the helpers decline -- the option off, or a backend without `attention_i8_varlen` -- each attention block runs the
    existing code on the batch scattered to [3, 50, d] and gathers the valid rows back: equal to the padded forward of the same
    configuration, and no variable-length launch anywhere"""
    from harness.bert import pack_batch
    from quantization import options
    from tests._exact_backend import ExactBackend
    from tests._packed_twin import PackedTwin
    ids, am = _batch(LENGTHS)
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    _cpu_model()                                              # (calibrated under the default, before the switch)
    if config == 'option-off':
        assert options.INT8_RAGGED is False
        make = PackedTwin
    else:
        monkeypatch.setattr(options, 'INT8_RAGGED', True)
        assert not hasattr(ExactBackend, VARLEN)
        make = ExactBackend
    padded, _, census_p, logits_p = _twin_run(_cpu_model(), make(), lambda m: m(ids, am))
    packed, _, census, logits = _twin_run(_cpu_model(), make(), lambda m: m.forward_packed(p_ids, p_pos, seq_start, max_len))
    assert not [e for e in census + census_p if e[0].startswith('attention_i8')]
    assert [e[0] for e in census] == [e[0] for e in census_p]
    _assert_valid_rows_equal(packed, padded, seq_start, what=config + ': ')
    assert torch.equal(logits, logits_p)


def test_packed_forward_is_inference_only_cpu(monkeypatch):
    from harness.bert import pack_batch
    from quantization import _hip, options
    from tests._packed_twin import PackedTwin
    model = _cpu_model()
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    args = pack_batch(*_batch(LENGTHS))
    prev = _hip.set_backend(PackedTwin())
    try:
        with pytest.raises(RuntimeError, match='inference only'):
            model.forward_packed(*args)                        # autograd is on
        model.layers[1].attention_self.context_act_quantizer.activation_quantizer.estimate_ranges()
        with torch.no_grad(), pytest.raises(RuntimeError, match='estimating'):
            model.forward_packed(*args)
    finally:
        _hip.set_backend(prev)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def _census_with_varlen(monkeypatch):
    from quantization import _hip
    log = _hip_census(monkeypatch)
    orig = _hip.HipBackend.attention_i8_varlen

    def counted(self, *a, **k):
        log.append((VARLEN, tuple(a[0].shape)))
        return orig(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, VARLEN, counted)
    return log


def _equal_records(a, b, what):
    for where in ('emb', 'attn', 'h'):
        for l, (r, e) in enumerate(zip(a[where], b[where])):
            assert torch.equal(r[0], e[0]) and r[1] is not None and e[1] is not None and torch.equal(r[1], e[1]), f'{what}: {where} {l}'


# (lengths, other lengths of the same B, the same M and no sequence longer than max(lengths))
GPU_CASES = [((50, 37, 12), (40, 49, 10)), ((72, 64, 5, 1, 33, 72, 20, 9), (60, 72, 10, 3, 30, 70, 22, 9))]


@pytest.mark.gpu
@pytest.mark.parametrize('lengths,other', GPU_CASES, ids=['B3-M99', 'B8-M276'])
def test_packed_route_equals_the_twin(lengths, other, monkeypatch):
    from harness.bert import PackedForward, pack_batch
    from quantization import _hip, options
    from quantization.autoquant_utils import INT8_STATS
    from quantization.fused import PackedSequences
    from quantization.graphs import GraphedForward
    from tests._packed_twin import PackedTwin
    assert options.INT8_LINEAR == 'auto' and sum(lengths) == sum(other) and len(lengths) == len(other) and max(other) <= max(lengths)
    model = _gpu_model()
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    p_ids, p_pos, seq_start, max_len = pack_batch(*_batch(lengths))
    o_ids, o_pos, o_start, o_max = pack_batch(*_batch(other, seed=4))
    M = p_ids.shape[1]
    assert o_ids.shape == p_ids.shape and o_max <= max_len
    args, o_args = tuple(t.cuda() for t in (p_ids, p_pos, seq_start)), tuple(t.cuda() for t in (o_ids, o_pos, o_start))
    twin = _twin_of(model)
    log = _census_with_varlen(monkeypatch)
    with torch.no_grad(), _PackedCapture(model) as cap:
        k0, fb0 = INT8_STATS['kernel_calls'], INT8_STATS['unsigned_weight_fallbacks']
        logits = model.forward_packed(*args, max_len).clone()
        torch.cuda.synchronize()
        calls = INT8_STATS['kernel_calls'] - k0
        assert INT8_STATS['unsigned_weight_fallbacks'] == fb0
        census = list(log)
        gpu = _host(cap.runs[-1])
        o_logits = model.forward_packed(*o_args, max_len).clone()           # the other batch, eager, under the SAME max_len
        o_gpu = _host(cap.runs[-1])
        g = GraphedForward(PackedForward(model, max_len), *args)
        static = cap.runs[-1]                                   # the capture pass: the graph's own tensors
        r_logits = g(*args).clone()
        torch.cuda.synchronize()
        replay = _host(static)
        ro_logits = g(*o_args).clone()                          # other lengths copied into the static inputs
        torch.cuda.synchronize()
        o_replay = _host(static)
    _equal_records(replay, gpu, 'hipGraph replay differs from the eager forward')
    _equal_records(o_replay, o_gpu, 'hipGraph replay with other lengths differs from the eager forward of that batch')
    assert torch.equal(r_logits, logits) and torch.equal(ro_logits, o_logits) and not torch.equal(o_logits, logits)
    assert logits.shape == (len(lengths), 2) and torch.isfinite(logits).all()

    be = PackedTwin(rules=_hip.backend())
    chained, twin_calls, twin_census, _ = _twin_run(twin, be, lambda m: m.forward_packed(p_ids, p_pos, seq_start, max_len))
    print(f'{lengths}: M = {M}, {len(census)} launches ({calls} integer Linears)')
    assert calls == twin_calls == LAYERS * 6, (calls, twin_calls)
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    stair = [e[-1] for e in census if e[0] == 'linear_i8' and e[2] == 3072]
    assert len(stair) == LAYERS and len(set(stair)) == 1 and census == _packed_census(LAYERS, M, stair=stair[0])
    # `_compare` re-runs single twin layers on the GPU's input where the chained run cannot serve: what it hands them as the mask
    # is, for a packed batch, the PackedSequences
    monkeypatch.setattr(exact, '_additive_mask', lambda am, B, T: PackedSequences(seq_start, max_len))
    for name, rec in (('eager', gpu), ('replay', replay)):
        out = _compare(f'packed {name} {lengths}', model, twin, be, rec, chained, None, LAYERS)
        assert all(torch.isfinite(h).all() for h, _ in rec['h'])
        print(name, out)
