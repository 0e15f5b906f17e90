"""The head of a PACKED batch on the integer route (options.INT8_RAGGED and options.INT8_HEAD): `forward_packed` runs the pooler
as a skinny integer Linear that reads the first token of sequence b -- row seq_start[b] of the [1, M, d] hidden state's int8
indices -- through a device row table (tq_linear_i16x8_skinny_fwd, x_rows = seq_start[:-1]), and the classifier follows it on
whichever skinny entry its input grid asks for.

The statement: the packed logits are `torch.equal` to those of the same batch padded to its longest sequence under the same
options, and to the exact CPU twin's (tests/_packed_twin.PackedTwin composed with tests/_skinny16_twin.Skinny16Twin); a
`PackedForward` graph replay with other lengths of the same B and M equals the eager call on those lengths; the same once with
the head's sites 'P' and 'C' at 16 bits; with INT8_HEAD off the packed logits are what they were."""
import copy

import pytest
import torch

from tests.test_bert_exact_route import _calibrate, _ids, _twin_of
from tests.test_bert_packed_route import _batch, _packed_census
from tests.test_bert_ragged_route import _ragged_census

pytestmark = pytest.mark.default_route        # statements about the product's default route with two more switches on

OLD, NEW = 'linear_i8_skinny', 'linear_i16x8_skinny'
LENGTHS, OTHER = (50, 33, 12), (41, 44, 10)          # the same B, the same M = 95, nothing longer than 50
RECIPES = {'w8a8': {}, 'head16': {'P': 16, 'C': 16}}
ACT_NONE, ACT_TANH = 0, 3


def _twin_backend(rules=None):
    from tests._packed_twin import PackedTwin
    from tests._skinny16_twin import Skinny16Twin

    class PackedHeadTwin(PackedTwin, Skinny16Twin):
        name = 'exact-twin-packed-head'
    return PackedHeadTwin(rules=rules)


def _model(recipe, layers, device):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=layers, **qp)
    apply_quant_dict(model, RECIPES[recipe])
    return model.to(device).eval()


def _head(recipe, B):
    """the head's launches on a packed batch, in call order: the pooler with a row table on the [M, 768] indices, then the
    classifier on the pooled [B, 768] tensor's indices / planes"""
    if recipe == 'w8a8':
        return [(NEW, B, 768, 768, ACT_TANH, (768, 1), False, True, True, 'idx', True), (OLD, B, 2, 768, ACT_NONE, (768, 1), True, True)]
    return [(NEW, B, 768, 768, ACT_TANH, (768, 1), False, True, True, 'planes', True),
            (NEW, B, 2, 768, ACT_NONE, (768, 1), True, False, True, 'y', True)]


def _split(census, B=len(LENGTHS)):
    """(the head's launches, the rest).  With both options on an encoder Linear of a ragged M <= 256 keeps the skinny plan
    (tests/test_bert_ragged_route.py::test_skinny_plan_keeps_precedence_where_both_options_apply_cpu): a skinny launch belongs to
    the head when it has one row per sequence."""
    head = [e for e in census if e[0] in (OLD, NEW) and e[1] == B]
    return head, [e for e in census if e not in head]


def _encoder_like(census, expected):
    """the encoder's census with both options on: `expected` with the attention-output Linear (768 -> 768, ragged M <= 256, the
    one encoder Linear that asks for either plan) on the old skinny entry, everything else in place"""
    want = [(OLD, e[1][0] * e[1][1], 768, 768, ACT_NONE, (768, 1), False, True)
            if e[0] == 'linear_i8' and e[2] == 768 and e[1][2] == 768 and (e[1][0] * e[1][1]) % 32 else e for e in expected]
    return census == want


def _run(model, be, call):
    """call(model) under backend `be` (None: the HIP backend), no grad -> (logits on the host, census)"""
    from quantization import _hip
    prev = _hip.set_backend(be) if be is not None else None
    try:
        if be is not None:
            del be.census[:]
        with torch.no_grad():
            logits = call(model)
        return logits.detach().cpu().clone(), [] if be is None else list(be.census)
    finally:
        if be is not None:
            _hip.set_backend(prev)


# ---- CPU: host logic ------------------------------------------------------------------------------------------------------------
_CPU = {}


def _cpu_model(recipe):
    from quantization import _hip, options
    if recipe not in _CPU:
        assert options.INT8_HEAD is False and options.INT8_RAGGED is False
        prev = _hip.set_backend(_twin_backend())
        try:
            _CPU[recipe] = _calibrate(_model(recipe, 2, 'cpu'), 'w8a8', [_ids(10, 2, 64)])
        finally:
            _hip.set_backend(prev)
    return copy.deepcopy(_CPU[recipe])


@pytest.mark.parametrize('recipe', list(RECIPES))
def test_packed_head_census_and_logits_cpu(recipe, monkeypatch):
    from harness.bert import pack_batch
    from quantization import options
    ids, am = _batch(LENGTHS)
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    B, M = len(LENGTHS), sum(LENGTHS)
    packed = lambda m: m.forward_packed(p_ids, p_pos, seq_start, max_len)
    _cpu_model(recipe)                                        # (calibrated under the default, before the switches)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    off_logits, off_census = _run(_cpu_model(recipe), _twin_backend(), packed)
    assert _split(off_census) == ([], _packed_census(2, M)), 'INT8_HEAD off: the layered head'
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    logits, census = _run(_cpu_model(recipe), _twin_backend(), packed)
    skinny, encoder = _split(census)
    assert _encoder_like(encoder, _packed_census(2, M)), encoder
    assert skinny == _head(recipe, B) and census[-2:] == skinny, skinny
    padded_logits, padded_census = _run(_cpu_model(recipe), _twin_backend(), lambda m: m(ids, am))
    p_skinny, p_encoder = _split(padded_census)
    assert _encoder_like(p_encoder, _ragged_census(2, B, max(LENGTHS))) and len(p_skinny) == 2
    assert p_skinny[0][1:6] == (B, 768, 768, ACT_TANH, (max(LENGTHS) * 768, 1))          # the first-token view of the padded batch
    assert logits.shape == (B, 2) and torch.equal(logits, padded_logits), 'packed logits differ from the padded forward\'s'
    # without the new method the packed head is the parent's: layered
    from tests._packed_twin import PackedTwin
    from tests._skinny_twin import SkinnyTwin

    class Parent(PackedTwin, SkinnyTwin):
        pass
    parent_logits, parent_census = _run(_cpu_model(recipe), Parent(), packed)
    assert _split(parent_census)[0] == [] and torch.equal(parent_logits, off_logits)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
_GPU = {}


def _gpu_model(recipe):
    from quantization import options
    if recipe not in _GPU:
        assert options.INT8_RAGGED is False and options.INT8_HEAD is False
        _GPU[recipe] = _calibrate(_model(recipe, 2, 'cuda'), 'w8a8', [_ids(10, 4, 64).cuda(), _ids(11, 4, 64).cuda()])
    return _GPU[recipe]


@pytest.mark.gpu
@pytest.mark.parametrize('recipe', list(RECIPES))
def test_packed_head_equals_the_padded_forward_and_the_twin(recipe, monkeypatch):
    from harness.bert import PackedForward, pack_batch
    from quantization import _hip, options
    from quantization.graphs import GraphedForward
    from tests._skinny16_twin import count_hip_launches
    assert options.INT8_LINEAR == 'auto' and options.INT8_HEAD is False and options.INT8_RAGGED is False
    assert sum(LENGTHS) == sum(OTHER) and len(LENGTHS) == len(OTHER) and max(OTHER) <= max(LENGTHS)
    model = _gpu_model(recipe)
    B = len(LENGTHS)
    ids, am = _batch(LENGTHS)
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    o_ids, o_pos, o_start, o_max = pack_batch(*_batch(OTHER, seed=4))
    args, o_args = tuple(t.cuda() for t in (p_ids, p_pos, seq_start)), tuple(t.cuda() for t in (o_ids, o_pos, o_start))
    packed = lambda m: m.forward_packed(*args, max_len)
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    before = _run(model, None, packed)[0]                     # INT8_HEAD never touched: the layered head
    twin = _twin_of(model)
    log = count_hip_launches(monkeypatch)
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    logits = _run(model, None, packed)[0]
    torch.cuda.synchronize()
    assert _split(log)[0] == _head(recipe, B) and log[-2:] == _head(recipe, B), log
    padded = _run(model, None, lambda m: m(ids.cuda(), am.cuda()))[0]
    assert torch.equal(logits, padded), f'packed logits differ from the padded forward\'s: {(logits - padded).abs().max()}'
    t_logits, t_census = _run(twin, _twin_backend(rules=_hip.backend()), lambda m: m.forward_packed(p_ids, p_pos, seq_start, max_len))
    assert _split(t_census)[0] == _head(recipe, B)
    assert torch.equal(logits, t_logits), f'packed logits differ from the twin\'s: {(logits - t_logits).abs().max()}'
    assert logits.shape == (B, 2) and torch.isfinite(logits).all()
    # a graph captured on LENGTHS, replayed on OTHER: the row table is read on the device
    o_logits = _run(model, None, lambda m: m.forward_packed(*o_args, max_len))[0]
    with torch.no_grad():
        g = GraphedForward(PackedForward(model, max_len), *args)
        r_logits = g(*args).cpu().clone()
        ro_logits = g(*o_args).cpu().clone()
        torch.cuda.synchronize()
    assert torch.equal(r_logits, logits), 'hipGraph replay differs from the eager forward'
    assert torch.equal(ro_logits, o_logits) and not torch.equal(o_logits, logits), \
        'hipGraph replay with other lengths differs from the eager forward of that batch'
    monkeypatch.setattr(options, 'INT8_HEAD', False)
    n = len(log)
    after = _run(model, None, packed)[0]
    assert len(log) == n and torch.equal(after, before), 'the packed logits changed after INT8_HEAD was switched on and off'
