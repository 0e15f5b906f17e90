"""Host logic of options.INT8_PLANE_TAILS, replayed on the CPU with the exact twin (tests/_planes_twin.PlanesTwin): which
LayerNorm tails take the new entry (`residual_layernorm_quant_planes`), who reads the planes they leave in the record of
their output (FFN1's 16-bit integer Linear; the pooler behind a 16-bit last hidden state under options.INT8_HEAD), and where the
route keeps today's launches.  The twin answers the new method with the tail chain the existing method is answered with, so
the route with the option on must give `torch.equal` hidden states and logits to the route with it off."""
import copy

import pytest
import torch

from oracle import tq_oracle as O
from tests.test_bert_exact_route import _calibrate, _expected_census, _ids

pytestmark = pytest.mark.default_route

LAYERS, B, T, D = 3, 2, 64, 768
S = (B, T, D)
ENCODER = {'x': 16, 'h': 16, 'y': 16}
RECIPES = {'mp16': ENCODER, 'head': dict(ENCODER, z2=16, P=16, C=16)}
NEW, HILO, TAIL, SKINNY16, SKINNY8 = ('residual_layernorm_quant_planes', 'quantize_hilo', 'residual_layernorm_quant',
                                      'linear_i16x8_skinny', 'linear_i8_skinny')
ACT_NONE, ACT_TANH = 0, 3
_MEMO = {}


def _bert(recipe='mp16'):
    """3-layer BERT calibrated on the twin with every switch at its default; a fresh deep copy per call"""
    from quantization import _hip
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests._planes_twin import PlanesTwin
    from tests.harness_bert import apply_quant_dict, build_bert_base
    if recipe not in _MEMO:
        qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
                  weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
        model, _ = build_bert_base(seed=1000, num_layers=LAYERS, **qp)
        apply_quant_dict(model, RECIPES[recipe])
        prev = _hip.set_backend(PlanesTwin())
        try:
            _MEMO[recipe] = _calibrate(model.eval(), 'mp16', [_ids(10, B, T)])
        finally:
            _hip.set_backend(prev)
    return copy.deepcopy(_MEMO[recipe])


def _inputs():
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return _ids(3, B, T), am


def _run(model, on, be=None, head=False, no_grad=True):
    """-> (the double, logits, hidden state after every layer, (planes, indices) each hidden state carried)"""
    from quantization import _hip, options, provenance
    from tests._planes_twin import PlanesTwin
    be = be or PlanesTwin()
    prev = _hip.set_backend(be)
    saved = options.INT8_PLANE_TAILS, options.INT8_HEAD
    options.INT8_PLANE_TAILS, options.INT8_HEAD = on, head
    try:
        ids, am = _inputs()
        outs, recs = [], []

        def wrap(L):
            f = type(L).forward

            def forward(h, m):
                y = f(L, h, m)
                outs.append(y)
                recs.append((provenance.planes_of(y), provenance.indices_of(y)))
                return y
            return forward
        for L in model.layers:
            L.forward = wrap(L)
        try:
            with (torch.no_grad() if no_grad else torch.enable_grad()):
                y = model(ids, am)
        finally:
            for L in model.layers:
                del L.forward
    finally:
        options.INT8_PLANE_TAILS, options.INT8_HEAD = saved
        _hip.set_backend(prev)
    return be, y.detach(), [o.detach() for o in outs], recs


def _names(be):
    return [c[0] for c in be.census]


def _demoted(census):
    """a census with every plane tail written as the two launches it replaces"""
    out = []
    for c in census:
        out += [(TAIL, c[1], False), (HILO, c[1])] if c[0] == NEW else [c]
    return out


def _same(on, off):
    assert torch.equal(on[1], off[1]), 'logits differ'
    assert len(on[2]) == len(off[2]) and all(torch.equal(a, b) for a, b in zip(on[2], off[2])), 'hidden states differ'


def test_switch_is_off_by_default_cpu():
    from quantization import options
    assert options.INT8_PLANE_TAILS is False


def test_switch_on_the_attention_tails_write_the_planes_cpu():
    model = _bert()
    off = _run(model, False)
    on = _run(model, True)
    # switch off: today's census, one quantize_hilo per layer
    assert off[0].census == _expected_census('mp16', LAYERS, B, T), off[0].census
    names = _names(on[0])
    assert names.count(HILO) == 0
    assert names.count(NEW) == LAYERS and [c for c in on[0].census if c[0] == NEW] == [(NEW, S, 16)] * LAYERS
    assert names.count('linear_i16x8') == LAYERS
    assert names.count(TAIL) == LAYERS                          # the feed-forward tails (site z is 8-bit): today's launch
    assert _demoted(on[0].census) == off[0].census
    # per layer: QKV, core, attention-output Linear, plane tail, FFN1 (16-bit, index-only), FFN2, tail
    per_layer = ['linear_i8_grouped', 'attention_i8', 'linear_i8', NEW, 'linear_i16x8', 'linear_i8', TAIL]
    assert names == ['embeddings_layernorm_quant'] + per_layer * LAYERS
    _same(on, off)
    assert all(p is None and i is not None for p, i in on[3])    # layer outputs: 8-bit, int8 indices as ever
    # every tail still got ITS three quantizers in order
    ptr = lambda m: getattr(m, 'activation_quantizer', m).quantizer._delta.data_ptr()
    assert on[0].tail_bindings == [(ptr(b.dense.activation_quantizer), ptr(b.res_act_quantizer.activation_quantizer),
                                    ptr(b.LayerNorm.activation_quantizer)) for L in model.layers for b in (L.attention_output, L.output)]


def test_the_planes_are_the_bytes_of_the_oracle_index_of_x_cpu():
    """site x as FFN1 sees it: on its 16-bit grid, with planes in its record that are the oracle's index of it"""
    from quantization import _hip, options, provenance
    from tests._planes_twin import PlanesTwin
    from tests._skinny16_twin import index_of
    model = _bert()
    seen = []
    blk = model.layers[0].attention_output
    f = type(blk).forward
    blk.forward = lambda h, r: (seen.append(f(blk, h, r)), seen[-1])[1]
    prev, saved = _hip.set_backend(PlanesTwin()), options.INT8_PLANE_TAILS
    options.INT8_PLANE_TAILS = True
    try:
        with torch.no_grad():
            model(*_inputs())
        x = seen[0]
        q = blk.LayerNorm.activation_quantizer.quantizer
        planes = provenance.planes_like(x)
        assert planes is not None and provenance.indices_of(x) is None and provenance.quantizer_of(x) is q
        i, y = O.fake_quant(x, q._delta.reshape(()), q._zero_float.reshape(()), 16, False)
        assert torch.equal(y, x) and torch.equal(torch.from_numpy(index_of(*planes)).float(), i) and i.max() > 255
    finally:
        options.INT8_PLANE_TAILS = saved
        _hip.set_backend(prev)
        del blk.forward


def test_backend_without_the_entry_keeps_todays_calls_cpu():
    from tests._planes_twin import NoPlanesTwin
    model = _bert()
    off = _run(model, False, NoPlanesTwin())
    on = _run(model, True, NoPlanesTwin())
    assert on[0].census == off[0].census == _expected_census('mp16', LAYERS, B, T)
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


@pytest.mark.parametrize('prepare', [_hook, _save_target, _estimating], ids=['hook', 'save_target', 'estimating'])
def test_an_observed_or_estimating_tail_keeps_todays_launch_cpu(prepare):
    """layer 0's attention-output tail is not one for the fused launch: it runs what it runs with the switch off, the other
    layers write planes"""
    off = _run(prepare(_bert()), False)
    on = _run(prepare(_bert()), True)
    assert _names(on[0]).count(NEW) == LAYERS - 1
    assert _demoted(on[0].census) == off[0].census
    first = _names(on[0]).index('linear_i8_grouped', 2)          # layer 1's first launch
    assert NEW not in _names(on[0])[:first]
    _same(on, off)


def test_grad_mode_keeps_todays_launches_cpu():
    from quantization import options
    saved = options.INT8_LINEAR
    options.INT8_LINEAR = True                                   # (under 'auto' grad mode switches the whole route off)
    try:
        off = _run(_bert(), False, no_grad=False)
        on = _run(_bert(), True, no_grad=False)
    finally:
        options.INT8_LINEAR = saved
    assert NEW not in _names(on[0]) and on[0].census == off[0].census
    _same(on, off)


@pytest.mark.parametrize('how', ['add_', 'range re-set'])
def test_a_stale_record_is_not_used_cpu(how):
    """the planes are trusted for the unchanged tensor on an unchanged grid only: after an in-place change of x, or a re-set of
    its quantizer's range, FFN1's operands come from quantize_hilo"""
    from quantization import _hip, options, provenance
    from tests._planes_twin import PlanesTwin
    model = _bert()
    L = model.layers[0]
    be = PlanesTwin()
    prev, saved = _hip.set_backend(be), options.INT8_PLANE_TAILS
    options.INT8_PLANE_TAILS = True
    try:
        with torch.no_grad():
            h = model.embeddings(_inputs()[0])
            x = L.attention_output(L.attention_self(h, None), h)
            assert provenance.planes_like(x) is not None
            ffn1 = L.intermediate[0]
            plan = ffn1._int8_plan(x, with_output_quantizer=True, mp16=True)
            assert plan is not None and plan.kind == 'mp16'
            fresh = ffn1._int8_operands(x, plan)
            assert HILO not in _names(be) and fresh.x_idx is provenance.planes_like(x)[0] and fresh.x_lo is provenance.planes_like(x)[1]
            q = L.attention_output.LayerNorm.activation_quantizer.quantizer
            if how == 'add_':
                x.add_(0.0)
            else:
                q.set_quant_range(torch.tensor(-9.0), torch.tensor(9.5))
            assert provenance.planes_like(x) is None and provenance.of(x) is None
            stale = ffn1._int8_operands(x, plan)
            assert _names(be).count(HILO) == 1
            assert stale.x_idx is not fresh.x_idx and stale.x_lo is not fresh.x_lo
            if how == 'add_':                                    # same values on the same grid: the same planes, re-derived
                assert torch.equal(stale.x_idx, fresh.x_idx) and torch.equal(stale.x_lo, fresh.x_lo)
    finally:
        options.INT8_PLANE_TAILS = saved
        _hip.set_backend(prev)


def test_a_16_bit_hidden_state_stays_off_the_skinny_plan_cpu():
    """a [B, T, d] hidden state with planes is for the MP16 plan and the first-token helper: the generic integer branch of a
    Linear (skinny=True) does not take it, so a 16-bit Linear input at a ragged row count stays layered as before"""
    from quantization import _hip, options, provenance
    from tests._planes_twin import PlanesTwin
    model = _bert()
    L = model.layers[0]
    prev, saved = _hip.set_backend(PlanesTwin()), (options.INT8_PLANE_TAILS, options.INT8_HEAD)
    options.INT8_PLANE_TAILS, options.INT8_HEAD = True, True
    try:
        with torch.no_grad():
            h = model.embeddings(_inputs()[0])
            x = L.attention_output(L.attention_self(h, None), h)
            assert provenance.planes_like(x) is not None
            assert L.intermediate[0]._int8_plan(x, with_output_quantizer=True, skinny=True, ragged=True) is None
    finally:
        options.INT8_PLANE_TAILS, options.INT8_HEAD = saved
        _hip.set_backend(prev)


# ---- the pooler behind a 16-bit last hidden state ----------------------------------------------------------------------------
def _skinny(census):
    return [c for c in census if c[0] in (SKINNY16, SKINNY8)]


def test_pooler_reads_the_first_token_rows_of_the_planes_cpu():
    from tests._planes_twin import PlanesTwin
    from tests._skinny16_twin import index_of

    class Recording(PlanesTwin):
        def linear_i16x8_skinny(self, x, *a, **k):
            self.__dict__.setdefault('inputs', []).append(x)
            return super().linear_i16x8_skinny(x, *a, **k)

    model = _bert('head')
    layered = _run(model, False, head=True)                     # new switch off: the head stays layered as today
    assert _skinny(layered[0].census) == [] and NEW not in _names(layered[0])
    on = _run(model, True, Recording(), head=True)
    # the attention-output tails and the last feed-forward tail (site z of the last layer: 16 bits) write planes
    assert _names(on[0]).count(NEW) == LAYERS + 1 and _names(on[0]).count(HILO) == 0
    enc_on = [c for c in _demoted(on[0].census) if c[0] not in (SKINNY16, SKINNY8)]
    # the encoder: today's launches but for the last tail's quantize_hilo, which nobody asked for with the switch off
    last_hilo = max(i for i, c in enumerate(enc_on) if c[0] == HILO)
    assert enc_on[:last_hilo] + enc_on[last_hilo + 1:] == layered[0].census
    assert _skinny(on[0].census) == [
        (SKINNY16, B, D, D, ACT_TANH, (T * D, 1), True, False, True, 'planes', True),       # planes in, strides (T d, 1)
        (SKINNY16, B, 2, D, ACT_NONE, (D, 1), True, False, True, 'y', True)]
    assert on[0].census[-2:] == _skinny(on[0].census)
    assert all(torch.equal(a, b) for a, b in zip(on[2], layered[2])), 'hidden states differ'
    # what the pooler read: views of the last hidden state's planes, and those are the oracle's index of it
    h = on[2][-1]
    planes, idx = on[3][-1]
    assert planes is not None and idx is None
    hi, lo = on[0].inputs[0]
    assert hi.data_ptr() == planes[0].data_ptr() and lo.data_ptr() == planes[1].data_ptr() and hi.shape == (B, D)
    q = model.layers[-1].output.LayerNorm.activation_quantizer.quantizer
    i, y = O.fake_quant(h, q._delta.reshape(()), q._zero_float.reshape(()), 16, False)
    assert torch.equal(y, h) and torch.equal(torch.from_numpy(index_of(hi, lo)).float(), i[:, 0])
    # the logits: finite, on the classifier's 16-bit grid; the layered head's differ by its fp32 GEMMs' round-off at most
    logits = on[1]
    cq = model.classifier.activation_quantizer.quantizer
    assert torch.isfinite(logits).all() and torch.equal(O.fake_quant(logits, cq._delta.reshape(()), cq._zero_float.reshape(()), 16, False)[1], logits)
    assert float((logits - layered[1]).abs().max()) <= 64 * float(cq._delta) + 1e-3 * float(layered[1].abs().max())


def test_head_without_the_tail_switch_or_without_int8_head_is_todays_cpu():
    model = _bert('head')
    base = _run(model, False, head=False)
    for on, head in ((True, False), (False, True)):
        other = _run(model, on, head=head)
        assert _skinny(other[0].census) == []
        _same(other, base)                                        # the layered head on equal hidden states
