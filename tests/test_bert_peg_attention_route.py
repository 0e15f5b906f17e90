"""options.INT8_PEG_ATTENTION on the GPU: a 3-layer BERT-base-width model under `apply_activation_granularity(per_groups=6)`,
calibrated at [3, 64].  With the switch on the attention half of every layer is one grouped class-ordered Linear and one
attention core with a grid per head, and every layer's hidden state -- with the int8 indices it carries -- is `torch.equal` to
the exact CPU twin's (tests/_peg_attention_twin.py), eager and as a hipGraph replay, with the same launches on both sides.

The embedding block is layered under this recipe (per-column quantizers) and torch's LayerNorm differs between GPU and CPU, so
the comparison starts behind it: the encoder stack of both sides starts from ONE embedding output, computed once on the GPU and
shared as a plain tensor without a record; each side passes it through the embedding LayerNorm's fixed quantizer (idempotent on
its own grid), which gives it its record.

Against the layered route (INT8_LINEAR = False) the bar is tests/test_bert_peg_route.py's, 0.05 * max |layered|.  Confirmed on
the CPU first (tests/test_peg_attention_host.py::test_hidden_states_against_the_layered_modules_cpu: twin against
layered-on-CPU, 3 layers, seed 1000, [2, 64]): max |diff| = 0.032 / 0.093 / 0.096 at max |layered| = 4.09 / 4.02 / 4.15 in layers
0 / 1 / 2, i.e. at most 2.4 % against the bar's 5 %.  On the GPU at [3, 64] the test prints 0.063 / 0.092 / 0.099 of 4.03 / 4.01 /
4.08 (with the switch off: 0.032 / 0.092 / 0.099 -- from layer 1 on the difference is the feed-forward half's)."""
import copy

import pytest
import torch

from tests.test_bert_exact_route import _HIP_CENSUS

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]

LAYERS, D = 3, 768
GROUPED, CORE, RAGGED = 'linear_i8_cls_grouped', 'attention_i8', 'attention_i8_ragged'
_GPU = {}


def _ids(seed, B=3, T=64):
    return torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(seed))


def _gpu_model():
    if 'm' not in _GPU:
        from harness.bert import apply_activation_granularity
        from quantization import options
        from quantization.quantizers import QMethods
        from quantization.range_estimators import RangeEstimators
        from tests.harness_bert import build_bert_base
        from utils.utils import pass_data_for_range_estimation
        assert not (options.INT8_PEG_ATTENTION or options.INT8_RAGGED or options.INT8_RAGGED_RECIPES)
        qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
                  weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
        model, _ = build_bert_base(seed=1000, num_layers=LAYERS, **qp)
        apply_activation_granularity(model, per_groups=6)
        model = model.cuda().eval()
        with torch.no_grad():
            pass_data_for_range_estimation([(_ids(10).cuda(),), (_ids(11).cuda(),)], model, act_quant=True, weight_quant=True,
                                           max_num_batches=2)
            model.fix_ranges()
        _GPU['m'] = model
    return _GPU['m']


def _embedding_output(B, T):
    """one embedding output per shape, computed once on the GPU: a plain host tensor without a record"""
    key = ('h0', B, T)
    if key not in _GPU:
        with torch.no_grad():
            _GPU[key] = _gpu_model().embeddings(_ids(3, B, T).cuda()).detach().cpu().clone()
    return _GPU[key]


def _mask(B, T, device):
    am = torch.ones(B, T)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return ((1.0 - am[:, None, None, :]) * -10000.0).to(device)


class _Encoder(torch.nn.Module):
    """the encoder stack behind the embedding block; `states` holds every layer's (hidden state, int8 indices) of the last call"""

    def __init__(self, model):
        super().__init__()
        self.model, self.states = model, []

    def forward(self, h0, mask):
        from quantization import provenance
        m = self.model
        x = m.embeddings.LayerNorm.activation_quantizer(h0.clone())
        self.states = []
        for L in m.layers:
            x = L(x, mask)
            self.states.append((x, provenance.indices_of(x)))
        return x


def _host(states):
    return [(y.detach().cpu().clone(), None if i is None else i.detach().cpu().clone()) for y, i in states]


def _census(monkeypatch):
    """launches of the HIP backend in the form the twin records its own"""
    from quantization import _hip
    log = []
    wide = lambda a: any(q is not None and q[0].numel() != 1 for q in (a[6], a[7], a[8], a[11]))
    info = dict(_HIP_CENSUS)
    info[CORE] = lambda a, k: (tuple(a[0].shape),) + (('per-head',) if wide(a) else ())
    info[RAGGED] = info[CORE]
    info[GROUPED] = lambda a, k: (tuple(a[0].shape), a[1].shape[0], tuple(int(q[0].numel()) for q in a[9]), int(a[10]),
                                  k.get('want_y', False))
    for name, fn in info.items():
        orig = getattr(_hip.HipBackend, name)

        def counted(self, *a, _o=orig, _n=name, _i=fn, **k):
            log.append((_n,) + _i(a, k))
            return _o(self, *a, **k)
        monkeypatch.setattr(_hip.HipBackend, name, counted)
    return log


def _twin_states(model, h0, mask):
    from quantization import _hip
    from tests._peg_attention_twin import PegAttentionTwin
    be = PegAttentionTwin(rules=_hip.backend())
    enc = _Encoder(copy.deepcopy(model).cpu())
    prev = _hip.set_backend(be)
    try:
        with torch.no_grad():
            enc(h0, mask.cpu())
        return _host(enc.states), list(be.census)
    finally:
        _hip.set_backend(prev)


def _assert_states_equal(got, want, what):
    assert len(got) == len(want) == LAYERS
    for l, ((g, gi), (w, wi)) in enumerate(zip(got, want)):
        assert gi is not None and wi is not None, f'{what}: layer {l} carries no int8 indices'
        assert torch.equal(gi, wi), f'{what}: layer {l}: {int((gi != wi).sum())} int8 indices differ'
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), f'{what}: layer {l}: {int((g != w).sum())} values differ'
        assert torch.isfinite(g).all()


def _layer_on(core, B, T):
    s = (B, T, D)
    return [(GROUPED, s, 3 * D, (D, D, D), 128, False), (core, s, 'per-head')]


def _switch(monkeypatch, **kw):
    from quantization import options
    for k, v in kw.items():
        monkeypatch.setattr(options, k, v)


def test_every_hidden_state_equals_the_twin_eager_and_replayed(monkeypatch):
    from quantization.autoquant_utils import INT8_STATS
    from quantization.graphs import GraphedForward
    B, T = 3, 64
    model, h0 = _gpu_model(), _embedding_output(3, 64)
    mask = _mask(B, T, 'cuda')
    enc = _Encoder(model)
    log = _census(monkeypatch)
    with torch.no_grad():
        enc(h0.cuda(), mask)
        off_census, off = list(log), _host(enc.states)
        del log[:]
        _switch(monkeypatch, INT8_PEG_ATTENTION=True)
        k0 = INT8_STATS['kernel_calls']
        enc(h0.cuda(), mask)
        torch.cuda.synchronize()
        calls, census, eager = INT8_STATS['kernel_calls'] - k0, list(log), _host(enc.states)
        enc(h0.cuda(), mask)
        second = _host(enc.states)
        g = GraphedForward(enc, h0.cuda(), mask)
        static = enc.states                                     # the capture pass: the graph's own tensors
        g(h0.cuda(), mask)
        torch.cuda.synchronize()
        replay = _host(static)
    want, twin_census = _twin_states(model, h0, mask)
    assert calls == LAYERS * 6, calls                           # no Linear of the encoder is layered
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    assert [e for e in census if e[0] in (GROUPED, CORE)] == _layer_on(CORE, B, T) * LAYERS
    # with the switch off the census is today's: the attention half layered, everything behind it launch for launch the same
    assert not [e for e in off_census if e[0] in (GROUPED, CORE, 'linear_i8_grouped')]
    assert [e for e in census if e[0] not in (GROUPED, CORE)] == off_census
    _assert_states_equal(eager, want, 'eager against the twin')
    _assert_states_equal(second, eager, 'a second eager run')
    _assert_states_equal(replay, want, 'hipGraph replay against the twin')
    # against the layered route: measured, then the existing bar
    with torch.no_grad():
        _switch(monkeypatch, INT8_PEG_ATTENTION=False, INT8_LINEAR=False)
        enc(h0.cuda(), mask)
        layered = _host(enc.states)
    for l, ((h, _), (r, _)) in enumerate(zip(eager, layered)):
        d, top = float((h - r).abs().max()), float(r.abs().max())
        d_off = float((off[l][0] - r).abs().max())
        print(f'layer {l}: max |on - layered| = {d:.5f} (switch off: {d_off:.5f}), max |layered| = {top:.5f}')
        assert d <= 0.05 * top, (l, d, top)


def test_ragged_shape_equals_the_twin(monkeypatch):
    B, T = 3, 50
    model, h0 = _gpu_model(), _embedding_output(3, 50)
    mask = _mask(B, T, 'cuda')
    enc = _Encoder(model)
    _switch(monkeypatch, INT8_PEG_ATTENTION=True, INT8_RAGGED=True, INT8_RAGGED_RECIPES=True)
    log = _census(monkeypatch)
    with torch.no_grad():
        enc(h0.cuda(), mask)
        torch.cuda.synchronize()
        census, got = list(log), _host(enc.states)
    want, twin_census = _twin_states(model, h0, mask)
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    assert [e for e in census if e[0] in (GROUPED, RAGGED)] == _layer_on(RAGGED, B, T) * LAYERS
    _assert_states_equal(got, want, '[3,50] against the twin')


def test_index_residuals_on_top_give_the_same_hidden_states(monkeypatch):
    B, T = 3, 64
    model, h0 = _gpu_model(), _embedding_output(3, 64)
    mask = _mask(B, T, 'cuda')
    enc = _Encoder(model)
    with torch.no_grad():
        _switch(monkeypatch, INT8_PEG_ATTENTION=True)
        enc(h0.cuda(), mask)
        alone = _host(enc.states)
        _switch(monkeypatch, INT8_PEG_INDEX_RESIDUALS=True)
        log = _census(monkeypatch)
        enc(h0.cuda(), mask)
        both = _host(enc.states)
    assert [e for e in log if e[0] in (GROUPED, CORE)] == _layer_on(CORE, B, T) * LAYERS
    for l, ((a, _), (b, _)) in enumerate(zip(alone, both)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'layer {l}'


@pytest.mark.parametrize('per_groups,k_ops', [(12, 1536), (4, 1024)])
def test_attention_half_at_64_and_192_column_groups_equals_the_twin(per_groups, k_ops, monkeypatch):
    """per_groups = 12 / 4: the layer input's classes (64 / 192 columns) are padded to whole 128-column K slabs with zero weights
    (quantization/peg.py PaddedClassLayout) and the output grids are constant over blocks of 64 columns (64-wide tiles).  The other
    Linears of these recipes stay layered, so the exact statement is the attention half's: its context and int8 indices equal the
    twin's at [3, 64] and, with the ragged switches, at [3, 50] (the class-order gather writes into a roomy buffer of the
    padded width)."""
    from harness.bert import apply_activation_granularity
    from quantization import _hip, provenance
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests._peg_attention_twin import PegAttentionTwin
    from tests.harness_bert import build_bert_base
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=1, **qp)
    apply_activation_granularity(model, per_groups=per_groups)
    model = model.cuda().eval()
    with torch.no_grad():
        pass_data_for_range_estimation([(_ids(10).cuda(),), (_ids(11).cuda(),)], model, act_quant=True, weight_quant=True,
                                       max_num_batches=2)
        model.fix_ranges()
    twin = copy.deepcopy(model).cpu()
    log = _census(monkeypatch)
    _switch(monkeypatch, INT8_PEG_ATTENTION=True, INT8_RAGGED=True, INT8_RAGGED_RECIPES=True)

    def half(m, h0, mask):
        x = m.embeddings.LayerNorm.activation_quantizer(h0.clone())
        ctx = m.layers[0].attention_self(x, mask)
        return ctx.detach().cpu().clone(), provenance.indices_of(ctx).detach().cpu().clone()
    for (B, T), core in (((3, 64), CORE), ((3, 50), RAGGED)):
        with torch.no_grad():
            h0 = model.embeddings(_ids(3, B, T).cuda()).detach().cpu().clone()
            del log[:]
            got = half(model, h0.cuda(), _mask(B, T, 'cuda'))
            torch.cuda.synchronize()
            census = list(log)
            be = PegAttentionTwin(rules=_hip.backend())
            prev = _hip.set_backend(be)
            try:
                want = half(twin, h0, _mask(B, T, 'cpu'))
            finally:
                _hip.set_backend(prev)
        assert census == list(be.census) == [(GROUPED, (B, T, k_ops), 3 * D, (D, D, D), 64, False), (core, (B, T, D), 'per-head')], census
        assert torch.equal(got[1], want[1]), f'[{B},{T}]: {int((got[1] != want[1]).sum())} context indices differ'
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.isfinite(got[0]).all()
