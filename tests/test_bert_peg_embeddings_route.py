"""options.INT8_PEG_EMBEDDINGS on the GPU: the 3-layer BERT-base-width model of tests/test_bert_peg_attention_route.py under
`apply_activation_granularity(per_groups=6)`.  That test has to start behind the embedding block (layered there: torch's
LayerNorm sums differently on GPU and CPU).  With the switch on the block is one launch that is exact against the CPU chain, so
here BOTH sides start from the input ids: the embedding output and every layer's hidden state -- with the int8 indices they
carry -- are `torch.equal` between the GPU and the exact CPU twin (tests/_peg_embeddings_twin.py), eager, as a hipGraph replay,
at a ragged shape and with per-row position ids (the packed form), with one embedding launch per forward on both sides.

Against the switch off (the layered block) the bar is the existing one, 0.05 * max |layered|: the two arms differ by torch's
LayerNorm order."""
import copy

import pytest
import torch

from tests._peg_embeddings_twin import NAME
from tests.test_bert_peg_attention_route import CORE, GROUPED, LAYERS, RAGGED, _census, _gpu_model, _host, _ids, _mask, _switch

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]

D = 768
ON = dict(INT8_PEG_EMBEDDINGS=True, INT8_PEG_ATTENTION=True, INT8_RAGGED=True, INT8_RAGGED_RECIPES=True)


class _FromIds(torch.nn.Module):
    """embedding block + encoder stack; `states` holds (values, int8 indices) of the embedding output and of every layer"""

    def __init__(self, model):
        super().__init__()
        self.model, self.states = model, []

    def forward(self, ids, mask, pos=None):
        from quantization import provenance
        m = self.model
        x = m.embeddings(ids) if pos is None else m.embeddings(ids, pos)
        self.states = [(x, provenance.indices_of(x))]
        for L in m.layers:
            x = L(x, mask)
            self.states.append((x, provenance.indices_of(x)))
        return x


def _count_embeddings(monkeypatch, log):
    """the new launch into the census `log` of tests/test_bert_peg_attention_route.py, in the form the twin records its own"""
    from quantization import _hip
    orig = _hip.HipBackend.embeddings_layernorm_quant_axis

    def counted(self, *a, **k):
        log.append((NAME, tuple(a[1].shape), tuple(None if q is None else int(q[0].numel()) for q in (a[6], a[7], a[11])),
                    k.get('want_idx', False)))
        return orig(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, 'embeddings_layernorm_quant_axis', counted)


def _twin_states(model, ids, mask, pos=None):
    from quantization import _hip
    from tests._peg_embeddings_twin import PegEmbeddingsTwin
    be = PegEmbeddingsTwin(rules=_hip.backend())
    enc = _FromIds(copy.deepcopy(model).cpu())
    prev = _hip.set_backend(be)
    try:
        with torch.no_grad():
            enc(ids, None if mask is None else mask.cpu(), pos)
        return _host(enc.states), list(be.census)
    finally:
        _hip.set_backend(prev)


def _assert_states_equal(got, want, what, n=LAYERS + 1):
    assert len(got) == len(want) == n
    for l, ((g, gi), (w, wi)) in enumerate(zip(got, want)):
        where = 'embedding output' if l == 0 else f'layer {l - 1}'
        assert gi is not None and wi is not None, f'{what}: {where} carries no int8 indices'
        assert torch.equal(gi, wi), f'{what}: {where}: {int((gi != wi).sum())} int8 indices differ'
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), f'{what}: {where}: {int((g != w).sum())} values differ'
        assert torch.isfinite(g).all()


def _one_embedding_launch(census, shape):
    assert [e for e in census if e[0] == NAME] == [(NAME, shape, (D, D, D), True)] and census[0][0] == NAME, census[:2]


def test_from_the_input_ids_equals_the_twin_eager_and_replayed(monkeypatch):
    from quantization.graphs import GraphedForward
    B, T = 3, 64
    model, ids, mask = _gpu_model(), _ids(3, B, T), _mask(B, T, 'cuda')
    enc = _FromIds(model)
    log = _census(monkeypatch)
    _count_embeddings(monkeypatch, log)
    with torch.no_grad():
        _switch(monkeypatch, **dict(ON, INT8_PEG_EMBEDDINGS=False))
        enc(ids.cuda(), mask)
        off_census, off = list(log), _host(enc.states)
        del log[:]
        _switch(monkeypatch, **ON)
        enc(ids.cuda(), mask)
        torch.cuda.synchronize()
        census, eager = list(log), _host(enc.states)
        enc(ids.cuda(), mask)
        second = _host(enc.states)
        g = GraphedForward(enc, ids.cuda(), mask)
        static = enc.states                                     # the capture pass: the graph's own tensors
        g(ids.cuda(), mask)
        torch.cuda.synchronize()
        replay = _host(static)
    want, twin_census = _twin_states(model, ids, mask)
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    _one_embedding_launch(census, (B, T))
    assert [e[0] for e in census if e[0] in (GROUPED, CORE)] == [GROUPED, CORE] * LAYERS
    # with the switch off the block is layered (no census entry) and everything behind it is launch for launch the same
    assert not [e for e in off_census if e[0] == NAME] and census[1:] == off_census
    _assert_states_equal(eager, want, 'eager against the twin')
    _assert_states_equal(second, eager, 'a second eager run')
    _assert_states_equal(replay, want, 'hipGraph replay against the twin')
    # against the layered block (switch off): measured, then the existing bar
    for l, ((h, _), (r, _)) in enumerate(zip(eager, off)):
        d, top = float((h - r).abs().max()), float(r.abs().max())
        print(f'{"embedding output" if l == 0 else f"layer {l - 1}"}: max |on - off| = {d:.5f}, max |off| = {top:.5f}')
        assert d <= 0.05 * top, (l, d, top)


def test_ragged_shape_from_the_input_ids_equals_the_twin(monkeypatch):
    B, T = 3, 50
    model, ids, mask = _gpu_model(), _ids(4, B, T), _mask(B, T, 'cuda')
    enc = _FromIds(model)
    _switch(monkeypatch, **ON)
    log = _census(monkeypatch)
    _count_embeddings(monkeypatch, log)
    with torch.no_grad():
        enc(ids.cuda(), mask)
        torch.cuda.synchronize()
        census, got = list(log), _host(enc.states)
    want, twin_census = _twin_states(model, ids, mask)
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    _one_embedding_launch(census, (B, T))
    assert [e[0] for e in census if e[0] in (GROUPED, RAGGED)] == [GROUPED, RAGGED] * LAYERS
    _assert_states_equal(got, want, '[3,50] against the twin')


VARLEN = 'attention_i8_varlen'


def _count_varlen(monkeypatch, log):
    """the variable-length core into the census `log`, in the form the twin records its own"""
    from quantization import _hip
    orig = _hip.HipBackend.attention_i8_varlen

    def counted(self, *a, **k):
        wide = any(q is not None and q[0].numel() != 1 for q in (a[8], a[9], a[10], a[13]))
        log.append((VARLEN, tuple(a[0].shape)) + (('per-head',) if wide else ()))
        return orig(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, VARLEN, counted)


def test_forward_packed_from_the_input_ids_equals_the_twin(monkeypatch):
    """`forward_packed` hands the block its per-row position ids through the same call: [1, M] ids of three sequences without
    their pad tokens.  With INT8_PEG_EMBEDDINGS on, the attention half of a packed batch takes the grouped class-ordered Linear
    and the variable-length core with a grid per head (INT8_PEG_ATTENTION alone declines packed batches and would run it
    layered), so the embedding output AND every layer's hidden state equal the twin's; `forward_packed` itself makes the same
    launches as the loop of this file."""
    from harness.bert import pack_batch
    from quantization import _hip
    from quantization.fused import PackedSequences
    from tests._peg_embeddings_twin import PegEmbeddingsTwin
    B, T = 3, 50
    model = _gpu_model()
    am = torch.ones(B, T, dtype=torch.long)
    am[1, 37:] = 0
    am[2, 13:] = 0
    p_ids, p_pos, seq_start, max_len = pack_batch(_ids(5, B, T), am)
    M = p_ids.shape[1]
    enc = _FromIds(model)
    _switch(monkeypatch, **ON)
    log = _census(monkeypatch)
    _count_embeddings(monkeypatch, log)
    _count_varlen(monkeypatch, log)
    with torch.no_grad():
        enc(p_ids.cuda(), PackedSequences(seq_start.cuda(), max_len), p_pos.cuda())
        torch.cuda.synchronize()
        census, got = list(log), _host(enc.states)
        del log[:]
        logits = model.forward_packed(p_ids.cuda(), p_pos.cuda(), seq_start.cuda(), max_len).cpu().clone()
        packed_census = list(log)
    assert logits.shape[0] == B and torch.isfinite(logits).all()        # (pooler and classifier are layered: no exact statement)
    be = PegEmbeddingsTwin(rules=_hip.backend())
    tenc = _FromIds(copy.deepcopy(model).cpu())
    prev = _hip.set_backend(be)
    try:
        with torch.no_grad():
            tenc(p_ids, PackedSequences(seq_start, max_len), p_pos)
            want, twin_census = _host(tenc.states), list(be.census)
    finally:
        _hip.set_backend(prev)
    for l, ((g, gi), (w, wi)) in enumerate(zip(got, want)):
        print(f'{"embedding output" if l == 0 else f"layer {l - 1}"}: {int((gi != wi).sum())} of {gi.numel()} int8 indices differ, '
              f'max |difference| of the values {float((g - w).abs().max()):.5f}')
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    _one_embedding_launch(census, (1, M))
    assert [e for e in census if e[0] in (GROUPED, VARLEN)] == [(GROUPED, (1, M, D), 3 * D, (D, D, D), 128, False),
                                                                  (VARLEN, (1, M, D), 'per-head')] * LAYERS
    assert [e for e in packed_census if e[0] in (NAME, GROUPED, VARLEN)] == [e for e in census if e[0] in (NAME, GROUPED, VARLEN)]
    _assert_states_equal(got, want, 'forward_packed against the twin')


def test_per_embedding_grids_embedding_output_equals_the_twin(monkeypatch):
    """`per_embd=True` (768 distinct grids per site): the embedding output alone, from the input ids -- GPU == twin, one launch,
    and against the layered block the existing bar"""
    from harness.bert import apply_activation_granularity
    from quantization import _hip, provenance
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests._peg_embeddings_twin import PegEmbeddingsTwin
    from tests.harness_bert import build_bert_base
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=1, **qp)
    apply_activation_granularity(model, per_embd=True)
    model = model.cuda().eval()
    with torch.no_grad():
        pass_data_for_range_estimation([(_ids(10).cuda(),), (_ids(11).cuda(),)], model, act_quant=True, weight_quant=True,
                                       max_num_batches=2)
        model.fix_ranges()
    E = model.embeddings
    assert E.LayerNorm.activation_quantizer.quantizer._delta.numel() == D
    B, T = 3, 64
    ids = _ids(3, B, T)
    log = []
    _count_embeddings(monkeypatch, log)
    with torch.no_grad():
        off = E(ids.cuda()).cpu().clone()
        assert not log
        _switch(monkeypatch, INT8_PEG_EMBEDDINGS=True)
        y = E(ids.cuda())
        got = (y.cpu().clone(), provenance.indices_of(y).cpu().clone())
    assert log == [(NAME, (B, T), (D, D, D), True)]
    be = PegEmbeddingsTwin(rules=_hip.backend())
    twin = copy.deepcopy(E).cpu()
    prev = _hip.set_backend(be)
    try:
        with torch.no_grad():
            w = twin(ids)
            want = (w.clone(), provenance.indices_of(w).clone())
    finally:
        _hip.set_backend(prev)
    assert be.census == log
    _assert_states_equal([got], [want], 'per-embedding grids', n=1)
    d, top = float((got[0] - off).abs().max()), float(off.abs().max())
    print(f'per_embd embedding output: max |on - off| = {d:.5f}, max |off| = {top:.5f}')
    assert d <= 0.05 * top, (d, top)
