"""Host logic of options.INT8_MOBILE_EMBEDDINGS, replayed on the CPU with the twin (tests/_mobile_embeddings_twin.py): with the
switch on MobileBERT's embedding block is ONE call of `mobile_embeddings_nonorm_quant` whose output carries int8 indices; the
switch is off by default; every decline reaches the layered lines without that call."""
import copy

import pytest
import torch

from tests._mobile_embeddings_twin import NAME, MobileEmbeddingsTwin
from tests._oracle_backend import OracleBackend
from tests.test_peg_attention_host import _under

pytestmark = pytest.mark.default_route

_BLOCK = []


def _ids(seed=3, B=2, T=20):
    return torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(seed))


def _block():
    """the embedding block of a 1-layer W4A4 MobileBERT, calibrated once on the twin (calibrating forwards are layered)"""
    if not _BLOCK:
        from tests.test_mobilebert_e2e import _build
        from utils.utils import pass_data_for_range_estimation
        model, _ = _build('cpu', num_layers=1)
        with _under(MobileEmbeddingsTwin()), torch.no_grad():
            pass_data_for_range_estimation([(_ids(10),)], model, act_quant=True, weight_quant=True, max_num_batches=1)
            model.fix_ranges()
        _BLOCK.append(model.embeddings)
    return copy.deepcopy(_BLOCK[0])


def _run(E, monkeypatch, on=True, be=None, grad=False, helper=False, **switches):
    """-> (E(ids), or the helper's answer; the names the backend was called with)"""
    from quantization import fused, options
    for k, v in dict(INT8_MOBILE_EMBEDDINGS=on, **switches).items():
        monkeypatch.setattr(options, k, v)
    be = be or MobileEmbeddingsTwin()
    with _under(be), (torch.enable_grad() if grad else torch.no_grad()):
        out = fused.mobile_embeddings_nonorm_quant(E, _ids()) if helper else E(_ids())
    return out, [e[0] for e in getattr(be, 'census', [])]


def test_off_by_default_and_one_call_with_indices_when_on_cpu(monkeypatch):
    from quantization import options, provenance
    assert options.INT8_MOBILE_EMBEDDINGS is False and options.INT8_LINEAR == 'auto'
    assert not options.int8_mobile_embeddings(MobileEmbeddingsTwin())
    E = _block()
    off, names = _run(E, monkeypatch, on=False)
    assert NAME not in names
    on, names = _run(E, monkeypatch)
    assert names == [NAME] and on.shape == off.shape == (2, 20, 512)
    assert provenance.quantizer_of(on) is E.LayerNorm.activation_quantizer.quantizer
    assert provenance.indices_of(on).dtype == torch.int8 and provenance.indices_of(off) is not None
    # the exact value the layered block's fp32 GEMM approximates: a few 4-bit steps apart at most, mostly equal
    step = float(E.LayerNorm.activation_quantizer.quantizer._delta)
    assert float((on - off).abs().max()) <= 2.5 * step and float((on != off).float().mean()) < 0.05


def _hook(m):
    m.register_forward_hook(lambda mod, a, o: None)


def _set_signed(E, value):
    E.word_embeddings.weight_quantizer.quantizer._signed = torch.tensor(value)


def _wide(E):
    q = E.sum_input_pos_embd_act_quantizer.activation_quantizer.quantizer
    q._delta, q._zero_float = q._delta.reshape(1).repeat(512), q._zero_float.reshape(1).repeat(512)


# (what, change to the block, keyword arguments of _run, does the layered block still run?)
DECLINES = [
    ('trigram_input off', lambda E: setattr(E, 'trigram_input', False), {}, False),
    ('a word grid of 16 bits', lambda E: setattr(E.word_embeddings.weight_quantizer.quantizer, 'n_bits', 16), {}, True),
    ('an unsigned word grid', lambda E: _set_signed(E, False), {}, True),
    ('an estimating word grid', lambda E: E.word_embeddings.weight_quantizer.estimate_ranges(), {}, True),
    ('an estimating transformation weight', lambda E: E.embedding_transformation.weight_quantizer.estimate_ranges(), {}, True),
    ('an estimating site', lambda E: E.sum_token_type_embd_act_quantizer.activation_quantizer.estimate_ranges(), {}, True),
    ('a learnable output range', lambda E: E.LayerNorm.activation_quantizer.learn_ranges(), {}, True),
    ('a per-column site', _wide, {}, False),
    ('a log-domain site', lambda E: setattr(E.embedding_transformation.activation_quantizer.quantizer, 'scale_domain', 'log'), {},
     False),
    ('a hooked Linear', lambda E: _hook(E.embedding_transformation), {}, True),
    ('a hooked weight quantizer', lambda E: _hook(E.word_embeddings.weight_quantizer), {}, True),
    ('a hooked block', _hook, {}, True),
    ('a save target', lambda E: (setattr(E.LayerNorm, 'activation_save_target', {}), setattr(E.LayerNorm, 'activation_save_name', 'n')),
     {}, True),
    ('a training NoNorm', lambda E: E.LayerNorm.train(), {}, True),
    ('grad mode', lambda E: None, dict(grad=True), True),
    ('a float64 position table', lambda E: E.position_embeddings.double(), {}, False),
    ('(E, N) without an instantiation', lambda E: None, dict(be=type('Other', (MobileEmbeddingsTwin,), {'MOBILE_EMBEDDING_SIZE': 64})),
     True),
    ('a backend without the method', lambda E: None, dict(be=OracleBackend), True),
]


@pytest.mark.parametrize('what,change,kw,layered_runs', DECLINES, ids=[d[0] for d in DECLINES])
def test_declines_reach_the_layered_lines_without_the_call_cpu(what, change, kw, layered_runs, monkeypatch):
    kw = dict(kw)
    make_be = kw.pop('be', MobileEmbeddingsTwin)
    E = _block()
    assert _run(E, monkeypatch, helper=True, grad=False)[0] is not None          # premise: this block takes the route
    change(E)
    answer, names = _run(copy.deepcopy(E), monkeypatch, helper=True, be=make_be(), **kw)
    assert answer is None and NAME not in names, what
    if layered_runs:                       # (an estimating quantizer changes its state with every forward: copies)
        want, _ = _run(copy.deepcopy(E), monkeypatch, on=False, be=make_be(), **kw)
        got, names = _run(copy.deepcopy(E), monkeypatch, be=make_be(), **kw)
        assert NAME not in names and torch.equal(got, want), what
