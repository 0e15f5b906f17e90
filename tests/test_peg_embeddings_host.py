"""Host logic of options.INT8_PEG_EMBEDDINGS, replayed on the CPU with the exact twin (tests/_peg_embeddings_twin.py): under
`apply_activation_granularity(model, per_groups=N | permute | per_embd)` the embedding block is ONE call of
`embeddings_layernorm_quant_axis` whose output is the chain's; with the switch off, or on a per-tensor model, the launches are
the ones from before there was a switch; every decline reaches the layered modules without a backend call."""
import copy

import pytest
import torch

from tests._peg_embeddings_twin import NAME, NoPegEmbeddingsTwin, PegEmbeddingsTwin
from tests.test_peg_attention_host import _ids, _model, _under

pytestmark = pytest.mark.default_route

D = 768
PER_TENSOR = 'embeddings_layernorm_quant'


def _run(call, monkeypatch, on=True, be=None, grad=False, **switches):
    """-> (output, backend) of `call()` on a fresh twin"""
    from quantization import options
    assert options.INT8_LINEAR == 'auto' and options.INT8_PEG_EMBEDDINGS is False
    for k, v in dict(INT8_PEG_EMBEDDINGS=on, **switches).items():
        monkeypatch.setattr(options, k, v)
    be = be or PegEmbeddingsTwin()
    with _under(be), (torch.enable_grad() if grad else torch.no_grad()):
        out = call()
    monkeypatch.setattr(options, 'INT8_PEG_EMBEDDINGS', False)
    return out, be


def _seven(mgr):
    q = mgr.quantizer
    return (q._delta.reshape(-1), q._zero_float.reshape(-1), None, q.n_bits, False, False, q.eps)


def _chain_of(E, ids, pos=None):
    """the block's output by the chain, from the modules' own tables and buffers -> (y [B, T, d], int8 indices)"""
    from tests._exact_backend import _p, embeddings_chain
    B, T = ids.shape
    tabs = [e.get_params()[0].detach().float() for e in (E.word_embeddings, E.token_type_embeddings, E.position_embeddings)]
    pos = torch.arange(T).expand(B, T) if pos is None else pos.expand(B, T)
    qs = [_p(_seven(m.activation_quantizer)) for m in (E.sum_input_token_type_embd_act_quantizer, E.sum_pos_embd_act_quantizer,
                                                        E.LayerNorm)]
    ln_w, ln_b = E.LayerNorm.get_params()
    y, idx, _ = embeddings_chain(tabs[0], ids.reshape(-1), tabs[1], torch.zeros(B * T, dtype=torch.long), tabs[2],
                                 pos.reshape(-1), qs[0], qs[1], ln_w.detach().float(), ln_b.detach().float(), E.LayerNorm.eps,
                                 qs[2])
    return y.view(B, T, -1), (idx - 128).to(torch.int8).view(B, T, -1)


@pytest.mark.parametrize('recipe', [dict(per_groups=6), dict(permute=True), dict(per_embd=True)],
                         ids=['per_groups6', 'permuted', 'per_embd'])
def test_one_call_whose_output_is_the_chains_cpu(recipe, monkeypatch):
    from quantization import provenance
    model, ids = _model(1, **recipe), _ids(3)
    E = model.embeddings
    for m in (E.sum_input_token_type_embd_act_quantizer, E.sum_pos_embd_act_quantizer, E.LayerNorm):
        assert m.activation_quantizer.quantizer._delta.numel() == D
    with _under(PegEmbeddingsTwin()), torch.no_grad():
        want, want_idx = _chain_of(E, ids)
    y, be = _run(lambda: E(ids), monkeypatch)
    assert be.embedding_calls == 1 and be.census == [(NAME, (2, 64), (D, D, D), True)], be.census
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    assert torch.equal(provenance.indices_of(y), want_idx) and provenance.quantizer_of(y) is E.LayerNorm.activation_quantizer.quantizer
    # the whole forward: one such call, in front of everything else
    _, be = _run(lambda: model(ids), monkeypatch)
    assert be.embedding_calls == 1 and be.census[0][0] == NAME and NAME not in [e[0] for e in be.census[1:]]
    # its own position ids, one row per token (the packed form)
    pos = torch.randint(0, 64, (2, 64), generator=torch.Generator().manual_seed(5))
    with _under(PegEmbeddingsTwin()), torch.no_grad():
        want, _ = _chain_of(E, ids, pos)
    y, be = _run(lambda: E(ids, pos), monkeypatch)
    assert be.embedding_calls == 1 and torch.equal(y, want)


def test_switch_off_and_per_tensor_models_keep_their_launches_cpu(monkeypatch):
    model, ids = _model(1), _ids(3)
    off, be_off = _run(lambda: model(ids)[0], monkeypatch, on=False)
    assert be_off.embedding_calls == 0 and not [e for e in be_off.census if e[0] in (NAME, PER_TENSOR)]
    on, be_on = _run(lambda: model(ids)[0], monkeypatch)
    # everything behind the block is launch for launch the same
    assert be_on.census[0][0] == NAME and be_on.census[1:] == be_off.census
    d = float((on - off).abs().max())
    assert d <= 0.05 * float(off.abs().max()), d
    # a per-tensor model: the switch changes nothing, the per-tensor launch stays
    plain = _model(1, per_groups=None)
    off, be_off = _run(lambda: plain(ids)[0], monkeypatch, on=False)
    on, be_on = _run(lambda: plain(ids)[0], monkeypatch)
    assert be_on.census == be_off.census and be_on.census[0][0] == PER_TENSOR and be_on.embedding_calls == 0
    assert torch.equal(on, off)


def _declines(E, ids, monkeypatch, what, be=None, **kw):
    off, on = copy.deepcopy(E), copy.deepcopy(E)            # (an estimating quantizer changes its state with every forward)
    want, be_off = _run(lambda: off(ids), monkeypatch, on=False, **kw)
    got, be_on = _run(lambda: on(ids), monkeypatch, be=be, **kw)
    assert getattr(be_on, 'embedding_calls', 0) == 0 and be_on.census == be_off.census == [], (what, be_on.census)
    assert torch.equal(got, want), what


def test_declines_reach_the_layered_modules_without_a_backend_call_cpu(monkeypatch):
    from quantization import options
    ids = _ids(7)
    base = _model(1).embeddings
    _, be = _run(lambda: base(ids), monkeypatch)
    assert be.embedding_calls == 1                            # premise: this block takes the route

    def mutated(change):
        E = copy.deepcopy(base)
        change(E)
        return E
    hook = lambda m: m.register_forward_hook(lambda mod, a, o: None)
    _declines(mutated(lambda E: hook(E.sum_pos_embd_act_quantizer)), ids, monkeypatch, 'a hooked site')
    _declines(mutated(lambda E: hook(E.LayerNorm.activation_quantizer.quantizer)), ids, monkeypatch, 'a hooked quantizer')
    _declines(mutated(lambda E: hook(E.word_embeddings)), ids, monkeypatch, 'a hooked table')
    _declines(mutated(lambda E: E.LayerNorm.train()), ids, monkeypatch, 'a training LayerNorm')
    _declines(mutated(lambda E: E.position_embeddings.train()), ids, monkeypatch, 'a training table')
    _declines(mutated(lambda E: E.sum_input_token_type_embd_act_quantizer.activation_quantizer.estimate_ranges()), ids,
              monkeypatch, 'an estimating range')
    _declines(mutated(lambda E: E.LayerNorm.activation_quantizer.estimate_ranges()), ids, monkeypatch,
              'an estimating output range')
    _declines(base, ids, monkeypatch, 'a backend without the method', be=NoPegEmbeddingsTwin())
    _declines(base, ids, monkeypatch, 'grad mode', grad=True)
    assert options.INT8_PEG_EMBEDDINGS is False


@pytest.mark.parametrize('d', [96, 2048])
def test_row_lengths_without_an_instantiation_decline_cpu(d, monkeypatch):
    """d = 96 (24 vectors: no tail kernel has that shape) and d = 2048 (the per-column tables do not fit in LDS); d = 128 with
    the same construction takes the route"""
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertEmbeddings
    from harness.bert import QEmbeddings
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from utils.per_embd_quant_utils import set_act_quant_axis_and_groups
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    ids = torch.randint(0, 200, (2, 16), generator=torch.Generator().manual_seed(d))

    def block(width):
        torch.manual_seed(width)
        hf = BertEmbeddings(BertConfig(hidden_size=width, vocab_size=200, max_position_embeddings=32)).eval()
        E = QEmbeddings(hf, **qp)
        for m in (E.sum_input_token_type_embd_act_quantizer, E.sum_pos_embd_act_quantizer, E.LayerNorm):
            set_act_quant_axis_and_groups(m, axis=2, n_groups=None, permute=False)
        E.eval()
        with _under(PegEmbeddingsTwin()), torch.no_grad():
            pass_data_for_range_estimation([(ids,)], E, act_quant=True, weight_quant=True, max_num_batches=1)
            E.fix_ranges()
        assert E.LayerNorm.activation_quantizer.quantizer._delta.numel() == width
        return E
    _declines(block(d), ids, monkeypatch, f'd = {d}')
    _, be = _run(lambda E=block(128): E(ids), monkeypatch)
    assert be.embedding_calls == 1 and be.census == [(NAME, (2, 16), (128, 128, 128), True)]


def test_packed_batches_take_the_attention_route_with_the_switch_cpu(monkeypatch):
    """`forward_packed` under per_groups = 6: with INT8_PEG_ATTENTION alone the attention half of a packed batch stays layered
    (tests/test_peg_attention_host.py); with INT8_PEG_EMBEDDINGS also on it is the grouped class-ordered Linear over the M rows
    and the variable-length core with a grid per head, and the hidden state equals the padded forward's on the valid rows"""
    from harness.bert import pack_batch
    from quantization.fused import PackedSequences
    model = _model(1)
    ids = _ids(9, 3, 50)
    am = torch.ones(3, 50, dtype=torch.long)
    am[1, 37:] = 0
    am[2, 13:] = 0
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    M = p_ids.shape[1]
    sw = dict(INT8_PEG_ATTENTION=True, INT8_RAGGED=True, INT8_RAGGED_RECIPES=True)

    def packed(m):
        h = m.embeddings(p_ids, p_pos)
        return m.layers[0](h, PackedSequences(seq_start, max_len))

    def padded(m):
        return m.layers[0](m.embeddings(ids), ((1.0 - am.float()) * -10000.0)[:, None, None, :])
    got, be = _run(lambda: packed(model), monkeypatch, **sw)
    names = [e[0] for e in be.census]
    assert names[:3] == [NAME, 'linear_i8_cls_grouped', 'attention_i8_varlen'], names
    assert be.census[2] == ('attention_i8_varlen', (1, M, D), 'per-head') and be.census[1][1] == (1, M, D)
    want, _ = _run(lambda: padded(model), monkeypatch, **sw)
    assert torch.equal(got[0], want[am.bool()])
    _, be_off = _run(lambda: packed(model), monkeypatch, on=False, **sw)
    assert not [e for e in be_off.census if e[0] in (NAME, 'linear_i8_cls_grouped', 'attention_i8_varlen')]
