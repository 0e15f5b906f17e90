"""options.INT8_INDEX_RESIDUALS on the GPU: BERT-base (3 layers, W8A8, fixed ranges) computes the same bits with the option
on as with it off -- every hidden state and the logits, eager and as a hipGraph replay, alone and together with
options.INT8_RAGGED, packed batches and options.INT8_HEAD -- and a hidden state with a NaN row goes through a layer as it
does today.  The launches with the option on: two of the new entry per layer, none of the old tail."""
import pytest
import torch

from tests.test_bert_exact_route import _ids
from tests.test_bert_ragged_route import LAYERS, _gpu_model

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]


def _batch(B, T, pad_from):
    ids = _ids(3, B, T).cuda()
    am = torch.ones(B, T, dtype=torch.long, device='cuda')
    am[1, pad_from:] = 0                                      # one padded sample
    return ids, am


class _Hidden:
    """the hidden state after every layer of every forward while installed (instance-level wrappers, no module hooks)"""

    def __init__(self, model):
        self.model, self.outs = model, []

    def __enter__(self):
        for L in self.model.layers:
            L.forward = (lambda h, m, _f=type(L).forward, _L=L: (self.outs.append(_f(_L, h, m)), self.outs[-1])[1])
        return self

    def __exit__(self, *exc):
        for L in self.model.layers:
            del L.forward
        return False

    def take(self):
        out, self.outs = [h.clone() for h in self.outs], []
        return out


def _tail_calls(monkeypatch):
    from quantization import _hip
    log = []
    for name in ('residual_layernorm_quant', 'residual_layernorm_quant_axis', 'residual_layernorm_quant_ires'):
        orig = getattr(_hip.HipBackend, name)

        def counted(self, *a, _o=orig, _n=name, **k):
            log.append((_n, k.get('want_y', True)))
            return _o(self, *a, **k)
        monkeypatch.setattr(_hip.HipBackend, name, counted)
    return log


def _bits(t):
    return t.contiguous().view(torch.int32)


def _arms(monkeypatch, call, model, graph_args=None):
    """call() with the option off and on -> asserts equal hidden states and logits (eager; with graph_args also as a hipGraph
    replay of the option-on forward); returns the tail launches of the option-on eager forward"""
    from quantization import options
    from quantization.graphs import GraphedForward
    log = _tail_calls(monkeypatch)
    with torch.no_grad(), _Hidden(model) as hid:
        monkeypatch.setattr(options, 'INT8_INDEX_RESIDUALS', False)
        ref = call().clone()
        ref_h = hid.take()
        assert all(n != 'residual_layernorm_quant_ires' for n, _ in log)
        del log[:]
        monkeypatch.setattr(options, 'INT8_INDEX_RESIDUALS', True)
        out = call().clone()
        out_h = hid.take()
        on_log = list(log)
        assert len(ref_h) == len(out_h) == LAYERS
        assert torch.equal(_bits(out), _bits(ref)) and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out_h, ref_h))
        if graph_args is not None:
            module, args = graph_args
            g = GraphedForward(module, *args)
            static = hid.outs[-LAYERS:]                        # the capture pass: the graph's own tensors
            replay = g(*args).clone()
            torch.cuda.synchronize()
            assert torch.equal(_bits(replay), _bits(ref))
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(static, ref_h))
            hid.take()
    assert torch.isfinite(ref).all()
    return on_log


def _expect_index_form(on_log):
    assert on_log == [('residual_layernorm_quant_ires', False), ('residual_layernorm_quant_ires', True)] * LAYERS, on_log


def test_option_on_equals_option_off_eager_and_replayed(monkeypatch):
    model = _gpu_model()
    ids, am = _batch(3, 64, 40)
    on_log = _arms(monkeypatch, lambda: model(ids, am), model, graph_args=(model, (ids, am)))
    _expect_index_form(on_log)       # two new-entry launches per layer, no launch of the old tail (res_ln_quant_k)


def test_with_ragged_token_counts(monkeypatch):
    from quantization import options
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    model = _gpu_model()
    ids, am = _batch(3, 50, 33)
    _expect_index_form(_arms(monkeypatch, lambda: model(ids, am), model))


def test_through_forward_packed(monkeypatch):
    from harness.bert import pack_batch
    from quantization import options
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    model = _gpu_model()
    ids, am = _batch(3, 50, 33)
    am[2, 12:] = 0
    p_ids, p_pos, seq_start, max_len = pack_batch(ids.cpu(), am.cpu())
    args = tuple(t.cuda() for t in (p_ids, p_pos, seq_start))
    _expect_index_form(_arms(monkeypatch, lambda: model.forward_packed(*args, max_len), model))


def test_with_the_integer_head(monkeypatch):
    from quantization import options
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    model = _gpu_model()
    ids, am = _batch(3, 64, 40)
    _expect_index_form(_arms(monkeypatch, lambda: model(ids, am), model))


def test_a_nan_row_goes_through_a_layer_as_it_does_today(monkeypatch):
    """one QLayer on a tagged hidden state (values, int8 indices, row flags) whose row (0, 5) is NaN: the same output bits"""
    from quantization import options, provenance
    model = _gpu_model()
    ids, am = _batch(3, 64, 40)
    mask = (1.0 - am[:, None, None, :].float()) * -10000.0
    layer = model.layers[1]
    outs = {}
    with torch.no_grad():
        monkeypatch.setattr(options, 'INT8_INDEX_RESIDUALS', False)
        h0 = model.layers[0](model.embeddings(ids), mask)
        q, idx = provenance.of(h0)
        assert idx is not None
        h = h0.clone()
        h[0, 5] = float('nan')
        flags = torch.zeros(h.shape[:-1], dtype=torch.uint8, device='cuda')
        flags[0, 5] = 1
        provenance.tag(h, q, idx.clone(), row_nan=flags)      # (the index bytes of a NaN row mean nothing)
        log = _tail_calls(monkeypatch)
        for on in (False, True):
            monkeypatch.setattr(options, 'INT8_INDEX_RESIDUALS', on)
            outs[on] = layer(h, mask).clone()
            assert provenance.row_nan_of(h) is flags          # the record is still valid
    assert [n for n, _ in log] == ['residual_layernorm_quant'] * 2 + ['residual_layernorm_quant_ires'] * 2
    assert torch.isnan(outs[False][0, 5]).all() and int(torch.isnan(outs[False]).any(-1).sum()) == 1
    assert torch.equal(_bits(outs[True]), _bits(outs[False]))
