"""options.INT8_MOBILE_EMBEDDINGS on the GPU: a 2-layer W4A4 harness MobileBERT (built like tests/test_mobilebert_e2e._build)
with fixed ranges on the default integer route.  With the switch on the embedding output AND the last hidden state equal a
CPU twin (tests/_mobile_embeddings_twin.py) that starts from the input ids as well -- no fp32 GEMM is left in front of the
encoder --, eager and as a hipGraph replay; the block is one launch and layer 1's input bottlenecks take the grouped launch.
[2, 50]: a ragged token count (options.INT8_RAGGED keeps the encoder's Linears and attention core on the integer route; the
grouped bottleneck launch takes whole 64-row tiles only, so the census of the grouped launch is stated at [8, 128])."""
import copy

import pytest
import torch

from tests._mobile_embeddings_twin import MobileEmbeddingsMethod
from tests._ragged_twin import RaggedTwin

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]

LAYERS = 2
_MODELS = {}


class _Twin(MobileEmbeddingsMethod, RaggedTwin):
    name = 'exact-twin-mobile-embeddings'


class _Encoder(torch.nn.Module):
    """ids -> (embedding output, last hidden state)"""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, ids):
        from harness.bert import constant
        e = h = self.model.embeddings(ids)
        mask = constant('mask', ids.shape[0], ids.shape[1], ids.device)
        for layer in self.model.layers:
            h = layer(h, mask)
        return e, h


def _ids(B, T):
    return torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(B * 1000 + T))


def _model(B, T):
    """calibrated once per shape on its own ids (calibrating forwards are layered), ranges fixed"""
    if (B, T) not in _MODELS:
        from tests.test_mobilebert_e2e import _build, _calibrate_and_run
        model, _ = _build('cuda', num_layers=LAYERS)
        _calibrate_and_run(model, _ids(B, T))
        _MODELS[(B, T)] = model
    return _MODELS[(B, T)]


def _counted(monkeypatch, names):
    from quantization import _hip
    seen = {n: 0 for n in names}
    for n in names:
        def counted(self, *a, _orig=getattr(_hip.HipBackend, n), _n=n, **k):
            seen[_n] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(_hip.HipBackend, n, counted)
    return seen


@pytest.mark.parametrize('B,T', [(2, 50), (8, 128)])
def test_forward_equals_cpu_twin_from_the_ids_on(B, T, monkeypatch):
    from quantization import _hip, options
    from quantization.graphs import GraphedForward
    assert options.INT8_LINEAR == 'auto' and options.INT8_MOBILE_EMBEDDINGS is False
    model, ids = _model(B, T), _ids(B, T)
    twin = _Encoder(copy.deepcopy(model).cpu())
    monkeypatch.setattr(options, 'INT8_MOBILE_EMBEDDINGS', True)
    monkeypatch.setattr(options, 'INT8_RAGGED', (B * T) % 64 != 0)
    seen = _counted(monkeypatch, ('mobile_embeddings_nonorm_quant', 'linear_i8_nonorm_grouped'))
    run = _Encoder(model)
    with torch.no_grad():
        e_gpu, h_gpu = run(ids.cuda())
        assert seen['mobile_embeddings_nonorm_quant'] == 1
        if (B * T) % 64 == 0:
            assert seen['linear_i8_nonorm_grouped'] == LAYERS             # layer 1 included: its input has provenance now
        cpu_be = _Twin(rules=_hip.backend())
        prev = _hip.set_backend(cpu_be)
        try:
            e_cpu, h_cpu = twin(ids)
        finally:
            _hip.set_backend(prev)
        assert [c for c in cpu_be.census if c[0] == 'mobile_embeddings_nonorm_quant'] == [('mobile_embeddings_nonorm_quant', (B, T), True)]
        assert torch.isfinite(h_gpu).all()
        assert torch.equal(e_gpu.cpu(), e_cpu) and torch.equal(h_gpu.cpu(), h_cpu)
        graphed = GraphedForward(run, ids.cuda())
        for _ in range(3):                                                # several replays against the eager result
            e_rep, h_rep = graphed(ids.cuda())
            torch.cuda.synchronize()
            assert torch.equal(e_rep, e_gpu) and torch.equal(h_rep, h_gpu)


def test_switch_off_keeps_the_layered_block(monkeypatch):
    from quantization import fused, options
    model, ids = _model(8, 128), _ids(8, 128).cuda()
    E = model.embeddings
    with torch.no_grad():
        monkeypatch.setattr(options, 'INT8_MOBILE_EMBEDDINGS', True)
        monkeypatch.setattr(fused, 'mobile_embeddings_nonorm_quant', lambda *a: None)       # declined: the layered lines
        layered = E(ids)

        def never(*a):
            raise AssertionError('the helper was called with the switch off')
        monkeypatch.setattr(options, 'INT8_MOBILE_EMBEDDINGS', False)
        monkeypatch.setattr(fused, 'mobile_embeddings_nonorm_quant', never)
        off = E(ids)
    assert torch.equal(off, layered)
