"""BERT-base with the README's PEG recipe ({'x', 'h', 'y'}: 'ng6') on the GPU: the first feed-forward Linear of every
layer takes its per-embedding-group input (site x) through the class-ordered integer Linear (tq_linear_i8_cls_fwd) on
the default route, a hipGraph replay equals the eager forward bit for bit, and the output stays close to the layered
route's.  A hook on the site or autograd keeps the layered route."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(num_layers):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=num_layers, **qp)
    apply_quant_dict(model, {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'})
    return model.cuda().eval()


def _ids(seed, B=8, T=128):
    return torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _counted(monkeypatch):
    from quantization import _hip
    n = [0]
    orig = _hip.HipBackend.linear_i8_cls

    def counted(self, *a, **k):
        n[0] += 1
        return orig(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, 'linear_i8_cls', counted)
    return n


def _calibrated(num_layers):
    from utils.utils import pass_data_for_range_estimation
    model = _model(num_layers)
    with torch.no_grad():
        pass_data_for_range_estimation([(_ids(10),), (_ids(11),)], model, act_quant=True, weight_quant=True,
                                       max_num_batches=2)
        model.fix_ranges()
    return model


def _out(t):
    return t[0] if isinstance(t, (tuple, list)) else t


def test_peg_recipe_ffn1_on_the_integer_route(monkeypatch):
    from quantization import options
    from quantization.graphs import GraphedForward
    n = _counted(monkeypatch)
    model = _calibrated(3)
    assert n[0] == 0                                        # calibrating forwards: per-tensor only
    ids = _ids(3)
    saved = options.INT8_LINEAR
    try:
        with torch.no_grad():
            options.INT8_LINEAR = False
            layered = _out(model(ids)).clone()
            assert n[0] == 0
            options.INT8_LINEAR = 'auto'
            fast = _out(model(ids)).clone()
            assert n[0] == 3                                # FFN1 of every layer
            again = _out(model(ids)).clone()
        assert torch.equal(fast, again)
        g = GraphedForward(model, ids)
        replay = _out(g(ids)).clone()
        assert torch.equal(replay, fast)
        d = (fast.float() - layered.float()).abs()
        assert float(d.max()) <= 0.05 * float(layered.abs().max())
        # an observer on a stage the fused launch would skip keeps that Linear layered
        k = n[0]
        h = model.layers[0].intermediate[0].activation_quantizer.register_forward_hook(lambda m, a, o: None)
        try:
            with torch.no_grad():
                model(ids)
        finally:
            h.remove()
        assert n[0] == k + 2
        # autograd: layered
        options.INT8_LINEAR = True
        model(ids)
        assert n[0] == k + 2
    finally:
        options.INT8_LINEAR = saved
