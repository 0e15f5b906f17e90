"""BERT-base with the README's mixed-precision recipe ({'x': 16, 'h': 16, 'y': 16}) on the GPU: on the default route the
first feed-forward Linear of every layer takes its 16-bit per-tensor input (site x) as two byte planes (tq_quantize_hilo_fwd)
through the 16-bit integer Linear (tq_linear_i16x8_fwd), index-only; the second consumes those indices; both residual +
LayerNorm tails stay fused.  A second eager run and a hipGraph replay equal the first bit for bit, and the output stays
close to the layered route's.

Measured on MI355X, 3 layers at [8,128]: max |default - layered| = 1.6012e-02 with max |layered| = 4.5793e-01 (3.5 %;
the bar is 5 %)."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]


def _model(num_layers):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=num_layers, **qp)
    apply_quant_dict(model, {'x': 16, 'h': 16, 'y': 16})
    return model.cuda().eval()


def _ids(seed, B=8, T=128):
    return torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(seed)).cuda()


def _counted(monkeypatch):
    """launch log of the backend methods the statement is about: (name, K of the input, want_y)"""
    from quantization import _hip
    log = []

    def wrap(name, info):
        orig = getattr(_hip.HipBackend, name)

        def counted(self, *a, **k):
            log.append((name,) + info(a, k))
            return orig(self, *a, **k)
        monkeypatch.setattr(_hip.HipBackend, name, counted)
    wrap('quantize_hilo', lambda a, k: (a[0].shape[-1], None))
    wrap('linear_i16x8', lambda a, k: (a[0].shape[-1], k.get('want_y', True)))
    wrap('linear_i8', lambda a, k: (a[0].shape[-1], k.get('want_y', True)))
    wrap('residual_layernorm_quant', lambda a, k: (a[0].shape[-1], None))
    return log


def _out(t):
    return t[0] if isinstance(t, (tuple, list)) else t


def test_mp16_recipe_ffn_on_the_integer_route(monkeypatch):
    from quantization import options
    from quantization.graphs import GraphedForward
    from utils.utils import pass_data_for_range_estimation
    log = _counted(monkeypatch)
    L = 3
    model = _model(L)
    with torch.no_grad():
        pass_data_for_range_estimation([(_ids(10),), (_ids(11),)], model, act_quant=True, weight_quant=True, max_num_batches=2)
        model.fix_ranges()
    assert not [e for e in log if e[0] in ('quantize_hilo', 'linear_i16x8')]      # calibrating forwards stay layered
    ids = _ids(3)
    saved = options.INT8_LINEAR
    try:
        with torch.no_grad():
            options.INT8_LINEAR = False
            layered = _out(model(ids)).clone()
            assert not [e for e in log if e[0] in ('quantize_hilo', 'linear_i16x8')]
            options.INT8_LINEAR = 'auto'
            del log[:]
            fast = _out(model(ids)).clone()
            per_layer = lambda name, *rest: sum(1 for e in log if e[0] == name and e[1:] == rest)
            assert per_layer('quantize_hilo', 768, None) == L                     # one pair of byte planes per layer
            assert per_layer('linear_i16x8', 768, False) == L                     # FFN1: index-only
            assert sum(1 for e in log if e[0] == 'linear_i16x8') == L
            assert per_layer('linear_i8', 3072, True) == L                        # FFN2 on FFN1's indices
            assert per_layer('residual_layernorm_quant', 768, None) == 2 * L      # both tails of every layer
            again = _out(model(ids)).clone()
        assert torch.equal(fast, again)
        g = GraphedForward(model, ids)
        replay = _out(g(ids)).clone()
        assert torch.equal(replay, fast)
        d = (fast.float() - layered.float()).abs()
        print('max |default - layered| = %.4e, max |layered| = %.4e' % (float(d.max()), float(layered.abs().max())))
        assert float(d.max()) <= 0.05 * float(layered.abs().max())
        # an observed feed-forward Linear keeps the layered modules; so does autograd
        n = sum(1 for e in log if e[0] == 'linear_i16x8')
        h = model.layers[0].intermediate[0].register_forward_hook(lambda m, a, o: None)
        try:
            with torch.no_grad():
                model(ids)
        finally:
            h.remove()
        assert sum(1 for e in log if e[0] == 'linear_i16x8') == n + L - 1
        options.INT8_LINEAR = True
        model(ids)
        assert sum(1 for e in log if e[0] == 'linear_i16x8') == n + L - 1
    finally:
        options.INT8_LINEAR = saved
