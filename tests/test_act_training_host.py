"""options.FUSED_ACT_TRAINING where the route is not taken, on the CPU: a backend without `bias_act_quant_bwd` (the CPU oracle
double), and -- on a double that has the entry and fails when it is called -- a Tanh layer, a hooked layer and an estimating
output quantizer.  `linear_act_quant_training` answers None, and output and gradients are the option-off ones bit for bit."""
import copy

import pytest
import torch

from tests import test_act_training_route as R
from tests._oracle_backend import OracleBackend


class _WithEntry(OracleBackend):
    def bias_act_quant(self, *a, **kw):
        raise AssertionError('the route was taken')
    bias_act_quant_bwd = bias_act_quant


@pytest.mark.parametrize('decline', ['backend', 'tanh', 'hook', 'estimating'])
def test_declines_keep_the_layered_line(decline):
    from quantization import _hip, options
    from quantization.fused import linear_act_quant_training
    be = OracleBackend() if decline == 'backend' else _WithEntry()
    assert options.FUSED_ACT_TRAINING is False and hasattr(be, 'bias_act_quant_bwd') == (decline != 'backend')
    prev = _hip.set_backend(be)
    try:
        _, layer, x, gy = R._site('gelu', decline != 'estimating', dev='cpu', act=torch.nn.Tanh() if decline == 'tanh' else None)
        if decline == 'hook':
            layer.register_forward_hook(lambda *a: None)
        if decline == 'estimating':
            layer.estimate_ranges_train()
        off = R._grads(copy.deepcopy(layer), x, gy)         # (copies: an estimating forward moves the ranges)
        options.FUSED_ACT_TRAINING = True
        assert options.fused_act_training(be) == (decline != 'backend')
        assert linear_act_quant_training(copy.deepcopy(layer), x.clone().requires_grad_(True)) is None
        on = R._grads(copy.deepcopy(layer), x, gy)
        assert set(on) == set(off) and all(torch.equal(on[k], off[k]) for k in off)
    finally:
        options.FUSED_ACT_TRAINING = False
        _hip.set_backend(prev)
