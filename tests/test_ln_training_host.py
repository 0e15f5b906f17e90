"""options.FUSED_LN_TRAINING with a backend that has no `residual_layernorm_quant_bwd` (the CPU oracle double): the helper runs
the layered modules and its gradients are the option-off ones, bit for bit.  The switch defaults to off."""
import torch

from tests import test_ln_training_route as R
from tests._oracle_backend import OracleBackend


def test_backend_without_the_backward_keeps_the_layered_line():
    from quantization import _hip, options
    assert options.FUSED_LN_TRAINING is False and not options.fused_ln_training(OracleBackend())      # off by default
    prev = _hip.set_backend(OracleBackend())
    try:
        assert not hasattr(_hip.backend(), 'residual_layernorm_quant_bwd')
        site = R._block(True, dev='cpu')
        off = R._grads(*site)
        options.FUSED_LN_TRAINING = True
        on = R._grads(*site)
        assert len(on) == 10 and all(torch.equal(on[k], off[k]) for k in off)
    finally:
        options.FUSED_LN_TRAINING = False
        _hip.set_backend(prev)
