"""options.FUSED_SOFTMAX_TRAINING with a backend that has no `scores_softmax_quant_bwd` (the CPU oracle double): a training
forward takes the layered lines and its gradients are the option-off ones, bit for bit."""
import torch

from tests import test_softmax_training_route as R
from tests._oracle_backend import OracleBackend


def test_backend_without_the_backward_keeps_the_layered_chain():
    from quantization import _hip, options
    prev = _hip.set_backend(OracleBackend())
    try:
        assert not hasattr(_hip.backend(), 'scores_softmax_quant_bwd')
        sites = R._sites(True, 32, 'cpu')
        off = R._grads(*sites)
        options.FUSED_SOFTMAX_TRAINING = True
        on = R._grads(*sites)
        assert len(on) == 6 and all(torch.equal(a, b) for a, b in zip(on, off))
    finally:
        options.FUSED_SOFTMAX_TRAINING = False
        _hip.set_backend(prev)
