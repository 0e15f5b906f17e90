"""options.FUSED_NONORM_TRAINING without a GPU: off by default, needs a backend with the backward entry, and with such a backend
missing the helper returns the layered result bit for bit."""
import torch

from tests._oracle_backend import OracleBackend
from tests.test_ln_training_route import _block, _grads


def test_switch_is_off_by_default_and_needs_the_entry():
    from quantization import _hip, options
    assert options.FUSED_NONORM_TRAINING is False and not options.fused_nonorm_training(_hip.HipBackend)
    options.FUSED_NONORM_TRAINING = True
    try:
        assert options.fused_nonorm_training(_hip.HipBackend) and not options.fused_nonorm_training(OracleBackend())
    finally:
        options.FUSED_NONORM_TRAINING = False


def test_backend_without_the_entry_keeps_the_layered_line():
    from quantization import _hip, options
    prev = _hip.set_backend(OracleBackend())
    try:
        blk, x, r, gy = _block(True, dev='cpu', nonorm=True)
        off = _grads(blk, x, r, gy)
        options.FUSED_NONORM_TRAINING = True
        on = _grads(blk, x, r, gy)
    finally:
        options.FUSED_NONORM_TRAINING = False
        _hip.set_backend(prev)
    assert set(on) == set(off) and len(on) == 10 and all(torch.equal(on[k], off[k]) for k in on)
