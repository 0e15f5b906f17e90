"""options.FUSED_ACT_AXIS_TRAINING where the route is not taken, on the CPU: a backend without `bias_act_quant_axis_bwd` (the CPU
oracle double), and -- on a double that has the entry and fails when it is called -- a Tanh layer, a hooked layer, an
estimating, a per-tensor and a per-channel output quantizer.  `linear_act_quant_training` answers None, and output and gradients
are the option-off ones bit for bit.  And the C entries' argument checks, which come before any device call."""
import copy
import ctypes as C

import pytest
import torch

from tests import test_act_axis_training_route as R
from tests._oracle_backend import OracleBackend


class _WithEntry(OracleBackend):
    def bias_act_quant_axis(self, *a, **kw):
        raise AssertionError('the route was taken')
    bias_act_quant_axis_bwd = bias_act_quant_axis


@pytest.mark.parametrize('decline', ['backend', 'tanh', 'hook', 'estimating', 'per_tensor', 'per_channel'])
def test_declines_keep_the_layered_line(decline):
    from quantization import _hip, options
    from quantization.fused import linear_act_quant_training
    be = OracleBackend() if decline == 'backend' else _WithEntry()
    assert options.FUSED_ACT_AXIS_TRAINING is False and hasattr(be, 'bias_act_quant_axis_bwd') == (decline != 'backend')
    prev = _hip.set_backend(be)
    try:
        _, layer, x, gy = R._site(True, decline != 'estimating', dev='cpu', act=torch.nn.Tanh() if decline == 'tanh' else None,
                                  per_column=decline != 'per_tensor', per_channel=decline == 'per_channel')
        if decline == 'hook':
            layer.register_forward_hook(lambda *a: None)
        if decline == 'estimating':
            layer.estimate_ranges_train()
        off = R._grads(copy.deepcopy(layer), x, gy)         # (copies: an estimating forward moves the ranges)
        options.FUSED_ACT_AXIS_TRAINING = True
        assert options.fused_act_axis_training(be) == (decline != 'backend')
        assert linear_act_quant_training(copy.deepcopy(layer), x.clone().requires_grad_(True)) is None
        on = R._grads(copy.deepcopy(layer), x, gy)
        assert set(on) == set(off) and all(torch.equal(on[k], off[k]) for k in off)
    finally:
        options.FUSED_ACT_AXIS_TRAINING = False
        _hip.set_backend(prev)


def test_entries_check_their_arguments_before_any_device_call():
    from quantization import _hip
    lib = _hip.load_library()
    buf = (C.c_float * 64)()                            # 16-byte aligned host memory: never dereferenced
    ptr = C.cast((C.addressof(buf) + 15) & ~15, C.c_void_p)
    desc = lambda n_params: C.byref(_hip.tq_quantizer(ptr, ptr, None, 8, 0, 0, 1e-8, n_params, 1))
    fwd = lib.tq_bias_act_quant_axis_fwd
    # (TQ_EINVAL = -1)
    assert fwd(None, ptr, ptr, 3, 8, _hip.ACT_NONE, desc(8), None) == -1
    assert fwd(ptr, ptr, ptr, 3, 8, _hip.ACT_NONE, desc(1), None) == -1
    assert fwd(ptr, ptr, ptr, 3, 8, _hip.ACT_NONE, None, None) == -1
    assert fwd(ptr, ptr, ptr, 3, 8, _hip.ACT_TANH, desc(8), None) == -1
    assert fwd(ptr, ptr, ptr, 0, 8, _hip.ACT_NONE, desc(8), None) == 0
    assert lib.tq_bias_act_quant_axis_bwd_workspace_bytes(700, 3072) == 170 * 12 * 768 * 4
