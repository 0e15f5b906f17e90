"""tq_residual_layernorm_quant_axis_bwd validates its arguments before any HIP call (the pointers are never dereferenced), and
options.FUSED_LN_AXIS_TRAINING is off by default and needs a backend with the method."""
import ctypes as C

import pytest

from tests._oracle_backend import OracleBackend

BUF, D = 1 << 20, 768                                  # an aligned address nobody reads


def _call(lib, q=(None, None, None), a=BUF, d=D, rows=4, gq=(None, None, None), gw=None, ws=None, ws_bytes=0):
    from quantization import _hip
    mk = lambda n: None if n is None else C.byref(_hip.tq_quantizer(BUF, BUF, None, 8, 0, 0, 1e-8, *n))
    return lib.tq_residual_layernorm_quant_axis_bwd(a, BUF, BUF, rows, d, mk(q[0]), mk(q[1]), BUF, BUF, 1e-12, mk(q[2]), BUF, BUF,
                                                    gw, None, *gq, None, ws, ws_bytes, None)


@pytest.mark.parametrize('kw,code,word', [
    (dict(rows=0, a=None), 0, None),                                                     # empty problem: no-op
    (dict(a=None), -1, 'NULL'),
    (dict(a=BUF + 4), -1, 'alignment'),
    (dict(d=48, q=((48, 1), None, None)), -4, 'row length'),                             # TQ_EUNSUPPORTED
    (dict(q=((6, 1), None, None)), -1, 'n_params'),
    (dict(q=(None, (2 * D, 1), None)), -1, None),
    (dict(q=(None, None, (D, 2))), -1, None),
    (dict(q=((D, 1), None, None), gq=(None, BUF, None)), -1, 'absent quantizer'),
    (dict(q=((D, 1), None, None), gq=(BUF, None, None)), -3, 'workspace'),               # TQ_EWORKSPACE: NULL
    (dict(gw=BUF, ws=BUF, ws_bytes='short'), -3, 'workspace'),
])
def test_argument_errors_before_any_launch(kw, code, word):
    from quantization import _hip
    lib = _hip.load_library()
    need = lib.tq_residual_layernorm_quant_axis_bwd_workspace_bytes(4, D)
    assert need == 1 * 8 * D * 4 + 6 * D * 8 and lib.tq_residual_layernorm_quant_axis_bwd_workspace_bytes(4, 48) == 0
    if kw.get('ws_bytes') == 'short':
        kw = dict(kw, ws_bytes=need - 1)
    assert _call(lib, **kw) == code and (word is None or word in lib.tq_last_error().decode())


def test_switch_is_off_by_default_and_needs_the_method():
    from quantization import _hip, options
    assert options.FUSED_LN_AXIS_TRAINING is False and not options.fused_ln_axis_training(_hip.HipBackend)
    options.FUSED_LN_AXIS_TRAINING = True
    try:
        assert options.fused_ln_axis_training(_hip.HipBackend) and not options.fused_ln_axis_training(OracleBackend())
    finally:
        options.FUSED_LN_AXIS_TRAINING = False
