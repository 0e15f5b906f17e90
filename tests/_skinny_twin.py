"""TEST INFRASTRUCTURE: the reference chain of tq_linear_i8_skinny_fwd and the exact CPU twin that answers
`linear_i8_skinny` with it (options.INT8_HEAD: BERT's pooler and classifier).

    pre   = oracle/tq_int_oracle.c lin_pre through oracle.int_oracle.linear_i8 (activation 0, no quantizer)
    act   = none | ReLU (oracle code 1) | GELU = oracle code 4, the correctly rounded erf form |
            Tanh = np.tanh(pre as float64) narrowed once to fp32 (written here: the oracle's code 3 is tanhf)
    q_out = oracle.int_oracle.epilogue (q_index: IEEE division, rne, clamp; scale * (index - zp))

tests/test_linear_i8_skinny.py holds the kernel to `skinny_reference`; `SkinnyTwin` binds the same function to the backend
method, so the twin computes what the kernel was tested against.  Nothing outside tests/ imports this."""
import numpy as np
import torch

from oracle import int_oracle
from tests._exact_backend import ExactBackend

ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH = 0, 1, 2, 3


def skinny_pre(x_idx, w_idx, bias, x_q, w_delta, w_eps):
    """fp32 [M, N] pre-activations; x_idx int8 [M, K] (any strides), x_q = (delta, zero_float, n_bits, eps) as floats"""
    return int_oracle.linear_i8(x_idx.contiguous(), w_idx, bias, x_q, w_delta, w_eps, 0, None)[0]


def skinny_epilogue(pre, activation, q7):
    """-> (y fp32, int8(index - 128)) of pre's shape; q7: the backend 7-tuple with python scalars, or None"""
    if activation == ACT_TANH:
        t = torch.from_numpy(np.tanh(pre.numpy().astype(np.float64)).astype(np.float32))
        return int_oracle.epilogue(t, 0, q7)
    return int_oracle.epilogue(pre, {ACT_NONE: 0, ACT_RELU: 1, ACT_GELU: 4}[activation], q7)


def skinny_reference(x_idx, w_idx, bias, x_q, w_delta, w_eps, activation, q7):
    return skinny_epilogue(skinny_pre(x_idx, w_idx, bias, x_q, w_delta, w_eps), activation, q7)


class SkinnyTwin(ExactBackend):
    """ExactBackend with `linear_i8_skinny`; every call leaves a census entry
    ('linear_i8_skinny', M, N, K, activation, strides of x_idx, output quantizer present?, want_y)"""
    name = 'exact-twin-skinny'
    SKINNY_MAX_ROWS, SKINNY_MAX_K = 256, 16384

    def linear_i8_skinny(self, x_idx, w_idx, w_rowsum, bias, x_q, w_delta, w_eps, activation, q_out, out_dtype, want_idx=False,
                         want_y=True):
        assert x_idx.dim() == 2 and x_idx.dtype == torch.int8 and x_idx.stride(1) == 1
        M, K = x_idx.shape
        self._count('linear_i8_skinny', M, w_idx.shape[0], K, int(activation), tuple(x_idx.stride()), q_out is not None, want_y)
        y, yi = skinny_reference(x_idx, w_idx, bias, tuple(float(v) for v in x_q), w_delta, w_eps, int(activation),
                                 self._q7(q_out))
        y = y.to(out_dtype) if want_y else None
        return (y, yi) if want_idx else y
