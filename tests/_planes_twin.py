"""TEST INFRASTRUCTURE: the exact CPU twin that answers `residual_layernorm_quant_planes` (options.INT8_PLANE_TAILS) and the
reference tests/test_fused_ln_planes.py holds tq_residual_layernorm_quant_planes_fwd to.

    y       tests/_exact_backend.ln_tail_chain with the statistics in the kernels' summation order: the reference of
            tq_residual_layernorm_quant_fwd, so "y equals the existing tail" holds for the twin by construction
    planes  the two bytes of the index that chain's output quantizer computed (oracle/tq_oracle.fake_quant), hi = (index >> 8)
            - 128, lo = (index & 255) - 128 -- the index the tail holds, not one re-derived from y

`PlanesTwin` binds it to the backend method on top of Skinny16Twin (the head behind a 16-bit hidden state reads the planes
through `linear_i16x8_skinny`).  Nothing outside tests/ imports this."""
import torch

from tests._exact_backend import _p, ln_tail_chain
from tests._skinny16_twin import Skinny16Twin


def planes_tail_reference(a, r, q1, q2, w, b, eps, q3):
    """a, r fp32 [rows, d]; q1..q3: the chains' quantizer specs (tests/_exact_backend._p), q3 present, asymmetric, <= 16 bits.
    -> (y fp32 [rows, d], (hi, lo) int8 [rows, d])"""
    assert q3 is not None and not q3[3] and 1 <= q3[2] <= 16
    y, idx, _ = ln_tail_chain(a, r, q1, q2, w, b, eps, q3)
    idx = torch.nan_to_num(idx, nan=0.0).long()                       # NaN rows: their planes are unspecified
    return y, (((idx >> 8) - 128).to(torch.int8), ((idx & 255) - 128).to(torch.int8))


class PlanesTwin(Skinny16Twin):
    """Skinny16Twin with `residual_layernorm_quant_planes`; every call leaves a census entry
    ('residual_layernorm_quant_planes', shape of the GEMM output, n_bits of the output grid)"""
    name = 'exact-twin-planes'

    def residual_layernorm_quant_planes(self, dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out):
        d = dense_out.shape[-1]
        assert dense_out.dtype == torch.float32 and residual.dtype == torch.float32 and residual.shape == dense_out.shape
        assert q_out is not None and not q_out[4] and not q_out[5] and 1 <= q_out[3] <= 16
        for q in (q_dense, q_sum, q_out):
            assert q is None or q[0].numel() == 1, 'per-tensor entry point'
        self._count('residual_layernorm_quant_planes', tuple(dense_out.shape), int(q_out[3]))
        self.tail_bindings.append(tuple(None if q is None else q[0].data_ptr() for q in (q_dense, q_sum, q_out)))
        y, (hi, lo) = planes_tail_reference(dense_out.detach().reshape(-1, d), residual.detach().reshape(-1, d), _p(q_dense),
                                            _p(q_sum), ln_weight.detach().float(), ln_bias.detach().float(), ln_eps, _p(q_out))
        return y.reshape(dense_out.shape), (hi.reshape(dense_out.shape), lo.reshape(dense_out.shape))


class NoPlanesTwin(Skinny16Twin):
    """the parent commit's double: no plane tail"""
