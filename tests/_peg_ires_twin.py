"""TEST INFRASTRUCTURE: the exact CPU twin that answers `residual_layernorm_quant_axis_ires` (options.INT8_PEG_INDEX_RESIDUALS)
and the residual tests/test_fused_ln_axis_ires.py hands the existing per-column tail.

    residual  fp32 as given; from int8 indices scale_c * ((idx + 128) - zero_point_c) -- (scale_c, zero_point_c) =
              (max(delta_c, eps), clamp(round(zero_float_c), 0, 2^n_bits - 1)) per tensor or per column, one exact fp32
              subtraction and one rounded fp32 multiplication; flagged rows NaN
    y, idx    ExactBackend._tail on that residual (tests/_exact_backend.ln_tail_chain: the reference of every tail entry)
    flags     the rows of y that are NaN as a whole

`PegIresTwin` binds it to the backend method on top of ExactBackend.  Nothing outside tests/ imports this."""
import torch

from tests._exact_backend import ExactBackend


def dequantized_axis_residual(q_res, res_idx, res_row_nan=None):
    """q_res: backend 7-tuple of an asymmetric linear-domain <= 8-bit grid, per-tensor or per-column (buffers of d elements
    along the last axis) -> fp32 residual of the indices' shape"""
    delta, zf, _, n_bits, symmetric, log_domain, eps = q_res
    d = res_idx.shape[-1]
    assert not symmetric and not log_domain and n_bits <= 8 and res_idx.dtype == torch.int8
    assert delta.numel() in (1, d) and zf.numel() == delta.numel()
    scale = torch.maximum(delta.detach().float().reshape(-1), torch.tensor(eps, dtype=torch.float32, device=delta.device))
    zp = torch.clamp(torch.round(zf.detach().float().reshape(-1)), 0, 2 ** n_bits - 1)
    r = scale * ((res_idx.float() + 128.0) - zp)
    if res_row_nan is not None:
        assert res_row_nan.dtype == torch.uint8 and res_row_nan.shape == r.shape[:-1]
        r[res_row_nan.bool()] = float('nan')
    return r


class PegIresTwin(ExactBackend):
    """ExactBackend with `residual_layernorm_quant_axis_ires`; every call leaves a census entry
    ('residual_layernorm_quant_axis_ires', shape of the GEMM output, parameters per quantizer (q_dense, q_sum, q_out), residual
    kind 'f32' | 'idx', parameters of the residual grid or None, flags given, want_y, want_idx)"""
    name = 'exact-twin-peg-index-residuals'

    def residual_layernorm_quant_axis_ires(self, dense_out, residual, res_idx, q_res, res_row_nan, q_dense, q_sum, ln_weight,
                                           ln_bias, ln_eps, q_out, want_y=True, want_idx=True):
        d = dense_out.shape[-1]
        assert dense_out.dtype == torch.float32 and d in (64, 128, 256, 384, 512, 768)
        assert (residual is None) != (res_idx is None) and (res_row_nan is None or res_idx is not None)
        assert want_y or want_idx
        assert not want_idx or (q_out is not None and not q_out[4] and not q_out[5] and q_out[3] <= 8)
        self._count('residual_layernorm_quant_axis_ires', tuple(dense_out.shape),
                    tuple(None if q is None else q[0].numel() for q in (q_dense, q_sum, q_out)),
                    'f32' if residual is not None else 'idx', None if q_res is None else q_res[0].numel(),
                    res_row_nan is not None, want_y, want_idx)
        if res_idx is not None:
            assert res_idx.shape == dense_out.shape and res_idx.is_contiguous()
            residual = dequantized_axis_residual(q_res, res_idx, res_row_nan)
        assert residual.dtype == torch.float32 and residual.shape == dense_out.shape
        if q_out is not None and not q_out[4]:
            y, idx = self._tail(dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out, True)
        else:
            y, idx = self._tail(dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out, False), None
        return (y if want_y else None), (idx if want_idx else None), torch.isnan(y).any(-1).to(torch.uint8)


class NoPegIresTwin(ExactBackend):
    """the parent commit's double: no per-column index-residual tail"""
