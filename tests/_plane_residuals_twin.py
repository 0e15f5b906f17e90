"""TEST INFRASTRUCTURE: the exact CPU twin that answers `residual_layernorm_quant_pres` (options.INT8_PLANE_RESIDUALS) and the
reference tests/test_fused_ln_pres.py holds tq_residual_layernorm_quant_pres_fwd to.

    residual  fp32 as given; from int8 indices scale * ((idx + 128) - zero_point); from byte planes scale * ((256 (hi + 128) +
              (lo + 128)) - zero_point) -- (scale, zero_point) = (max(delta, eps), clamp(round(zero_float), 0, 2^n_bits - 1)),
              one exact fp32 subtraction and one rounded fp32 multiplication; flagged rows NaN
    y, idx    tests/_exact_backend.ln_tail_chain on that residual (the reference of every tail entry)
    planes    the two bytes of the index the chain's output quantizer computed, as tests/_planes_twin takes them
    flags     the rows of y that are NaN as a whole

`PlaneResidualsTwin` binds it to the backend method on top of PlanesTwin.  Nothing outside tests/ imports this."""
import torch

from tests._exact_backend import _p, ln_tail_chain
from tests._planes_twin import PlanesTwin


def dequantized_residual(q_res, res_idx=None, res_planes=None, res_row_nan=None):
    """q_res: backend 7-tuple of a per-tensor asymmetric linear-domain grid -> fp32 residual of the indices' / planes' shape"""
    delta, zf, _, n_bits, symmetric, log_domain, eps = q_res
    assert not symmetric and not log_domain and delta.numel() == 1 and (res_idx is None) != (res_planes is None)
    if res_idx is not None:
        assert n_bits <= 8 and res_idx.dtype == torch.int8
        index = res_idx.float() + 128.0
    else:
        hi, lo = res_planes
        assert n_bits <= 16 and hi.dtype == lo.dtype == torch.int8 and hi.shape == lo.shape
        index = (256 * (hi.int() + 128) + (lo.int() + 128)).float()                 # < 2^16: exact
    scale = torch.maximum(delta.detach().float().reshape(()), torch.tensor(eps, dtype=torch.float32))
    zp = torch.clamp(torch.round(zf.detach().float().reshape(())), 0, 2 ** n_bits - 1)
    r = scale * (index - zp)
    if res_row_nan is not None:
        assert res_row_nan.dtype == torch.uint8 and res_row_nan.shape == r.shape[:-1]
        r[res_row_nan.bool()] = float('nan')
    return r


def pres_tail_reference(a, r, q1, q2, w, b, eps, q3):
    """a, r fp32 [rows, d]; q1..q3 the chains' quantizer specs (tests/_exact_backend._p), q3 present and asymmetric.
    -> (y fp32, index of y as float (NaN on NaN rows), (hi, lo) int8, row_nan uint8 [rows])"""
    assert q3 is not None and not q3[3]
    y, idx, _ = ln_tail_chain(a, r, q1, q2, w, b, eps, q3)
    i = torch.nan_to_num(idx, nan=0.0).long()                         # NaN rows: their indices / planes are unspecified
    return y, idx, (((i >> 8) - 128).to(torch.int8), ((i & 255) - 128).to(torch.int8)), torch.isnan(y).any(-1).to(torch.uint8)


class PlaneResidualsTwin(PlanesTwin):
    """PlanesTwin with `residual_layernorm_quant_pres`; every call leaves a census entry
    ('residual_layernorm_quant_pres', shape of the GEMM output, residual kind 'f32' | 'idx' | 'planes', flags given, want_y,
    want_idx, want_planes)"""
    name = 'exact-twin-plane-residuals'

    def residual_layernorm_quant_pres(self, dense_out, residual, res_idx, res_planes, q_res, res_row_nan, q_dense, q_sum,
                                      ln_weight, ln_bias, ln_eps, q_out, want_y=True, want_idx=False, want_planes=False):
        d = dense_out.shape[-1]
        assert dense_out.dtype == torch.float32
        assert (residual is not None) + (res_idx is not None) + (res_planes is not None) == 1
        assert res_row_nan is None or residual is None
        kind = 'f32' if residual is not None else 'idx' if res_idx is not None else 'planes'
        # the two forms of the entry
        if kind == 'planes':
            assert want_y and not want_planes, 'planes in: y [, idx] out'
        else:
            assert want_planes and not want_y and not want_idx, 'fp32 / indices in: planes out alone'
        assert q_out is not None and not q_out[4] and not q_out[5] and q_out[3] <= (16 if want_planes else 8 if want_idx else 24)
        for q in (q_dense, q_sum, q_out):
            assert q is None or q[0].numel() == 1, 'per-tensor entry point'
        self._count('residual_layernorm_quant_pres', tuple(dense_out.shape), kind, res_row_nan is not None, want_y, want_idx,
                    want_planes)
        self.tail_bindings.append(tuple(None if q is None else q[0].data_ptr() for q in (q_dense, q_sum, q_out)))
        if residual is None:
            for t in ((res_idx,) if res_idx is not None else res_planes):
                assert t.shape == dense_out.shape and t.is_contiguous()
            residual = dequantized_residual(q_res, res_idx, res_planes, res_row_nan)
        assert residual.dtype == torch.float32 and residual.shape == dense_out.shape
        y, idx, planes, row_nan = pres_tail_reference(dense_out.detach().reshape(-1, d), residual.detach().reshape(-1, d),
                                                      _p(q_dense), _p(q_sum), ln_weight.detach().float(),
                                                      ln_bias.detach().float(), ln_eps, _p(q_out))
        s = dense_out.shape
        idx8 = (torch.nan_to_num(idx, nan=128.0) - 128).to(torch.int8).reshape(s) if want_idx else None
        return (y.reshape(s) if want_y else None, idx8, tuple(p.reshape(s) for p in planes) if want_planes else None,
                row_nan.reshape(s[:-1]))


class NoPlaneResidualsTwin(PlanesTwin):
    """the parent commit's double: no plane-residual tail"""
