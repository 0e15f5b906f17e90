"""Host logic of the integer route for 16-bit activation inputs (mixed precision W8A16), replayed on the CPU: BERT with the
README's recipe ({'x': 16, 'h': 16, 'y': 16}) sends the first feed-forward Linear of every layer -- its input is site x, a
16-bit per-tensor grid -- through `quantize_hilo` and `linear_i16x8`, index-only, and the second feed-forward Linear
consumes those indices; calibrating forwards, autograd, INT8_LINEAR = False and observed modules keep the layered route.
The doubles below restate the formula of include/tq_hip.h (tests/test_linear_i16x8.py holds the kernels to it bit for bit
on the GPU)."""
import numpy as np
import pytest
import torch

from tests._oracle_backend import OracleBackend


class _Mp16Oracle(OracleBackend):
    """OracleBackend + the byte-plane producer and the 16-bit integer Linear"""
    STAIR_BINS, STAIR_BINS_BIG = 768, 1536

    def __init__(self):
        self.hilo_calls, self.x16_calls, self.i8_calls = [], [], []

    def i16x8_stair_bins_for(self, M, N, K):
        return None

    def quantize_hilo(self, x, q4):
        from oracle import tq_oracle as O
        delta, zf, n_bits, eps = q4
        idx, _ = O.fake_quant(x.float(), delta.reshape(()), zf.reshape(()), n_bits, False, False, eps, 'linear')
        idx = idx.long()
        self.hilo_calls.append(tuple(x.shape))
        return ((idx >> 8) - 128).to(torch.int8), ((idx & 255) - 128).to(torch.int8)

    def linear_i16x8(self, x_hi, x_lo, w_idx, w_rowsum, bias, x_q, w_delta, w_eps, activation, q_out, out_dtype,
                     want_idx=False, want_y=True, stair=None):
        from oracle import tq_oracle as O
        K, N = x_hi.shape[-1], w_idx.shape[0]
        delta, zf, n_bits, eps = x_q
        w = w_idx.double()
        a_hi = (x_hi.reshape(-1, K).double() @ w.T).long()
        a_lo = (x_lo.reshape(-1, K).double() @ w.T).long()
        z = int(np.clip(np.rint(float(zf)), 0, 2 ** n_bits - 1))
        assert torch.equal(w_rowsum.long(), w_idx.long().sum(1))
        tot = 256 * a_hi + a_lo + (32896 - z) * w_rowsum.long()[None, :]
        sw = torch.clamp_min(w_delta.float(), w_eps).expand(N) if w_delta.numel() == 1 else torch.clamp_min(w_delta.float(), w_eps)
        sx = torch.clamp_min(delta.float().reshape(()), eps)
        pre = torch.from_numpy(tot.numpy().astype(np.float32)) * (sx * sw)[None, :]
        if bias is not None:
            pre = pre + bias.float()[None, :]
        if activation == 2:
            pre = torch.nn.functional.gelu(pre)
        elif activation == 1:
            pre = torch.relu(pre)
        idx = None
        if q_out is not None:
            d, zo, sg, nb, sym, log, qeps = q_out
            idx, pre = O.fake_quant(pre, d.reshape(()), None if zo is None else zo.reshape(()), nb, sym, False, qeps, 'linear')
        shape = x_hi.shape[:-1] + (N,)
        y = pre.reshape(shape).to(out_dtype) if want_y else None
        yi = (idx.reshape(shape) - 128).to(torch.int8) if want_idx else None
        self.x16_calls.append({'shape': tuple(x_hi.shape), 'bits': n_bits, 'want_y': want_y, 'idx': yi})
        return (y, yi) if want_idx else y

    def linear_i8(self, x_idx, *a, **k):
        self.i8_calls.append(x_idx)
        return super().linear_i8(x_idx, *a, **k)


def _model(num_layers):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=num_layers, **qp)
    apply_quant_dict(model, {'x': 16, 'h': 16, 'y': 16})
    return model.eval()


@pytest.mark.default_route          # the route belongs to the fused feed-forward block, which the layered pass switches off
def test_mp16_ffn1_takes_the_16_bit_integer_linear_cpu():
    from quantization import _hip, options
    from utils.utils import pass_data_for_range_estimation
    be = _Mp16Oracle()
    prev = _hip.set_backend(be)
    saved = options.INT8_LINEAR
    try:
        model = _model(2)
        assert model.layers[0].attention_output.LayerNorm.activation_quantizer.quantizer.n_bits == 16
        g = torch.Generator().manual_seed(0)
        calib = torch.randint(1000, 30000, (2, 64), generator=g)
        ids = torch.randint(1000, 30000, (2, 64), generator=g)
        with torch.no_grad():
            pass_data_for_range_estimation([(calib,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
            assert be.hilo_calls == [] and be.x16_calls == []       # calibrating forwards stay layered
            model.fix_ranges()
            options.INT8_LINEAR = False
            layered = model(ids)
            assert be.hilo_calls == [] and be.x16_calls == []
            options.INT8_LINEAR = 'auto'                    # the product default
            del be.i8_calls[:]
            fast = model(ids)
            # FFN1 of both layers: one pair of byte planes, one index-only 16-bit Linear; FFN2 consumes those very indices
            assert be.hilo_calls == [(2, 64, 768)] * 2
            assert len(be.x16_calls) == 2
            for c in be.x16_calls:
                assert c['shape'] == (2, 64, 768) and c['bits'] == 16 and c['want_y'] is False and c['idx'] is not None
                assert any(x is c['idx'] for x in be.i8_calls), 'FFN2 did not consume the indices of the 16-bit Linear'
            fast, layered = (t[0] if isinstance(t, (tuple, list)) else t for t in (fast, layered))
            d = (fast.float() - layered.float()).abs()
            print('max |fast - layered| = %.3e, max |layered| = %.3e' % (float(d.max()), float(layered.abs().max())))
            assert float(d.max()) <= 0.05 * float(layered.abs().max())
            # an observed feed-forward Linear: the layered modules run
            n = len(be.x16_calls)
            h = model.layers[0].intermediate.register_forward_hook(lambda m, i, o: None)
            model(ids)
            h.remove()
            assert len(be.x16_calls) == n + 1               # layer 1 only
            h = model.layers[0].intermediate[0].register_forward_hook(lambda m, i, o: None)
            model(ids)
            h.remove()
            assert len(be.x16_calls) == n + 2
        # autograd (parameters require grad, grad mode on): the 16-bit plan declines
        n = len(be.x16_calls)
        options.INT8_LINEAR = True
        model(ids)
        assert len(be.x16_calls) == n and len(be.hilo_calls) == n
    finally:
        options.INT8_LINEAR = saved
        _hip.set_backend(prev)
