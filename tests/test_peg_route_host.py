"""Host logic of the integer route for per-embedding-group (PEG) inputs, replayed on the CPU: BERT with the README's PEG
recipe ({'x', 'h', 'y'}: 'ng6') sends the first feed-forward Linear of every layer -- its input is site x, a PEG grid --
to the class-ordered integer Linear (`linear_i8_cls`), with operands in class order and per-class row sums; calibrating
forwards and autograd keep the layered route.  The oracle double of the kernel below restates the formula of
include/tq_hip.h (tests/test_linear_i8_peg.py holds the kernel to it bit for bit on the GPU)."""
import numpy as np
import torch

from tests._oracle_backend import OracleBackend


class _ClsOracle(OracleBackend):
    """OracleBackend + the class-ordered integer Linear"""
    STAIR_BINS, STAIR_BINS_BIG = 768, 1536

    def __init__(self):
        self.cls_calls = []

    def cls_table(self, ends, reps):
        return (tuple(int(e) for e in ends), tuple(int(r) for r in reps))

    def cls_stair_bins_for(self, M, N, K, n_classes):
        return None

    def linear_i8_cls(self, x_idx, w_idx, cls_rowsum, bias, x_q, cls, w_delta, w_eps, activation, q_out, out_dtype,
                      want_idx=False, want_y=True, stair=None):
        from oracle import tq_oracle as O
        ends, reps = cls
        K = x_idx.shape[-1]
        N = w_idx.shape[0]
        x = x_idx.reshape(-1, K).double()
        w = w_idx.double()
        sw = torch.clamp_min(w_delta.float(), w_eps).expand(N) if w_delta.numel() == 1 else torch.clamp_min(w_delta.float(), w_eps)
        delta, zf, n_bits, eps = x_q
        acc = None
        s = 0
        for c, (e, r) in enumerate(zip(ends, reps)):
            A = (x[:, s:e] @ w[:, s:e].T).long()
            assert torch.equal(cls_rowsum[c].long(), w_idx[:, s:e].long().sum(1))
            z = int(np.clip(np.rint(float(zf.reshape(-1)[r])), 0, 2 ** n_bits - 1))
            T = A + (128 - z) * cls_rowsum[c].long()[None, :]
            sx = torch.clamp_min(delta.reshape(-1)[r].float(), eps)
            pc = T.float() * (sx * sw)[None, :]
            acc = pc if acc is None else acc + pc
            s = e
        pre = acc + (bias.float()[None, :] if bias is not None else 0.0)
        if activation == 2:
            pre = torch.nn.functional.gelu(pre)
        elif activation == 1:
            pre = torch.relu(pre)
        idx = None
        if q_out is not None:
            d, z, sg, nb, sym, log, qeps = q_out
            idx, pre = O.fake_quant(pre, d.reshape(()), None if z is None else z.reshape(()), nb, sym, False, qeps, 'linear')
        self.cls_calls.append((x_idx.shape, tuple(ends)))
        shape = x_idx.shape[:-1] + (N,)
        y = pre.reshape(shape).to(out_dtype) if want_y else None
        if want_idx:
            return y, (idx.reshape(shape) - 128).to(torch.int8)
        return y


def _model(num_layers):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=num_layers, **qp)
    apply_quant_dict(model, {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'})
    return model.eval()


def test_peg_ffn1_takes_the_class_ordered_integer_linear_cpu():
    from quantization import _hip, options
    from utils.utils import pass_data_for_range_estimation
    be = _ClsOracle()
    prev = _hip.set_backend(be)
    saved = options.INT8_LINEAR
    try:
        model = _model(2)
        g = torch.Generator().manual_seed(0)
        calib = torch.randint(1000, 30000, (2, 64), generator=g)
        ids = torch.randint(1000, 30000, (2, 64), generator=g)
        with torch.no_grad():
            pass_data_for_range_estimation([(calib,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
            assert be.cls_calls == []                       # calibrating forwards stay per-tensor only
            model.fix_ranges()
            options.INT8_LINEAR = False
            layered = model(ids)
            assert be.cls_calls == []
            options.INT8_LINEAR = 'auto'                    # the product default
            fast = model(ids)
        assert len(be.cls_calls) == 2                       # FFN1 of both layers
        assert all(shape == (2, 64, 768) and ends == (128, 256, 384, 512, 640, 768) for shape, ends in be.cls_calls)
        fast, layered = (t[0] if isinstance(t, (tuple, list)) else t for t in (fast, layered))
        d = (fast.float() - layered.float()).abs()
        assert float(d.max()) <= 0.05 * float(layered.abs().max()) + 1e-6
        # autograd (parameters require grad, grad mode on): the PEG plan declines
        n = len(be.cls_calls)
        options.INT8_LINEAR = True
        model(ids)
        assert len(be.cls_calls) == n
    finally:
        options.INT8_LINEAR = saved
        _hip.set_backend(prev)
