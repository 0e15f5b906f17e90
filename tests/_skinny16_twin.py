"""TEST INFRASTRUCTURE: the reference of tq_linear_i16x8_skinny_fwd and the exact CPU twin that answers
`linear_i16x8_skinny` with it (options.INT8_HEAD under the mixed-precision recipes and on packed batches).

    tot   = int64 contraction of the grid indices themselves: sum_k index w - z_x rowsum, the index rebuilt from the planes
            (256 (hi + 128) + (lo + 128); 8-bit form: lo + 128) -- equal to the header's plane formula term by term
    pre   = np.float32(tot) * (max(x_delta, eps) * max(w_delta[n], eps)) + b[n]          (np.float32(int64): one rounding)
    act, q_out = tests/_skinny_twin.skinny_epilogue (the C oracle's epilogue; Tanh = np.tanh in float64 narrowed once)
    index of a wide q_out: oracle.tq_oracle.fake_quant at n_bits on the activation's value (the oracle's int8 index output
            does not hold it)

tests/test_linear_i16x8_skinny.py holds the kernel to `skinny16_reference`; `Skinny16Twin` binds the same function to the
backend method.  Nothing outside tests/ imports this."""
import numpy as np
import torch

from oracle import tq_oracle as O
from tests._skinny_twin import SkinnyTwin, skinny_epilogue


def planes_of(idx):
    """int64 / int32 indices in [0, 65535] -> (hi, lo) int8 numpy planes"""
    idx = np.asarray(idx).astype(np.int64)
    return ((idx >> 8) - 128).astype(np.int8), ((idx & 255) - 128).astype(np.int8)


def index_of(hi, lo):
    """planes (numpy or torch int8; hi None: the 8-bit form) -> int64 numpy indices"""
    n = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    lo64 = n(lo).astype(np.int64) + 128
    return lo64 if hi is None else 256 * (n(hi).astype(np.int64) + 128) + lo64


def skinny16_tot(hi, lo, w, x_zf, n_bits):
    """int64 [M, N]: 256 A_hi + A_lo + (32896 - z) rowsum (8-bit form: A_lo + (128 - z) rowsum) == sum_k index w - z rowsum"""
    w64 = (w.detach().cpu().numpy() if torch.is_tensor(w) else np.asarray(w)).astype(np.int64)
    z = int(np.clip(np.rint(np.float32(x_zf)), 0, 2 ** n_bits - 1))
    return index_of(hi, lo) @ w64.T - z * w64.sum(1)[None, :]


def skinny16_pre(tot, x_delta, x_eps, w_delta, w_eps, bias):
    """fp32 [M, N] numpy; every fp32 operation rounded on its own"""
    f = lambda t: None if t is None else (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float32)
    sw = np.maximum(f(w_delta).reshape(-1), np.float32(w_eps)).astype(np.float32)
    sx = np.float32(max(np.float32(x_delta), np.float32(x_eps)))
    pre = tot.astype(np.float32) * (sx * np.broadcast_to(sw, (tot.shape[1],))).astype(np.float32)[None, :]
    if bias is not None:
        pre = (pre + f(bias)[None, :]).astype(np.float32)
    return pre.astype(np.float32)


def skinny16_reference(hi, lo, w, bias, x_q, w_delta, w_eps, activation, q7, rows=None):
    """x_q = (delta, zero_float, n_bits, eps) as floats; q7 the backend 7-tuple with python scalars or None; rows: None or
    row numbers into the planes (clamped like the kernel's).  -> (y fp32 [M, N], index int64 [M, N] or None)"""
    if rows is not None:
        r = np.clip(np.asarray(rows).astype(np.int64), 0, lo.shape[0] - 1)
        hi, lo = (None if hi is None else index_rows(hi, r)), index_rows(lo, r)
    tot = skinny16_tot(hi, lo, w, x_q[1], x_q[2])
    pre = torch.from_numpy(skinny16_pre(tot, x_q[0], x_q[3], w_delta, w_eps, bias))
    y, yi = skinny_epilogue(pre, activation, q7)
    if q7 is None:
        return y, None
    d, z, sg, n_bits, sym, logd, eps = q7
    if sym or n_bits > 8:
        act = skinny_epilogue(pre, activation, None)[0]
        idx = O.fake_quant(act, torch.tensor(d, dtype=torch.float32), None if z is None else torch.tensor(z, dtype=torch.float32),
                           n_bits, bool(sym), bool(sg), eps, 'linear')[0].long()
    else:
        idx = yi.long() + 128
    return y, idx.numpy()


def index_rows(t, r):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a[r])


def count_hip_launches(monkeypatch):
    """wrap HipBackend.linear_i16x8_skinny and HipBackend.linear_i8_skinny: -> the list their launches are appended to, in the
    form of the twins' census entries"""
    from quantization import _hip
    log = []
    new, old = _hip.HipBackend.linear_i16x8_skinny, _hip.HipBackend.linear_i8_skinny

    def counted_new(self, x, *a, **k):
        hi, lo = x if isinstance(x, (tuple, list)) else (None, x)
        rows = k.get('rows')
        form = 'planes' if k.get('want_planes') else 'idx' if k.get('want_idx') else 'y'
        log.append(('linear_i16x8_skinny', lo.shape[0] if rows is None else rows.numel(), a[0].shape[0], lo.shape[1], int(a[6]),
                    tuple(lo.stride()), hi is not None, rows is not None, a[7] is not None, form, k.get('want_y', True)))
        return new(self, x, *a, **k)

    def counted_old(self, *a, **k):
        log.append(('linear_i8_skinny', a[0].shape[0], a[1].shape[0], a[0].shape[1], int(a[7]), tuple(a[0].stride()),
                    a[8] is not None, k.get('want_y', True)))
        return old(self, *a, **k)
    monkeypatch.setattr(_hip.HipBackend, 'linear_i16x8_skinny', counted_new)
    monkeypatch.setattr(_hip.HipBackend, 'linear_i8_skinny', counted_old)
    return log


class Skinny16Twin(SkinnyTwin):
    """SkinnyTwin with `linear_i16x8_skinny`; every call leaves a census entry
    ('linear_i16x8_skinny', M, N, K, activation, strides of the lo plane, planes in?, row table?, output quantizer present?,
     output form 'y' / 'idx' / 'planes', want_y)"""
    name = 'exact-twin-skinny16'

    def linear_i16x8_skinny(self, x, w_idx, w_rowsum, bias, x_q, w_delta, w_eps, activation, q_out, out_dtype, want_idx=False,
                            want_planes=False, want_y=True, rows=None):
        hi, lo = x if isinstance(x, (tuple, list)) else (None, x)
        assert lo.dim() == 2 and lo.dtype == torch.int8 and lo.stride(1) == 1
        assert hi is None or (hi.shape == lo.shape and hi.dtype == torch.int8 and hi.stride() == lo.stride())
        assert rows is None or (rows.dtype == torch.int32 and rows.dim() == 1)
        assert not (want_idx and want_planes) and (want_y or want_idx or want_planes)
        n_bits = int(x_q[2])
        assert 1 <= n_bits <= (16 if hi is not None else 8)
        M, K = (rows.numel() if rows is not None else lo.shape[0]), lo.shape[1]
        form = 'planes' if want_planes else 'idx' if want_idx else 'y'
        self._count('linear_i16x8_skinny', M, w_idx.shape[0], K, int(activation), tuple(lo.stride()), hi is not None,
                    rows is not None, q_out is not None, form, want_y)
        q7 = self._q7(q_out)
        if want_planes:
            assert q7 is not None and not q7[4] and not q7[5] and q7[3] <= 16
        if want_idx:
            assert q7 is not None and not q7[4] and q7[3] <= 8
        y, idx = skinny16_reference(hi, lo, w_idx, bias, tuple(float(v) for v in x_q), w_delta, w_eps, int(activation), q7,
                                    None if rows is None else rows.detach().cpu().numpy())
        y = y.to(out_dtype) if want_y else None
        if want_planes:
            ph, pl = planes_of(idx)
            return y, (torch.from_numpy(ph), torch.from_numpy(pl))
        return (y, torch.from_numpy((idx - 128).astype(np.int8))) if want_idx else y
