"""tq_scores_softmax_quant_bwd against a float64 reference of the formulas in include/tq_hip.h, built from oracle.tq_oracle.

Reference: u = Q_scores(x) in fp32 as the forward computes it, then float64: p = softmax(u / denom + m), in2 from
rint(p / s2) + zp2, gp, dot, gt, gu, gx.  O.ste_param_grad_terms(x, gu) gives Q_scores' mask and terms (index and mask in fp32).
Q_probs' xi2 - zp2 = rint(y / s2) is read from the GPU forward's own y (a probability on a rounding tie may land one step
away: test_fused_softmax.py); in2 comes from the float64 chain under the condition, asserted on the reference alone, that no
p / s2 lies within 1e-3 of the clamp thresholds hi2 - zp2 + 0.5 and lo2 - zp2 - 0.5 (seeds picked on the CPU).
Tolerance: the gradient is multilinear in p, which the forward's contract gives to rtol 1e-5; u = 2^-24, L = the row-sum chain
(NV * 4 lane-local adds + log2(LPR) butterfly steps), 8 roundings in the products and quotients:
    |gx_j - ref_j| <= (2e-5 + (L + 8) u) |p_j| (|gp_j| + A_row) / |denom|,   A_row = sum_j |gp_j p_j|
Range gradients: (L_block + 16) u A |chain| + 2e-5 A_p |chain|; A = the terms' magnitudes (A_d, A_z of ste_param_grad_terms),
A_p the part whose terms contain p (all of Q_scores': gu does; t2 of Q_probs), L_block = rows per thread * NV * 4 + 6 wave
steps + 4 LDS adds (the block partials are added in float64); the one-hot probes use L_block = 0.
Grid: at most 2048 blocks; T = 32 runs 32 rows x R = 2 per block, so 131 100 rows (16.8 MB a tensor) take a second trip."""
import ctypes as C
import math

import pytest
import torch

from oracle import tq_oracle as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DENOM = 8.0
EPS = 1e-8


def _be():
    from quantization import _hip
    return _hip.backend()


def _quantizer(kind):
    """-> None or dict(delta, zf, signed, symmetric, domain) on the CPU; 'probs': [0, 0.5], else Q_scores on [-70, 80]"""
    if kind is None:
        return None
    lo, hi = (0.0, 0.5) if kind == 'probs' else (-70.0, 80.0)
    if kind == 'sym':
        d, sg = O.sym_params_from_range(lo, hi, 8)
        return dict(delta=d, zf=None, signed=bool(sg), symmetric=True, domain='linear')
    d, z = O.asym_params_from_range(lo, hi, 8)
    log = kind == 'log'
    return dict(delta=torch.log(d.double()).float() if log else d, zf=z, signed=False, symmetric=False, domain='log' if log else 'linear')


def _quantizers(kind1, on2):
    return _quantizer(kind1), _quantizer('probs' if on2 else None)


def _dev(q):
    if q is None:
        return None
    sg = torch.tensor([1 if q['signed'] else 0], dtype=torch.uint8).cuda() if q['symmetric'] else None
    return (q['delta'].reshape(1).cuda(), None if q['zf'] is None else q['zf'].reshape(1).cuda(), sg, 8, q['symmetric'],
            q['domain'] == 'log', EPS)


def _inputs(T, rows_shape, seed, with_mask):
    B, H, Tq = rows_shape
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, H, Tq, T, generator=g) * 24
    gy = torch.randn(B, H, Tq, T, generator=g)
    mask = None
    if with_mask:
        keep = (torch.rand(B, T, generator=g) > 0.2).float()
        keep[:, 0] = keep[:, T - 1] = 1                 # (the one-hot probes at the first and the last element meet p != 0)
        mask = (1 - keep) * -10000.0
        mask[0, T // 2:] = -float('inf')
    return s, gy, mask


def _reference(s, gy, mask, q1, q2, y_gpu):
    """float64 gradients, their bounds' magnitudes and the range-gradient terms (see the module docstring)"""
    B, H, Tq, T = s.shape
    u = s if q1 is None else O.fake_quant(s, q1['delta'], q1['zf'], 8, q1['symmetric'], q1['signed'], EPS, q1['domain'])[1]
    t = u.double() / DENOM
    if mask is not None:
        t = t + mask.double().reshape(B, 1, 1, T)
    p = torch.softmax(t, dim=-1)
    g64 = gy.double()
    out = {}
    if q2 is not None:
        s2 = float(torch.clamp(q2['delta'], min=EPS))         # (Q_probs is in the linear domain in every case)
        lo, hi = O.grid_limits(8, False)
        zp2 = float(torch.clamp(torch.round(q2['zf']), lo, hi))
        quo = p / s2
        for edge in (hi - zp2 + 0.5, lo - zp2 - 0.5):
            assert float((quo - edge).abs().min()) > 1e-3, 'seed puts a probability on a clamp threshold'
        r2 = torch.round(quo) + zp2
        in2 = (r2 >= lo) & (r2 <= hi)
        gp = torch.where(in2, g64, torch.zeros_like(g64))
        hm2 = torch.round(y_gpu.double() / s2)
        t1, t2 = g64 * hm2, torch.where(in2, g64 * p / s2, torch.zeros_like(p))
        tz = torch.where(in2, torch.zeros_like(p), -g64 * s2)
        zr = float(torch.round(q2['zf']))
        out['q2'] = dict(d=float((t1 - t2).sum()), z=float(tz.sum()) * float(lo <= zr <= hi), A=float((t1.abs() + t2.abs()).sum()),
                         Ap=float(t2.abs().sum()), Az=float(tz.abs().sum()), in2=in2)
    else:
        gp = g64
    a_row = (gp * p).abs().sum(-1, keepdim=True)
    gu = p * (gp - (gp * p).sum(-1, keepdim=True)) / DENOM
    out['mag'] = p.abs() * (gp.abs() + a_row) / DENOM
    if q1 is not None:
        tr = O.ste_param_grad_terms(s, gu, q1['delta'], q1['zf'], 8, q1['symmetric'], q1['signed'], EPS,
                                    scale_domain=q1['domain'])
        out['gx'] = torch.where(tr['mask'], gu, torch.zeros_like(gu))
        out['q1'] = dict(d=float(tr['d_delta']), z=float(tr['d_zero_float']), A=float(tr['A_d'] * tr['chain_delta'].abs()),
                         Az=float(tr['A_z']), in1=tr['mask'])
        out['q1']['Ap'] = out['q1']['A']
    else:
        out['gx'] = gu
    return out                                          # (Q_probs' chain factor is 1: delta >= eps)


def _param_bounds(r, name, L_block):
    """(bound of d loss / d _delta, of d loss / d _zero_float) from the reference terms r of quantizer q1 | q2"""
    return (L_block + 16) * U * r['A'] + 2e-5 * r['Ap'], (L_block + 16) * U * r['Az'] + (2e-5 * r['Az'] if name == 'q1' else 0.0)


def _run(s, gy, mask, q1, q2, param_grads=True):
    be = _be()
    B, H, Tq, T = s.shape
    m = None if mask is None else mask.cuda()
    k1, k2 = _dev(q1), _dev(q2)
    want = (param_grads and q1 is not None, param_grads and q2 is not None)
    y_fwd = be.scores_softmax_quant(s.cuda(), m, H * Tq, DENOM, k1, k2)
    gx, g1, g2, y = be.scores_softmax_quant_bwd(s.cuda(), gy.cuda(), m, H * Tq, DENOM, k1, k2, param_grads=want, want_probs=True)
    return gx.cpu(), (None if g1 is None else g1.cpu()), (None if g2 is None else g2.cpu()), y.cpu(), y_fwd.cpu()


def _check(s, gy, mask, q1, q2, rows_per_thread, L_block=None):
    T = s.shape[-1]
    lpr = min(T // 4, 64)
    L = T // lpr + int(math.log2(lpr))
    if L_block is None:
        L_block = rows_per_thread * (T // lpr) + 10
    gx, g1, g2, y, y_fwd = _run(s, gy, mask, q1, q2)
    assert torch.equal(y, y_fwd)
    ref = _reference(s, gy, mask, q1, q2, y)
    err, bound = (gx.double() - ref['gx']).abs(), (2e-5 + (L + 8) * U) * ref['mag']
    assert bool((err <= bound).all())
    for name, g in (('q1', g1), ('q2', g2)):
        if g is not None:
            bd, bz = _param_bounds(ref[name], name, L_block)
            assert abs(float(g[0]) - ref[name]['d']) <= bd and abs(float(g[1]) - ref[name]['z']) <= bz
    return gx, ref


@pytest.mark.parametrize('T', [32, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize('kind1,on2,with_mask', [('asym', True, True), (None, True, True), ('asym', False, True),
                                                 (None, False, False), ('asym', True, False)])
def test_backward_vs_float64(T, kind1, on2, with_mask):
    """42 rows: no multiple of any rows-per-block, so the clamped tail rows run; both clamps of Q_scores and the upper one of
    Q_probs cut; -10000 pads and the first sequence with -inf on its upper half (p == 0: a gradient of exactly 0)."""
    s, gy, mask = _inputs(T, (3, 2, 7), 100 + T, with_mask)
    q1, q2 = _quantizers(kind1, on2)
    gx, ref = _check(s, gy, mask, q1, q2, rows_per_thread=1)
    if with_mask:
        assert bool((gx[0, :, :, T // 2:] == 0).all())
    if q1 is not None:
        assert not bool(ref['q1']['in1'].all())
    if q2 is not None and (with_mask or T < 1024):      # (1024 unmasked 3 * randn logits hold no probability above 0.5)
        assert not bool(ref['q2']['in2'].all())


@pytest.mark.parametrize('T,Tq,seed,kind1,rows_per_thread', [(128, 7, 7, 'log', 1), (128, 7, 7, 'sym', 1), (32, 21850, 12, 'asym', 4)])
def test_log_domain_symmetric_and_second_grid_stride_trip(T, Tq, seed, kind1, rows_per_thread):
    s, gy, mask = _inputs(T, (3, 2, Tq), seed, True)            # Tq = 21850: 131 100 rows > 2048 blocks x 64 rows
    _check(s, gy, mask, *_quantizers(kind1, True), rows_per_thread=rows_per_thread)


@pytest.mark.parametrize('where', ['first', 'last', 'block_end', 'clamped1', 'clamped2'])
def test_one_hot_probes(where):
    """grad_probs is 1.25 at one element: every other row of grad_scores is exactly 0 and the range gradients are that row's
    alone (L_block = 0) -- a tail row that is recomputed and counted twice fails here."""
    T = 128
    s, gy, mask = _inputs(T, (3, 2, 7), 228, True)
    q1, q2 = _quantizers('asym', True)
    ref0 = _reference(s, gy, mask, q1, q2, _run(s, gy, mask, q1, q2, param_grads=False)[3])
    flat = {'first': 0, 'last': 42 * T - 1, 'block_end': 7 * T + 5,          # T = 128: 8 rows per block
            'clamped1': int((~ref0['q1']['in1']).reshape(-1).nonzero()[0]),
            'clamped2': int((~ref0['q2']['in2']).reshape(-1).nonzero()[0])}[where]
    gy = torch.zeros_like(gy)
    gy.view(-1)[flat] = 1.25
    gx, _ = _check(s, gy, mask, q1, q2, rows_per_thread=1, L_block=0)
    others = torch.ones(42, dtype=torch.bool)
    others[flat // T] = False
    assert bool((gx.reshape(42, T)[others] == 0).all())
    if where != 'clamped2':                         # (a clamped probability passes no gradient: the whole row is 0)
        assert bool((gx.reshape(42, T)[flat // T] != 0).any())


@pytest.mark.parametrize('fast', ['0', '1'])
def test_recomputed_probs_are_the_forward_and_null_gradients_change_nothing(fast, monkeypatch):
    monkeypatch.setenv('TQ_SM_FAST', fast)
    s, gy, mask = _inputs(128, (3, 2, 7), 5, True)
    q1, q2 = _quantizers('asym', True)
    gx, _, _, y, y_fwd = _run(s, gy, mask, q1, q2)
    gx0, g1, g2, y0, _ = _run(s, gy, mask, q1, q2, param_grads=False)
    assert g1 is None and g2 is None
    assert torch.equal(y, y_fwd) and torch.equal(y0, y_fwd) and torch.equal(gx.view(torch.int32), gx0.view(torch.int32))


def test_nan_row():
    """a NaN score: its row of grad_scores is NaN inside Q_scores' clamp range (0 outside), both d loss / d _delta are NaN"""
    s, gy, mask = _inputs(128, (3, 2, 7), 5, True)
    s[1, 0, 3, 9] = float('nan')
    gx, g1, g2, y, _ = _run(s, gy, mask, *_quantizers('asym', True))
    inside = (s[1, 0, 3] > -60) & (s[1, 0, 3] < 70)
    assert bool(torch.isnan(gx[1, 0, 3][inside]).all()) and bool(torch.isnan(y[1, 0, 3]).all())
    assert int(torch.isnan(gx).any(-1).sum()) == 1 and bool(torch.isnan(g1[0])) and bool(torch.isnan(g2[0]))


@pytest.mark.parametrize('bad', ['cols', 'misaligned', 'workspace'])
def test_bad_arguments_raise_before_any_write(bad):
    be, cols = _be(), 48 if bad == 'cols' else 64
    buf = torch.randn(8 * cols + 4, device='cuda')
    gy = buf.clone()[1:8 * cols + 1] if bad == 'misaligned' else buf.clone()[:8 * cols]
    gx, g1, ws = torch.full((8 * cols,), 7.5, device='cuda'), torch.zeros(2, device='cuda'), torch.zeros(4, device='cuda')
    k1 = _dev(_quantizers('asym', False)[0])
    rc = be.lib.tq_scores_softmax_quant_bwd(buf.data_ptr(), gy.data_ptr(), gx.data_ptr(), 8, cols, None, 8, DENOM,
                                            C.byref(be._qdesc(*k1, 1, 1)), None, g1.data_ptr() if bad == 'workspace' else None,
                                            None, None, ws.data_ptr(), 4 if bad == 'workspace' else 0, None)
    from quantization import _hip
    with pytest.raises(_hip.TQError):
        _hip._check(rc, be.lib)
    torch.cuda.synchronize()
    assert bool((gx == 7.5).all())
