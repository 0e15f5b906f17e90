"""tq_residual_layernorm_quant_bwd against a float64 reference of the formulas in include/tq_hip.h, built from oracle.tq_oracle.

Reference: t = Q1(g) + r, u = Q2(t) and the masks in1 / in2 in fp32 exactly as the forward computes them (O.fake_quant,
O.ste_param_grad_terms); from the statistics on everything is float64.  Q3's clamped index xi3 - zp3 = rint(y / s3) is read
from the forward launch's own y (a z on a rounding tie may land one step away: test_fused_ln.py).
Statistics contract (tests/test_fused_ln.py: the LayerNorm output to rtol 2e-5 + atol 1e-5): |dz| <= 2e-5 |z| + 1e-5, taken
as E = 2e-5 relative on rstd and E (|xh| + 1) on xh.  in3 needs, asserted on the reference alone, that no z / s3 lies within
MARGIN = 2 max(2e-5 |z| + 1e-5) / s3 grid steps of Q3's clamp thresholds hi3 - zp3 + 0.5 and lo3 - zp3 - 0.5 (seeds picked on
the CPU); no element is excluded from any comparison.
Tolerance, u = 2^-24, L = d / LPR lane-local adds + log2(LPR) butterfly steps (the row sums m1, m2).  gu is rstd times a sum
of three terms, each carrying E once from rstd, at most twice more from xh (in m2 and in xh * m2) and 12 roundings:
    |gt_j - ref|, |gg_j - ref| <= B_j = (3 E + (L + 12) u) rstd (|gxh_j| + A1 / d + (1 + |xh_j|) A2 / d),
    A1 = sum_j |gxh_j|,  A2 = sum_j |gxh_j| (1 + |xh_j|)
Column sums: a lane adds its rows (trips of the grid-stride loop), the block its 256 / LPR lane groups, the final launch in
float64: Lc = trips + 256 / LPR + 2;  bias (Lc u) sum |gz|,  weight (E + (Lc + 2) u) sum |gz| (1 + |xh|)  per column.
Range gradients: Lb = trips * d / LPR + 6 wave steps + 4 LDS adds (block partials are added in float64):
    (Lb + 16) u A |chain| + (the terms' sums with the incoming gradient replaced by its bound: B for Q1 and Q2; for Q3 the
    part of t2 that contains z, |gy| (2e-5 |z| + 1e-5) / s3),  A = A_d | A_z of ste_param_grad_terms.
Grid: at most 512 blocks of 256 / LPR rows, so 8200 / 4100 / 2052 rows take a second trip at LPR = 16 / 32 / 64."""
import math

import pytest
import torch

from oracle import tq_oracle as O

pytestmark = pytest.mark.gpu
U, E, EPS, LN_EPS = 2.0 ** -24, 2e-5, 1e-8, 1e-12
LPR = {64: 16, 128: 32, 256: 64, 384: 32, 512: 64, 768: 64, 1024: 64}
RANGES = ((-2.5, 2.2), (-3.0, 3.4), (-2.0, 2.3))          # Q_dense, Q_sum, Q_out: every clamp cuts randn data
ALL = ('asym', 'asym', 'asym')


def _spec(kind, lo, hi):
    """-> None or the backend's QSpec with one-element CPU buffers; 'div': a 23-bit grid, which the vote sends to the division body"""
    from quantization.int8_route import QSpec
    if kind is None:
        return None
    bits = 23 if kind == 'div' else 8
    if kind == 'sym':
        d, sg = O.sym_params_from_range(lo, hi, bits)
        return QSpec(d.reshape(1), None, sg.reshape(1).to(torch.uint8), bits, True, False, EPS)
    d, z = O.asym_params_from_range(lo, hi, bits)
    return QSpec((torch.log(d.double()).float() if kind == 'log' else d).reshape(1), z.reshape(1), None, bits, False, kind == 'log', EPS)


def _inputs(rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    a, r, gy = (torch.randn(rows, d, generator=g) for _ in range(3))
    return a, r, gy, 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)


def _reference(a, r, gy, w, b, qs, y_gpu, trips):
    """float64 gradients and their bounds (see the module docstring) -> {name: (value, bound)}"""
    q1, q2, q3 = qs
    cpu = lambda t: None if t is None else t.detach().cpu().reshape(())
    kw = lambda q: dict(delta=cpu(q.delta), zero_float=cpu(q.zero_float), n_bits=q.n_bits, symmetric=q.symmetric, eps=q.eps,
                        signed=q.symmetric and bool(q.signed), scale_domain='log' if q.log_domain else 'linear')
    fq = lambda x, q: x if q is None else O.fake_quant(x, **kw(q))[1]
    terms = lambda x, g, q: O.ste_param_grad_terms(x, g, **kw(q))
    d = a.shape[-1]
    L, Lb, Lc = d // LPR[d] + int(math.log2(LPR[d])), trips * d // LPR[d] + 10, trips + 256 // LPR[d] + 2
    t = fq(a, q1) + r
    u = fq(t, q2).double()
    mean = u.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((u - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    xh = (u - mean) * rstd
    z = xh * w.double() + b.double()
    gz, out = gy.double(), {}

    def range_grads(name, tr, t1, extra_d, extra_z):
        dsum, A = (t1 - tr['t2']).sum(), (t1.abs() + tr['t2'].abs()).sum()
        chain = float(tr['chain_delta'].abs())
        out[name] = (torch.stack([dsum * float(tr['chain_delta']), tr['d_zero_float'].sum()]),
                     torch.stack([((Lb + 16) * U * A + extra_d) * chain, (Lb + 16) * U * tr['A_z'].sum() + extra_z]))

    if q3 is not None:
        k3 = kw(q3)
        s3 = float(O.effective_scale(k3['delta'].double(), EPS, k3['scale_domain']).float())
        lo, hi = O.grid_limits(k3['n_bits'], k3['symmetric'], k3['signed'])
        zp3 = 0.0 if k3['symmetric'] else float(O.effective_zero_point(k3['zero_float'], k3['n_bits']))
        dz = E * z.abs() + 1e-5
        for edge in (hi - zp3 + 0.5, lo - zp3 - 0.5):
            assert float((z / s3 - edge).abs().min()) > 2 * float(dz.max()) / s3, 'seed puts a z on a clamp threshold of Q_out'
        tr = terms(z.float(), gy, q3)
        range_grads('q_out', tr, gz * torch.round(y_gpu.double() / s3), (tr['mask'] * gz.abs() * dz / s3).sum(), 0.0)
        gz = torch.where(tr['mask'], gz, torch.zeros_like(gz))
    out['ln_bias'] = (gz.sum(0), Lc * U * gz.abs().sum(0))
    out['ln_weight'] = ((gz * xh).sum(0), (E + (Lc + 2) * U) * (gz.abs() * (1 + xh.abs())).sum(0))
    gxh = gz * w.double()
    gu = rstd * (gxh - gxh.mean(-1, keepdim=True) - xh * (gxh * xh).mean(-1, keepdim=True))
    A1, A2 = gxh.abs().sum(-1, keepdim=True), (gxh.abs() * (1 + xh.abs())).sum(-1, keepdim=True)
    B = (3 * E + (L + 12) * U) * rstd * (gxh.abs() + A1 / d + (1 + xh.abs()) * A2 / d)
    for name, outname, v, q in (('q_sum', 'residual', t, q2), ('q_dense', 'dense', a, q1)):
        if q is not None:
            tr, trb = terms(v, gu, q), terms(v, B, q)
            range_grads(name, tr, tr['t1'], trb['A_d'].sum(), trb['A_z'].sum())
            gu = torch.where(tr['mask'], gu, torch.zeros_like(gu))
        out[outname] = (gu, B)
    return out


def _launch(data, kinds, ranges=RANGES, want=None, trips=1, compare=True):
    """both launches on data = (a, r, gy, w, b) -> (the backward's outputs, the forward's y), on the CPU; `compare`: see below"""
    from quantization import _hip
    qs = [_spec(k, *rng) for k, rng in zip(kinds, ranges)]
    cuda = lambda t: t.cuda() if torch.is_tensor(t) else t
    (a, r, gy, w, b), (k1, k2, k3) = map(cuda, data), (q and type(q)(*map(cuda, q)) for q in qs)
    want = want or ['dense', 'residual', 'ln_weight', 'ln_bias', 'y'] + [n for n, q in zip(('q_dense', 'q_sum', 'q_out'), qs) if q]
    got = _hip.backend().residual_layernorm_quant_bwd(a, r, gy, k1, k2, w, b, LN_EPS, k3, want=want)
    got, y_fwd = {k: v.cpu() for k, v in got.items()}, _hip.backend().residual_layernorm_quant(a, r, k1, k2, w, b, LN_EPS, k3).cpu()
    if compare:
        assert torch.equal(got['y'].view(torch.int32), y_fwd.view(torch.int32))
        ref = _reference(*data, qs, y_fwd, trips)
        for name in set(got) - {'y'}:
            assert bool(((got[name].double() - ref[name][0]).abs() <= ref[name][1]).all()), name
    return got, y_fwd


@pytest.mark.parametrize('rows,d', [(rows, d) for d in sorted(LPR) for rows in (1, 21)] + [(8200, 64), (4100, 128), (2052, 256)])
def test_every_row_length_and_a_second_grid_stride_trip(rows, d):
    """21 rows: no multiple of the 4 / 8 / 16 rows of a block, so lane groups past the end run clamped; rows = 1: one group; the
    large ones: a second trip per lane-group form (half a million elements always hold a z within MARGIN of a threshold:
    Q_out's range is wide there and never clamps).  Two runs give identical bits."""
    seed, ranges = (11, (RANGES[0], RANGES[1], (-8.0, 8.0))) if rows > 21 else (1700 + d + rows, RANGES)
    got, _ = _launch(_inputs(rows, d, seed), ALL, ranges, trips=2 if rows > 21 else 1)
    again, _ = _launch(_inputs(rows, d, seed), ALL, ranges, compare=False)
    assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got)


@pytest.mark.parametrize('kinds', [(k1, k2, k3) for k1 in (None, 'asym') for k2 in (None, 'asym') for k3 in (None, 'asym')]
                         + [('asym', 'sym', 'log'), ('div', 'asym', 'asym')])
@pytest.mark.parametrize('range_grads', [True, False])
def test_quantizer_mixes(kinds, range_grads):
    """the eight present / absent mixes, a symmetric and a log-domain quantizer,
    and a 23-bit Q_dense that sends the launch through the division body -- y equals the forward launch in both bodies"""
    _launch(_inputs(21, 384, 61), kinds, want=None if range_grads else ['dense', 'residual', 'ln_weight', 'ln_bias', 'y'])


@pytest.mark.parametrize('row,col', [(0, 0), (7, 3), (8, 4), (20, 127)])
def test_one_hot_probes(row, col):
    """d = 128: 8 rows per block, a lane owns 4 columns.  grad_y is 1.25 at the first / last row of a block and of the tensor,
    the first / last column of a lane and of the row: the bias gradient is that element's alone, in exactly that column"""
    a, r, gy, w, b = _inputs(21, 128, 5)
    gy.zero_()[row, col] = 1.25
    got, _ = _launch((a, r, gy, w, b), ('asym', 'asym', None))
    assert got['ln_bias'].nonzero().tolist() == [[col]] and got['ln_weight'].nonzero().tolist() == [[col]]
    others = torch.arange(21) != row
    assert bool((got['dense'][others] == 0).all()) and bool((got['residual'][others] == 0).all())


@pytest.mark.parametrize('kinds', [ALL, ('div', 'asym', 'asym')])
def test_nan_row(kinds):
    """a NaN input: its row is NaN inside the clamp ranges (0 outside), every column sum and every d loss / d _delta is NaN,
    every other row is what it is without the NaN"""
    data = _inputs(21, 256, 9)
    clean, _ = _launch(data, kinds)
    data[0][13, 77] = float('nan')
    got, y_fwd = _launch(data, kinds, compare=False)
    others = torch.arange(21) != 13
    for k in ('dense', 'residual'):
        assert torch.equal(got[k][others], clean[k][others]) and bool((got[k][13].isnan() | (got[k][13] == 0)).all())
        assert int(got[k][13].isnan().sum()) > 128
    assert bool(got['y'][13].isnan().all()) and torch.equal(got['y'].isnan(), y_fwd.isnan())
    assert all(bool(got[k].isnan().all()) for k in ('ln_weight', 'ln_bias'))
    assert all(bool(got[k][0].isnan()) for k in ('q_dense', 'q_sum', 'q_out'))
