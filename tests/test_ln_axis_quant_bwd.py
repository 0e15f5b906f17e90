"""tq_residual_layernorm_quant_axis_bwd (per-column quantizers) against a float64 reference built from oracle.tq_oracle with
axis=1 (the column of a [rows, d] input).  The derivation is tests/test_ln_quant_bwd.py's (K): the front and its masks in fp32 as the forward computes them,
float64 from the statistics on, Q_out's clamped index read from the forward launch's own y, the statistics contract E, the data
bound B_j and the column bounds of the affine gradients.  What changes: every range sum is a sum PER COLUMN, so it takes the
column-sum length Lc = trips + 256 / LPR + 2 where K has Lb,
    ((Lc + 16) u A_c + the terms with the incoming gradient replaced by its bound, summed over the column) |chain_c|,
and a per-tensor quantizer in the mix is the float64 sum of its column sums: values and bounds added over the columns (the
float64 additions: 2^-52 d of the magnitudes, added).  The margin assertion (no reference z / s3_c within the statistics margin
of a clamp threshold of Q_out, per column) is on the reference alone; seeds picked on the CPU; no element is excluded.
Parameters: six groups of columns with ranges (0.85 + 0.06 g) x K.RANGES, contiguous or (`perm`) scattered over the row."""
import math

import pytest
import torch

from oracle import tq_oracle as O
from tests.test_ln_quant_bwd import E, EPS, LN_EPS, LPR, RANGES, U, _inputs

pytestmark = pytest.mark.gpu
PEG = ('col', 'col', 'col')
DATA = ['dense', 'residual', 'ln_weight', 'ln_bias', 'y']


def _spec(kind, lo, hi, d, perm):
    """None | 'col' / 'sym' / 'div' (per-column: asymmetric, symmetric, 23-bit asymmetric -> the division body) | 'pt' (per-tensor)"""
    from quantization.int8_route import QSpec
    if kind is None:
        return None
    bits = 23 if kind == 'div' else 8
    if kind == 'pt':
        dl, z = O.asym_params_from_range(lo, hi, bits)
        return QSpec(dl.reshape(1), z.reshape(1), None, bits, False, False, EPS)
    group = torch.arange(d) * 6 // d
    f = 0.85 + 0.06 * (group[torch.randperm(d, generator=torch.Generator().manual_seed(3))] if perm else group).float()
    if kind == 'sym':
        dl, sg = O.sym_params_from_range(lo * f, hi * f, bits)
        return QSpec(dl, None, sg.reshape(1).to(torch.uint8), bits, True, False, EPS)
    dl, z = O.asym_params_from_range(lo * f, hi * f, bits)
    return QSpec(dl, z, None, bits, False, False, EPS)


def _reference(a, r, gy, w, b, qs, y_gpu, trips):
    """float64 gradients and their bounds -> {name: (value, bound)}; range gradients [2, n_params]"""
    q1, q2, q3 = qs
    kw = lambda q: dict(delta=q.delta, zero_float=q.zero_float, n_bits=q.n_bits, symmetric=q.symmetric, eps=q.eps,
                        signed=q.symmetric and bool(q.signed), axis=1)
    fq = lambda x, q: x if q is None else O.fake_quant(x, **kw(q))[1]
    terms = lambda x, g, q: O.ste_param_grad_terms(x, g, **kw(q))
    d = a.shape[-1]
    L, Lc = d // LPR[d] + int(math.log2(LPR[d])), trips + 256 // LPR[d] + 2
    t = fq(a, q1) + r
    u = fq(t, q2).double()
    mean = u.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((u - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    xh = (u - mean) * rstd
    z = xh * w.double() + b.double()
    gz, out = gy.double(), {}

    def range_grads(name, q, tr, t1, extra_d, extra_z):
        cols = [(t1 - tr['t2']).sum(0), tr['tz'].sum(0), (Lc + 16) * U * (t1.abs() + tr['t2'].abs()).sum(0) + extra_d.sum(0),
                (Lc + 16) * U * tr['tz'].abs().sum(0) + extra_z.sum(0)]
        if q.delta.numel() == 1:
            cols = [c.sum().reshape(1) for c in cols]
            cols[2] += 2.0 ** -52 * d * (t1.abs() + tr['t2'].abs()).sum()
        out[name] = (torch.stack([cols[0] * tr['chain_delta'], cols[1] * tr['chain_zero_float']]),
                     torch.stack([cols[2] * tr['chain_delta'].abs(), cols[3]]))

    if q3 is not None:
        s3 = O.effective_scale(q3.delta, EPS).double()
        lo, hi = O.grid_limits(q3.n_bits, q3.symmetric, q3.symmetric and bool(q3.signed))
        zp3 = 0.0 if q3.symmetric else O.effective_zero_point(q3.zero_float, q3.n_bits).double()
        dz = E * z.abs() + 1e-5
        for edge in (hi - zp3 + 0.5, lo - zp3 - 0.5):
            assert bool(((z / s3 - edge).abs() > 2 * dz.max() / s3).all()), 'seed puts a z on a clamp threshold of Q_out'
        tr = terms(z.float(), gy, q3)
        range_grads('q_out', q3, tr, gz * torch.round(y_gpu.double() / s3), tr['mask'] * gz.abs() * dz / s3, torch.zeros_like(z))
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
            range_grads(name, q, tr, tr['t1'], trb['t1'].abs() + trb['t2'].abs(), trb['tz'].abs())
            gu = torch.where(tr['mask'], gu, torch.zeros_like(gu))
        out[outname] = (gu, B)
    return out


def _launch(data, kinds, ranges=RANGES, want=None, trips=1, compare=True, perm=False):
    """both launches on data = (a, r, gy, w, b) -> (the backward's outputs, the forward's y), on the CPU"""
    from quantization import _hip
    qs = [_spec(k, *rng, data[0].shape[-1], perm) for k, rng in zip(kinds, ranges)]
    cuda = lambda t: t.cuda() if torch.is_tensor(t) else t
    (a, r, gy, w, b), (k1, k2, k3) = map(cuda, data), (q and type(q)(*map(cuda, q)) for q in qs)
    want = want or DATA + [n for n, q in zip(('q_dense', 'q_sum', 'q_out'), qs) if q]
    be = _hip.backend()
    got = {k: v.cpu() for k, v in be.residual_layernorm_quant_axis_bwd(a, r, gy, k1, k2, w, b, LN_EPS, k3, want=want).items()}
    y_fwd = be.residual_layernorm_quant_axis(a, r, k1, k2, w, b, LN_EPS, k3).cpu()
    if compare:
        assert torch.equal(got['y'].view(torch.int32), y_fwd.view(torch.int32))
        ref = _reference(*data, qs, y_fwd, trips)
        for name in set(got) - {'y'}:
            assert got[name].shape == ref[name][0].shape, name
            assert bool(((got[name].double() - ref[name][0]).abs() <= ref[name][1]).all()), name
    return got, y_fwd


@pytest.mark.parametrize('rows,d,perm', [(rows, d, False) for d in sorted(LPR) for rows in (1, 21)]
                         + [(8200, 64, False), (4100, 128, False), (2052, 256, False), (21, 768, True)])
def test_every_row_length_and_a_second_grid_stride_trip(rows, d, perm):
    """K's shapes (21 rows: lane groups past the end run clamped; the large ones: a second trip per lane-group form, with a
    Q_out range that never clamps) with six column groups per quantizer, once scattered.  Two runs give identical bits."""
    # (d = 512: K's seed puts a z on a clamp threshold of the per-column Q_out; the next one does not)
    seed, ranges = (11, (RANGES[0], RANGES[1], (-8.0, 8.0))) if rows > 21 else (1700 + d + rows + (d == 512), RANGES)
    got, _ = _launch(_inputs(rows, d, seed), PEG, ranges, trips=2 if rows > 21 else 1, perm=perm)
    again, _ = _launch(_inputs(rows, d, seed), PEG, ranges, compare=False, perm=perm)
    assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got)


@pytest.mark.parametrize('kinds', [PEG, ('col', None, None), (None, 'col', None), (None, None, 'col'), ('pt', 'col', 'pt'),
                                   ('col', 'pt', 'col'), ('pt', 'pt', 'col'), ('col', None, 'pt'), (None, 'col', 'col'),
                                   ('sym', 'col', 'col'), ('col', 'sym', 'pt'), ('div', 'col', 'col')])
@pytest.mark.parametrize('range_grads', [True, False])
def test_quantizer_mixes(kinds, range_grads):
    """absent / per-tensor / per-column in each place (at least one per-column), a symmetric per-column quantizer, and a 23-bit
    Q_dense that sends the launch through the division body -- y equals the forward launch in both bodies"""
    _launch(_inputs(21, 384, 61), kinds, want=None if range_grads else DATA)


@pytest.mark.parametrize('row,col', [(0, 0), (7, 3), (8, 4), (20, 127)])
def test_one_hot_probes(row, col):
    """d = 128: 8 rows per block, a lane owns 4 columns.  grad_y is 1.25 at the first / last row of a block and of the tensor,
    the first / last column of a lane and of the row: the bias gradient and Q_out's range gradient are that column's alone"""
    a, r, gy, w, b = _inputs(21, 128, 5)
    gy.zero_()[row, col] = 1.25
    got, _ = _launch((a, r, gy, w, b), PEG)
    assert got['ln_bias'].nonzero().tolist() == [[col]] and got['q_out'][0].nonzero().tolist() == [[col]]
    others = torch.arange(21) != row
    assert bool((got['dense'][others] == 0).all()) and bool((got['residual'][others] == 0).all())


@pytest.mark.parametrize('kinds', [PEG, ('div', 'col', 'pt')])
def test_nan_row(kinds):
    """a NaN input: its row is NaN inside the clamp ranges (0 outside); the sums of every column the row's NaN terms fall in are
    NaN -- all of them for the affine, Q_out's and Q_sum's _delta; for Q_dense's _delta and Q_sum's _zero_float exactly the
    columns where the row's residual gradient is NaN / 0 -- and every per-tensor sum; every other row is what it is without"""
    data = _inputs(21, 256, 10)
    clean, _ = _launch(data, kinds)
    data[0][13, 77] = float('nan')
    got, y_fwd = _launch(data, kinds, compare=False)
    others, inside = torch.arange(21) != 13, got['residual'][13].isnan()
    for k in ('dense', 'residual'):
        assert torch.equal(got[k][others], clean[k][others]) and bool((got[k][13].isnan() | (got[k][13] == 0)).all())
        assert int(got[k][13].isnan().sum()) > 128
    assert bool(got['y'][13].isnan().all()) and torch.equal(got['y'].isnan(), y_fwd.isnan())
    assert all(bool(got[k].isnan().all()) for k in ('ln_weight', 'ln_bias')) and bool(got['q_sum'][0].isnan().all())
    assert bool(got['q_out'][0].isnan().all())
    assert torch.equal(got['q_sum'][1].isnan(), ~inside)
    keep = torch.arange(256) != 77
    assert torch.equal(got['q_dense'][0].isnan()[keep], inside[keep])
