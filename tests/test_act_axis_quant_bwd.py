"""tq_bias_act_quant_axis_fwd / tq_bias_act_quant_axis_bwd (one output-quantizer parameter per column) against a float64 reference
built from oracle.tq_oracle with axis=1.  The derivation is tests/test_act_quant_bwd.py's (K): a, h, act'(a) and every sum in
float64 with K's activation bounds EH and ED; the clamped index xi - zp_c = rint(y / s_c) is read from the forward launch's own
y, the mask is the oracle's on the reference h.  The reference alone asserts that no h / s_c lies within 2 max(EH) / s_c grid
steps of a clamp threshold of ITS column (seeds picked on the CPU); no element is excluded.  Bounds, u = 2^-24:
    grad_gemm: K's B = |gh| (ED + 4 u |act'|); grad_bias: sum over rows of B + Lc u sum |ga|, Lc = trips + 4 + 2 (K's)
What changes: every range sum is a COLUMN sum -- a lane adds its rows (one per trip), the block its four row groups, then
float64 -- so it takes the column-sum length Lc where K has Lb, per column c:
    ((Lc + 16) u A_c + sum over rows of in |gy| EH / s_c) |chain_c|,    (Lc + 16) u A_z,c      (A of ste_param_grad_terms)
Parameters: six groups of columns with ranges (0.85 + 0.06 g) x the base range, contiguous or (`perm`) scattered: T._spec."""
import pytest
import torch

from oracle import tq_oracle as O
from tests import test_act_quant_bwd as K
from tests import test_ln_axis_quant_bwd as T
from tests.test_act_quant_bwd import EPS, GELU, NONE, RANGE, RELU, U, WIDE, _inputs, _trips

pytestmark = pytest.mark.gpu
bits = lambda t: t.view(torch.int32)


def _reference(g, bias, gy, act, q, y_gpu, trips):
    """-> {name: (float64 value, bound)}; 'q_out' is [2, cols]"""
    a, h, dact, EH, ED, _, _ = K._forward64(g, bias, act, None)
    kw = dict(delta=q.delta, zero_float=q.zero_float, n_bits=q.n_bits, symmetric=q.symmetric, eps=q.eps,
              signed=q.symmetric and bool(q.signed), axis=1)
    s = O.effective_scale(q.delta, EPS).double()
    lo, hi = O.grid_limits(q.n_bits, q.symmetric, kw['signed'])
    zp = 0.0 if q.symmetric else O.effective_zero_point(q.zero_float, q.n_bits).double()
    for edge in (hi - zp + 0.5, lo - zp - 0.5):
        assert bool(((h / s - edge).abs() > 2 * EH.max() / s).all()), 'seed puts an h on a clamp threshold of its column'
    tr, gh, Lc = O.ste_param_grad_terms(h.float(), gy, **kw), gy.double(), trips + 6
    t1 = gh * torch.round(y_gpu.double() / s)
    A_d = (Lc + 16) * U * (t1.abs() + tr['t2'].abs()).sum(0) + (tr['mask'] * gh.abs() * EH / s).sum(0)
    out = {'h': (h, EH),
           'q_out': (torch.stack([(t1 - tr['t2']).sum(0) * tr['chain_delta'], tr['tz'].sum(0) * tr['chain_zero_float']]),
                     torch.stack([A_d * tr['chain_delta'].abs(), (Lc + 16) * U * tr['tz'].abs().sum(0)]))}
    gh = torch.where(tr['mask'], gh, torch.zeros_like(gh))
    ga, B = gh * dact, gh.abs() * (ED + 4 * U * dact.abs())
    out['gemm'] = (ga, B)
    out['bias'] = (ga.sum(0), B.sum(0) + Lc * U * ga.abs().sum(0))
    return out


def _launch(data, act, kind, rng=RANGE, with_bias=True, compare=True, perm=False, far_column=None):
    """both launches on data = (g, bias, gy) -> the backward's outputs on the CPU, everything it can give asked for.
    far_column: that column's scale is 2^101, beyond the branch-free body's range"""
    from quantization import _hip
    be, (g, bias, gy), q = _hip.backend(), data, T._spec(kind, *rng, data[0].shape[1], perm)
    if far_column is not None:
        q.delta[far_column] = 2.0 ** 101
    bias = bias if with_bias else None
    cuda = lambda t: t.cuda() if torch.is_tensor(t) else t
    gc, bc, gyc, qc = cuda(g), cuda(bias), cuda(gy), type(q)(*map(cuda, q))
    got = be.bias_act_quant_axis_bwd(gc, bc, gyc, act, qc, want=['gemm', 'h', 'y', 'q_out'] + (['bias'] if with_bias else []))
    y_fwd = be.bias_act_quant_axis(gc, bc, act, qc)
    if compare:
        assert torch.equal(bits(got['y']), bits(y_fwd))
        assert torch.equal(bits(y_fwd), bits(be.fake_quant(got['h'], *qc, g.shape[1], 1)[0]))
        ref = _reference(g, bias, gy, act, q, y_fwd.cpu(), _trips(*g.shape))
        for name in set(got) - {'y'}:
            assert got[name].shape == ref[name][0].shape, name
            assert bool(((got[name].cpu().double() - ref[name][0]).abs() <= ref[name][1]).all()), name
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize('rows,cols', [(rows, cols) for cols in (4, 68, 3072) for rows in (1, 21)] + [(8200, 4), (700, 3072)])
def test_shapes_and_a_second_grid_stride_trip(rows, cols):
    """one lane, a ragged strip, twelve strips; 21 rows: row groups past the end; the large ones: a second trip with one strip
    (2048 chunks) and with twelve (170 chunks), Q's range wide there.  Scattered groups at 68 columns and at [700, 3072].  Two
    runs give identical bits."""
    # ([21, 3072]: K's seed 5493 and the four behind it put an h on a clamp threshold of its column; 5498 does not)
    seed, rng = (3, WIDE) if rows > 21 else (2400 + cols + rows + 5 * (rows * cols == 21 * 3072), RANGE)
    perm = cols == 68 or rows == 700
    got = _launch(_inputs(rows, cols, seed), GELU, 'col', rng, perm=perm)
    again = _launch(_inputs(rows, cols, seed), GELU, 'col', rng, compare=False, perm=perm)
    assert all(torch.equal(bits(got[k]), bits(again[k])) for k in got)


@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('kind', ['col', 'sym', 'div'])
@pytest.mark.parametrize('act', [NONE, RELU, GELU])
def test_activation_quantizer_bias_mixes(act, kind, with_bias):
    """'div': a 23-bit grid, which every strip's vote sends through the division body -- y equals tq_fake_quant_fwd's in both"""
    _launch(_inputs(21, 68, 77), act, kind, with_bias=with_bias)


def test_strips_vote_by_themselves():
    """cols = 516: the last strip (4 columns) holds a column the branch-free body cannot take and runs the division body, the two
    full strips vote branch-free.  The quantizer descriptor has ONE n_bits, so the column is put out of the vote by its scale
    (2^101), not by a 23-bit grid; at such a scale the range term (gy s h) / (s s) has no fp32 value (s s overflows), so that
    column's grad_y is zero here: its y, its zeros and every other column are checked as everywhere."""
    g, bias, gy = _inputs(21, 516, 78)
    gy[:, 515] = 0
    _launch((g, bias, gy), GELU, 'col', far_column=515)


@pytest.mark.parametrize('clamped', [False, True])
@pytest.mark.parametrize('row,col', [(0, 0), (3, 3), (4, 255), (20, 256), (20, 515)])
def test_one_hot_probes(row, col, clamped):
    """cols = 516: two strips and one lane of a third; 4 rows per block.  grad_y is 1.25 at the first / last row of a block and
    the tensor, the first / last column of a lane, a strip and the tensor.  Inside the grid: one grad_gemm element, that column
    alone in grad_bias and in the _delta row (the _zero_float term of an element inside is zero); with a range that cuts every
    element: that column alone in both rows of grad_q_out, and no data gradient."""
    g, bias, gy = _inputs(21, 516, 5)
    gy.zero_()[row, col] = 1.25
    got = _launch((g, bias, gy), NONE, 'col', (-0.02, 0.02) if clamped else WIDE)
    assert got['q_out'][0].nonzero().tolist() == [[col]]
    assert got['q_out'][1].nonzero().tolist() == ([[col]] if clamped else [])
    assert got['bias'].nonzero().tolist() == ([] if clamped else [[col]])
    assert got['gemm'].nonzero().tolist() == ([] if clamped else [[row, col]])


@pytest.mark.parametrize('act,kind', [(GELU, 'col'), (RELU, 'div')])
def test_nan_element(act, kind):
    """a NaN in gemm: NaN there in grad_gemm, in that column of grad_bias and in that column's _delta gradient; everything else
    has the clean run's bits (that column's _zero_float sum takes the NaN element as one outside the grid: finite)"""
    data = _inputs(21, 68, 9)
    clean = _launch(data, act, kind)
    data[0][13, 37] = float('nan')
    got = _launch(data, act, kind, compare=False)
    for k in ('gemm', 'bias', 'y', 'q_out'):
        nan = torch.zeros_like(clean[k], dtype=torch.bool)
        nan[{'bias': 37, 'q_out': (0, 37)}.get(k, (13, 37))] = True
        assert torch.equal(got[k].isnan(), nan), k
        nan[..., 37] |= k == 'q_out'
        assert torch.equal(got[k][~nan], clean[k][~nan]), k
