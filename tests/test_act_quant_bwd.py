"""tq_bias_act_quant_fwd / tq_bias_act_quant_bwd against a float64 reference of the formulas in include/tq_hip.h, built from
oracle.tq_oracle: a = g + bias, h = act(a), act'(a) and every sum in float64; the clamped index xi - zp = rint(y / s) is read
from the forward launch's own y, the mask is the oracle's on the reference h.  The reference alone asserts that no h / s lies
within MARGIN = 2 max(EH) / s grid steps of the clamp thresholds hi - zp + 0.5 and lo - zp - 0.5 (seeds picked on the CPU); no
element is excluded.  Bounds, u = 2^-24.  The kernel's a carries one rounding, u |a|, which reaches h through |act'| <= 1.13
and act' through |act''| <= 0.4; csrc/tq_act_bwd.hip states 9.0e-8 |a| + 2^-23 |GELU(a)| and 2.5e-7 for its GELU and GELU':
    EH = (9.0e-8 + 1.2 u) |a| + 2 u |h|, ED = 2.5e-7 + u |a|  (GELU)    EH = u |a|, ED = 0  (none, ReLU: [a > 0] survives)
    ga = gh * act' with gh = (gy s) / s: three roundings      |ga - ref| <= B = |gh| (ED + 4 u |act'|)
Column sums (a lane adds its rows, one per trip of the grid-stride loop; the block its 4 row groups; then float64), per column:
    sum over rows of B + Lc u sum |ga|,  Lc = trips + 4 + 2
Range gradients, Lb = 4 trips lane-local adds + 6 wave steps + 4 LDS adds (block partials are added in float64):
    ((Lb + 16) u A_d + sum in |gy| EH / s) |chain|,    (Lb + 16) u A_z            (A_d, A_z of ste_param_grad_terms)
Grid: strips of 256 columns x min(ceil(rows / 4), 2048 / strips) chunks of 4 rows."""
import math

import pytest
import torch

from oracle import tq_oracle as O
from tests.test_ln_quant_bwd import EPS, U, _spec

pytestmark = pytest.mark.gpu
NONE, RELU, GELU = 0, 1, 2
RANGE, WIDE = (-0.1, 1.8), (-8.0, 8.0)                  # RANGE cuts the data of every activation function on both sides


def _inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, generator=g), 0.1 * torch.randn(cols, generator=g), torch.randn(rows, cols, generator=g)


_trips = lambda rows, cols: -(-rows // (4 * min(-(-rows // 4), max(1, 2048 // -(-cols // 256)))))      # per lane


def _forward64(g, bias, act, q):
    """float64 a, h, act', the bounds EH and ED, and (with a quantizer) its oracle arguments and scale; asserts MARGIN"""
    a = g.double() + (0 if bias is None else bias.double())
    if act == GELU:
        Phi = 0.5 * (1 + torch.erf(a / math.sqrt(2)))
        h, dact = a * Phi, Phi + a * torch.exp(-a * a / 2) / math.sqrt(2 * math.pi)
        EH, ED = (9.0e-8 + 1.2 * U) * a.abs() + 2 * U * h.abs(), 2.5e-7 + U * a.abs()
    else:
        h, dact = (a.clamp(min=0), (a > 0).double()) if act == RELU else (a, torch.ones_like(a))
        EH, ED = U * a.abs(), torch.zeros_like(a)
    if q is None:
        return a, h, dact, EH, ED, None, None
    cpu = lambda t: None if t is None else t.detach().cpu().reshape(())
    kw = dict(delta=cpu(q.delta), zero_float=cpu(q.zero_float), n_bits=q.n_bits, symmetric=q.symmetric, eps=q.eps,
              signed=q.symmetric and bool(q.signed), scale_domain='log' if q.log_domain else 'linear')
    s = float(O.effective_scale(kw['delta'].double(), EPS, kw['scale_domain']).float())
    lo, hi = O.grid_limits(kw['n_bits'], kw['symmetric'], kw['signed'])
    zp = 0.0 if kw['symmetric'] else float(O.effective_zero_point(kw['zero_float'], kw['n_bits']))
    for edge in (hi - zp + 0.5, lo - zp - 0.5):
        assert float((h / s - edge).abs().min()) > 2 * float(EH.max()) / s, 'seed puts an h on a clamp threshold'
    return a, h, dact, EH, ED, kw, s


def _reference(g, bias, gy, act, q, y_gpu, trips):
    """-> {name: (float64 value, bound)} (see the module docstring)"""
    a, h, dact, EH, ED, kw, s = _forward64(g, bias, act, q)
    gh, out = gy.double(), {'h': (h, EH)}
    Lc, Lb = trips + 6, 4 * trips + 10
    if q is not None:
        tr = O.ste_param_grad_terms(h.float(), gy, **kw)
        t1 = gh * torch.round(y_gpu.double() / s)
        chain = float(tr['chain_delta'].abs())
        extra = (tr['mask'] * gh.abs() * EH / s).sum()
        out['q_out'] = (torch.stack([(t1 - tr['t2']).sum() * float(tr['chain_delta']), tr['d_zero_float'].sum()]),
                        torch.stack([((Lb + 16) * U * (t1.abs() + tr['t2'].abs()).sum() + extra) * chain,
                                     (Lb + 16) * U * tr['A_z'].sum()]))
        gh = torch.where(tr['mask'], gh, torch.zeros_like(gh))
    ga, B = gh * dact, gh.abs() * (ED + 4 * U * dact.abs())
    out['gemm'] = (ga, B)
    out['bias'] = (ga.sum(0), B.sum(0) + Lc * U * ga.abs().sum(0))
    return out


def _launch(data, act, kind, rng=RANGE, with_bias=True, compare=True):
    """both launches on data = (g, bias, gy) -> the backward's outputs on the CPU, everything it can give asked for"""
    from quantization import _hip
    be, (g, bias, gy), q = _hip.backend(), data, _spec(kind, *rng)
    bias = bias if with_bias else None
    cuda = lambda t: t.cuda() if torch.is_tensor(t) else t
    gc, bc, gyc, qc = cuda(g), cuda(bias), cuda(gy), q and type(q)(*map(cuda, q))
    want = ['gemm', 'h', 'y'] + (['bias'] if with_bias else []) + (['q_out'] if q else [])
    got = be.bias_act_quant_bwd(gc, bc, gyc, act, qc, want=want)
    y_fwd = be.bias_act_quant(gc, bc, act, qc)
    if compare:
        bits = lambda t: t.view(torch.int32)
        assert torch.equal(bits(got['y']), bits(y_fwd))
        assert torch.equal(bits(y_fwd), bits(got['h'] if q is None else be.fake_quant(got['h'], *qc, 1, 1)[0]))
        ref = _reference(g, bias, gy, act, q, y_fwd.cpu(), _trips(*g.shape))
        for name in set(got) - {'y'}:
            assert bool(((got[name].cpu().double() - ref[name][0]).abs() <= ref[name][1]).all()), name
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize('rows,cols', [(rows, cols) for cols in (4, 68, 3072) for rows in (1, 21)] + [(8200, 4), (700, 3072)])
def test_shapes_and_a_second_grid_stride_trip(rows, cols):
    """one lane, a ragged strip, twelve strips; 21 rows: row groups past the end; the large ones: a second trip with one strip
    (2048 chunks) and with twelve (170 chunks), Q's range wide there.  Two runs give identical bits."""
    seed, rng = (3, WIDE) if rows > 21 else (2400 + cols + rows, RANGE)
    got = _launch(_inputs(rows, cols, seed), GELU, 'asym', rng)
    again = _launch(_inputs(rows, cols, seed), GELU, 'asym', rng, compare=False)
    assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got)


@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('kind', [None, 'asym', 'sym', 'log', 'div'])
@pytest.mark.parametrize('act', [NONE, RELU, GELU])
def test_activation_quantizer_bias_mixes(act, kind, with_bias):
    """'div': a 23-bit grid, which the vote sends through the division body -- y equals tq_fake_quant_fwd's in both bodies"""
    _launch(_inputs(21, 68, 77), act, kind, with_bias=with_bias)


@pytest.mark.parametrize('row,col', [(0, 0), (3, 3), (4, 255), (20, 256), (20, 515)])
def test_one_hot_probes(row, col):
    """cols = 516: two strips and one lane of a third; 4 rows per block.  grad_y is 1.25 at the first / last row of a block and
    the tensor, the first / last column of a lane, a strip and the tensor: one non-zero grad_bias column, one grad_gemm element"""
    g, bias, gy = _inputs(21, 516, 5)
    gy.zero_()[row, col] = 1.25
    got = _launch((g, bias, gy), NONE, 'asym', WIDE)
    assert got['bias'].nonzero().tolist() == [[col]] and got['gemm'].nonzero().tolist() == [[row, col]]


@pytest.mark.parametrize('act,kind', [(GELU, 'asym'), (RELU, 'div'), (NONE, None)])
def test_nan_element(act, kind):
    """a NaN in gemm: NaN there in grad_gemm, in that column of grad_bias and in d loss / d _delta; nothing else changes"""
    data = _inputs(21, 68, 9)
    clean = _launch(data, act, kind)
    data[0][13, 37] = float('nan')
    got = _launch(data, act, kind, compare=False)
    for k in ('gemm', 'bias', 'y'):
        nan = torch.zeros_like(clean[k], dtype=torch.bool)
        nan[(13, 37) if k != 'bias' else 37] = True
        assert torch.equal(got[k].isnan(), nan) and torch.equal(got[k][~nan], clean[k][~nan]), k
    assert kind is None or bool(got['q_out'][0].isnan())
