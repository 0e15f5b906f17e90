"""tq_residual_nonorm_quant_bwd against a float64 reference of the formulas in include/tq_hip.h, built from oracle.tq_oracle.

Reference: NoNorm has no statistics, so the whole forward -- a = Q1(g), t = a + r, u = Q2(t), z = u * w + b (two roundings),
y = Q3(z), the three masks and xi3 -- is reproduced EXACTLY in fp32 on the CPU (O.fake_quant, O.ste_param_grad_terms); every
gradient and sum is then formed in float64.  No element is excluded and no clamp margin is needed; the backward's y is
bit-equal to the forward launch and to the oracle's y.
Tolerance, u = 2^-24, gam(n) = n u / (1 - n u) for n fp32 roundings.  Data gradients: gz = (gy s3) / s3 carries 2 roundings,
gu = gz w 3, gt = (gu s2) / s2 5, gg = (gt s1) / s1 7:  |gt - ref| <= gam(5) |ref|,  |gg - ref| <= gam(7) |ref|.
Column sums: a lane adds its `trips` rows (grid-stride trips), the block its 4 waves x S row slots (S = 4, 2, 1 for d = 64,
128, >= 256) in LDS, the final launch in float64 and rounds once: Lc = trips + 4 S + 1 additions over terms of 2 (gz) and
3 (gz u) roundings:  bias gam(Lc + 2) sum |gz|,  weight gam(Lc + 3) sum |gz u|  per column.
Range sums: a lane adds 4 trips terms, the wave 6 butterfly steps, the block 4 waves in LDS, the final launch in float64 with one
rounding and one multiplication by the chain: Lb = 4 trips + 6 + 4 + 2.  A term g (xi - zp) - (g s v) / (s s) is 6 roundings on
top of at most 5 in its incoming gradient g, a term -(g s) 1 on top of 5:
    d: gam(Lb + 11) A_d |chain|,  z: gam(Lb + 6) A_z      (A_d = sum |t1| + |t2|, A_z = sum |tz| of ste_param_grad_terms).
Grid: strips = ceil(d / 256) x chunks = min(ceil(rows / 4 S), 2048 / strips) blocks, so 32769 / 16385 / 4097 rows take a second
trip at d = 64 / 128 / 512."""
import pytest
import torch

from oracle import tq_oracle as O
from tests.test_ln_quant_bwd import ALL, RANGES, U, _inputs, _spec

pytestmark = pytest.mark.gpu
NAMES = ('q_dense', 'q_sum', 'q_out')
gam = lambda n: n * U / (1 - n * U)


def _trips(rows, d):
    rpb, strips = 4 * max(1, 256 // d), -(-d // 256)
    return -(-rows // (min(-(-rows // rpb), 2048 // strips) * rpb))


def _reference(a, r, gy, w, b, qs, trips):
    """-> ({name: (float64 value, bound)}, the oracle's fp32 y)"""
    cpu = lambda t: None if t is None else t.detach().cpu().reshape(())
    kw = lambda q: dict(delta=cpu(q.delta), zero_float=cpu(q.zero_float), n_bits=q.n_bits, symmetric=q.symmetric, eps=q.eps,
                        signed=q.symmetric and bool(q.signed), scale_domain='log' if q.log_domain else 'linear')
    fq = lambda x, q: x if q is None else O.fake_quant(x, **kw(q))[1]
    d = a.shape[-1]
    Lc, Lb = trips + 4 * max(1, 256 // d) + 1, 4 * trips + 12
    t = fq(a, qs[0]) + r
    u = fq(t, qs[1])
    z = u * w + b
    g, out = gy.double(), {}
    for name, v, q in zip(NAMES[::-1], (z, t, a), qs[::-1]):
        if q is not None:
            tr = O.ste_param_grad_terms(v, g, **kw(q))
            chain = tr['chain_delta'].reshape(())
            out[name] = (torch.stack([(tr['t1'] - tr['t2']).sum() * chain, tr['d_zero_float'].sum()]),
                         torch.stack([gam(Lb + 11) * tr['A_d'].sum() * chain.abs(), gam(Lb + 6) * tr['A_z'].sum()]))
            g = torch.where(tr['mask'].bool(), g, torch.zeros_like(g))
        if name == 'q_out':
            out['ln_bias'] = (g.sum(0), gam(Lc + 2) * g.abs().sum(0))
            out['ln_weight'] = ((g * u.double()).sum(0), gam(Lc + 3) * (g * u.double()).abs().sum(0))
            g = g * w.double()
        if name == 'q_sum':
            out['residual'] = (g, gam(5) * g.abs())
    out['dense'] = (g, gam(7) * g.abs())
    return out, fq(z, qs[2])


def _launch(data, kinds, ranges=RANGES, want=None, compare=True):
    """both launches on data = (a, r, gy, w, b) -> the backward's outputs on the CPU"""
    from quantization import _hip
    qs = [_spec(k, *rng) for k, rng in zip(kinds, ranges)]
    cuda = lambda t: t.cuda() if torch.is_tensor(t) else t
    (a, r, gy, w, b), (k1, k2, k3) = map(cuda, data), (q and type(q)(*map(cuda, q)) for q in qs)
    want = want or ['dense', 'residual', 'ln_weight', 'ln_bias', 'y'] + [n for n, q in zip(NAMES, qs) if q]
    be = _hip.backend()
    got = {k: v.cpu() for k, v in be.residual_nonorm_quant_bwd(a, r, gy, k1, k2, w, b, k3, want=want).items()}
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(got['y']), bits(be.residual_layernorm_quant(a, r, k1, k2, w, b, None, k3).cpu()))
    if compare:
        ref, y = _reference(*data, qs, _trips(*data[0].shape))
        assert torch.equal(bits(got['y']), bits(y))
        for name in set(got) - {'y'}:
            err, bound = (got[name].double() - ref[name][0]).abs(), ref[name][1]
            print(name, 'max error / bound', float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), name
    return got


@pytest.mark.parametrize('rows,d', [(rows, d) for d in (64, 128, 256, 384, 512, 3072) for rows in (1, 21)]
                         + [(32769, 64), (16385, 128), (4097, 512)])
def test_every_form_and_a_second_grid_stride_trip(rows, d):
    """4, 2 and 1 rows per wave with a partly empty last trip (21 rows), the ragged strip (d = 384), the widest row, and per form
    the smallest row count whose last block takes a second trip at the grid cap.  Two runs give identical bits."""
    got = _launch(_inputs(rows, d, 2600 + d + rows), ALL)
    again = _launch(_inputs(rows, d, 2600 + d + rows), ALL, compare=False)
    assert all(torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)) for k in got)


@pytest.mark.parametrize('kinds', [ALL, ('asym', None, None), (None, 'asym', None), (None, None, 'asym'), (None, None, None),
                                   ('asym', 'sym', 'asym'), ('div', 'asym', 'asym')])
@pytest.mark.parametrize('range_grads', [True, False])
def test_quantizer_mixes(kinds, range_grads):
    """all three, each alone, none, one symmetric, and a 23-bit Q_dense that sends the launch through the division body"""
    _launch(_inputs(21, 384, 61), kinds, want=None if range_grads else ['dense', 'residual', 'ln_weight', 'ln_bias', 'y'])


@pytest.mark.parametrize('kinds', [ALL, ('div', 'asym', 'asym')])
def test_nan_is_element_local(kinds):
    """a NaN in g: that element's y and data gradients, its column of the affine gradients and every d loss / d _delta are
    NaN; every other element and column has the bits of the run without the NaN"""
    data = _inputs(21, 128, 9)
    clean = _launch(data, kinds)
    data[0][13, 77] = float('nan')
    got = _launch(data, kinds, compare=False)
    for k, at in (('y', (13, 77)), ('dense', (13, 77)), ('residual', (13, 77)), ('ln_weight', (77,)), ('ln_bias', (77,))):
        hit = torch.zeros_like(got[k], dtype=torch.bool)
        hit[at] = True
        assert torch.equal(got[k].isnan(), hit) and torch.equal(got[k][~hit].view(torch.int32), clean[k][~hit].view(torch.int32)), k
    assert all(bool(got[k][0].isnan()) for k in NAMES)
