"""tq_residual_layernorm_quant_axis_ires_fwd (the per-column fp32 LayerNorm tail with its residual as int8 indices and one NaN
flag per row) against two references:

  * the GPU sibling, `HipBackend.residual_layernorm_quant_axis` on the fp32 dequantized residual (existing code, pinned to the
    oracle by tests/test_fused_ln_axis.py), in every case;
  * the CPU chain, tests/_exact_backend.ln_tail_chain, on the 37-row cases.

Every comparison is exact: y as int32 bit patterns, y_idx with torch.equal; where NaN rows are planted the NaN row set is
asserted first, then every other row of the indices is compared (the index bytes of a NaN row are unspecified).  Nothing else
is excluded.  The dequantized residual is computed here as the header states it -- max(delta_c, eps) * ((index + 128) -
clamp(round(zero_float_c))), one subtraction and one multiplication -- and is asserted to be the fp32 value the producing
quantizer launch wrote, bit for bit, before it is used.

Launch forms (`launch_form` restates tail_geom of csrc/tq_fused_ln.hip for fp32 rows): rows per block rpb = 256 / LPR, a second
trip of the row loop beyond rpb * 2048 rows, streaming loads / stores from rows * d * 4 >= 64 MiB.

Measured once on an MI355X (pytest --durations): the 60 cases together take 3.7 s, the slowest 0.98 s (the first one: it loads
the library); the two at-size cases 0.05 s and less.
"""
import collections
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-8
LN_EPS = 1e-12
WIDTHS = (64, 128, 256, 384, 512, 768)
NAN = float('nan')
INF = float('inf')

_LANES = {16: (16, 1), 32: (32, 1), 64: (64, 1), 96: (32, 3), 128: (64, 2), 192: (64, 3)}
Form = collections.namedtuple('Form', 'lpr nv rpb iters grid nt')


def launch_form(rows, d):
    lpr, nv = _LANES[d // 4]
    rpb = 256 // lpr
    iters = max(1, min(2, -(-rows // (rpb * 2048))))
    return Form(lpr, nv, rpb, iters, max(-(-rows // (rpb * iters)), 1), rows * d * 4 >= (64 << 20))


@pytest.fixture(autouse=True)
def _no_tuning_override(monkeypatch):
    monkeypatch.delenv('TQ_TAIL_ITERS', raising=False)


@pytest.fixture(scope='module')
def be():
    from quantization import _hip
    return _hip.backend()


# ranges of the sites: a ~ N(0, 2), a + r ~ N(0, 2.5), LayerNorm output ~ N(0, 1), residual ~ N(0, 1.5); some groups clip
SITES = {'dense': ((-7.0, -1.0), (1.0, 7.5)), 'sum': ((-20.0, -2.0), (2.0, 22.0)), 'out': ((-6.0, -0.5), (0.5, 11.0)),
         'res': ((-5.0, -1.0), (1.0, 5.0))}


def _grid(layout, d, site, bits=8, seed=0, eps=EPS):
    """backend 7-tuple of an asymmetric quantizer on the device: 'tensor' (one range), 'contig6' (6 runs of columns), 'scatter6'
    (6 groups over a random column permutation: PEG with permutation) or 'embd' (d distinct ranges)"""
    g = torch.Generator().manual_seed(seed * 131 + d + len(site) + {'tensor': 1, 'contig6': 2, 'scatter6': 3, 'embd': 4}[layout])
    n = {'tensor': 1, 'contig6': 6, 'scatter6': 6, 'embd': d}[layout]
    (l0, l1), (h0, h1) = SITES[site]
    lo = l0 + (l1 - l0) * torch.rand(n, generator=g)
    hi = h0 + (h1 - h0) * torch.rand(n, generator=g)
    delta = (hi - lo) / (2 ** bits - 1)
    zf = -lo / delta
    if layout != 'tensor':
        group = (torch.arange(d) * n) // d
        if layout == 'scatter6':
            group = group[torch.randperm(d, generator=g)]
        delta, zf = delta[group], zf[group]
    return (delta.contiguous().to(DEV), zf.contiguous().to(DEV), None, bits, False, False, eps)


def _dequant(q, idx, flags=None):
    """the header's R: scale_c * ((float)(idx + 128) - zp_c), one exact subtraction and one rounded multiplication"""
    delta, zf, _, bits, _, _, eps = q
    scale = torch.maximum(delta, torch.tensor(eps, device=DEV))
    zp = torch.clamp(torch.round(zf), 0, 2 ** bits - 1)
    r = (idx.float() + 128.0) - zp
    r = scale * r
    if flags is not None:
        r[flags.bool()] = NAN
    return r


def _residual(be, rows, d, q_res, g, spread=1.5):
    """a residual as one quantizer launch pair writes it: (fp32 values, int8 indices) on the grid q_res"""
    r0 = torch.randn(rows, d, device=DEV, generator=g) * spread
    n = q_res[0].numel()
    r, _ = be.fake_quant(r0, q_res[0], q_res[1], None, q_res[3], False, False, q_res[6], n, 1)
    r_idx = be.quantize_to_int8(r0, q_res[0], q_res[1], None, q_res[3], False, False, q_res[6], n, 1, minus_128=True)
    return r, r_idx


def _inputs(be, rows, d, q_res, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + 7919 * d + rows)
    a = torch.randn(rows, d, device=DEV, generator=g) * 2.0
    r, r_idx = _residual(be, rows, d, q_res, g)
    w = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=g)
    b = 0.1 * torch.randn(d, device=DEV, generator=g)
    return a, r, r_idx, w, b


def _bits(t):
    return t.contiguous().view(torch.int32)


def _emits(q):
    return q is not None and not q[4] and q[3] <= 8


def _cpu_chain(a, R, q1, q2, w, b, q3):
    from tests._exact_backend import _p, ln_tail_chain
    host = lambda q: None if q is None else tuple(t.cpu() if torch.is_tensor(t) else t for t in q)
    y, idx, _ = ln_tail_chain(a.cpu(), R.cpu(), _p(host(q1)), _p(host(q2)), w.cpu(), b.cpu(), LN_EPS, _p(host(q3)))
    return y, idx


def _compare(be, a, r, r_idx, q_res, flags_in, q1, q2, q3, w, b, forms=('idx/f32', 'idx/idx', 'y+idx/idx'), chain=False):
    """the axis tail on R (the dequantized residual, flagged rows NaN) against the new entry; forms: output form / residual form.
    -> (y of the axis tail, its NaN rows)"""
    plain = _dequant(q_res, r_idx)
    assert torch.equal(_bits(plain), _bits(r)), 'the dequantized index is not the value the quantizer launch wrote'
    R = _dequant(q_res, r_idx, flags_in)
    has_idx = _emits(q3)
    old = be.residual_layernorm_quant_axis(a, R, q1, q2, w, b, LN_EPS, q3, want_idx=has_idx)
    y_old, idx_old = old if has_idx else (old, None)
    nan_old = torch.isnan(y_old).any(-1)
    keep = ~nan_old
    for form in forms:
        out, resform = form.split('/')
        want_y, want_idx = out != 'idx', out != 'y'
        if want_idx and not has_idx:
            continue
        res = (None, r_idx, q_res, flags_in) if resform == 'idx' else (R, None, None, None)
        y, idx, flags = be.residual_layernorm_quant_axis_ires(a, *res, q1, q2, w, b, LN_EPS, q3, want_y=want_y, want_idx=want_idx)
        assert flags.dtype == torch.uint8 and flags.shape == a.shape[:-1]
        assert torch.equal(flags.bool(), nan_old), form                       # the NaN row set first
        assert (y is None) == (not want_y) and (idx is None) == (not want_idx), form
        if want_y:
            assert torch.equal(_bits(y), _bits(y_old)), form
        if want_idx:
            assert torch.equal(idx[keep], idx_old[keep]), form
    if chain:
        y_c, idx_c = _cpu_chain(a, R, q1, q2, w, b, q3)
        assert torch.equal(torch.isnan(y_c).any(-1), nan_old.cpu())
        k = keep.cpu()
        assert torch.equal(_bits(y_c[k]), _bits(y_old.cpu()[k]))
        if has_idx:
            assert torch.equal(idx_c[k], idx_old.cpu()[k].float() + 128)
    return y_old, nan_old


def _peg_layouts(d):
    """the two tails of a PEG layer: (q_dense, q_sum, q_out, q_res)"""
    attn = (_grid('tensor', d, 'dense'), _grid('tensor', d, 'sum'), _grid('contig6', d, 'out'), _grid('tensor', d, 'res'))
    ffn = (_grid('contig6', d, 'dense', seed=1), _grid('contig6', d, 'sum', seed=1), _grid('tensor', d, 'out'),
           _grid('contig6', d, 'res', seed=1))
    return attn, ffn


@pytest.mark.parametrize('d', WIDTHS)
def test_every_width_37_rows(be, d):
    """37 rows: a partly filled last block for every rows-per-block value (4, 8, 16); both PEG tail layouts, the three operating
    forms, the GPU sibling and the CPU chain"""
    rows = 37
    assert rows % launch_form(rows, d).rpb != 0
    for q1, q2, q3, qr in _peg_layouts(d):
        a, r, r_idx, w, b = _inputs(be, rows, d, qr)
        flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
        flags_in[3] = 1
        a[11, d // 2] = NAN
        _, nan = _compare(be, a, r, r_idx, qr, flags_in, q1, q2, q3, w, b, chain=True)
        assert nan.nonzero().flatten().tolist() == [3, 11]


def test_second_trip_of_the_row_loop_d768(be):
    rows, d = 8197, 768
    f = launch_form(rows, d)
    assert f.iters == 2 and not f.nt and launch_form(8192, d).iters == 1 and rows % (f.rpb * f.iters) != 0
    q1, q2, q3, qr = _peg_layouts(d)[1]
    a, r, r_idx, w, b = _inputs(be, rows, d, qr)
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[[4, 8195]] = 1                # a second-trip row of the first block, a first-trip row of the last one
    a[8196, 1] = NAN
    _, nan = _compare(be, a, r, r_idx, qr, flags_in, q1, q2, q3, w, b)
    assert nan.nonzero().flatten().tolist() == [4, 8195, 8196]


def test_streaming_form_d768(be):
    rows, d = 21846, 768
    f = launch_form(rows, d)
    assert f.nt and not launch_form(rows - 1, d).nt and rows * d * 4 >= 64 << 20 > (rows - 1) * d * 4
    q1, q2, q3, qr = _peg_layouts(d)[1]
    a, r, r_idx, w, b = _inputs(be, rows, d, qr)
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[rows - 1] = 1
    _, nan = _compare(be, a, r, r_idx, qr, flags_in, q1, q2, q3, w, b)
    assert nan.nonzero().flatten().tolist() == [rows - 1]


@pytest.mark.parametrize('mix', [('tensor', 'tensor', 'contig6'), ('contig6', 'contig6', 'tensor'),
                                 ('scatter6', 'scatter6', 'scatter6'), ('embd', 'embd', 'embd')],
                         ids=['peg-attn', 'peg-ffn', 'all-scatter6', 'all-embd'])
@pytest.mark.parametrize('res', ['tensor', 'contig6', 'scatter6'])
def test_quantizer_mixes_and_groups(be, mix, res):
    """the two PEG layouts, all per-column; 6 contiguous and 6 scattered groups; every residual grid kind behind each"""
    rows, d = 37, 768
    q1, q2, q3 = (_grid(lay, d, site, seed=2) for lay, site in zip(mix, ('dense', 'sum', 'out')))
    qr = _grid(res, d, 'res', seed=2)
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=1)
    a[2, 5] = NAN
    a[6, 0], a[6, 767] = INF, -INF
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[20] = 1
    _, nan = _compare(be, a, r, r_idx, qr, flags_in, q1, q2, q3, w, b, forms=('idx/f32', 'idx/idx', 'y+idx/idx', 'y/idx'),
                      chain=True)
    assert nan.nonzero().flatten().tolist() == [2, 20]


def test_all_per_tensor_equals_the_per_tensor_index_tail(be):
    rows, d = 37, 768
    q1, q2, q3, qr = (_grid('tensor', d, s, seed=3) for s in ('dense', 'sum', 'out', 'res'))
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=2)
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[36] = 1
    a[0, 0] = NAN
    _compare(be, a, r, r_idx, qr, flags_in, q1, q2, q3, w, b, chain=True)
    for want_y in (True, False):
        y0, i0, n0 = be.residual_layernorm_quant_ires(a, None, r_idx, qr, flags_in, q1, q2, w, b, LN_EPS, q3, want_y=want_y)
        y1, i1, n1 = be.residual_layernorm_quant_axis_ires(a, None, r_idx, qr, flags_in, q1, q2, w, b, LN_EPS, q3, want_y=want_y)
        assert torch.equal(n0, n1) and n1.nonzero().flatten().tolist() == [0, 36]
        keep = ~n1.bool()
        assert torch.equal(i0[keep], i1[keep])
        assert (y1 is None) == (not want_y) and (y1 is None or torch.equal(_bits(y0), _bits(y1)))


@pytest.mark.parametrize('use', list(itertools.product((1, 0), repeat=3)))
def test_eight_on_off_combinations_per_column(be, use):
    """the eight mixes of present and absent per-column quantizers; NaN in dense_out everywhere, +-inf where Q_dense clamps it"""
    rows, d = 37, 768
    qs = [_grid('scatter6', d, site, seed=4) for site in ('dense', 'sum', 'out')]
    q1, q2, q3 = (q if u else None for q, u in zip(qs, use))
    qr = _grid('contig6', d, 'res', seed=4)
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=3)
    a[2, 5] = NAN
    if q1 is not None:
        a[6, 0], a[6, 767] = INF, -INF
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[20] = 1
    _, nan = _compare(be, a, r, r_idx, qr, flags_in, q1, q2, q3, w, b, forms=('idx/f32', 'idx/idx', 'y+idx/idx', 'y/idx', 'y/f32'),
                      chain=True)
    assert nan.nonzero().flatten().tolist() == [2, 20]


@pytest.mark.parametrize('bits', [8, 4, 1])
@pytest.mark.parametrize('layout,zero', [('tensor', '0'), ('tensor', 'top'), ('tensor', 'mid'), ('embd', '0'), ('embd', 'top'),
                                         ('embd', 'mid'), ('embd', 'mixed')])
def test_residual_grids(be, layout, bits, zero):
    """per-tensor and per-column residual grids of 8, 4 and 1 bits with the zero point at 0, at 2^n - 1, mid-grid, and (per
    column) all three mixed"""
    rows, d = 37, 384
    top = 2 ** bits - 1
    zs = {'0': [0.0], 'top': [float(top)], 'mid': [float(top // 2 + (bits == 1))], 'mixed': [0.0, float(top), float(top // 2)]}[zero]
    n = 1 if layout == 'tensor' else d
    g = torch.Generator().manual_seed(bits * 7 + len(zero))
    delta = ({8: 0.01, 4: 0.1, 1: 0.5}[bits] * (1 + torch.rand(n, generator=g))).to(DEV)
    zf = torch.tensor([zs[c % len(zs)] for c in range(n)], device=DEV) + (0.3 if zero == 'mid' else 0.0)
    qr = (delta, zf, None, bits, False, False, EPS)
    q1, q2, q3, _ = _peg_layouts(d)[1]
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=4)
    r_idx[0, :], r_idx[1, :] = -128, top - 128                                  # both ends of the grid in every column
    r = _dequant(qr, r_idx)
    _compare(be, a, r, r_idx, qr, None, q1, q2, q3, w, b, chain=True)


@pytest.mark.parametrize('which', [0, 1, 2])
def test_division_path(be, which):
    """one column of one quantizer with a scale outside [2^-100, 2^100] sends the whole launch down the division path"""
    rows, d = 37, 768
    q1, q2, q3, qr = (_grid(lay, d, s, seed=5) for lay, s in (('embd', 'dense'), ('embd', 'sum'), ('embd', 'out'), ('embd', 'res')))
    qs = [q1, q2, q3]
    delta = qs[which][0].clone()
    delta[301] = 3e30
    qs[which] = (delta,) + qs[which][1:]
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=5)
    a[2, 5] = NAN
    a[6, 0], a[6, 767] = INF, -INF
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[[0, 36]] = 1
    _, nan = _compare(be, a, r, r_idx, qr, flags_in, *qs, w, b, forms=('idx/f32', 'idx/idx', 'y+idx/idx', 'y/idx'), chain=True)
    assert nan.nonzero().flatten().tolist() == [0, 2, 36]


def test_special_values_and_flagged_rows(be):
    """NaN / +-inf in dense_out; flagged residual rows: the first, the last, two adjacent ones of one block -- also a row that is
    flagged AND has a NaN of its own"""
    rows, d = 37, 768
    assert launch_form(rows, d).rpb == 4
    for q1, q2, q3, qr in _peg_layouts(d):
        a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=6)
        a[1, 0], a[1, 300], a[1, 767] = INF, -INF, INF
        a[13, 766] = NAN
        a[9, 3] = NAN
        flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
        flags_in[[0, 8, 9, 36]] = 1                         # rows 8 and 9 share the block of rows 8..11
        y_old, nan = _compare(be, a, r, r_idx, qr, flags_in, q1, q2, q3, w, b)
        assert nan.nonzero().flatten().tolist() == [0, 8, 9, 13, 36]
        assert torch.isnan(y_old[nan]).all() and not torch.isnan(y_old[~nan]).any()
        _, nan = _compare(be, a, r, r_idx, qr, None, q1, q2, q3, w, b)
        assert nan.nonzero().flatten().tolist() == [9, 13]


def test_infinite_sum_without_quantizers_is_a_flagged_nan_row(be):
    """no quantizer clamps an inf: the statistics turn the row NaN, and the flag says so"""
    rows, d = 9, 256
    qr = _grid('contig6', d, 'res', seed=7)
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=7)
    a[4, 17] = INF
    y_old, nan = _compare(be, a, r, r_idx, qr, None, None, None, None, w, b, forms=('y/idx', 'y/f32'))
    assert nan.nonzero().flatten().tolist() == [4] and torch.isnan(y_old[4]).all()


def test_chained_launches_carry_the_nan_row(be):
    """two tails in a row, as in a PEG encoder layer: the first launch's indices + flags, on a per-column grid, are the second's
    residual; away from NaN rows the dequantized residual is the y launch 1 would have written, -0.0 inputs included"""
    rows, d = 37, 768
    (q1, q2, q3, qr), (f1, f2, f3, _) = _peg_layouts(d)
    a1, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=8)
    a2 = _inputs(be, rows, d, qr, seed=9)[0]
    a1[5, 100] = NAN
    a1[7, :8] = torch.tensor([-0.0, 0.0, -1e-9, 1e-9, -0.0, 0.0, -1e-9, 1e-9], device=DEV)
    r_idx[7, :8] = int(torch.clamp(torch.round(qr[1]), 0, 255).item()) - 128      # a residual of exactly zero there
    r = _dequant(qr, r_idx)
    y1_old, i1_old = be.residual_layernorm_quant_axis(a1, r, q1, q2, w, b, LN_EPS, q3, want_idx=True)
    y2_old, i2_old = be.residual_layernorm_quant_axis(a2, y1_old, f1, f2, w, b, LN_EPS, f3, want_idx=True)
    _, i1, n1 = be.residual_layernorm_quant_axis_ires(a1, None, r_idx, qr, None, q1, q2, w, b, LN_EPS, q3, want_y=False)
    y2, i2, n2 = be.residual_layernorm_quant_axis_ires(a2, None, i1, q3, n1, f1, f2, w, b, LN_EPS, f3)
    assert n1.nonzero().flatten().tolist() == [5] and n2.nonzero().flatten().tolist() == [5]
    keep = ~n1.bool()
    assert torch.equal(_bits(_dequant(q3, i1)[keep]), _bits(y1_old[keep]))
    assert torch.isnan(y2_old[5]).all()
    assert torch.equal(_bits(y2), _bits(y2_old))
    assert torch.equal(i1[keep], i1_old[keep]) and torch.equal(i2[keep], i2_old[keep])


def test_index_only_output_feeds_the_class_ordered_linear(be):
    """the index-only output, in natural column order on a 6-group grid, is what tq_linear_i8_cls_fwd reads: the Linear on it
    equals the Linear on the axis tail's y_idx"""
    from quantization import _hip
    rows, d, N = 64, 768, 128
    q1, q2, q3, qr = _peg_layouts(d)[0]
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=10)
    _, idx_old = be.residual_layernorm_quant_axis(a, r, q1, q2, w, b, LN_EPS, q3, want_idx=True)
    _, idx, flags = be.residual_layernorm_quant_axis_ires(a, None, r_idx, qr, None, q1, q2, w, b, LN_EPS, q3, want_y=False)
    assert not bool(flags.any())
    g = torch.Generator(device=DEV).manual_seed(11)
    w_idx = torch.randint(-127, 128, (N, d), device=DEV, generator=g).to(torch.int8)
    ends = [128 * (c + 1) for c in range(6)]
    reps = [128 * c for c in range(6)]
    rs = torch.stack([be.rowsum_i8(w_idx[:, e - 128:e].contiguous()) for e in ends]).contiguous()
    table = be.cls_table(ends, reps)
    wd = torch.full((1,), 0.004, device=DEV)
    xq = (q3[0], q3[1], 8, EPS)
    ys = [be.linear_i8_cls(i, w_idx, rs, None, xq, table, wd, EPS, _hip.ACT_NONE, None, torch.float32) for i in (idx, idx_old)]
    assert torch.equal(_bits(ys[0]), _bits(ys[1])) and bool(ys[0].abs().max() > 0)


# ------------------------------------------------------------------------------------------------------------------
# the C entry point: bounds and argument errors

def _entry(be):
    st = torch.cuda.current_stream().cuda_stream
    ref = lambda q: None if q is None else (q if not isinstance(q, tuple) else C.byref(be._qdesc(*q, q[0].numel(), 1)))
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())

    def call(a, r, ri, q_res, rn, y, yi, yn, rows, d, q1, q2, w, b, q3):
        return be.lib.tq_residual_layernorm_quant_axis_ires_fwd(p(a), p(r), p(ri), ref(q_res), p(rn), p(y), p(yi), p(yn), rows, d,
                                                                ref(q1), ref(q2), p(w), p(b), LN_EPS, ref(q3), st)
    return call


@pytest.mark.parametrize('rows,d', [(37, 768), (5, 64)])
def test_nothing_is_written_past_the_rows(be, rows, d):
    """inputs sized exactly, outputs in sentinel-padded buffers (also with the flags not requested)"""
    call = _entry(be)
    q1, q2, q3, qr = _peg_layouts(d)[1]
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=12)
    a, r_idx = a.clone(), r_idx.clone()                      # exactly rows * d elements each
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[rows - 1] = 1
    n, pad = rows * d, 4096
    y_old, i_old = be.residual_layernorm_quant_axis(a, _dequant(qr, r_idx, flags_in), q1, q2, w, b, LN_EPS, q3, want_idx=True)
    for with_y, with_flags in ((True, True), (False, True), (True, False), (False, False)):
        y = torch.full((n + pad,), -7.25, device=DEV)
        yi = torch.full((n + pad,), 77, dtype=torch.int8, device=DEV)
        yn = torch.full((rows + pad,), 9, dtype=torch.uint8, device=DEV)
        rc = call(a, None, r_idx, qr, flags_in, y if with_y else None, yi, yn if with_flags else None, rows, d, q1, q2, w, b, q3)
        assert rc == 0, be.lib.tq_last_error()
        torch.cuda.synchronize()
        assert bool((yi[n:] == 77).all()) and torch.equal(yi[:n].view(rows, d)[:-1], i_old[:-1])
        if with_y:
            assert bool((y[n:] == -7.25).all()) and torch.equal(_bits(y[:n]), _bits(y_old).flatten())
        else:
            assert bool((y == -7.25).all())                 # passed nowhere: intact
        if with_flags:
            assert bool((yn[rows:] == 9).all()) and yn[:rows].tolist() == [0] * (rows - 1) + [1]
        else:
            assert bool((yn == 9).all())


def test_argument_errors(be):
    """every refusal comes back before any device access (the buffers of the bad calls are never touched: sentinels below)"""
    call = _entry(be)
    err = lambda: be.lib.tq_last_error().decode()
    rows, d = 8, 768
    q1, q2, q3, qr = _peg_layouts(d)[1]
    t1, t2, t3, tr = (_grid('tensor', d, s, seed=9) for s in ('dense', 'sum', 'out', 'res'))
    a, r, r_idx, w, b = _inputs(be, rows, d, qr, seed=13)
    rn = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    y, yi, yn = torch.empty_like(a), torch.empty_like(r_idx), torch.empty_like(rn)
    ok = dict(a=a, r=None, ri=r_idx, q_res=qr, rn=rn, y=y, yi=yi, yn=yn, rows=rows, d=d, q1=q1, q2=q2, w=w, b=b, q3=q3)
    go = lambda **kw: call(**dict(ok, **kw))
    assert go() == 0 and go(rows=0) == 0
    assert go(ri=None, q_res=None, rn=None, r=r) == 0                          # the fp32 mode
    assert go(q_res=tr) == 0                                                   # a per-tensor residual grid
    assert go(y=None) == 0 and go(yi=None) == 0 and go(yn=None) == 0 and go(rn=None) == 0
    torch.cuda.synchronize()
    y.fill_(-7.25), yi.fill_(77), yn.fill_(9)
    torch.cuda.synchronize()
    assert go(r=r) == -1 and 'one of the two' in err()                          # both residual forms
    assert go(ri=None, rn=None) == -1 and 'one of the two' in err()             # neither
    assert go(ri=None, r=r) == -1 and 'res_row_nan' in err()                    # flags with an fp32 residual
    assert go(y=None, yi=None) == -1 and 'y_idx' in err()                       # y == NULL without y_idx
    sym = (torch.tensor(0.03, device=DEV), None, torch.ones(1, dtype=torch.uint8, device=DEV), 8, True, False, EPS)
    assert go(q3=sym) == -1 and 'asymmetric' in err()                           # y_idx behind a symmetric q_out
    assert go(q3=None) == -1 and 'y_idx' in err()
    assert go(q_res=None) == -1 and 'q_res' in err()
    for bad in (sym, tr[:3] + (9,) + tr[4:], tr[:5] + (True, EPS), qr[:3] + (9,) + qr[4:]):
        assert go(q_res=bad) == -1 and 'q_res' in err()                         # symmetric, 9-bit, log-domain q_res
    half = be._qdesc(qr[0][:d // 2].contiguous(), qr[1][:d // 2].contiguous(), None, 8, False, False, EPS, d // 2, 1)
    assert go(q_res=C.byref(half)) == -1 and 'q_res' in err()                   # n_params neither 1 nor d
    inner = be._qdesc(qr[0], qr[1], None, 8, False, False, EPS, d, 2)
    assert go(q_res=C.byref(inner)) == -1 and 'q_res' in err()
    assert go(q1=C.byref(half)) == -1 and 'per-column' in err()
    per_tensor = dict(q1=t1, q2=t2, q3=t3, q_res=tr)
    assert go(d=1024, rows=6, **per_tensor) == -4 and 'row length' in err() and '768' in err()      # TQ_EUNSUPPORTED
    assert go(d=100, **per_tensor) == -4 and 'row length' in err()
    assert go(a=a.data_ptr() + 4) == -1 and '16-byte' in err()
    assert go(y=y.data_ptr() + 8) == -1 and '16-byte' in err()
    assert go(ri=None, q_res=None, rn=None, r=r.data_ptr() + 4) == -1 and '16-byte' in err()
    assert go(ri=r_idx.data_ptr() + 2) == -1 and '4-byte' in err()
    assert go(yi=yi.data_ptr() + 1) == -1 and '4-byte' in err()
    assert go(a=None) == -1 and 'NULL' in err()
    torch.cuda.synchronize()
    assert bool((y == -7.25).all()) and bool((yi == 77).all()) and bool((yn == 9).all())
    assert go(rn=rn.data_ptr() + 1, rows=rows - 1) == 0 and go(yn=yn.data_ptr() + 3, rows=rows - 3) == 0   # flags: any alignment
    torch.cuda.synchronize()
    with pytest.raises(Exception):
        be.residual_layernorm_quant_axis_ires(a, r, r_idx, qr, None, q1, q2, w, b, LN_EPS, q3)
    with pytest.raises(Exception):
        be.residual_layernorm_quant_axis_ires(a, None, None, None, None, q1, q2, w, b, LN_EPS, q3)
    with pytest.raises(Exception):
        be.residual_layernorm_quant_axis_ires(a.bfloat16(), r, None, None, None, q1, q2, w, b, LN_EPS, q3)
    wide = torch.zeros(8, 1024, device=DEV)
    with pytest.raises(Exception, match='768'):
        be.residual_layernorm_quant_axis_ires(wide, wide, None, None, None, t1, t2, w, b, LN_EPS, t3)
