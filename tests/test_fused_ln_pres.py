"""tq_residual_layernorm_quant_pres_fwd (the fp32 LayerNorm tail whose residual or output travels as the two int8 byte planes of
a <= 16-bit grid index) against the launches it stands in for on the same GPU, and against the CPU chain
(tests/_plane_residuals_twin.pres_tail_reference: ln_tail_chain with kernel-order statistics) where its siblings' tests do.

  F1 (residual fp32 or int8 indices [+ flags]; planes + flags out, no y)
        planes == `HipBackend.residual_layernorm_quant_planes(dense_out, R)` on every row that is not NaN, flags == the rows
        that launch turns NaN as a whole; R the fp32 residual with its flagged rows NaN
  F2 (residual as planes [+ flags]; y [, y_idx], flags out)
        y (int32 bit patterns), y_idx (rows that are not NaN) and flags == `HipBackend.residual_layernorm_quant_ires(dense_out,
        residual=R)`, R = scale * ((256 (hi + 128) + (lo + 128)) - zero_point) evaluated by torch on the GPU (one exact
        subtraction, one rounded multiplication), flagged rows NaN

Every comparison is exact.  The set of NaN rows is asserted to be the planted one BEFORE planes / indices are compared on the
other rows.  Launch forms (the launcher restates `launch_res_ln_ires`; `launch_form` below restates it once more, and the
at-size cases assert their premise with it first): rows per block rpb = 256 / LPR, a second trip of the row loop beyond
rpb * 2048 rows, streaming loads / stores from rows * d * 4 >= 64 MiB.  The at-size cases compare GPU with GPU only.

Measured once on an MI355X (pytest --durations): the 70 cases together take 4.0 s, the slowest 1.1 s (the first one: it
loads the library and the oracle); the at-size cases less than 0.01 s each.
"""
import collections
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-8
LN_EPS = 1e-12
WIDTHS = (64, 128, 256, 384, 512, 768, 1024, 1536, 2048, 3072)
NAN = float('nan')
INF = float('inf')

_LANES = {16: (16, 1), 32: (32, 1), 64: (64, 1), 96: (32, 3), 128: (64, 2), 192: (64, 3), 256: (64, 4), 384: (64, 6),
          512: (64, 8), 768: (64, 12)}
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


def _asym(scale, zp, bits=8, eps=EPS):
    return (torch.tensor(float(scale), device=DEV), torch.tensor(float(zp), device=DEV), None, bits, False, False, eps)


def _sym(scale, bits=8):
    return (torch.tensor(float(scale), device=DEV), None, torch.ones(1, dtype=torch.uint8, device=DEV), bits, True, False, EPS)


Q1 = Q2 = Q3 = QR = None            # Q_dense, Q_sum, F2's 8-bit Q_out, the 8-bit grid of F1's index residual
Q_OUT = {}                          # n_bits -> F1's Q_out (LayerNorm outputs lie in about [-5, 5])
Q_RES = {}                          # n_bits -> the grid of F2's residual planes (residuals lie in about [-6, 6])


@pytest.fixture(autouse=True, scope='module')
def _grids():
    global Q1, Q2, Q3, QR
    Q1, Q2, Q3, QR = _asym(0.05, 120), _asym(0.07, 131), _asym(0.03, 128), _asym(0.04, 127)
    Q_OUT.update({16: _asym(2.0e-4, 30000, 16), 12: _asym(3.0e-3, 2048, 12), 9: _asym(0.02, 256, 9)})
    Q_RES.update({16: _asym(2.0e-4, 30000, 16), 12: _asym(3.0e-3, 2048, 12), 9: _asym(0.02, 256, 9), 8: _asym(0.04, 127, 8),
                  1: _asym(1.0, 0, 1)})


def _inputs(rows, d, seed=0):
    """dense output, raw residual values, LayerNorm weight and bias"""
    g = torch.Generator(device=DEV).manual_seed(seed + 7919 * d + rows)
    a = torch.randn(rows, d, device=DEV, generator=g) * 2.0
    r0 = torch.randn(rows, d, device=DEV, generator=g) * 1.5
    w = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=g)
    b = 0.1 * torch.randn(d, device=DEV, generator=g)
    return a, r0, w, b


def _bits(t):
    return t.contiguous().view(torch.int32)


def _index(hi, lo):
    return 256 * (hi.int() + 128) + (lo.int() + 128)


def _emits(q):
    return q is not None and not q[4] and q[3] <= 8


def _flags(rows, which):
    f = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    if which:
        f[list(which)] = 1
    return f


def _rows_of(mask):
    return mask.nonzero().flatten().tolist()


def _cpu_q(q):
    return None if q is None else tuple(None if t is None else (t.cpu() if torch.is_tensor(t) else t) for t in q)


def _grid_params(q):
    """(scale, zero_point) of an asymmetric linear-domain grid as every kernel derives them, as fp32 device scalars"""
    scale = torch.maximum(q[0].float().reshape(()), torch.tensor(q[6], dtype=torch.float32, device=DEV))
    zp = torch.clamp(torch.round(q[1].float().reshape(())), 0, 2 ** q[3] - 1)
    return scale, zp


def _dequant_planes(planes, q_res, flags_in=None):
    """the header's R: scale * ((256 (hi + 128) + (lo + 128)) - zero_point), flagged rows NaN -- two torch launches, every
    fp32 operation rounded on its own"""
    scale, zp = _grid_params(q_res)
    R = scale * (_index(*planes).float() - zp)
    if flags_in is not None:
        R[flags_in.bool()] = NAN
    return R


def _f1(be, a, r0, flags_in, q1, q2, q3, w, b, planted, cpu=False, q_res=None, kinds=('f32', 'idx')):
    """the planes-out form in both residual kinds against the plane tail on R; r0 is put on the 8-bit grid q_res first (the
    residual of the 'idx' kind must be one).  planted: the rows that must come out NaN.  -> (index int32, NaN rows)"""
    q_res = q_res or QR
    r, r_idx = be.fake_quant_int8(r0, q_res[0], q_res[1], q_res[3], q_res[6])
    R = r.clone()
    if flags_in is not None:
        R[flags_in.bool()] = NAN
    y_ref, (hi_ref, lo_ref) = be.residual_layernorm_quant_planes(a, R, q1, q2, w, b, LN_EPS, q3)
    nan_ref = torch.isnan(y_ref).any(-1)
    assert _rows_of(nan_ref) == sorted(planted), (_rows_of(nan_ref), planted)
    keep = ~nan_ref
    for kind in kinds:
        res = (R, None, None, None, None) if kind == 'f32' else (None, r_idx, None, q_res, flags_in)
        y, idx, planes, flags = be.residual_layernorm_quant_pres(a, *res, q1, q2, w, b, LN_EPS, q3, want_y=False, want_planes=True)
        assert y is None and idx is None and flags.dtype == torch.uint8 and flags.shape == a.shape[:-1], kind
        hi, lo = planes
        assert hi.dtype == lo.dtype == torch.int8 and hi.shape == lo.shape == a.shape
        assert _rows_of(flags) == sorted(planted) and set(flags.unique().tolist()) <= {0, 1}, (kind, _rows_of(flags))
        assert torch.equal(hi[keep], hi_ref[keep]), f'{kind}: hi plane differs from the plane tail'
        assert torch.equal(lo[keep], lo_ref[keep]), f'{kind}: lo plane differs from the plane tail'
    if cpu:
        from tests._exact_backend import _p
        from tests._plane_residuals_twin import pres_tail_reference
        ry, _, (rhi, rlo), rnan = pres_tail_reference(a.cpu(), R.cpu(), _p(_cpu_q(q1)), _p(_cpu_q(q2)), w.cpu(), b.cpu(), LN_EPS,
                                                      _p(_cpu_q(q3)))
        kc = keep.cpu()
        assert _rows_of(rnan) == sorted(planted)
        assert torch.equal(hi.cpu()[kc], rhi[kc]) and torch.equal(lo.cpu()[kc], rlo[kc]), 'planes differ from the CPU chain'
    return _index(hi, lo), nan_ref


def _f2(be, a, planes, q_res, flags_in, q1, q2, q3, w, b, planted, cpu=False):
    """the planes-in form, with and without y_idx, against the index-residual entry on the fp32 R.  -> (y, NaN rows)"""
    R = _dequant_planes(planes, q_res, flags_in)
    has_idx = _emits(q3)
    y_ref, idx_ref, flags_ref = be.residual_layernorm_quant_ires(a, R, None, None, None, q1, q2, w, b, LN_EPS, q3, want_y=True,
                                                                 want_idx=has_idx)
    nan_ref = torch.isnan(y_ref).any(-1)
    assert _rows_of(nan_ref) == sorted(planted) == _rows_of(flags_ref), (_rows_of(nan_ref), planted)
    keep = ~nan_ref
    for want_idx in ((False, True) if has_idx else (False,)):
        y, idx, out_planes, flags = be.residual_layernorm_quant_pres(a, None, None, planes, q_res, flags_in, q1, q2, w, b, LN_EPS,
                                                                     q3, want_y=True, want_idx=want_idx)
        what = f'want_idx={want_idx}'
        assert out_planes is None and (idx is None) == (not want_idx) and y.dtype == torch.float32 and y.shape == a.shape
        assert torch.equal(flags, flags_ref) and flags.shape == a.shape[:-1], what
        assert torch.equal(_bits(y), _bits(y_ref)), f'{what}: y differs from the index-residual entry on R'
        if want_idx:
            assert idx.dtype == torch.int8 and torch.equal(idx[keep], idx_ref[keep]), what
    if cpu:
        from tests._exact_backend import _p
        from tests._plane_residuals_twin import dequantized_residual, pres_tail_reference
        Rc = dequantized_residual(_cpu_q(q_res), res_planes=tuple(p.cpu() for p in planes),
                                  res_row_nan=None if flags_in is None else flags_in.cpu())
        assert torch.equal(_bits(Rc[keep.cpu()]), _bits(R.cpu()[keep.cpu()])), 'the two restatements of R differ'
        ry, ridx, _, rnan = pres_tail_reference(a.cpu(), Rc, _p(_cpu_q(q1)), _p(_cpu_q(q2)), w.cpu(), b.cpu(), LN_EPS, _p(_cpu_q(q3)))
        kc = keep.cpu()
        assert _rows_of(rnan) == sorted(planted)
        assert torch.equal(_bits(y.cpu()[kc]), _bits(ry[kc])), 'y differs from the CPU chain'
        if has_idx:
            assert torch.equal(idx.cpu()[kc].int() + 128, ridx[kc].int()), 'y_idx differs from the CPU chain'
    return y_ref, nan_ref


def _planes(be, r0, q_res):
    return be.quantize_hilo(r0.contiguous(), (q_res[0], q_res[1], q_res[3], q_res[6]))


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', WIDTHS)
def test_every_width_37_rows(be, d):
    """37 rows: a partly filled last block for every rows-per-block value (4, 8, 16); both residual kinds of F1, F2 with and
    without y_idx; a flagged residual row and a NaN of dense_out's own"""
    rows = 37
    assert rows % launch_form(rows, d).rpb != 0
    a, r0, w, b = _inputs(rows, d)
    a[11, d // 2] = NAN
    flags_in = _flags(rows, [3])
    idx, _ = _f1(be, a, r0, flags_in, Q1, Q2, Q_OUT[16], w, b, planted=[3, 11], cpu=True)
    keep = [i for i in range(rows) if i not in (3, 11)]
    assert int(idx[keep].max()) >= 32768 and int(idx[keep].min()) < 32768            # both signs of the hi plane
    planes = _planes(be, r0, Q_RES[16])
    assert int(_index(*planes).max()) >= 32768 and int(_index(*planes).min()) < 32768
    _f2(be, a, planes, Q_RES[16], flags_in, Q1, Q2, Q3, w, b, planted=[3, 11], cpu=True)


def test_second_trip_of_the_row_loop_d768(be):
    rows, d = 8193, 768
    f = launch_form(rows, d)
    assert f.iters == 2 and not f.nt and launch_form(8192, d).iters == 1 and rows % (f.rpb * f.iters) != 0
    a, r0, w, b = _inputs(rows, d)
    a[8192, 1] = NAN
    flags_in = _flags(rows, [4])                    # a second-trip row of the first block
    _f1(be, a, r0, flags_in, Q1, Q2, Q_OUT[16], w, b, planted=[4, 8192])
    _f2(be, a, _planes(be, r0, Q_RES[16]), Q_RES[16], flags_in, Q1, Q2, Q3, w, b, planted=[4, 8192])


def test_streaming_form_d768(be):
    rows, d = 21846, 768
    f = launch_form(rows, d)
    assert f.nt and f.iters == 2 and not launch_form(rows - 1, d).nt and rows * d * 4 >= 64 << 20
    a, r0, w, b = _inputs(rows, d)
    a[rows - 1, 0] = NAN
    _f1(be, a, r0, None, Q1, Q2, Q_OUT[16], w, b, planted=[rows - 1])
    _f2(be, a, _planes(be, r0, Q_RES[16]), Q_RES[16], None, Q1, Q2, Q3, w, b, planted=[rows - 1])


USES = [(1, 1), (1, 0), (0, 1), (0, 0)]


@pytest.mark.parametrize('bits', [16, 12, 9])
@pytest.mark.parametrize('use', USES)
def test_f1_quantizer_mixes_and_output_grids(be, use, bits):
    """the four mixes of present and absent Q_dense / Q_sum behind output grids of 16, 12 and 9 bits"""
    rows, d = 37, 768
    a, r0, w, b = _inputs(rows, d, seed=1)
    q1, q2 = (q if u else None for q, u in zip((Q1, Q2), use))
    a[2, 5] = NAN
    idx, nan = _f1(be, a, r0, _flags(rows, [20]), q1, q2, Q_OUT[bits], w, b, planted=[2, 20], cpu=True)
    assert 0 <= int(idx[~nan].min()) and int(idx[~nan].max()) <= (1 << bits) - 1


@pytest.mark.parametrize('bits', [16, 12, 9, 8, 1])
@pytest.mark.parametrize('use', USES)
def test_f2_quantizer_mixes_and_residual_grids(be, use, bits):
    """the four mixes behind residual grids of 16, 12, 9, 8 bits and one bit"""
    rows, d = 37, 768
    a, r0, w, b = _inputs(rows, d, seed=2)
    q1, q2 = (q if u else None for q, u in zip((Q1, Q2), use))
    a[2, 5] = NAN
    planes = _planes(be, r0, Q_RES[bits])
    assert int(_index(*planes).max()) <= (1 << bits) - 1
    if bits <= 8:
        assert bool((planes[0] == -128).all())
    _f2(be, a, planes, Q_RES[bits], _flags(rows, [20]), q1, q2, Q3, w, b, planted=[2, 20], cpu=True)


@pytest.mark.parametrize('bits,zp', [(16, 0), (16, 65535), (16, 30000), (12, 4095), (9, 0)])
def test_zero_points_of_the_output_grid_f1(be, bits, zp):
    rows, d = 37, 384
    a, r0, w, b = _inputs(rows, d, seed=3)
    idx, _ = _f1(be, a, r0, None, Q1, Q2, _asym({16: 2.0e-4, 12: 3.0e-3, 9: 0.02}[bits], zp, bits), w, b, planted=[])
    if zp in (0, (1 << bits) - 1):
        assert int(idx.min() if zp == 0 else idx.max()) == zp


@pytest.mark.parametrize('bits,zp', [(16, 0), (16, 65535), (16, 30000), (12, 0), (12, 4095), (8, 255), (8, 100), (1, 1)])
def test_zero_points_of_the_residual_grid_f2(be, bits, zp):
    """the zero point at 0, at the top of the grid and mid-grid; both ends of the grid occur in the planes"""
    rows, d = 37, 384
    a, r0, w, b = _inputs(rows, d, seed=4)
    q_res = _asym({16: 1.0e-4, 12: 1.0e-3, 8: 0.01, 1: 0.5}[bits], zp, bits)
    planes = _planes(be, r0 + float(q_res[0]) * ((1 << bits) / 2 - zp), q_res)     # centred on the grid: both ends clamp
    index = _index(*planes)
    assert int(index.min()) == 0 and int(index.max()) == (1 << bits) - 1
    _f2(be, a, planes, q_res, None, Q1, Q2, Q3, w, b, planted=[], cpu=bits == 16)


@pytest.mark.parametrize('which', [0, 1, 2])
def test_division_path(be, which):
    """a scale outside [2^-100, 2^100] sends the whole launch down the division path (chosen as tests/test_fused_ln_ires.py
    chooses it); which = 2: the output quantizer itself"""
    rows, d = 37, 768
    a, r0, w, b = _inputs(rows, d, seed=5)
    a[2, 5] = NAN
    a[6, 0], a[6, 767] = INF, -INF
    flags_in = _flags(rows, [0, 36])
    wild = lambda bits, zp: _asym(2.0 ** -101 if which != 1 else 2.0 ** 101, zp, bits, eps=0.0)     # (eps is a floor under the scale)
    qs = [Q1, Q2, Q_OUT[16]]
    qs[which] = wild(16, 30000) if which == 2 else wild(8, 128)
    idx, nan = _f1(be, a, r0, flags_in, *qs, w, b, planted=[0, 2, 36])
    if which == 2:
        assert sorted(idx[~nan].unique().tolist()) == [0, 65535]          # every value is far outside such a grid: both ends
    qs = [Q1, Q2, Q3]
    qs[which] = wild(8, 128)
    _f2(be, a, _planes(be, r0, Q_RES[16]), Q_RES[16], flags_in, *qs, w, b, planted=[0, 2, 36])


def test_range_ends(be):
    """outputs that clamp to index 0 and to 2^n - 1 (F1); residual planes at both ends of their grid behind an output that clamps
    to both ends of its own (F2)"""
    rows, d = 37, 768
    a, r0, w, b = _inputs(rows, d, seed=6)
    for bits, q3 in ((16, _asym(1.0e-5, 32768, 16)), (12, _asym(1.0e-4, 2048, 12)), (9, _asym(1.0e-3, 256, 9))):
        idx, _ = _f1(be, a, r0, None, Q1, Q2, q3, w, b, planted=[], cpu=bits == 16)
        assert int(idx.min()) == 0 and int(idx.max()) == (1 << bits) - 1
    q_res = _asym(1.0e-5, 32768, 16)
    planes = _planes(be, r0, q_res)
    assert int(_index(*planes).min()) == 0 and int(_index(*planes).max()) == 65535
    q3 = _asym(1.0e-3, 128, 8)
    y, _ = _f2(be, a, planes, q_res, None, Q1, Q2, q3, w, b, planted=[], cpu=True)
    assert float(y.min()) == -128 * float(q3[0]) and float(y.max()) == pytest.approx(127 * float(q3[0]), rel=1e-6)


def test_special_values(be):
    """NaN in dense_out; flagged residual rows (the first, the last, two adjacent ones of one block, one that also has a NaN of
    its own); +-inf where Q_dense clamps it and where nothing does"""
    rows, d = 37, 768
    assert launch_form(rows, d).rpb == 4
    a, r0, w, b = _inputs(rows, d, seed=7)
    a[1, 0], a[1, 300], a[1, 767] = INF, -INF, INF
    a[13, 766] = NAN
    a[9, 3] = NAN
    flags_in = _flags(rows, [0, 8, 9, 36])               # rows 8 and 9 share the block of rows 8..11
    planes = _planes(be, r0, Q_RES[16])
    _f1(be, a, r0, flags_in, Q1, Q2, Q_OUT[16], w, b, planted=[0, 8, 9, 13, 36], cpu=True)
    y, nan = _f2(be, a, planes, Q_RES[16], flags_in, Q1, Q2, Q3, w, b, planted=[0, 8, 9, 13, 36], cpu=True)
    assert torch.isnan(y[nan]).all() and bool((_bits(y[nan]) == 0x7fc00000).all()) and not torch.isnan(y[~nan]).any()
    # without flags those rows are plain grid values
    _f1(be, a, r0, None, Q1, Q2, Q_OUT[16], w, b, planted=[9, 13])
    _f2(be, a, planes, Q_RES[16], None, Q1, Q2, Q3, w, b, planted=[9, 13])
    # without Q_dense the inf of row 1 reaches the statistics and the row's centred values are NaN.  What comes out is the
    # reference launch's business: the exact path's output quantizer maps a NaN element to a grid value and only rows with an
    # unordered INPUT are NaN as a whole (no Q_out at all: the row is NaN, and flagged)
    _f1(be, a, r0, flags_in, None, None, Q_OUT[16], w, b, planted=[0, 8, 9, 13, 36])
    _f1(be, a, r0, flags_in, None, Q2, Q_OUT[12], w, b, planted=[0, 8, 9, 13, 36])
    _f2(be, a, planes, Q_RES[16], flags_in, None, None, Q3, w, b, planted=[0, 8, 9, 13, 36])
    _f2(be, a, planes, Q_RES[16], flags_in, None, None, None, w, b, planted=[0, 1, 8, 9, 13, 36])


@pytest.mark.parametrize('bits', [16, 12, 9])
def test_the_planes_dequantize_to_the_y_the_plane_tail_wrote(be, bits):
    """the premise of carrying x as planes: on every row that is not NaN, R from the plane tail's planes IS the y it wrote
    beside them -- on the exact path and on the division path"""
    rows, d = 37, 768
    a, r0, w, b = _inputs(rows, d, seed=8)
    a[5, 100] = NAN
    for q3 in (Q_OUT[bits], _asym(float(Q_OUT[bits][0]), 0, bits), _asym(2.0 ** -101, 300, bits, eps=0.0)):
        y, planes = be.residual_layernorm_quant_planes(a, r0, Q1, Q2, w, b, LN_EPS, q3)
        keep = ~torch.isnan(y).any(-1)
        assert _rows_of(~keep) == [5]
        assert torch.equal(_bits(_dequant_planes(planes, q3)[keep]), _bits(y[keep]))


def test_chain_f1_linear_f2_equals_todays_chain(be):
    """a layer's second half: F1 -> linear_i16x8 -> F2 equals plane tail -> linear_i16x8 -> existing tail; a planted NaN row
    comes out NaN as a whole with its flag set"""
    rows, d = 64, 768
    a1, r0, w, b = _inputs(rows, d, seed=9)
    w2, b2 = _inputs(rows, d, seed=10)[2:]
    a1[5, 100] = NAN
    q_x = Q_OUT[16]
    x_q = (q_x[0], q_x[1], q_x[3], q_x[6])
    h, h_idx = be.fake_quant_int8(r0, QR[0], QR[1], QR[3], QR[6])
    g = torch.Generator(device=DEV).manual_seed(11)
    w_idx = torch.randint(-127, 128, (d, d), device=DEV, generator=g, dtype=torch.int32).to(torch.int8)
    rowsum = be.rowsum_i8(w_idx)
    bias = torch.randn(d, device=DEV, generator=g) * 0.1
    w_delta = torch.full((1,), 0.0005, device=DEV)
    linear = lambda hi, lo: be.linear_i16x8(hi, lo, w_idx, rowsum, bias, x_q, w_delta, EPS, 0, None, torch.float32)
    # today's
    x, x_planes = be.residual_layernorm_quant_planes(a1, h, Q1, Q2, w, b, LN_EPS, q_x)
    y_old, i_old = be.residual_layernorm_quant(linear(*x_planes), x, Q1, Q2, w2, b2, LN_EPS, Q3, want_idx=True)
    # x as planes and flags alone
    _, _, planes, x_nan = be.residual_layernorm_quant_pres(a1, None, h_idx, None, QR, None, Q1, Q2, w, b, LN_EPS, q_x,
                                                           want_y=False, want_planes=True)
    y, i, _, y_nan = be.residual_layernorm_quant_pres(linear(*planes), None, None, planes, q_x, x_nan, Q1, Q2, w2, b2, LN_EPS, Q3,
                                                      want_y=True, want_idx=True)
    assert _rows_of(x_nan) == [5] and _rows_of(y_nan) == [5] and _rows_of(torch.isnan(y_old).any(-1)) == [5]
    assert torch.isnan(y[5]).all() and torch.isfinite(y[y_nan == 0]).all()
    assert torch.equal(_bits(y), _bits(y_old))
    keep = y_nan == 0
    assert torch.equal(i[keep], i_old[keep])


# ------------------------------------------------------------------------------------------------------------------
# the C entry point: bounds and argument errors

def _entry(be):
    st = torch.cuda.current_stream().cuda_stream
    ref = lambda q: None if q is None else (q if isinstance(q, C.Structure) else be._qdesc(*q, 1, 1))
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())

    def call(a=None, r=None, ri=None, rh=None, rl=None, qr=None, rn=None, y=None, yi=None, yh=None, yl=None, yn=None, rows=0, d=0,
             q1=None, q2=None, w=None, b=None, q3=None):
        q = [None if x is None else C.byref(x) for x in (ref(qr), ref(q1), ref(q2), ref(q3))]
        return be.lib.tq_residual_layernorm_quant_pres_fwd(p(a), p(r), p(ri), p(rh), p(rl), q[0], p(rn), p(y), p(yi), p(yh), p(yl),
                                                           p(yn), rows, d, q[1], q[2], p(w), p(b), LN_EPS, q[3], st)
    return call


@pytest.mark.parametrize('rows,d', [(37, 768), (5, 64), (19, 3072)])
def test_nothing_is_written_past_the_rows(be, rows, d):
    """inputs sized exactly, outputs in sentinel-padded buffers: planes, flags, y and y_idx end at `rows`"""
    call = _entry(be)
    a, r0, w, b = _inputs(rows, d, seed=12)
    a = a.clone()
    r, r_idx = be.fake_quant_int8(r0, QR[0], QR[1], QR[3], QR[6])
    r, r_idx = r.clone(), r_idx.clone()                        # exactly rows * d elements each
    flags_in = _flags(rows, [rows - 1]).clone()
    n, pad = rows * d, 4096
    i8 = lambda v, m: torch.full((m,), v, dtype=torch.int8, device=DEV)
    u8 = lambda v, m: torch.full((m,), v, dtype=torch.uint8, device=DEV)
    q3 = Q_OUT[16]
    R = r.clone()
    R[rows - 1] = NAN
    _, (hi_ref, lo_ref) = be.residual_layernorm_quant_planes(a, R, Q1, Q2, w, b, LN_EPS, q3)
    for kind in ('f32', 'idx'):
        hi, lo, fl = i8(77, n + pad), i8(55, n + pad), u8(9, rows + pad)
        res = dict(r=R) if kind == 'f32' else dict(ri=r_idx, qr=QR, rn=flags_in)
        rc = call(a=a, yh=hi, yl=lo, yn=fl, rows=rows, d=d, q1=Q1, q2=Q2, w=w, b=b, q3=q3, **res)
        assert rc == 0, be.lib.tq_last_error()
        torch.cuda.synchronize()
        m = (rows - 1) * d
        assert bool((hi[n:] == 77).all()) and torch.equal(hi[:m], hi_ref.flatten()[:m]), kind
        assert bool((lo[n:] == 55).all()) and torch.equal(lo[:m], lo_ref.flatten()[:m]), kind
        assert bool((fl[rows:] == 9).all()) and fl[:rows].tolist() == [0] * (rows - 1) + [1], kind
    planes = tuple(t.clone() for t in _planes(be, r0, Q_RES[16]))
    y_ref, i_ref, f_ref = be.residual_layernorm_quant_ires(a, _dequant_planes(planes, Q_RES[16], flags_in), None, None, None, Q1, Q2,
                                                           w, b, LN_EPS, Q3)
    y, yi, fl = torch.full((n + pad,), -7.25, device=DEV), i8(33, n + pad), u8(9, rows + pad)
    rc = call(a=a, rh=planes[0], rl=planes[1], qr=Q_RES[16], rn=flags_in, y=y, yi=yi, yn=fl, rows=rows, d=d, q1=Q1, q2=Q2, w=w, b=b,
              q3=Q3)
    assert rc == 0, be.lib.tq_last_error()
    torch.cuda.synchronize()
    m = (rows - 1) * d
    assert bool((y[n:] == -7.25).all()) and torch.equal(_bits(y[:n]), _bits(y_ref).flatten())
    assert bool((yi[n:] == 33).all()) and torch.equal(yi[:m], i_ref.flatten()[:m])
    assert bool((fl[rows:] == 9).all()) and torch.equal(fl[:rows], f_ref)


def test_argument_errors(be):
    call = _entry(be)
    err = lambda: be.lib.tq_last_error().decode()
    rows, d = 8, 768
    a, r0, w, b = _inputs(rows, d, seed=13)
    r, ri = be.fake_quant_int8(r0, QR[0], QR[1], QR[3], QR[6])
    rh, rl = _planes(be, r0, Q_RES[16])
    i8 = lambda: torch.empty(rows, d, dtype=torch.int8, device=DEV)
    y, yi, yh, yl = torch.empty_like(a), i8(), i8(), i8()
    rn, yn = _flags(rows, []), torch.empty(rows, dtype=torch.uint8, device=DEV)
    base = dict(a=a, rows=rows, d=d, q1=Q1, q2=Q2, w=w, b=b)
    f1 = dict(base, ri=ri, qr=QR, rn=rn, yh=yh, yl=yl, yn=yn, q3=Q_OUT[16])
    f1f = dict(base, r=r, yh=yh, yl=yl, yn=yn, q3=Q_OUT[16])
    f2 = dict(base, rh=rh, rl=rl, qr=Q_RES[16], rn=rn, y=y, yi=yi, yn=yn, q3=Q3)
    go = lambda form, **kw: call(**dict(form, **kw))
    for form in (f1, f1f, f2):
        assert go(form) == 0, err()
        assert go(form, yn=None) == 0 and go(form, q1=None, q2=None) == 0       # flags out, Q_dense, Q_sum: optional
        assert go(form, rows=0) == 0
        assert call(rows=0, d=d) == 0                                           # no rows: nothing is looked at
        for name in ('a', 'w', 'b'):
            assert go(form, **{name: None}) == -1 and 'NULL' in err(), name
        assert go(form, a=a.data_ptr() + 4) == -1 and '16-byte' in err()
        assert go(form, d=100) == -4 and 'row length' in err()                  # TQ_EUNSUPPORTED
        assert go(form, d=772) == -4 and 'row length' in err()
    assert go(f1, rn=None) == 0 and go(f2, rn=None) == 0 and go(f2, yi=None) == 0
    # the residual: exactly one of the three kinds, planes as a pair, flags not with fp32, a grid that fits
    assert go(f1, r=r) == -1 and 'exactly one' in err()
    assert go(f2, r=r) == -1 and 'exactly one' in err()
    assert go(f2, ri=ri) == -1 and 'exactly one' in err()
    assert go(f1, ri=None) == -1 and 'exactly one' in err()
    assert go(f2, rl=None) == -1 and 'pair' in err()
    assert go(f2, rh=None) == -1 and 'pair' in err()
    assert go(f1f, rn=rn) == -1 and 'res_row_nan' in err()
    assert go(f1, qr=None) == -1 and 'q_res' in err()
    assert go(f2, qr=None) == -1 and 'q_res' in err()
    assert go(f1, qr=_asym(0.01, 256, 9)) == -1 and 'n_bits <= 8' in err()
    assert go(f2, qr=_asym(0.01, 256, 17)) == -1 and 'n_bits <= 16' in err()
    assert go(f2, qr=_sym(0.01, 16)) == -1 and 'q_res' in err()
    assert go(f2, qr=Q_RES[16][:5] + (True, EPS)) == -1 and 'linear-domain' in err()
    per_col = be._qdesc(torch.full((d,), 2.0e-4, device=DEV), torch.full((d,), 30000.0, device=DEV), None, 16, False, False, EPS, d, 1)
    assert go(f2, qr=per_col) == -1 and 'per-tensor' in err()
    assert go(f1, q3=per_col) == -1 and 'per-tensor' in err()
    # the outputs: planes as a pair, something to write, grids that fit
    assert go(f1, yl=None) == -1 and 'pair' in err()
    assert go(f1, yh=None) == -1 and 'pair' in err()
    assert go(f1, yh=None, yl=None) == -1 and 'nothing to write' in err()
    assert go(f2, y=None, yi=None) == -1 and 'nothing to write' in err()
    assert go(f2, q3=Q_OUT[16]) == -1 and 'y_idx' in err()
    assert go(f2, q3=None) == -1 and 'y_idx' in err()
    assert go(f2, q3=None, yi=None) == 0                                        # y alone needs no output quantizer
    assert go(f1, q3=None) == -1 and 'y_hi' in err()
    assert go(f1, q3=_sym(0.03, 16)) == -1 and 'asymmetric' in err()
    assert go(f1, q3=_asym(2.0e-4, 30000, 17)) == -1 and '16 bits' in err()
    assert go(f1, q3=Q_OUT[16][:5] + (True, EPS)) == -1 and 'linear-domain' in err()
    # alignment: 16 bytes for fp32, 4 for indices and planes, none for the flags
    assert go(f1f, r=r.data_ptr() + 4) == -1 and '16-byte' in err()
    assert go(f2, y=y.data_ptr() + 8) == -1 and '16-byte' in err()
    for form, name, t in ((f1, 'ri', ri), (f1, 'yh', yh), (f1, 'yl', yl), (f2, 'rh', rh), (f2, 'rl', rl), (f2, 'yi', yi)):
        assert go(form, **{name: t.data_ptr() + 2}) == -1 and '4-byte' in err(), name
    assert go(f1, ri=ri.data_ptr() + 4, yh=yh.data_ptr() + 4, yl=yl.data_ptr() + 4, rn=rn.data_ptr() + 1, yn=yn.data_ptr() + 1,
              rows=rows - 1) == 0
    assert go(f2, rh=rh.data_ptr() + 4, rl=rl.data_ptr() + 4, yi=yi.data_ptr() + 4, rn=rn.data_ptr() + 1, yn=yn.data_ptr() + 1,
              rows=rows - 1) == 0
    # every combination that is neither form: TQ_EUNSUPPORTED, with the two forms named
    unsupported = [
        dict(f1f, y=y),                                  # fp32 residual: y beside the planes
        dict(f1f, y=y, yh=None, yl=None),                # ... y alone (tq_residual_layernorm_quant_ires_fwd has it)
        dict(f1, y=y),                                   # index residual: y beside the planes
        dict(f1, y=y, yh=None, yl=None),                 # ... y alone
        dict(f1, yi=yi, yh=None, yl=None, q3=Q3),        # ... indices alone
        dict(f1, yi=yi, q3=Q3),                          # ... indices beside the planes
        dict(f1f, yi=yi, q3=Q3),
        dict(f2, yh=yh, yl=yl),                          # plane residual: planes out beside y
        dict(f2, y=None, yi=None, yh=yh, yl=yl),         # ... planes out alone
        dict(f2, y=None),                                # ... indices alone
    ]
    for kw in unsupported:
        assert call(**kw) == -4 and 'supported are (1)' in err() and '(2)' in err(), sorted(k for k, v in kw.items() if v is not None)
    torch.cuda.synchronize()
    with pytest.raises(Exception):
        be.residual_layernorm_quant_pres(a, r, ri, None, QR, None, Q1, Q2, w, b, LN_EPS, Q_OUT[16], want_y=False, want_planes=True)
    with pytest.raises(Exception):
        be.residual_layernorm_quant_pres(a, None, None, None, None, None, Q1, Q2, w, b, LN_EPS, Q3)
    with pytest.raises(Exception):
        be.residual_layernorm_quant_pres(a.bfloat16(), r, None, None, None, None, Q1, Q2, w, b, LN_EPS, Q_OUT[16], want_y=False,
                                         want_planes=True)
