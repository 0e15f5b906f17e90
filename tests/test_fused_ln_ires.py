"""tq_residual_layernorm_quant_ires_fwd (the fp32 LayerNorm tail with its residual as int8 indices and one NaN flag per row)
against the existing tail kernel, `HipBackend.residual_layernorm_quant`, on the same GPU.

The contract is the existing kernel's result on the dequantized residual, so every comparison here is exact:
  * y as int32 bit patterns (NaN rows included),
  * y_idx with torch.equal on the rows whose flag is 0 (the index bytes of a NaN row are unspecified),
  * the flags against isnan(y_old).any(-1).
The residual's (index, value) pairs come from the fake-quant launch that emits indices (`fake_quant_int8`), so the fp32
values the old kernel reads are the producer's own bits.  Every case runs the new entry twice: with the residual as indices
(+ flags) and with the same residual as fp32, which must equal the old kernel everywhere and raise the same flags.

Launch forms (the new launcher restates `launch_res_ln` for fp32; `launch_form` below restates it once more, and the two
at-size cases assert their premise with it first): rows per block rpb = 256 / LPR, a second trip of the row loop beyond
rpb * 2048 rows, streaming loads / stores from rows * d * 4 >= 64 MiB.

Measured once on an MI355X (pytest --durations): the 37 cases together take 3.2 s, the slowest 0.54 s (the first one: it
loads the library); the two at-size cases 0.05 s and less.
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

# ------------------------------------------------------------------------------------------------------------------
# launch_res_ln_ires's arithmetic (csrc/tq_fused_ln.hip), restated: the (lanes per row, vectors per lane) table of TQ_LNI,
# `iters`, `grid` and `nt`.
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


Q1 = Q2 = Q3 = QR = None            # Q_dense, Q_sum, Q_out and the residual's grid (device tensors: made by the fixture below)


@pytest.fixture(autouse=True, scope='module')
def _grids():
    global Q1, Q2, Q3, QR
    Q1, Q2, Q3, QR = _asym(0.05, 120), _asym(0.07, 131), _asym(0.03, 128), _asym(0.04, 127)


def _inputs(rows, d, q_res=None, seed=0):
    """dense output, the residual as (fp32 values, int8 indices) of one quantizer launch, LayerNorm weight and bias"""
    from quantization import _hip
    q_res = q_res or QR
    g = torch.Generator(device=DEV).manual_seed(seed + 7919 * d + rows)
    a = torch.randn(rows, d, device=DEV, generator=g) * 2.0
    r0 = torch.randn(rows, d, device=DEV, generator=g) * 1.5
    r, r_idx = _hip.backend().fake_quant_int8(r0, q_res[0], q_res[1], q_res[3], q_res[6])
    w = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=g)
    b = 0.1 * torch.randn(d, device=DEV, generator=g)
    return a, r, r_idx, w, b


def _bits(t):
    return t.contiguous().view(torch.int32)


def _emits(q):
    return q is not None and not q[4] and q[3] <= 8


def _compare(be, a, r, r_idx, q_res, flags_in, q1, q2, q3, w, b, forms=('y+idx', 'idx', 'y')):
    """old kernel on R (the residual with its flagged rows NaN) against the new entry in both residual modes and the given
    output forms; -> (y_old, flags)"""
    R = r.clone()
    if flags_in is not None:
        R[flags_in.bool()] = NAN
    has_idx = _emits(q3)
    old = be.residual_layernorm_quant(a, R, q1, q2, w, b, LN_EPS, q3, want_idx=has_idx)
    y_old, idx_old = old if has_idx else (old, None)
    nan_old = torch.isnan(y_old).any(-1)
    for mode in ('indices', 'fp32'):
        res = (None, r_idx, q_res, flags_in) if mode == 'indices' else (R, None, None, None)
        for form in forms:
            want_y, want_idx = form != 'idx', form != 'y'
            if want_idx and not has_idx:
                continue
            y, idx, flags = be.residual_layernorm_quant_ires(a, *res, q1, q2, w, b, LN_EPS, q3, want_y=want_y, want_idx=want_idx)
            what = f'{mode} / {form}'
            assert flags.dtype == torch.uint8 and flags.shape == a.shape[:-1]
            assert torch.equal(flags.bool(), nan_old), what
            assert (y is None) == (not want_y) and (idx is None) == (not want_idx), what
            if want_y:
                assert torch.equal(_bits(y), _bits(y_old)), what
            if want_idx:
                keep = ~nan_old
                assert torch.equal(idx[keep], idx_old[keep]), what
    return y_old, nan_old


@pytest.mark.parametrize('d', WIDTHS)
def test_every_width_37_rows(be, d):
    """37 rows: a partly filled last block for every rows-per-block value (4, 8, 16)"""
    rows = 37
    assert rows % launch_form(rows, d).rpb != 0
    a, r, r_idx, w, b = _inputs(rows, d)
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[3] = 1
    a[11, d // 2] = NAN
    _, nan = _compare(be, a, r, r_idx, QR, flags_in, Q1, Q2, Q3, w, b)
    assert nan.nonzero().flatten().tolist() == [3, 11]


def test_second_trip_of_the_row_loop_d768(be):
    rows, d = 8197, 768
    f = launch_form(rows, d)
    assert f.iters == 2 and not f.nt and launch_form(8192, d).iters == 1 and rows % (f.rpb * f.iters) != 0
    a, r, r_idx, w, b = _inputs(rows, d)
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[[4, 8195]] = 1                # a second-trip row of the first block, a first-trip row of the last one
    a[8196, 1] = NAN
    _, nan = _compare(be, a, r, r_idx, QR, flags_in, Q1, Q2, Q3, w, b)
    assert nan.nonzero().flatten().tolist() == [4, 8195, 8196]


def test_streaming_form_d3072(be):
    rows, d = 5465, 3072
    f = launch_form(rows, d)
    assert f.nt and f.iters == 1 and not launch_form(5461, d).nt
    a, r, r_idx, w, b = _inputs(rows, d)
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[5464] = 1
    _, nan = _compare(be, a, r, r_idx, QR, flags_in, Q1, Q2, Q3, w, b, forms=('y+idx', 'idx'))
    assert nan.nonzero().flatten().tolist() == [5464]


@pytest.mark.parametrize('use', [(i, j, k) for i in (1, 0) for j in (1, 0) for k in (1, 0)])
def test_quantizer_mixes(be, use):
    """the eight mixes of present and absent quantizers; NaN in dense_out everywhere, +-inf where Q_dense clamps it"""
    rows, d = 37, 768
    a, r, r_idx, w, b = _inputs(rows, d, seed=1)
    q1, q2, q3 = (q if u else None for q, u in zip((Q1, Q2, Q3), use))
    a[2, 5] = NAN
    if q1 is not None:
        a[6, 0], a[6, 767] = INF, -INF
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[20] = 1
    _, nan = _compare(be, a, r, r_idx, QR, flags_in, q1, q2, q3, w, b)
    assert nan.nonzero().flatten().tolist() == [2, 20]


def test_infinite_sum_without_quantizers_is_a_flagged_nan_row(be):
    """no quantizer clamps an inf: the statistics turn the row NaN, and the flag says so"""
    rows, d = 9, 256
    a, r, r_idx, w, b = _inputs(rows, d, seed=2)
    a[4, 17] = INF
    for q3 in (None, Q3):
        y_old, nan = _compare(be, a, r, r_idx, QR, None, None, None, q3, w, b)
        assert bool(nan[4]) == bool(torch.isnan(y_old[4]).any())
    assert _compare(be, a, r, r_idx, QR, None, None, None, None, w, b)[1].nonzero().flatten().tolist() == [4]


@pytest.mark.parametrize('which', [0, 1, 2])
def test_division_path(be, which):
    """a scale outside [2^-100, 2^100] sends the whole launch down the division path"""
    rows, d = 37, 768
    a, r, r_idx, w, b = _inputs(rows, d, seed=3)
    qs = [Q1, Q2, Q3]
    qs[which] = _asym(2.0 ** -101 if which != 1 else 2.0 ** 101, 128, eps=0.0)      # (eps is a floor under the scale)
    a[2, 5] = NAN
    a[6, 0], a[6, 767] = INF, -INF
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[[0, 36]] = 1
    _, nan = _compare(be, a, r, r_idx, QR, flags_in, *qs, w, b)
    assert nan.nonzero().flatten().tolist() == [0, 2, 36]


@pytest.mark.parametrize('bits,zp', [(8, 0), (8, 255), (4, 0), (4, 15), (8, 127), (1, 1)])
def test_residual_grids(be, bits, zp):
    """residual grids of 8 and 4 bits (and one bit) with the zero point at either end of the grid"""
    rows, d = 37, 384
    q_res = _asym({8: 0.01, 4: 0.1, 1: 0.5}[bits], zp, bits)
    a, r, r_idx, w, b = _inputs(rows, d, q_res=q_res, seed=4)
    assert int(r_idx.min()) == -128 and int(r_idx.max()) == (1 << bits) - 1 - 128      # both ends of the grid occur
    _compare(be, a, r, r_idx, q_res, None, Q1, Q2, Q3, w, b)


def test_special_values_and_flagged_rows(be):
    """NaN / +-inf in dense_out; flagged residual rows: the first, the last, two adjacent ones of one block -- also a row that
    is flagged AND has a NaN of its own"""
    rows, d = 37, 768
    assert launch_form(rows, d).rpb == 4
    a, r, r_idx, w, b = _inputs(rows, d, seed=5)
    a[1, 0], a[1, 300], a[1, 767] = INF, -INF, INF
    a[13, 766] = NAN
    a[9, 3] = NAN
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[[0, 8, 9, 36]] = 1                         # rows 8 and 9 share the block of rows 8..11
    y_old, nan = _compare(be, a, r, r_idx, QR, flags_in, Q1, Q2, Q3, w, b)
    assert nan.nonzero().flatten().tolist() == [0, 8, 9, 13, 36]
    assert torch.isnan(y_old[nan]).all() and not torch.isnan(y_old[~nan]).any()
    # without flags the indices of those rows are plain grid values
    _, nan = _compare(be, a, r, r_idx, QR, None, Q1, Q2, Q3, w, b)
    assert nan.nonzero().flatten().tolist() == [9, 13]


def test_chained_launches_carry_the_nan_row(be):
    """two tails in a row, as in an encoder layer: the first launch's indices + flags are the second's residual"""
    rows, d = 37, 768
    a1, r, r_idx, w, b = _inputs(rows, d, seed=6)
    a2 = _inputs(rows, d, seed=7)[0]
    a1[5, 100] = NAN
    y1_old, i1_old = be.residual_layernorm_quant(a1, r, Q1, Q2, w, b, LN_EPS, Q3, want_idx=True)
    y2_old, i2_old = be.residual_layernorm_quant(a2, y1_old, Q1, Q2, w, b, LN_EPS, Q2, want_idx=True)
    _, i1, n1 = be.residual_layernorm_quant_ires(a1, None, r_idx, QR, None, Q1, Q2, w, b, LN_EPS, Q3, want_y=False)
    y2, i2, n2 = be.residual_layernorm_quant_ires(a2, None, i1, Q3, n1, Q1, Q2, w, b, LN_EPS, Q2)
    assert n1.nonzero().flatten().tolist() == [5] and n2.nonzero().flatten().tolist() == [5]
    assert torch.isnan(y2_old[5]).all()
    assert torch.equal(_bits(y2), _bits(y2_old))
    keep = ~n2.bool()
    assert torch.equal(i1[keep], i1_old[keep]) and torch.equal(i2[keep], i2_old[keep])


def test_y_only_behind_a_symmetric_output_quantizer(be):
    rows, d = 37, 512
    a, r, r_idx, w, b = _inputs(rows, d, seed=8)
    a[30, 2] = NAN
    for q3 in (_sym(0.03), _asym(0.001, 30000, 16)):
        _, nan = _compare(be, a, r, r_idx, QR, None, Q1, Q2, q3, w, b, forms=('y',))
        assert nan.nonzero().flatten().tolist() == [30]


# ------------------------------------------------------------------------------------------------------------------
# the C entry point: bounds and argument errors

def _entry(be):
    st = torch.cuda.current_stream().cuda_stream
    ref = lambda q: None if q is None else C.byref(be._qdesc(*q, 1, 1))
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())

    def call(a, r, ri, q_res, rn, y, yi, yn, rows, d, q1, q2, w, b, q3):
        return be.lib.tq_residual_layernorm_quant_ires_fwd(p(a), p(r), p(ri), ref(q_res), p(rn), p(y), p(yi), p(yn), rows, d,
                                                           ref(q1), ref(q2), p(w), p(b), LN_EPS, ref(q3), st)
    return call


@pytest.mark.parametrize('rows,d', [(37, 768), (5, 64), (19, 3072)])
def test_nothing_is_written_past_the_rows(be, rows, d):
    """inputs sized exactly, outputs in sentinel-padded buffers (also with the flags not requested)"""
    call = _entry(be)
    a, r, r_idx, w, b = _inputs(rows, d, seed=9)
    a, r_idx = a.clone(), r_idx.clone()                      # exactly rows * d elements each
    flags_in = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    flags_in[rows - 1] = 1
    n, pad = rows * d, 4096
    y_old, i_old = be.residual_layernorm_quant(a, torch.where(flags_in.bool()[:, None], torch.full_like(r, NAN), r), Q1, Q2, w, b,
                                               LN_EPS, Q3, want_idx=True)
    for with_y, with_flags in ((True, True), (False, True), (True, False), (False, False)):
        y = torch.full((n + pad,), -7.25, device=DEV)
        yi = torch.full((n + pad,), 77, dtype=torch.int8, device=DEV)
        yn = torch.full((rows + pad,), 9, dtype=torch.uint8, device=DEV)
        rc = call(a, None, r_idx, QR, flags_in, y if with_y else None, yi, yn if with_flags else None, rows, d, Q1, Q2, w, b, Q3)
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
    call = _entry(be)
    err = lambda: be.lib.tq_last_error().decode()
    rows, d = 8, 768
    a, r, r_idx, w, b = _inputs(rows, d, seed=10)
    rn = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    y, yi, yn = torch.empty_like(a), torch.empty_like(r_idx), torch.empty_like(rn)
    ok = dict(a=a, r=None, ri=r_idx, q_res=QR, rn=rn, y=y, yi=yi, yn=yn, rows=rows, d=d, q1=Q1, q2=Q2, w=w, b=b, q3=Q3)
    go = lambda **kw: call(**dict(ok, **kw))
    assert go() == 0 and go(rows=0) == 0
    assert go(ri=None, q_res=None, rn=None, r=r) == 0                          # the fp32 mode
    assert go(y=None) == 0 and go(yi=None) == 0 and go(yn=None) == 0 and go(rn=None) == 0
    assert go(r=r) == -1 and 'one of the two' in err()                          # both residual forms
    assert go(ri=None, rn=None) == -1 and 'one of the two' in err()             # neither
    assert go(ri=None, r=r) == -1 and 'res_row_nan' in err()                    # flags without indices
    assert go(y=None, yi=None) == -1 and 'y_idx' in err()
    assert go(q3=_sym(0.03)) == -1 and 'asymmetric' in err()
    assert go(q3=_asym(0.001, 300, 16)) == -1 and '8-bit' in err()
    assert go(q3=None) == -1 and 'y_idx' in err()
    assert go(q_res=None) == -1 and 'q_res' in err()
    for bad in (_sym(0.04), _asym(0.04, 127, 9), _asym(0.04, 127)[:5] + (True, EPS)):
        assert go(q_res=bad) == -1 and 'q_res' in err()
    per_col = be._qdesc(torch.full((d,), 0.04, device=DEV), torch.full((d,), 127.0, device=DEV), None, 8, False, False, EPS, d, 1)
    st = torch.cuda.current_stream().cuda_stream
    rc = be.lib.tq_residual_layernorm_quant_ires_fwd(a.data_ptr(), None, r_idx.data_ptr(), C.byref(per_col), None, y.data_ptr(),
                                                     yi.data_ptr(), None, rows, d, None, None, w.data_ptr(), b.data_ptr(), LN_EPS,
                                                     C.byref(be._qdesc(*Q3, 1, 1)), st)
    assert rc == -1 and 'per-tensor' in err()
    assert go(d=772) == -4 and 'row length' in err()                            # TQ_EUNSUPPORTED
    assert go(d=100) == -4 and 'row length' in err()
    assert go(a=a.data_ptr() + 4) == -1 and '16-byte' in err()
    assert go(y=y.data_ptr() + 8) == -1 and '16-byte' in err()
    assert go(ri=None, q_res=None, rn=None, r=r.data_ptr() + 4) == -1 and '16-byte' in err()
    assert go(ri=r_idx.data_ptr() + 2) == -1 and '4-byte' in err()
    assert go(yi=yi.data_ptr() + 1) == -1 and '4-byte' in err()
    assert go(rn=rn.data_ptr() + 1, rows=rows - 1) == 0 and go(yn=yn.data_ptr() + 3, rows=rows - 3) == 0   # flags: any alignment
    assert go(a=None) == -1 and 'NULL' in err()
    torch.cuda.synchronize()
    with pytest.raises(Exception):
        be.residual_layernorm_quant_ires(a, r, r_idx, QR, None, Q1, Q2, w, b, LN_EPS, Q3)
    with pytest.raises(Exception):
        be.residual_layernorm_quant_ires(a, None, None, None, None, Q1, Q2, w, b, LN_EPS, Q3)
