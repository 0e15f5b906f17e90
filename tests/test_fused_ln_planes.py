"""tq_residual_layernorm_quant_planes_fwd (the fp32 LayerNorm tail that also writes the two int8 byte planes of its output's
grid index) against the launches it replaces on the same GPU -- `HipBackend.residual_layernorm_quant` for y,
`HipBackend.quantize_hilo(y)` for the planes -- and against the CPU chain (tests/_planes_twin.planes_tail_reference:
ln_tail_chain with kernel-order statistics + the oracle's index).

Every comparison is exact:
  * y as int32 bit patterns (rows the kernel turns NaN as a whole included),
  * the planes with torch.equal on every row that is not NaN (the planes of a NaN row are unspecified).

Launch forms (the launcher restates `launch_res_ln_ires`; `launch_form` below restates it once more, and the two at-size
cases assert their premise with it first): rows per block rpb = 256 / LPR, a second trip of the row loop beyond rpb * 2048
rows, streaming loads / stores from rows * d * 4 >= 64 MiB.  The at-size cases compare GPU with GPU only.

Measured once on an MI355X (pytest --durations): the 42 cases together take 3.1 s, the slowest 0.43 s (the first one: it
loads the library); the two at-size cases less than 0.01 s each.
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


Q1 = Q2 = None                      # Q_dense, Q_sum (device tensors: made by the fixture below)
Q_OUT = {}                          # n_bits -> Q_out


@pytest.fixture(autouse=True, scope='module')
def _grids():
    global Q1, Q2
    Q1, Q2 = _asym(0.05, 120), _asym(0.07, 131)
    # LayerNorm outputs lie in about [-5, 5]: every grid covers them; 16 bits with the zero point low enough that indices
    # >= 32768 occur (hi plane >= 0)
    Q_OUT.update({16: _asym(2.0e-4, 30000, 16), 12: _asym(3.0e-3, 2048, 12), 9: _asym(0.02, 256, 9), 8: _asym(0.03, 128, 8),
                  1: _asym(1.0, 0, 1)})


def _inputs(rows, d, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + 7919 * d + rows)
    a = torch.randn(rows, d, device=DEV, generator=g) * 2.0
    r = torch.randn(rows, d, device=DEV, generator=g) * 1.5
    w = 1.0 + 0.1 * torch.randn(d, device=DEV, generator=g)
    b = 0.1 * torch.randn(d, device=DEV, generator=g)
    return a, r, w, b


def _bits(t):
    return t.contiguous().view(torch.int32)


def _index(hi, lo):
    return 256 * (hi.int() + 128) + (lo.int() + 128)


def _compare(be, a, r, q1, q2, q3, w, b, cpu=False):
    """the new entry against the existing tail + quantize_hilo on the GPU [and the CPU chain]; -> (y, index int32, NaN rows)"""
    y_old = be.residual_layernorm_quant(a, r, q1, q2, w, b, LN_EPS, q3)
    hi_old, lo_old = be.quantize_hilo(y_old, (q3[0], q3[1], q3[3], q3[6]))
    y, (hi, lo) = be.residual_layernorm_quant_planes(a, r, q1, q2, w, b, LN_EPS, q3)
    assert y.dtype == torch.float32 and hi.dtype == lo.dtype == torch.int8 and y.shape == hi.shape == lo.shape == a.shape
    assert torch.equal(_bits(y), _bits(y_old)), 'y differs from the existing tail'
    nan = torch.isnan(y_old).any(-1)
    keep = ~nan
    assert torch.equal(hi[keep], hi_old[keep]), 'hi plane differs from quantize_hilo(y)'
    assert torch.equal(lo[keep], lo_old[keep]), 'lo plane differs from quantize_hilo(y)'
    if cpu:
        from tests._exact_backend import _p
        from tests._planes_twin import planes_tail_reference
        c = lambda q: None if q is None else tuple(None if t is None else (t.cpu() if torch.is_tensor(t) else t) for t in q)
        ry, (rhi, rlo) = planes_tail_reference(a.cpu(), r.cpu(), _p(c(q1)), _p(c(q2)), w.cpu(), b.cpu(), LN_EPS, _p(c(q3)))
        kc = keep.cpu()
        assert torch.equal(_bits(y.cpu()[kc]), _bits(ry[kc])), 'y differs from the CPU chain'
        assert torch.equal(torch.isnan(ry).any(-1), nan.cpu())
        assert torch.equal(hi.cpu()[kc], rhi[kc]) and torch.equal(lo.cpu()[kc], rlo[kc]), 'planes differ from the CPU chain'
    return y, _index(hi, lo), nan


@pytest.mark.parametrize('d', WIDTHS)
def test_every_width_37_rows(be, d):
    """37 rows: a partly filled last block for every rows-per-block value (4, 8, 16)"""
    rows = 37
    assert rows % launch_form(rows, d).rpb != 0
    a, r, w, b = _inputs(rows, d)
    _, idx, nan = _compare(be, a, r, Q1, Q2, Q_OUT[16], w, b, cpu=True)
    assert not nan.any() and int(idx.max()) >= 32768 and int(idx.min()) < 32768      # both signs of the hi plane


@pytest.mark.parametrize('bits', [16, 12, 9, 8, 1])
@pytest.mark.parametrize('use', [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_quantizer_mixes_d768(be, use, bits):
    """the four mixes of present and absent Q_dense / Q_sum behind output grids of 16, 12, 9, 8 bits and one bit"""
    rows, d = 37, 768
    a, r, w, b = _inputs(rows, d, seed=1)
    q1, q2 = (q if u else None for q, u in zip((Q1, Q2), use))
    q3 = Q_OUT[bits]
    y, idx, nan = _compare(be, a, r, q1, q2, q3, w, b, cpu=True)
    assert not nan.any() and 0 <= int(idx.min()) and int(idx.max()) <= (1 << bits) - 1
    if bits == 16:
        assert int(idx.max()) >= 32768                               # hi plane >= 0 occurs
    if bits <= 8:
        # the hi plane is constantly -128 and the lo plane is y_idx of the existing entry
        _, (hi, lo) = be.residual_layernorm_quant_planes(a, r, q1, q2, w, b, LN_EPS, q3)
        _, y_idx = be.residual_layernorm_quant(a, r, q1, q2, w, b, LN_EPS, q3, want_idx=True)
        assert bool((hi == -128).all()) and torch.equal(lo, y_idx)
    if bits == 1:
        assert sorted(idx.unique().tolist()) == [0, 1]


@pytest.mark.parametrize('which', [0, 1, 2])
def test_division_path(be, which):
    """a scale outside [2^-100, 2^100] sends the whole launch down the division path (chosen as tests/test_fused_ln_ires.py
    chooses it); which = 2: the output quantizer itself"""
    rows, d = 37, 768
    a, r, w, b = _inputs(rows, d, seed=3)
    qs = [Q1, Q2, Q_OUT[16]]
    qs[which] = _asym(2.0 ** -101 if which != 1 else 2.0 ** 101, 128 if which != 2 else 30000, 8 if which != 2 else 16, eps=0.0)
    _, idx, nan = _compare(be, a, r, *qs, w, b)
    assert not nan.any()
    if which == 2:
        assert sorted(idx.unique().tolist()) == [0, 65535]          # every value is far outside such a grid: both ends


def test_range_ends(be):
    """inputs that clamp to index 0 and to 2^n - 1"""
    rows, d = 37, 768
    a, r, w, b = _inputs(rows, d, seed=4)
    for bits, q3 in ((16, _asym(1.0e-5, 32768, 16)), (12, _asym(1.0e-4, 2048, 12)), (9, _asym(1.0e-3, 256, 9))):
        _, idx, nan = _compare(be, a, r, Q1, Q2, q3, w, b, cpu=bits == 16)
        assert not nan.any() and int(idx.min()) == 0 and int(idx.max()) == (1 << bits) - 1
    # the zero point at either end of the grid
    for zp in (0, 65535):
        _, idx, _ = _compare(be, a, r, Q1, Q2, _asym(2.0e-4, zp, 16), w, b)
        assert int(idx.min() if zp == 0 else idx.max()) == zp


def test_special_values(be):
    """NaN in dense_out / in the residual: those rows are NaN as a whole with the existing kernel's bits, the planes are compared
    on the other rows; +-inf where Q_dense clamps it and where nothing does"""
    rows, d = 37, 768
    assert launch_form(rows, d).rpb == 4
    a, r, w, b = _inputs(rows, d, seed=5)
    a[9, 3] = NAN
    r[13, 766] = NAN
    a[1, 0], a[1, 300], a[1, 767] = INF, -INF, INF
    r[36, 5] = -INF
    y, _, nan = _compare(be, a, r, Q1, Q2, Q_OUT[16], w, b, cpu=True)
    assert nan.nonzero().flatten().tolist() == [9, 13]
    assert torch.isnan(y[nan]).all() and bool((_bits(y[nan]) == 0x7fc00000).all())
    # without Q_dense / Q_sum an inf reaches the statistics: whatever the existing kernel makes of the row, bit for bit
    _compare(be, a, r, None, None, Q_OUT[16], w, b)
    _compare(be, a, r, None, Q2, Q_OUT[12], w, b)


def test_second_trip_of_the_row_loop_d768(be):
    rows, d = 8193, 768
    f = launch_form(rows, d)
    assert f.iters == 2 and not f.nt and launch_form(8192, d).iters == 1 and rows % (f.rpb * f.iters) != 0
    a, r, w, b = _inputs(rows, d)
    a[8192, 1] = NAN
    a[4, 7] = NAN                                   # a second-trip row of the first block
    _, _, nan = _compare(be, a, r, Q1, Q2, Q_OUT[16], w, b)
    assert nan.nonzero().flatten().tolist() == [4, 8192]


def test_streaming_form_d768(be):
    rows, d = 21846, 768
    f = launch_form(rows, d)
    assert f.nt and f.iters == 2 and not launch_form(rows - 1, d).nt and rows * d * 4 >= 64 << 20
    a, r, w, b = _inputs(rows, d)
    a[rows - 1, 0] = NAN
    _, _, nan = _compare(be, a, r, Q1, Q2, Q_OUT[16], w, b)
    assert nan.nonzero().flatten().tolist() == [rows - 1]


def test_planes_feed_the_16_bit_linear(be):
    """the chain the planes are for: linear_i16x8 on the tail's planes == linear_i16x8 on quantize_hilo(y)"""
    rows, d, N = 64, 768, 256
    a, r, w, b = _inputs(rows, d, seed=6)
    q3 = Q_OUT[16]
    x_q = (q3[0], q3[1], q3[3], q3[6])
    y, (hi, lo) = be.residual_layernorm_quant_planes(a, r, Q1, Q2, w, b, LN_EPS, q3)
    hi2, lo2 = be.quantize_hilo(y, x_q)
    g = torch.Generator(device=DEV).manual_seed(11)
    w_idx = torch.randint(-127, 128, (N, d), device=DEV, generator=g, dtype=torch.int32).to(torch.int8)
    rowsum = be.rowsum_i8(w_idx)
    bias = torch.randn(N, device=DEV, generator=g) * 0.1
    w_delta = torch.full((1,), 0.002, device=DEV)
    run = lambda h, l: be.linear_i16x8(h, l, w_idx, rowsum, bias, x_q, w_delta, EPS, 0, None, torch.float32)
    out, want = run(hi, lo), run(hi2, lo2)
    assert torch.equal(_bits(out), _bits(want)) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------------
# the C entry point: bounds and argument errors

def _entry(be):
    st = torch.cuda.current_stream().cuda_stream
    ref = lambda q: None if q is None else C.byref(be._qdesc(*q, 1, 1))
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())

    def call(a, r, y, hi, lo, rows, d, q1, q2, w, b, q3):
        return be.lib.tq_residual_layernorm_quant_planes_fwd(p(a), p(r), p(y), p(hi), p(lo), rows, d, ref(q1), ref(q2), p(w), p(b),
                                                             LN_EPS, ref(q3), st)
    return call


@pytest.mark.parametrize('rows,d', [(37, 768), (5, 64), (19, 3072)])
def test_nothing_is_written_past_the_rows(be, rows, d):
    """inputs sized exactly, outputs in sentinel-padded buffers"""
    call = _entry(be)
    a, r, w, b = _inputs(rows, d, seed=9)
    a, r = a.clone(), r.clone()                              # exactly rows * d elements each
    n, pad = rows * d, 4096
    q3 = Q_OUT[16]
    y_old = be.residual_layernorm_quant(a, r, Q1, Q2, w, b, LN_EPS, q3)
    hi_old, lo_old = be.quantize_hilo(y_old, (q3[0], q3[1], q3[3], q3[6]))
    y = torch.full((n + pad,), -7.25, device=DEV)
    hi = torch.full((n + pad,), 77, dtype=torch.int8, device=DEV)
    lo = torch.full((n + pad,), 55, dtype=torch.int8, device=DEV)
    rc = call(a, r, y, hi, lo, rows, d, Q1, Q2, w, b, q3)
    assert rc == 0, be.lib.tq_last_error()
    torch.cuda.synchronize()
    assert bool((y[n:] == -7.25).all()) and torch.equal(_bits(y[:n]), _bits(y_old).flatten())
    assert bool((hi[n:] == 77).all()) and torch.equal(hi[:n], hi_old.flatten())
    assert bool((lo[n:] == 55).all()) and torch.equal(lo[:n], lo_old.flatten())


def test_argument_errors(be):
    call = _entry(be)
    err = lambda: be.lib.tq_last_error().decode()
    rows, d = 8, 768
    a, r, w, b = _inputs(rows, d, seed=10)
    y = torch.empty_like(a)
    hi, lo = torch.empty(rows, d, dtype=torch.int8, device=DEV), torch.empty(rows, d, dtype=torch.int8, device=DEV)
    ok = dict(a=a, r=r, y=y, hi=hi, lo=lo, rows=rows, d=d, q1=Q1, q2=Q2, w=w, b=b, q3=Q_OUT[16])
    go = lambda **kw: call(**dict(ok, **kw))
    assert go() == 0 and go(rows=0) == 0 and go(q1=None) == 0 and go(q2=None) == 0 and go(q1=None, q2=None) == 0
    assert go(rows=0, y=None, hi=None, lo=None) == 0                          # no rows: nothing is looked at
    for name in ('y', 'hi', 'lo', 'a', 'r', 'w', 'b'):
        assert go(**{name: None}) == -1 and 'NULL' in err(), name
    assert go(q3=None) == -1 and 'output quantizer' in err()
    assert go(q3=_sym(0.03, 16)) == -1 and 'asymmetric' in err()
    assert go(q3=_asym(2.0e-4, 30000, 17)) == -1 and '16 bits' in err()
    assert go(q3=_asym(2.0e-4, 30000, 16)[:5] + (True, EPS)) == -1 and 'linear-domain' in err()
    per_col = be._qdesc(torch.full((d,), 2.0e-4, device=DEV), torch.full((d,), 30000.0, device=DEV), None, 16, False, False, EPS, d, 1)
    st = torch.cuda.current_stream().cuda_stream
    rc = be.lib.tq_residual_layernorm_quant_planes_fwd(a.data_ptr(), r.data_ptr(), y.data_ptr(), hi.data_ptr(), lo.data_ptr(), rows,
                                                       d, None, None, w.data_ptr(), b.data_ptr(), LN_EPS, C.byref(per_col), st)
    assert rc == -1 and 'per-tensor' in err()
    assert go(y=y.data_ptr() + 8) == -1 and '16-byte' in err()
    assert go(a=a.data_ptr() + 4) == -1 and '16-byte' in err()
    assert go(r=r.data_ptr() + 4) == -1 and '16-byte' in err()
    assert go(hi=hi.data_ptr() + 2) == -1 and '4-byte' in err()
    assert go(lo=lo.data_ptr() + 1) == -1 and '4-byte' in err()
    assert go(hi=hi.data_ptr() + 4, lo=lo.data_ptr() + 4, rows=rows - 1) == 0  # the planes: 4-byte alignment is enough
    assert go(d=100) == -4 and 'row length' in err()                            # TQ_EUNSUPPORTED
    assert go(d=772) == -4 and 'row length' in err()
    torch.cuda.synchronize()
    with pytest.raises(Exception):
        be.residual_layernorm_quant_planes(a, r, Q1, Q2, w, b, LN_EPS, None)
    with pytest.raises(Exception):
        be.residual_layernorm_quant_planes(a.bfloat16(), r, Q1, Q2, w, b, LN_EPS, Q_OUT[16])
