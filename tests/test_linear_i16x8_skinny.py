"""Skinny integer Linear with plane inputs and a row table (tq_linear_i16x8_skinny_fwd).

    plane form:  tot = 256 A_hi + A_lo + (32896 - z_x) rowsum[n]   (exact, 64 bits)
    8-bit form:  tot = A_lo + (128 - z_x) rowsum[n]                (exact int32)
    pre = RN32(tot) * (s_x * s_w[n]) + b[n]

Bars, all at ZERO tolerance: y (uint32 views; bf16 as the narrowed reference) against tests/_skinny16_twin.skinny16_reference
-- an int64 contraction in numpy, np.float32(int64), the C oracle's epilogue -- for all four activations; the ends of the
operand range, where |tot| passes 2^31; the header's contracts (a)-(d) GPU against GPU (tq_linear_i8_skinny_fwd,
tq_linear_i16x8_fwd, the gathered call); the index planes against the reference index and tq_quantize_hilo_fwd on y;
sentinel-padded outputs; argument errors before any device access."""
import ctypes as C

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

EPS = 1e-8
ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH = 0, 1, 2, 3
ACTS = [ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH]

SHAPES = {
    'bare minimum': (1, 2, 16),
    'classifier': (3, 2, 768),
    'pooler': (8, 768, 768),
    'second group, two chunks a lane': (9, 67, 1040),
    'most rows, longest K': (256, 3, 16384),
}


def _problem(M, N, K, seed, n_bits=16, x_zf=None):
    """indices uniform on the n_bits grid, w uniform in +-127, scales that give pre a standard deviation of about 1:
    x_delta = 5 / 2^n_bits (std of index - z about 1.44 / x_delta), w_delta = 1 / (1.44 * 73.6 * sqrt K) (per-channel: times
    0.8 .. 1.2)"""
    from tests._skinny16_twin import planes_of
    rng = np.random.default_rng(seed)
    top = 2 ** n_bits
    idx = rng.integers(0, top, (M, K))
    hi, lo = planes_of(idx)
    wd = 1.0 / (1.44 * 73.6 * np.sqrt(K))
    return dict(idx=idx, hi=hi, lo=lo, w=rng.integers(-127, 128, (N, K)).astype(np.int8), n_bits=n_bits,
                x_delta=np.float32(5.0 / top), x_zf=np.float32(rng.uniform(0.45, 0.55) * top if x_zf is None else x_zf),
                wd_one=np.array([wd], np.float32), wd_row=(wd * rng.uniform(0.8, 1.2, N)).astype(np.float32),
                bias=(rng.standard_normal(N) * 0.1).astype(np.float32))


def _q_out(lo=-0.2, hi=3.0, n_bits=8, symmetric=False, dev='cpu'):
    if symmetric:
        return (torch.tensor([hi / (2 ** (n_bits - 1) - 1)], dtype=torch.float32, device=dev), None,
                torch.tensor([1], dtype=torch.uint8, device=dev), n_bits, True, False, EPS)
    top = 2 ** n_bits - 1
    return (torch.tensor([(hi - lo) / top], dtype=torch.float32, device=dev),
            torch.tensor([-lo / ((hi - lo) / top)], dtype=torch.float32, device=dev), None, n_bits, False, False, EPS)


def _q7(q):
    return None if q is None else (float(q[0]), None if q[1] is None else float(q[1]), None if q[2] is None else bool(q[2].item()),
                                   q[3], q[4], q[5], q[6])


def _to(q, dev):
    mv = lambda t: None if t is None else t.to(dev)
    return None if q is None else (mv(q[0]), mv(q[1]), mv(q[2])) + tuple(q[3:])


def _ref(p, per_channel, with_bias, activation, q=None, planes=True, rows=None):
    from tests._skinny16_twin import skinny16_reference
    return skinny16_reference(p['hi'] if planes else None, p['lo'], p['w'], p['bias'] if with_bias else None,
                              (float(p['x_delta']), float(p['x_zf']), p['n_bits'], EPS),
                              p['wd_row'] if per_channel else p['wd_one'], EPS, activation, _q7(q), rows)


def _device(p, per_channel=True, with_bias=True, dev='cuda'):
    from quantization import _hip
    be = _hip.backend()
    w = torch.from_numpy(p['w']).to(dev)
    xq = (torch.tensor([p['x_delta']], device=dev), torch.tensor([p['x_zf']], device=dev), p['n_bits'], EPS)
    wd = torch.from_numpy(p['wd_row'] if per_channel else p['wd_one']).to(dev)
    b = torch.from_numpy(p['bias']).to(dev) if with_bias else None
    return be, (torch.from_numpy(p['hi']).to(dev), torch.from_numpy(p['lo']).to(dev)), w, be.rowsum_i8(w), b, xq, wd


def _assert_bits(got, ref, what=''):
    got, ref = got.cpu().numpy(), np.ascontiguousarray(ref.numpy() if torch.is_tensor(ref) else ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
        f'{what}: {np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32))} of {got.size} outputs differ'


def _index(planes):
    return 256 * (planes[0].cpu().long() + 128) + (planes[1].cpu().long() + 128)


def _extreme(kind, M=8, N=4, K=16384):
    """the ends of the operand range at K = 16384 (tests/test_linear_i8_extremes.py's idea for the 16-bit planes)"""
    from tests._skinny16_twin import planes_of, skinny16_tot
    idx, w, zf = {
        'top index, z = 0, w = +127': (65535, np.full((N, K), 127), 0.0),
        'index 0, z = 65535, w = -128': (0, np.full((N, K), -128), 65535.0),
        'z = 1, mixed signs': (65535, 127 * np.where(np.arange(N) % 2 == 0, 1, -1)[:, None] * np.ones((1, K), np.int64), 1.0),
    }[kind]
    p = _problem(M, N, K, seed=5, x_zf=zf)
    p['idx'] = np.full((M, K), idx)
    p['hi'], p['lo'] = planes_of(p['idx'])
    p['w'] = w.astype(np.int8)
    return p, skinny16_tot(p['hi'], p['lo'], p['w'], zf, 16)


EXTREMES = ['top index, z = 0, w = +127', 'index 0, z = 65535, w = -128', 'z = 1, mixed signs']


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_reference_equals_the_integer_oracle_on_an_8_bit_grid_cpu():
    """hi plane constantly -128 (and the 8-bit form): skinny16_reference == oracle/tq_int_oracle.c through
    tests/_skinny_twin.skinny_reference, values and indices, all four activations; the plane formula of the header equals the
    contraction of the indices; a row table equals the gathered rows"""
    from tests._skinny16_twin import Skinny16Twin, index_of, skinny16_reference, skinny16_tot
    from tests._skinny_twin import skinny_reference
    for (M, N, K), per_channel in (((3, 2, 768), False), ((9, 67, 1040), True)):
        p = _problem(M, N, K, seed=M + N + K, n_bits=8)
        assert (p['hi'] == -128).all()
        q = _q_out(-1.0, 1.5)
        for act in ACTS:
            ry, ri = skinny_reference(torch.from_numpy(p['lo']), torch.from_numpy(p['w']), torch.from_numpy(p['bias']),
                                      (float(p['x_delta']), float(p['x_zf']), 8, EPS),
                                      torch.from_numpy(p['wd_row'] if per_channel else p['wd_one']), EPS, act, _q7(q))
            for planes in (True, False):
                y, idx = _ref(p, per_channel, True, act, q, planes=planes)
                assert np.array_equal(y.numpy().view(np.uint32), ry.numpy().view(np.uint32)), (M, N, K, act, planes)
                assert np.array_equal(idx, ri.numpy().astype(np.int64) + 128)
    p = _problem(5, 3, 64, seed=2, n_bits=16)
    z = int(np.clip(np.rint(p['x_zf']), 0, 65535))
    w64 = p['w'].astype(np.int64)
    by_planes = 256 * (p['hi'].astype(np.int64) @ w64.T) + p['lo'].astype(np.int64) @ w64.T + (32896 - z) * w64.sum(1)[None, :]
    assert np.array_equal(skinny16_tot(p['hi'], p['lo'], p['w'], p['x_zf'], 16), by_planes)
    assert np.array_equal(index_of(p['hi'], p['lo']), p['idx'])
    rows = np.array([4, 0, 0, 2, 7, -1], np.int32)                  # 7 and -1: clamped to rows 4 and 0
    a = _ref(p, True, True, ACT_TANH, rows=rows)[0]
    g = dict(p, hi=p['hi'][[4, 0, 0, 2, 4, 0]], lo=p['lo'][[4, 0, 0, 2, 4, 0]])
    assert torch.equal(a, _ref(g, True, True, ACT_TANH)[0])
    # the twin: planes out of one call are the planes into the next
    be = Skinny16Twin()
    q16 = _q_out(-1.0, 1.0, n_bits=16)
    xq = (torch.tensor([p['x_delta']]), torch.tensor([p['x_zf']]), 16, EPS)
    y, (h, l) = be.linear_i16x8_skinny((torch.from_numpy(p['hi']), torch.from_numpy(p['lo'])), torch.from_numpy(p['w']), None,
                                       torch.from_numpy(p['bias']), xq, torch.from_numpy(p['wd_row']), EPS, ACT_TANH, q16,
                                       torch.float32, want_planes=True)
    scale, zp = np.float32(q16[0]), np.clip(np.rint(np.float32(q16[1])), 0, 65535)
    assert np.array_equal(y.numpy(), (scale * (index_of(h, l).astype(np.float32) - zp)).astype(np.float32))
    assert be.census == [('linear_i16x8_skinny', 5, 3, 64, ACT_TANH, (64, 1), True, False, True, 'planes', True)]


@pytest.mark.parametrize('kind', EXTREMES)
def test_extreme_sums_pass_2_to_the_31_in_the_reference_cpu(kind):
    _, tot = _extreme(kind)
    assert np.abs(tot).min() > 2 ** 31, (kind, np.abs(tot).min())
    if 'mixed' in kind:
        assert (tot > 0).any() and (tot < 0).any()
    if kind.startswith('top'):
        assert tot.max() == 65535 * 127 * 16384            # 1.36e11


def test_argument_errors_without_a_launch():
    """every check of the C entry happens before any device access (host addresses, never dereferenced)"""
    from quantization import _hip
    lib = _hip.load_library()
    who = b'tq_linear_i16x8_skinny_fwd'
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 15) & ~15
    qa = lambda bits, sym=0, log=0: _hip.tq_quantizer(p, None if sym else p, p if sym else None, bits, sym, log, 1e-8, 1, 1)

    def call(hi=None, lo=p, stride=0, rows=None, n_rows=0, w=p, rs=p, y=p, y_hi=None, y_lo=None, M=8, N=4, K=64, xd=p, xz=p,
             bits=8, wd=p, wn=1, act=0, q=None):
        return lib.tq_linear_i16x8_skinny_fwd(hi, lo, stride, rows, n_rows, w, rs, None, y, y_hi, y_lo, 0, M, N, K, xd, xz, bits,
                                              1e-8, wd, wn, 1e-8, act, None if q is None else C.byref(q), None)

    assert call(M=0) == 0 and call(N=0) == 0                  # empty: TQ_OK without a launch
    bad = {
        'x_hi == NULL with x_n_bits = 9': dict(bits=9),
        'planes with x_n_bits = 17': dict(hi=p, bits=17),
        'x_n_bits = 0': dict(bits=0),
        'y_hi without y_lo': dict(y_hi=p, q=qa(16)),
        'planes with a symmetric q_out': dict(y_hi=p, y_lo=p, q=qa(8, sym=1)),
        'planes with a 17-bit q_out': dict(y_hi=p, y_lo=p, q=qa(17)),
        'planes with a log-domain q_out': dict(y_hi=p, y_lo=p, q=qa(16, log=1)),
        'planes without q_out': dict(y_hi=p, y_lo=p),
        'y_lo alone with a 9-bit q_out': dict(y_lo=p, q=qa(9)),
        'y_lo alone with a symmetric q_out': dict(y_lo=p, q=qa(8, sym=1)),
        'a misaligned x_rows': dict(rows=p + 2, n_rows=8),
        'x_n_rows == 0 with a table': dict(rows=p, n_rows=0),
        'M = 257': dict(M=257), 'K = 24': dict(K=24), 'K = 16400': dict(K=16400), 'K = 0': dict(K=0),
        'a stride below K': dict(stride=48), 'stride no multiple of 16': dict(stride=72),
        'NULL x_lo': dict(lo=None), 'NULL w': dict(w=None), 'NULL rowsum': dict(rs=None), 'NULL x_delta': dict(xd=None),
        'NULL x_zero_float': dict(xz=None), 'NULL w_delta': dict(wd=None), 'no output': dict(y=None),
        'unaligned x_lo': dict(lo=p + 4), 'unaligned x_hi': dict(hi=p + 4), 'weight scales': dict(wn=3),
        'activation 4': dict(act=4), 'per-column q_out': dict(q=_hip.tq_quantizer(p, p, None, 8, 0, 0, 1e-8, 4, 1)),
    }
    for name, kw in bad.items():
        rc = call(**kw)
        assert rc == -1 and who in lib.tq_last_error(), (name, rc, lib.tq_last_error())


# ---- GPU: against the reference -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('case', list(SHAPES))
@pytest.mark.parametrize('activation', ACTS)
def test_bit_exact_vs_the_reference(case, activation):
    """x_n_bits 16 / 12 / 9 x per-tensor and per-channel weight scales x with and without bias, y as fp32 and bf16"""
    M, N, K = SHAPES[case]
    for n_bits in (16, 12, 9):
        p = _problem(M, N, K, seed=M + N + K + n_bits + activation, n_bits=n_bits)
        for per_channel in (False, True):
            for with_bias in (False, True):
                be, x, w, rs, b, xq, wd = _device(p, per_channel, with_bias)
                ref = _ref(p, per_channel, with_bias, activation)[0]
                what = f'{case} act={activation} bits={n_bits} per_channel={per_channel} bias={with_bias}'
                _assert_bits(be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, activation, None, torch.float32), ref, what)
                yb = be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, activation, None, torch.bfloat16)
                assert torch.equal(yb.cpu(), ref.to(torch.bfloat16)), what


@gpu
@pytest.mark.parametrize('kind', EXTREMES)
def test_range_ends_are_exact(kind):
    p, tot = _extreme(kind)
    assert np.abs(tot).min() > 2 ** 31
    for per_channel in (False, True):
        be, x, w, rs, b, xq, wd = _device(p, per_channel, True)
        ref = _ref(p, per_channel, True, ACT_NONE)[0]
        _assert_bits(be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, ACT_NONE, None, torch.float32), ref, kind)
        nb = _ref(p, per_channel, False, ACT_NONE)[0]
        _assert_bits(be.linear_i16x8_skinny(x, w, rs, None, xq, wd, EPS, ACT_NONE, None, torch.float32), nb, kind + ', no bias')
        q = _q_out(float(ref.min()) - 1.0, float(ref.max()) + 1.0, n_bits=16)
        ry, ri = _ref(p, per_channel, True, ACT_NONE, q)
        y, planes = be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, ACT_NONE, _to(q, 'cuda'), torch.float32, want_planes=True)
        _assert_bits(y, ry, kind + ', quantized')
        assert np.array_equal(_index(planes).numpy(), ri)


# ---- GPU: the header's contracts, GPU against GPU ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('shape', [(1, 2, 16), (3, 2, 768), (8, 768, 768), (9, 67, 1040), (256, 3, 128), (9, 5, 16384)])
def test_contracts_a_and_b_equal_the_8_bit_skinny_entry(shape):
    """(a) x_hi == NULL: y and the int8 index == tq_linear_i8_skinny_fwd, all four activations; (b) planes with x_n_bits = 8
    (hi constantly -128): the same bits again"""
    M, N, K = shape
    p = _problem(M, N, K, seed=M + N + K, n_bits=8)
    be, (hi, lo), w, rs, b, xq, wd = _device(p, True, True)
    assert (hi == -128).all()
    q = _to(_q_out(-1.0, 1.5), 'cuda')
    for act in ACTS:
        old = be.linear_i8_skinny(lo, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        old_plain = be.linear_i8_skinny(lo, w, rs, b, xq, wd, EPS, act, None, torch.bfloat16)
        for x in (lo, (hi, lo)):
            new = be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
            assert torch.equal(new[0].view(torch.int32), old[0].view(torch.int32)) and torch.equal(new[1], old[1]), (shape, act)
            assert torch.equal(be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, act, None, torch.bfloat16), old_plain)


@gpu
def test_contract_a_on_the_strided_first_token_view():
    """indices [4, 5, 768] on the device, x = idx[:, 0] (row stride 3840) read in place, against the old entry on the view"""
    p = _problem(4, 67, 768, seed=11, n_bits=8)
    be, _, w, rs, b, xq, wd = _device(p)
    idx = torch.from_numpy((np.random.default_rng(12).integers(0, 256, (4, 5, 768)) - 128).astype(np.int8)).cuda()
    view = idx[:, 0]
    assert view.stride() == (3840, 1) and view.data_ptr() == idx.data_ptr()
    q = _to(_q_out(-1.0, 1.0), 'cuda')
    for act in (ACT_NONE, ACT_TANH):
        a = be.linear_i16x8_skinny(view, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        c = be.linear_i8_skinny(view, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        assert torch.equal(a[0].view(torch.int32), c[0].view(torch.int32)) and torch.equal(a[1], c[1])


@gpu
@pytest.mark.parametrize('shape', [(64, 64, 128), (128, 128, 768)])
def test_contract_c_equals_the_tiled_16_bit_linear(shape):
    M, N, K = shape
    p = _problem(M, N, K, seed=M + K, n_bits=16)
    be, (hi, lo), w, rs, b, xq, wd = _device(p, True, True)
    q = _to(_q_out(-0.2, 3.0), 'cuda')
    for act in (ACT_NONE, ACT_RELU):
        assert torch.equal(be.linear_i16x8_skinny((hi, lo), w, rs, b, xq, wd, EPS, act, None, torch.float32).view(torch.int32),
                           be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, act, None, torch.float32).view(torch.int32))
        a = be.linear_i16x8_skinny((hi, lo), w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        t = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        assert torch.equal(a[0].view(torch.int32), t[0].view(torch.int32)) and torch.equal(a[1], t[1])


@gpu
@pytest.mark.parametrize('planes', [True, False])
def test_contract_d_a_row_table_equals_the_gathered_rows(planes):
    """a table with repeats that is not monotone, stride > K, the x buffers exactly x_n_rows rows long (the last row ends
    with the allocation); entries -1 and x_n_rows give the clamped rows' results"""
    R, N, K, stride = 13, 67, 768, 800
    p = _problem(R, N, K, seed=31, n_bits=16 if planes else 8)
    be, (hi, lo), w, rs, b, xq, wd = _device(p, True, True)

    def strided(t):                      # [R, K] view of a buffer of exactly (R - 1) * stride + K bytes
        buf = torch.empty((R - 1) * stride + K, dtype=torch.int8, device='cuda')
        v = buf.as_strided((R, K), (stride, 1))
        v.copy_(t)
        return v

    x = (strided(hi), strided(lo)) if planes else strided(lo)
    table = [12, 3, 3, 0, 7, 12, 1, 11, 2, 5, 5]                          # 11 rows: a second row group with three valid rows
    q = _to(_q_out(-1.0, 1.0, n_bits=16 if planes else 8), 'cuda')
    kw = dict(want_planes=True) if planes else dict(want_idx=True)

    def run(tab):
        rows = torch.tensor(tab, dtype=torch.int32, device='cuda')
        return be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, ACT_TANH, q, torch.float32, rows=rows, **kw)

    def gathered(tab):
        sel = torch.tensor(tab, device='cuda')
        g = (hi[sel].contiguous(), lo[sel].contiguous()) if planes else lo[sel].contiguous()
        return be.linear_i16x8_skinny(g, w, rs, b, xq, wd, EPS, ACT_TANH, q, torch.float32, **kw)

    def same(a, c):
        ia, ic = (_index(a[1]), _index(c[1])) if planes else (a[1].cpu(), c[1].cpu())
        return torch.equal(a[0].view(torch.int32), c[0].view(torch.int32)) and torch.equal(ia, ic)

    got = run(table)
    assert got[0].shape == (len(table), N) and same(got, gathered(table))
    ry = _ref(p, True, True, ACT_TANH, q, planes=planes, rows=np.array(table))[0]
    _assert_bits(got[0], ry, 'row table against the reference')
    # a view of a longer table, as the packed route passes seq_start[:-1]
    longer = torch.tensor(table + [9], dtype=torch.int32, device='cuda')
    v = be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, ACT_TANH, q, torch.float32, rows=longer[:-1], **kw)
    assert same(v, got)
    assert same(run([-1, 4, R, 2 ** 31 - 1, -2 ** 31]), gathered([0, 4, R - 1, R - 1, 0]))


# ---- GPU: index planes -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('q_bits', [16, 12, 9])
def test_output_planes_are_the_reference_index_and_quantize_hilo_of_y(q_bits):
    """256 (hi + 128) + (lo + 128) == the reference index == tq_quantize_hilo_fwd applied to the fp32 y; the same planes with
    y == NULL; pooler shape (8-bit input, Tanh) and a 16-bit input with every activation"""
    M, N, K = 9, 67, 1040
    for planes_in, acts in ((False, [ACT_TANH]), (True, ACTS)):
        p = _problem(M, N, K, seed=q_bits + planes_in, n_bits=16 if planes_in else 8)
        be, (hi, lo), w, rs, b, xq, wd = _device(p, True, True)
        x = (hi, lo) if planes_in else lo
        for act in acts:
            q = _q_out(-1.0, 1.0, n_bits=q_bits) if act == ACT_TANH else _q_out(-0.5, 3.0, n_bits=q_bits)
            ry, ri = _ref(p, True, True, act, q, planes=planes_in)
            assert ri.min() == 0 or ri.max() == 2 ** q_bits - 1 or act == ACT_TANH      # the grid's ends are reached (clamp)
            qd = _to(q, 'cuda')
            y, pl = be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, act, qd, torch.float32, want_planes=True)
            _assert_bits(y, ry, f'q_bits={q_bits} act={act}')
            assert np.array_equal(_index(pl).numpy(), ri), (q_bits, act)
            h2, l2 = be.quantize_hilo(y, (qd[0], qd[1], q_bits, EPS))
            assert torch.equal(h2, pl[0]) and torch.equal(l2, pl[1])
            none, only = be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, act, qd, torch.float32, want_planes=True, want_y=False)
            assert none is None and torch.equal(only[0], pl[0]) and torch.equal(only[1], pl[1])
            yb, plb = be.linear_i16x8_skinny(x, w, rs, b, xq, wd, EPS, act, qd, torch.bfloat16, want_planes=True)
            assert torch.equal(yb.cpu(), ry.to(torch.bfloat16)) and torch.equal(plb[0], pl[0]) and torch.equal(plb[1], pl[1])


@gpu
def test_y_lo_alone_is_the_old_entrys_y_idx_and_planes_of_an_8_bit_grid_have_a_constant_hi():
    p = _problem(9, 67, 1040, seed=8, n_bits=8)
    be, (hi, lo), w, rs, b, xq, wd = _device(p, True, True)
    q = _to(_q_out(-0.2, 3.0), 'cuda')
    old = be.linear_i8_skinny(lo, w, rs, b, xq, wd, EPS, ACT_GELU, q, torch.float32, want_idx=True)
    new = be.linear_i16x8_skinny(lo, w, rs, b, xq, wd, EPS, ACT_GELU, q, torch.float32, want_idx=True)
    assert torch.equal(new[0].view(torch.int32), old[0].view(torch.int32)) and torch.equal(new[1], old[1])
    none, only = be.linear_i16x8_skinny(lo, w, rs, b, xq, wd, EPS, ACT_GELU, q, torch.float32, want_idx=True, want_y=False)
    assert none is None and torch.equal(only, old[1])
    _, pl = be.linear_i16x8_skinny(lo, w, rs, b, xq, wd, EPS, ACT_GELU, q, torch.float32, want_planes=True)
    assert (pl[0] == -128).all() and torch.equal(pl[1], old[1])


# ---- GPU: bounds -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('N', [2, 67])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_nothing_is_written_outside_the_outputs(N, dtype):
    """through the C entry into sentinel-filled buffers: y, y_hi and y_lo start 3 elements into theirs and end 4096 elements
    before the buffers do; only M * N elements change"""
    from quantization import _hip
    M, K, front, back = 11, 784, 3, 4096
    p = _problem(M, N, K, seed=N, n_bits=16)
    be, (hi, lo), w, rs, b, xq, wd = _device(p, True, True)
    q = _q_out(-0.2, 3.0, n_bits=16, dev='cuda')
    ybuf = torch.full((front + M * N + back,), -1.5, dtype=dtype, device='cuda')
    hbuf = torch.full((front + M * N + back,), 90, dtype=torch.int8, device='cuda')
    lbuf = torch.full((front + M * N + back,), 91, dtype=torch.int8, device='cuda')
    qd = be._qdesc(*q, 1, 1)
    rc = be.lib.tq_linear_i16x8_skinny_fwd(
        hi.data_ptr(), lo.data_ptr(), 0, None, 0, w.data_ptr(), rs.data_ptr(), b.data_ptr(),
        ybuf.data_ptr() + front * ybuf.element_size(), hbuf.data_ptr() + front, lbuf.data_ptr() + front, _hip._DTYPES[dtype],
        M, N, K, xq[0].data_ptr(), xq[1].data_ptr(), 16, EPS, wd.data_ptr(), N, EPS, ACT_RELU, C.byref(qd), _hip._stream())
    _hip._check(rc, be.lib)
    torch.cuda.synchronize()
    ry, ri = _ref(p, True, True, ACT_RELU, q)
    yh, hh, lh = ybuf.cpu(), hbuf.cpu(), lbuf.cpu()
    sl = slice(front, front + M * N)
    assert torch.equal(yh[sl].reshape(M, N), ry.to(dtype))
    assert np.array_equal(_index((hh[sl], lh[sl])).reshape(M, N).numpy(), ri)
    assert (yh[:front] == -1.5).all() and (yh[front + M * N:] == -1.5).all(), 'y written outside its M * N elements'
    assert (hh[:front] == 90).all() and (hh[front + M * N:] == 90).all(), 'y_hi written outside its M * N elements'
    assert (lh[:front] == 91).all() and (lh[front + M * N:] == 91).all(), 'y_lo written outside its M * N elements'
