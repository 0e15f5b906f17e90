"""Integer Linear for skinny shapes (tq_linear_i8_skinny_fwd): few rows, any number of output features.

    tot = sum_k x w + (128 - z_x) rowsum[n]   (exact int32)      pre = (float)tot * (s_x * s_w[n]) + b[n]

Bars, all at ZERO tolerance: `pre` against oracle/tq_int_oracle.c (uint32 views); ReLU and GELU behind an 8-bit asymmetric
output quantizer -- values and int8 indices -- against the oracle's codes 1 and 4 (GELU: the correctly rounded erf form);
Tanh against np.tanh in float64 narrowed once (tests/_skinny_twin.py holds the chain); a strided first-token view against its
contiguous copy; the tiled kernels where both take the shape; sentinel-padded outputs at N = 2, 3, 67.

Equality with the tiled kernels, GELU: at (64, 64, 128) tq_linear_i8_stair_fwd evaluates the accepted staircase table (the
correctly rounded GELU, this kernel's definition).  At (32, 96, 192) K is no multiple of 128, the LDS-free kernel runs and
ignores the table: its degree-7 fit agrees with the correctly rounded GELU on all but <= 2e-5 of the outputs
(quantization/options.py INT8_ACT_STAIR), here on all 3072 of the seeded problem."""
import ctypes as C

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

EPS = 1e-8
ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH = 0, 1, 2, 3

CASES = {
    'bare minimum': (1, 1, 16),
    'classifier': (3, 2, 768),
    'pooler': (8, 768, 768),
    'ragged K': (5, 67, 784),
    'rows across groups': (9, 5, 16384),
    'most rows': (256, 3, 128),
}
TANH_SHAPES = [(8, 768, 768), (5, 67, 784), (3, 2, 768), (9, 5, 16384)]
# seeds of the Tanh problems, picked on the CPU reference alone for the test's premise (std(pre) in [0.8, 1.3]): the six outputs
# of (3, 2, 768) scatter -- seeds 1..4 give 1.37 / 0.95 / 1.15 / 1.30 there; the other shapes hold it for every seed 1..8
TANH_SEEDS = {(8, 768, 768): 1, (5, 67, 784): 1, (3, 2, 768): 2, (9, 5, 16384): 1}


def _problem(M, N, K, seed, x_zf=None):
    """x uniform on the 8-bit grid, w uniform in +-127, scales that give pre a standard deviation of about 1:
    x_delta = 0.02, w_delta = 1 / (0.02 * 74 * 73.6 * sqrt K) (per-channel: times 0.8 .. 1.2)"""
    rng = np.random.default_rng(seed)
    wd = 1.0 / (0.02 * 74 * 73.6 * np.sqrt(K))
    return dict(x=(rng.integers(0, 256, (M, K)) - 128).astype(np.int8), w=rng.integers(-127, 128, (N, K)).astype(np.int8),
                x_delta=np.float32(0.02), x_zf=np.float32(rng.uniform(120, 135) if x_zf is None else x_zf),
                wd_one=np.array([wd], np.float32), wd_row=(wd * rng.uniform(0.8, 1.2, N)).astype(np.float32),
                bias=(rng.standard_normal(N) * 0.1).astype(np.float32))


def _q_out(lo=-0.2, hi=3.0, n_bits=8, symmetric=False, dev='cpu'):
    if symmetric:          # signed symmetric grid: delta alone, sign flag set
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


def _ref_pre(p, per_channel, with_bias):
    from tests._skinny_twin import skinny_pre
    return skinny_pre(torch.from_numpy(p['x']), torch.from_numpy(p['w']), torch.from_numpy(p['bias']) if with_bias else None,
                      (float(p['x_delta']), float(p['x_zf']), 8, EPS), torch.from_numpy(p['wd_row'] if per_channel else p['wd_one']),
                      EPS)


def _device(p, per_channel=True, with_bias=True, dev='cuda'):
    from quantization import _hip
    be = _hip.backend()
    w = torch.from_numpy(p['w']).to(dev)
    xq = (torch.tensor([p['x_delta']], device=dev), torch.tensor([p['x_zf']], device=dev), 8, EPS)
    wd = torch.from_numpy(p['wd_row'] if per_channel else p['wd_one']).to(dev)
    b = torch.from_numpy(p['bias']).to(dev) if with_bias else None
    return be, torch.from_numpy(p['x']).to(dev), w, be.rowsum_i8(w), b, xq, wd


def _assert_bits(got, ref, what=''):
    got, ref = got.cpu().numpy(), np.ascontiguousarray(ref.numpy() if torch.is_tensor(ref) else ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
        f'{what}: {np.count_nonzero(got.view(np.uint32) != ref.view(np.uint32))} of {got.size} outputs differ'


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    """Every check of the C entry happens before any device access: shapes, strides, bits, y_idx rule, NULL operands"""
    from quantization import _hip
    lib = _hip.load_library()
    who = b'tq_linear_i8_skinny_fwd'
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 15) & ~15                         # a 16-byte aligned host address: never dereferenced
    qs = _hip.tq_quantizer(p, None, p, 8, 1, 0, 1e-8, 1, 1)

    def call(x=p, stride=0, w=p, rs=p, y=p, y_idx=None, M=8, N=4, K=64, xd=p, xz=p, bits=8, wd=p, wn=1, act=0, q=None):
        return lib.tq_linear_i8_skinny_fwd(x, stride, w, rs, None, y, y_idx, 0, M, N, K, xd, xz, bits, 1e-8, wd, wn, 1e-8, act,
                                           None if q is None else C.byref(q), None)

    assert call(M=0) == 0 and call(N=0) == 0                  # empty: TQ_OK without a launch
    bad = {
        'M = 257': dict(M=257), 'K = 24': dict(K=24), 'K = 16400': dict(K=16400), 'K = 0': dict(K=0),
        'stride 8 < K': dict(stride=8), 'stride no multiple of 16': dict(stride=72), 'x_n_bits = 9': dict(bits=9),
        'x_n_bits = 0': dict(bits=0), 'y_idx with a symmetric q_out': dict(y_idx=p, q=qs), 'y_idx without q_out': dict(y_idx=p),
        'NULL x': dict(x=None), 'NULL w': dict(w=None), 'NULL rowsum': dict(rs=None), 'NULL x_delta': dict(xd=None),
        'NULL x_zero_float': dict(xz=None), 'NULL w_delta': dict(wd=None), 'no output': dict(y=None),
        'unaligned x': dict(x=p + 4), 'weight scales': dict(wn=3), 'activation 4': dict(act=4),
        'per-column q_out': dict(q=_hip.tq_quantizer(p, p, None, 8, 0, 0, 1e-8, 4, 1)),
    }
    for name, kw in bad.items():
        rc = call(**kw)
        assert rc == -1 and who in lib.tq_last_error(), (name, rc, lib.tq_last_error())
    # (what the checks accept is launched, and a launch would dereference the host addresses above: the accepting side --
    # y_idx with an asymmetric 8-bit q_out, strides >= K, unaligned y -- is covered by the GPU tests)


def test_reference_chain_is_the_header_formula_cpu():
    """tests/_skinny_twin.skinny_pre (the C oracle) == the numpy restatement of include/tq_hip.h at skinny shapes, and
    SkinnyTwin.linear_i8_skinny reads a strided first-token view like its contiguous copy"""
    from tests._skinny_twin import SkinnyTwin, skinny_reference
    for (M, N, K), per_channel in (((3, 2, 768), False), ((5, 67, 784), True), ((9, 5, 16384), True)):
        p = _problem(M, N, K, seed=M + N + K)
        z = int(np.clip(np.rint(p['x_zf']), 0, 255))
        tot = p['x'].astype(np.int64) @ p['w'].astype(np.int64).T + (128 - z) * p['w'].astype(np.int64).sum(1)[None, :]
        assert np.abs(tot).max() < 2 ** 31
        sw = np.maximum(p['wd_row'] if per_channel else p['wd_one'], np.float32(EPS)).astype(np.float32)
        pre = tot.astype(np.float32) * (np.float32(max(p['x_delta'], np.float32(EPS))) * np.broadcast_to(sw, (N,))).astype(np.float32)[None, :]
        pre = (pre + p['bias'][None, :]).astype(np.float32)
        assert np.array_equal(_ref_pre(p, per_channel, True).numpy().view(np.uint32), pre.view(np.uint32))
    be = SkinnyTwin()
    p = _problem(4, 6, 768, seed=3)
    idx = torch.from_numpy((np.random.default_rng(4).integers(0, 256, (4, 5, 768)) - 128).astype(np.int8))
    xq = (torch.tensor([0.02]), torch.tensor([127.3]), 8, EPS)
    q = _q_out(-1.0, 1.0)
    w, wd, b = torch.from_numpy(p['w']), torch.from_numpy(p['wd_row']), torch.from_numpy(p['bias'])
    a = be.linear_i8_skinny(idx[:, 0], w, None, b, xq, wd, EPS, ACT_TANH, q, torch.float32, want_idx=True)
    c = be.linear_i8_skinny(idx[:, 0].contiguous(), w, None, b, xq, wd, EPS, ACT_TANH, q, torch.float32, want_idx=True)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert [e[5] for e in be.census] == [(3840, 1), (768, 1)]
    r = skinny_reference(idx[:, 0], w, b, (0.02, 127.3, 8, EPS), wd, EPS, ACT_TANH, _q7(q))
    assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1]) and a[0].abs().max() <= 1.0 + 1e-6


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('case', list(CASES))
def test_pre_bit_exact_vs_the_oracle(case):
    """activation none, no output quantizer: per-tensor and per-channel w_delta x with and without bias x fp32 and bf16 y"""
    M, N, K = CASES[case]
    p = _problem(M, N, K, seed=M + N + K)
    for per_channel in (False, True):
        for with_bias in (False, True):
            be, x, w, rs, b, xq, wd = _device(p, per_channel, with_bias)
            ref = _ref_pre(p, per_channel, with_bias)
            y = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_NONE, None, torch.float32)
            _assert_bits(y, ref, f'{case} per_channel={per_channel} bias={with_bias}')
            yb = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_NONE, None, torch.bfloat16)
            assert torch.equal(yb.cpu(), ref.to(torch.bfloat16)), (case, per_channel, with_bias)


@gpu
@pytest.mark.parametrize('sign', ['plus', 'minus'])
def test_extreme_sums_are_exact(sign):
    """(8, 4, 16384): x = 127 everywhere with z_x = 0 ('plus') or x = -128 with z_x = 255 ('minus'), w = +-127 by column:
    |tot| ~ 5.3e8 on every output -- above 2^28, inside int32"""
    M, N, K = 8, 4, 16384
    p = _problem(M, N, K, seed=7, x_zf=0.0 if sign == 'plus' else 255.0)
    p['x'][:] = 127 if sign == 'plus' else -128
    p['w'] = (127 * np.where(np.arange(N) % 2 == 0, 1, -1)[:, None] * np.ones((1, K))).astype(np.int8)
    z = int(p['x_zf'])
    tot = p['x'].astype(np.int64) @ p['w'].astype(np.int64).T + (128 - z) * p['w'].astype(np.int64).sum(1)[None, :]
    assert np.abs(tot).min() > 2 ** 28 and np.abs(tot).max() < 2 ** 31, (np.abs(tot).min(), np.abs(tot).max())
    assert (tot > 0).any() and (tot < 0).any()
    for per_channel in (False, True):
        be, x, w, rs, b, xq, wd = _device(p, per_channel, True)
        ref = _ref_pre(p, per_channel, True)
        assert np.array_equal(ref.numpy(), (tot.astype(np.float32) * (np.float32(0.02) * (p['wd_row'] if per_channel else
                              np.broadcast_to(p['wd_one'], (N,))))[None, :].astype(np.float32) + p['bias'][None, :]).astype(np.float32))
        _assert_bits(be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_NONE, None, torch.float32), ref, sign)
        assert torch.equal(be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_NONE, None, torch.bfloat16).cpu(), ref.to(torch.bfloat16))
        nb = _ref_pre(p, per_channel, False)
        _assert_bits(be.linear_i8_skinny(x, w, rs, None, xq, wd, EPS, ACT_NONE, None, torch.float32), nb, sign + ', no bias')
        assert torch.equal(be.linear_i8_skinny(x, w, rs, None, xq, wd, EPS, ACT_NONE, None, torch.bfloat16).cpu(), nb.to(torch.bfloat16))
        q = _q_out(float(ref.min()) - 1.0, float(ref.max()) + 1.0)
        y, yi = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_NONE, _to(q, 'cuda'), torch.float32, want_idx=True)
        from tests._skinny_twin import skinny_epilogue
        ry, ri = skinny_epilogue(ref, ACT_NONE, _q7(q))
        _assert_bits(y, ry, sign)
        assert torch.equal(yi.cpu(), ri)


@gpu
@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('activation', [ACT_RELU, ACT_GELU])
def test_relu_gelu_behind_an_8_bit_quantizer(case, activation):
    """values and y_idx == the oracle's codes 1 / 4; y as fp32 and bf16; index-only (want_y=False) gives the same indices"""
    from tests._skinny_twin import skinny_epilogue
    M, N, K = CASES[case]
    p = _problem(M, N, K, seed=M + N + K + activation)
    q = _q_out(-0.2, 3.0)
    for per_channel, with_bias in ((False, True), (True, False)):
        be, x, w, rs, b, xq, wd = _device(p, per_channel, with_bias)
        ry, ri = skinny_epilogue(_ref_pre(p, per_channel, with_bias), activation, _q7(q))
        y, yi = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, activation, _to(q, 'cuda'), torch.float32, want_idx=True)
        _assert_bits(y, ry, f'{case} act={activation}')
        assert torch.equal(yi.cpu(), ri)
        yb, yib = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, activation, _to(q, 'cuda'), torch.bfloat16, want_idx=True)
        assert torch.equal(yb.cpu(), ry.to(torch.bfloat16)) and torch.equal(yib.cpu(), ri)
        none, only = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, activation, _to(q, 'cuda'), torch.float32, want_idx=True,
                                         want_y=False)
        assert none is None and torch.equal(only.cpu(), ri)
        plain = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, activation, _to(q, 'cuda'), torch.float32)
        _assert_bits(plain, ry, f'{case} act={activation} without y_idx')


@gpu
@pytest.mark.parametrize('kind', ['symmetric 8-bit', 'asymmetric 16-bit'])
def test_other_output_quantizers_values_only(kind):
    from quantization import _hip
    from tests._skinny_twin import skinny_epilogue
    M, N, K = CASES['ragged K']
    p = _problem(M, N, K, seed=21)
    q = _q_out(hi=3.0, symmetric=True) if kind.startswith('symmetric') else _q_out(-3.5, 3.5, n_bits=16)
    be, x, w, rs, b, xq, wd = _device(p, True, True)
    for activation in (ACT_NONE, ACT_GELU):
        ry, _ = skinny_epilogue(_ref_pre(p, True, True), activation, _q7(q))
        _assert_bits(be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, activation, _to(q, 'cuda'), torch.float32), ry, kind)
    with pytest.raises(_hip.TQError, match='y_idx needs an asymmetric <= 8-bit output quantizer'):
        be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_NONE, _to(q, 'cuda'), torch.float32, want_idx=True)


@gpu
@pytest.mark.parametrize('shape', TANH_SHAPES)
def test_tanh_is_the_float64_tanh_narrowed_once(shape):
    """reference: np.tanh(pre as float64) as float32 on the oracle's pre, then the oracle's quantizer on [-1, 1], 8 bits.
    Premise, asserted on the CPU reference: std(pre) in [0.8, 1.3] and >= 90 % of the indices strictly inside the grid."""
    from oracle import int_oracle
    M, N, K = shape
    p = _problem(M, N, K, seed=TANH_SEEDS[shape], x_zf=127.3)
    q = _q_out(-1.0, 1.0)
    pre = _ref_pre(p, False, True)
    t = torch.from_numpy(np.tanh(pre.numpy().astype(np.float64)).astype(np.float32))
    ry, ri = int_oracle.epilogue(t, 0, _q7(q))
    std, inside = float(pre.std()), float(((ri.int() > -128) & (ri.int() < 127)).float().mean())
    print(f'tanh {shape}: std(pre) {std:.3f}, {100 * inside:.1f} % of the indices strictly inside the grid')
    assert 0.8 <= std <= 1.3 and inside >= 0.9, (std, inside)
    be, x, w, rs, b, xq, wd = _device(p, False, True)
    y, yi = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_TANH, _to(q, 'cuda'), torch.float32, want_idx=True)
    _assert_bits(y, ry, f'tanh {shape}')
    assert torch.equal(yi.cpu(), ri)
    _assert_bits(be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_TANH, None, torch.float32), t, f'tanh {shape}, no quantizer')


@gpu
def test_strided_first_token_view_equals_its_contiguous_copy():
    """indices [4, 5, 768] on the device, x_idx = idx[:, 0] (row stride 3840) read in place"""
    p = _problem(4, 67, 768, seed=11)
    be, _, w, rs, b, xq, wd = _device(p)
    idx = torch.from_numpy((np.random.default_rng(12).integers(0, 256, (4, 5, 768)) - 128).astype(np.int8)).cuda()
    view = idx[:, 0]
    assert view.stride() == (3840, 1) and not view.is_contiguous() and view.data_ptr() == idx.data_ptr()
    q = _to(_q_out(-1.0, 1.0), 'cuda')
    for act in (ACT_NONE, ACT_TANH):
        a = be.linear_i8_skinny(view, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        c = be.linear_i8_skinny(view.contiguous(), w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    p['x'] = view.cpu().numpy()
    _assert_bits(be.linear_i8_skinny(view, w, rs, b, xq, wd, EPS, ACT_NONE, None, torch.float32), _ref_pre(p, True, True), 'strided')


@gpu
@pytest.mark.parametrize('shape', [(64, 64, 128), (32, 96, 192)])
def test_equals_the_tiled_kernels_where_both_take_the_shape(shape):
    """none and ReLU: bit-identical to linear_i8 without a table (with and without an 8-bit output quantizer, indices too);
    GELU: bit-identical to linear_i8 with a staircase table whose header says ok"""
    from tests._exact_backend import stair_header_ok
    M, N, K = shape
    p = _problem(M, N, K, seed=M + K)
    be, x, w, rs, b, xq, wd = _device(p, True, True)
    q = _to(_q_out(-0.2, 3.0), 'cuda')
    for act in (ACT_NONE, ACT_RELU):
        assert torch.equal(be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, act, None, torch.float32).view(torch.int32),
                           be.linear_i8(x, w, rs, b, xq, wd, EPS, act, None, torch.float32).view(torch.int32))
        a = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        t = be.linear_i8(x, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        assert torch.equal(a[0].view(torch.int32), t[0].view(torch.int32)) and torch.equal(a[1], t[1])
    stair = be.act_stair(ACT_GELU, q, be.stair_bins_for(M, N))
    assert stair_header_ok(stair[0]), 'the builder declined the table: pick a coarser output grid'
    a = be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, ACT_GELU, q, torch.float32, want_idx=True)
    t = be.linear_i8(x, w, rs, b, xq, wd, EPS, ACT_GELU, q, torch.float32, want_idx=True, stair=stair)
    assert torch.equal(a[0].view(torch.int32), t[0].view(torch.int32)) and torch.equal(a[1], t[1])


@gpu
@pytest.mark.parametrize('N', [2, 3, 67])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_nothing_is_written_outside_the_outputs(N, dtype):
    """through the C entry into sentinel-filled buffers: y and y_idx start 3 elements into theirs (rows of N = 2, 3, 67 are
    not 16-byte aligned anyway) and end 4096 elements before the buffers do; only M * N elements change"""
    from quantization import _hip
    from tests._skinny_twin import skinny_epilogue
    M, K, front, back = 11, 784, 3, 4096
    p = _problem(M, N, K, seed=N)
    be, x, w, rs, b, xq, wd = _device(p, True, True)
    q = _q_out(-0.2, 3.0, dev='cuda')
    ybuf = torch.full((front + M * N + back,), -1.5, dtype=dtype, device='cuda')
    ibuf = torch.full((front + M * N + back,), 90, dtype=torch.int8, device='cuda')
    qd = be._qdesc(*q, 1, 1)
    rc = be.lib.tq_linear_i8_skinny_fwd(
        x.data_ptr(), 0, w.data_ptr(), rs.data_ptr(), b.data_ptr(), ybuf.data_ptr() + front * ybuf.element_size(),
        ibuf.data_ptr() + front, _hip._DTYPES[dtype], M, N, K, xq[0].data_ptr(), xq[1].data_ptr(), 8, EPS, wd.data_ptr(), N, EPS,
        ACT_RELU, C.byref(qd), _hip._stream())
    _hip._check(rc, be.lib)
    torch.cuda.synchronize()
    ry, ri = skinny_epilogue(_ref_pre(p, True, True), ACT_RELU, _q7(q))
    yh, ih = ybuf.cpu(), ibuf.cpu()
    assert torch.equal(yh[front:front + M * N].reshape(M, N), ry.to(dtype)) and torch.equal(ih[front:front + M * N].reshape(M, N), ri)
    assert (yh[:front] == -1.5).all() and (yh[front + M * N:] == -1.5).all(), 'y written outside its M * N elements'
    assert (ih[:front] == 90).all() and (ih[front + M * N:] == 90).all(), 'y_idx written outside its M * N elements'
