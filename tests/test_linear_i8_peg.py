"""Integer Linear with a per-embedding-group (PEG) input grid: tq_linear_i8_cls_fwd.

The input quantizer has per-column buffers that take C distinct (delta, zero_float) pairs (classes); x and W are handed
over with their columns in class order.  Per output the kernel sums exact int32 class contractions, converts each with
its class scale and adds them in class order in fp32 (include/tq_hip.h).  Bars: bit-exact against a numpy restatement
of that formula; C = 1 bit-identical to tq_linear_i8_fwd; pre-quantizer outputs within 1e-5 of the row scale of the
reference's fp32 simulation F.linear(Q(x), Q(W), b); index-only / staircase outputs equal the full call's indices."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-8


def _classes(K, n_cls, permuted, rng):
    """class of every natural-order column: contiguous runs, or the same sizes scattered over the columns"""
    cls_of_col = np.repeat(np.arange(n_cls), K // n_cls)
    if permuted:
        cls_of_col = rng.permutation(cls_of_col)
    # class numbering = order of first appearance (the order quantization/peg.py uses)
    _, first = np.unique(cls_of_col, return_index=True)
    relabel = np.empty(n_cls, dtype=np.int64)
    relabel[np.argsort(first)] = np.arange(n_cls)
    return relabel[cls_of_col]


def _problem(M, N, K, n_cls, permuted, per_channel, n_bits, seed):
    rng = np.random.default_rng(seed)
    cls_of_col = _classes(K, n_cls, permuted, rng)
    top = 2 ** n_bits - 1
    dc = (rng.uniform(0.01, 0.2, n_cls)).astype(np.float32)
    zc = rng.uniform(0, top, n_cls).astype(np.float32)
    x_delta, x_zf = dc[cls_of_col], zc[cls_of_col]
    x_u = rng.integers(0, top + 1, (M, K))
    x_nat = (x_u - 128).astype(np.int8)
    wmax = 2 ** (n_bits - 1) - 1
    w_nat = rng.integers(-wmax, wmax + 1, (N, K)).astype(np.int8)
    w_delta = rng.uniform(0.001, 0.01, N if per_channel else 1).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    order = np.argsort(cls_of_col, kind='stable')
    sizes = np.bincount(cls_of_col)
    ends = np.cumsum(sizes)
    reps = np.array([np.flatnonzero(cls_of_col == c)[0] for c in range(n_cls)])
    return dict(cls_of_col=cls_of_col, x_delta=x_delta, x_zf=x_zf, x_nat=x_nat, w_nat=w_nat, w_delta=w_delta, bias=bias,
                order=order, ends=ends, reps=reps, n_bits=n_bits)


def _numpy_pre(p):
    """the formula of include/tq_hip.h on the class-ordered operands (tests/_exact_backend.py: the whole-model CPU twin of
    the HIP backend evaluates the same function)"""
    from tests._exact_backend import cls_pre
    order = p['order']
    return cls_pre(p['x_nat'][:, order], p['w_nat'][:, order], p['ends'], p['reps'], p['x_delta'], p['x_zf'], p['n_bits'], EPS,
                   p['w_delta'], EPS, p['bias'])


def _device_operands(be, p):
    dev = 'cuda'
    order = p['order']
    x_c = torch.from_numpy(np.ascontiguousarray(p['x_nat'][:, order])).to(dev)
    w_c = torch.from_numpy(np.ascontiguousarray(p['w_nat'][:, order])).to(dev)
    starts = np.concatenate([[0], p['ends'][:-1]])
    rs = torch.stack([be.rowsum_i8(w_c[:, s:e].contiguous()) for s, e in zip(starts, p['ends'])]).contiguous()
    xq = (torch.from_numpy(p['x_delta']).to(dev), torch.from_numpy(p['x_zf']).to(dev), p['n_bits'], EPS)
    table = be.cls_table(p['ends'], p['reps'])
    return x_c, w_c, rs, torch.from_numpy(p['bias']).to(dev), xq, table, torch.from_numpy(p['w_delta']).to(dev)


def _q_out(dev='cuda', lo=-0.3, hi=2.5, n_bits=8):
    top = 2 ** n_bits - 1
    delta = torch.tensor([(hi - lo) / top], dtype=torch.float32, device=dev)
    zf = torch.tensor([-lo / ((hi - lo) / top)], dtype=torch.float32, device=dev)
    return (delta, zf, None, n_bits, False, False, EPS)


@pytest.mark.parametrize('shape', [(1024, 3072, 768), (1024, 768, 768), (256, 128, 3072)])
@pytest.mark.parametrize('n_cls', [1, 2, 6])
@pytest.mark.parametrize('permuted', [False, True])
@pytest.mark.parametrize('cfg', [(8, False), (8, True), (4, True)])
def test_cls_kernel_bit_exact_vs_numpy(shape, n_cls, permuted, cfg):
    from quantization import _hip
    be = _hip.backend()
    M, N, K = shape
    n_bits, per_channel = cfg
    p = _problem(M, N, K, n_cls, permuted, per_channel, n_bits, seed=M + N + K + n_cls + 7 * permuted + n_bits)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    y = be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_NONE, None, torch.float32)
    ref = _numpy_pre(p)
    got = y.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
        f'{np.count_nonzero(got != ref)} of {got.size} outputs differ (max {np.abs(got - ref).max()})'


@pytest.mark.parametrize('shape', [(16384, 3072, 768), (4096, 768, 3072)])
def test_cls_kernel_bit_exact_vs_numpy_128_tiles(shape):
    """128 x 128 block tiles (the tile rule's large side)"""
    from quantization import _hip
    be = _hip.backend()
    M, N, K = shape
    p = _problem(M, N, K, 6, True, True, 8, seed=11)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    y = be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_NONE, None, torch.float32)
    ref = _numpy_pre(p)
    got = y.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize('shape', [(1024, 3072, 768), (16384, 3072, 768), (1024, 768, 768), (1024, 768, 3072)])
@pytest.mark.parametrize('act', ['none', 'gelu'])
@pytest.mark.parametrize('per_channel', [False, True])
def test_one_class_equals_tq_linear_i8_fwd(shape, act, per_channel):
    from quantization import _hip
    be = _hip.backend()
    M, N, K = shape
    p = _problem(M, N, K, 1, False, per_channel, 8, seed=M + K)
    dev = 'cuda'
    x = torch.from_numpy(p['x_nat']).to(dev)
    w = torch.from_numpy(p['w_nat']).to(dev)
    rs = be.rowsum_i8(w)
    b = torch.from_numpy(p['bias']).to(dev)
    wd = torch.from_numpy(p['w_delta']).to(dev)
    xq1 = (torch.from_numpy(p['x_delta'][:1].copy()).to(dev), torch.from_numpy(p['x_zf'][:1].copy()).to(dev), 8, EPS)
    table = be.cls_table([K], [0])
    code = _hip.ACT_GELU if act == 'gelu' else _hip.ACT_NONE
    q = _q_out() if act == 'gelu' else None
    want_idx = q is not None
    ref = be.linear_i8(x, w, rs, b, xq1, wd, EPS, code, q, torch.float32, want_idx=want_idx)
    got = be.linear_i8_cls(x, w, rs.reshape(1, -1).contiguous(), b, xq1, table, wd, EPS, code, q, torch.float32,
                           want_idx=want_idx)
    if want_idx:
        assert torch.equal(got[1], ref[1])
        got, ref = got[0], ref[0]
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    # the same per-column (one class spread over every column of a per-column buffer)
    xqd = (torch.from_numpy(p['x_delta']).to(dev), torch.from_numpy(p['x_zf']).to(dev), 8, EPS)
    got2 = be.linear_i8_cls(x, w, rs.reshape(1, -1).contiguous(), b, xqd, be.cls_table([K], [K // 2]), wd, EPS, code, q,
                            torch.float32)
    assert torch.equal(got2.view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize('shape', [(1024, 3072, 768), (1024, 768, 3072), (16384, 3072, 768)])
@pytest.mark.parametrize('n_bits', [8, 4])
def test_pre_quantizer_output_vs_fp32_simulation(shape, n_bits):
    from quantization import _hip
    be = _hip.backend()
    M, N, K = shape
    if M > 4096:
        M = 4096                                              # (the CPU simulation; the 128-tile case is bit-tested above)
    p = _problem(M, N, K, 6, True, True, n_bits, seed=3 + n_bits)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    y = be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_NONE, None, torch.float32).cpu()
    z = np.clip(np.rint(p['x_zf']), 0, 2 ** n_bits - 1).astype(np.float32)
    xq_f = torch.from_numpy(((p['x_nat'].astype(np.float32) + 128 - z[None, :]) * p['x_delta'][None, :]).astype(np.float32))
    wq_f = torch.from_numpy((p['w_nat'].astype(np.float32) * p['w_delta'].reshape(-1, 1)).astype(np.float32))
    sim = torch.nn.functional.linear(xq_f, wq_f, torch.from_numpy(p['bias']))
    scale = (xq_f.abs() @ wq_f.abs().T).amax(1, keepdim=True) + 1e-12
    assert float(((y - sim).abs() / scale).max()) <= 1e-5


@pytest.mark.parametrize('shape', [(1024, 3072, 768), (16384, 3072, 768)])
@pytest.mark.parametrize('stair', [False, True])
def test_index_only_and_staircase_give_the_full_calls_indices(shape, stair):
    from quantization import _hip
    be = _hip.backend()
    M, N, K = shape
    p = _problem(M, N, K, 6, True, True, 8, seed=5)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    q = _q_out(lo=-0.2, hi=3.0)
    tab = be.act_stair(_hip.ACT_GELU, q, be.STAIR_BINS) if stair else None
    _, full_i = be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True,
                                      stair=tab)
    _, only_i = be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True,
                                 want_y=False, stair=tab)
    assert torch.equal(full_i, only_i)
    if stair:                                                 # staircase vs arithmetic epilogue: the table's own contract
        _, ar_i = be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True)
        d = (ar_i.int() - full_i.int()).abs()
        assert int(d.max()) <= 1 and int((d > 0).sum()) <= max(1, full_i.numel() // 10000)


def _raw_call(be, x_c, w_c, rs, b, y, xq, table, wd, M, N, K, x_n_params=None):
    from quantization._hip import _ptr
    return be.lib.tq_linear_i8_cls_fwd(_ptr(x_c), _ptr(w_c), _ptr(rs), _ptr(b), _ptr(y), None, 0, M, N, K, _ptr(xq[0]),
                                       _ptr(xq[1]), xq[0].numel() if x_n_params is None else x_n_params, 8, EPS,
                                       C.byref(table), _ptr(wd), wd.numel(), EPS, 0, None, None, 0, None)


def test_unsupported_layouts_are_rejected():
    from quantization import _hip
    be = _hip.backend()
    M, N, K = 128, 128, 768
    p = _problem(M, N, K, 6, True, False, 8, seed=1)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    y = torch.empty(M, N, device='cuda')
    assert _raw_call(be, x_c, w_c, rs, b, y, xq, table, wd, M, N, K) == 0
    bad_tables = [
        be.cls_table([100, 768], [0, 1]),                     # class size not a multiple of 128
        be.cls_table([256, 512], [0, 1]),                     # classes do not cover K
        be.cls_table([512, 256, 768], [0, 1, 2]),             # not increasing
        be.cls_table([768], [768]),                           # representative column outside the buffers
        be.cls_table([], []),                                 # no class
    ]
    for t in bad_tables:
        assert _raw_call(be, x_c, w_c, rs, b, y, xq, t, wd, M, N, K) == -1           # TQ_EINVAL
    t = _hip.tq_cls_table()
    t.n_classes = _hip.CLS_MAX + 1
    assert _raw_call(be, x_c, w_c, rs, b, y, xq, t, wd, M, N, K) == -1
    # shapes the LDS-tiled kernels do not take
    assert _raw_call(be, x_c, w_c, rs, b, y, xq, table, wd, 96, N, K) == -1
    assert _raw_call(be, x_c, w_c, rs, b, y, xq, be.cls_table([640], [0]), wd, M, N, 640 - 64) == -1
    with pytest.raises(_hip.TQError):
        be.linear_i8_cls(x_c, w_c, rs, b, xq, bad_tables[0], wd, EPS, _hip.ACT_NONE, None, torch.float32)


@pytest.mark.parametrize('shape,n_cls', [((16384, 3072, 768), 6), ((16384, 3072, 3072), 24), ((1024, 3072, 3072), 24)])
def test_staircase_sized_by_the_cls_rule_is_taken_and_oversized_is_refused(shape, n_cls):
    """The class-ordered launcher refuses a table that does not fit beside the class row sums (it is never dropped
    silently); `cls_stair_bins_for` asks the library for the size that rule allows, and the table it sizes is accepted."""
    from quantization import _hip
    be = _hip.backend()
    M, N, K = shape
    p = _problem(M, N, K, n_cls, True, True, 8, seed=9)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    q = _q_out(lo=-0.2, hi=3.0)
    bins = be.cls_stair_bins_for(M, N, K, n_cls)
    if bins is not None:
        tab = be.act_stair(_hip.ACT_GELU, q, bins)
        be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, stair=tab)
    too_big = be.act_stair(_hip.ACT_GELU, q, 2048)
    with pytest.raises(_hip.TQError):
        be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True,
                         stair=too_big)
