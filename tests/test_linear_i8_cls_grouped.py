"""tq_linear_i8_cls_grouped_fwd: the class-ordered integer Linear (per-embedding-group input grid) for up to three Linears
stacked along N, each with an output grid of its own -- per-tensor, or per-column buffers over the group's columns that are
constant over every aligned block of `q_block` columns (BERT's query | key | value under --per-groups: include/tq_hip.h).

Contract: the arithmetic is tq_linear_i8_cls_fwd's up to `pre`; a tile then applies the parameters found at the first column of
its block.  Every case is held, bit for bit, to
  (a) tq_linear_i8_cls_fwd with q_out = NULL followed by the existing per-column fake-quant / quantize_to_int8 launch on its
      output with the same buffers (per-tensor groups expanded over their columns), and
  (b) the numpy formula: tests/_exact_backend.cls_pre, then oracle_epilogue block by block.
Main shape: M = 64 and 128, K = 256 in two classes of 128, three groups of 256 columns, q_block = 128 -- two blocks per group,
so a wrong block index shows; group 0 per-column, group 1 per-tensor, group 2 per-column with zero points at both ends of the
grid."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._exact_backend import cls_pre, oracle_epilogue
from tests.test_linear_i8_peg import EPS, _device_operands, _problem

DEV = 'cuda'


def _blocks(gc, q_block, pairs):
    """per-column buffers [gc]: pairs[j] = (delta, zero_float) of block j"""
    assert len(pairs) * q_block == gc
    d = np.repeat(np.array([p[0] for p in pairs], np.float32), q_block)
    z = np.repeat(np.array([p[1] for p in pairs], np.float32), q_block)
    return d, z


def _groups(gc, q_block, seed, n_groups=3):
    """host description of the output grids: per group ('col', delta[gc], zf[gc]) or ('one', delta, zf).  Group 0 per-column,
    group 1 per-tensor, group 2 per-column with zero points 0 and 255 in its first two blocks.  Steps of 1.5 .. 3: the
    pre-activations of tests/test_linear_i8_peg.py's problems have a standard deviation of 90 .. 140 (numpy formula, K = 256
    and 512), so most indices lie inside the grids (asserted where it matters)"""
    rng = np.random.default_rng(seed)
    nb = gc // q_block
    pair = lambda: (float(rng.uniform(1.5, 3.0)), float(rng.uniform(90, 160)))
    ends = [(2.0, 0.0), (2.5, 255.0)] + [pair() for _ in range(max(nb - 2, 0))]
    out = [('col',) + _blocks(gc, q_block, [pair() for _ in range(nb)]), ('one',) + pair(), ('col',) + _blocks(gc, q_block, ends[:nb])]
    return out[:n_groups]


def _q7(g):
    """backend 7-tuple of a group's grid, on the device"""
    t = lambda v: torch.from_numpy(np.atleast_1d(np.asarray(v, np.float32))).to(DEV)
    return (t(g[1]), t(g[2]), None, 8, False, False, EPS)


def _columns(groups, gc):
    """(delta[N], zf[N]): every group's grid over its columns"""
    d = np.concatenate([np.broadcast_to(np.asarray(g[1], np.float32), (gc,)) for g in groups])
    z = np.concatenate([np.broadcast_to(np.asarray(g[2], np.float32), (gc,)) for g in groups])
    return np.ascontiguousarray(d), np.ascontiguousarray(z)


def _numpy_reference(p, groups, gc, q_block, activation, with_bias=True):
    order = p['order']
    pre = cls_pre(p['x_nat'][:, order], p['w_nat'][:, order], p['ends'], p['reps'], p['x_delta'], p['x_zf'], p['n_bits'], EPS,
                  p['w_delta'], EPS, p['bias'] if with_bias else None)
    d, z = _columns(groups, gc)
    y, yi = np.empty_like(pre), np.empty(pre.shape, np.int8)
    for c0 in range(0, pre.shape[1], q_block):
        assert (d[c0:c0 + q_block] == d[c0]).all() and (z[c0:c0 + q_block] == z[c0]).all()
        by, bi = oracle_epilogue(np.ascontiguousarray(pre[:, c0:c0 + q_block]), activation,
                                 (float(d[c0]), float(z[c0]), None, 8, False, False, EPS))
        y[:, c0:c0 + q_block], yi[:, c0:c0 + q_block] = by.numpy(), bi.numpy()
    return y, yi


def _kernel_reference(be, ops, groups, gc, activation, with_bias=True):
    """(a): the class-ordered Linear without an output quantizer, then the per-column quantizer launches on its output"""
    x_c, w_c, rs, b, xq, table, wd = ops
    pre = be.linear_i8_cls(x_c, w_c, rs, b if with_bias else None, xq, table, wd, EPS, activation, None, torch.float32)
    d, z = _columns(groups, gc)
    N = d.size
    dd, zd = torch.from_numpy(d).to(DEV), torch.from_numpy(z).to(DEV)
    y, _ = be.fake_quant(pre, dd, zd, None, 8, False, False, EPS, N, 1)
    yi = be.quantize_to_int8(pre, dd, zd, None, 8, False, False, EPS, N, 1, True)
    return y.cpu().numpy(), yi.cpu().numpy()


def _assert_same(got_y, got_i, ref, what):
    ry, ri = ref
    if got_i is not None:
        gi = got_i.cpu().numpy()
        assert np.array_equal(gi, ri), f'{what}: {np.count_nonzero(gi != ri)} of {ri.size} indices differ'
    if got_y is not None:
        gy = got_y.cpu().numpy()
        assert np.array_equal(gy.view(np.uint32), ry.view(np.uint32)), f'{what}: {np.count_nonzero(gy != ry)} of {ry.size} values differ'


@pytest.mark.gpu
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'no-bias'])
@pytest.mark.parametrize('per_channel', [False, True], ids=['w-per-tensor', 'w-per-channel'])
@pytest.mark.parametrize('M', [64, 128])
def test_grouped_cls_linear_equals_both_references(M, per_channel, with_bias):
    from quantization import _hip
    be = _hip.backend()
    N, K, gc, q_block = 768, 256, 256, 128
    p = _problem(M, N, K, 2, False, per_channel, 8, seed=M + 3 * per_channel)
    ops = _device_operands(be, p)
    x_c, w_c, rs, b, xq, table, wd = ops
    groups = _groups(gc, q_block, seed=M)
    qs = [_q7(g) for g in groups]
    bias = b if with_bias else None
    y, yi = be.linear_i8_cls_grouped(x_c, w_c, rs, bias, xq, table, wd, EPS, _hip.ACT_NONE, qs, q_block, want_y=True)
    none, only = be.linear_i8_cls_grouped(x_c, w_c, rs, bias, xq, table, wd, EPS, _hip.ACT_NONE, qs, q_block)
    assert none is None and torch.equal(only, yi), 'the index-only launch differs from the full one'
    ref_np = _numpy_reference(p, groups, gc, q_block, _hip.ACT_NONE, with_bias)
    # the grids are live: most indices inside, both clamps reached in the blocks whose zero points sit at the grid's ends
    inside = float(((ref_np[1] > -128) & (ref_np[1] < 127)).mean())
    assert inside > 0.5 and (ref_np[1][:, 2 * gc:2 * gc + q_block] == -128).any() and (ref_np[1][:, 2 * gc + q_block:] == 127).any()
    _assert_same(y, yi, ref_np, 'numpy formula')
    _assert_same(y, yi, _kernel_reference(be, ops, groups, gc, _hip.ACT_NONE, with_bias), 'cls Linear + per-column quantizer launches')


@pytest.mark.gpu
def test_relu_and_bf16_output():
    from quantization import _hip
    be = _hip.backend()
    M, N, K, gc, q_block = 64, 768, 256, 256, 128
    p = _problem(M, N, K, 2, False, True, 8, seed=5)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    groups = _groups(gc, q_block, seed=6)
    qs = [_q7(g) for g in groups]
    y, yi = be.linear_i8_cls_grouped(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_RELU, qs, q_block, want_y=True)
    ref = _numpy_reference(p, groups, gc, q_block, _hip.ACT_RELU)
    _assert_same(y, yi, ref, 'ReLU')
    yb, yib = be.linear_i8_cls_grouped(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_RELU, qs, q_block, want_y=True,
                                       out_dtype=torch.bfloat16)
    assert torch.equal(yib, yi) and yb.dtype == torch.bfloat16 and torch.equal(yb.float(), y.to(torch.bfloat16).float())


@pytest.mark.gpu
@pytest.mark.parametrize('act', ['none', 'relu'])
def test_one_group_per_tensor_equals_the_class_ordered_linear(act):
    from quantization import _hip
    from tests.test_linear_i8_peg import _q_out
    be = _hip.backend()
    M, N, K = 128, 256, 256
    p = _problem(M, N, K, 2, True, True, 8, seed=21)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    code = _hip.ACT_NONE if act == 'none' else _hip.ACT_RELU
    q = _q_out()
    y, yi = be.linear_i8_cls_grouped(x_c, w_c, rs, b, xq, table, wd, EPS, code, [q], 128, want_y=True)
    ry, ri = be.linear_i8_cls(x_c, w_c, rs, b, xq, table, wd, EPS, code, q, torch.float32, want_idx=True)
    assert torch.equal(y, ry) and torch.equal(yi, ri)


@pytest.mark.gpu
def test_one_class_per_tensor_outputs_equal_the_grouped_linear():
    from quantization import _hip
    from tests.test_linear_i8_peg import _q_out
    be = _hip.backend()
    M, N, K = 128, 768, 256
    p = _problem(M, N, K, 1, False, True, 8, seed=22)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    qs = [_q_out(lo=-1.5, hi=1.2), _q_out(lo=-0.8, hi=2.0), _q_out(lo=-2.0, hi=0.7)]
    y, yi = be.linear_i8_cls_grouped(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_NONE, qs, 256, want_y=True)
    x_q = (xq[0][:1].contiguous(), xq[1][:1].contiguous(), xq[2], xq[3])
    ry, ri = be.linear_i8_grouped(x_c, w_c, rs[0].contiguous(), b, x_q, wd, EPS, _hip.ACT_NONE, qs, want_y=True)
    assert torch.equal(yi, ri) and torch.equal(y, ry)


def _plan_is_big(M, N, K, big_min=384):
    """csrc/tq_linear_i8.hip tile_plan, restated"""
    tiles = (M // 128) * (N // 128)
    return M % 128 == 0 and N % 128 == 0 and (tiles >= 1024 or (K >= 512 and tiles >= big_min))


@pytest.mark.gpu
def test_q_block_64_keeps_64_wide_tiles(monkeypatch):
    """two groups of 192 columns, q_block = 64 (three blocks per group: per_groups = 12 on BERT-base).  Premise: tile_plan
    alone would take 128 x 128 tiles here (the threshold lowered through the switch the launcher reads per call), and a
    128-wide tile would straddle the two groups at column 192; the launcher's rule -- q_block no multiple of 128 -> 64-wide
    tiles whatever tile_plan says -- keeps every tile inside one block."""
    from quantization import _hip
    be = _hip.backend()
    M, N, K, gc, q_block = 128, 384, 512, 192, 64
    monkeypatch.setenv('TQ_I8_BIG_MIN', '1')
    assert _plan_is_big(M, N, K, big_min=1) and q_block % 128 != 0 and gc % 128 != 0
    p = _problem(M, N, K, 4, False, True, 8, seed=31)
    ops = _device_operands(be, p)
    x_c, w_c, rs, b, xq, table, wd = ops
    groups = _groups(gc, q_block, seed=32, n_groups=3)[::2]           # both per-column
    qs = [_q7(g) for g in groups]
    y, yi = be.linear_i8_cls_grouped(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_NONE, qs, q_block, want_y=True)
    _assert_same(y, yi, _numpy_reference(p, groups, gc, q_block, _hip.ACT_NONE), 'numpy formula')
    _assert_same(y, yi, _kernel_reference(be, ops, groups, gc, _hip.ACT_NONE), 'cls Linear + per-column quantizer launches')


@pytest.mark.gpu
def test_128_tiles_over_the_whole_tensor(monkeypatch):
    """the smallest shape at which tile_plan takes 128 x 128 tiles: 384 tiles need K >= 512 (below that the rule asks for
    1024).  Three groups of 1024 columns, q_block = 128 (BERT-base's Q | K | V at per_groups = 6 has the same N); compared
    over the whole tensor"""
    from quantization import _hip
    be = _hip.backend()
    monkeypatch.delenv('TQ_I8_BIG_MIN', raising=False)
    M, N, K, gc, q_block = 2048, 3072, 512, 1024, 128
    assert _plan_is_big(M, N, K) and not _plan_is_big(M - 128, N, K) and not _plan_is_big(M, N, K - 128) and q_block % 128 == 0
    p = _problem(M, N, K, 4, False, True, 8, seed=41)
    ops = _device_operands(be, p)
    x_c, w_c, rs, b, xq, table, wd = ops
    groups = _groups(gc, q_block, seed=42)
    qs = [_q7(g) for g in groups]
    y, yi = be.linear_i8_cls_grouped(x_c, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_NONE, qs, q_block, want_y=True)
    _assert_same(y, yi, _kernel_reference(be, ops, groups, gc, _hip.ACT_NONE), 'cls Linear + per-column quantizer launches')
    _assert_same(y, yi, _numpy_reference(p, groups, gc, q_block, _hip.ACT_NONE), 'numpy formula')


@pytest.mark.gpu
def test_ragged_row_count_through_the_backend():
    """M = 65: the backend launches over 128 rows of roomy buffers; the pad rows of the operand hold arbitrary bytes and the
    65 rows equal the reference of the 65-row problem"""
    from quantization import _hip
    be = _hip.backend()
    M, N, K, gc, q_block = 65, 768, 256, 256, 128
    p = _problem(M, N, K, 2, False, True, 8, seed=51)
    x_c, w_c, rs, b, xq, table, wd = _device_operands(be, p)
    room = torch.randint(-128, 128, (128, K), dtype=torch.int8, device=DEV)
    room[:M] = x_c
    x_in = room[:M]                                         # a [65, K] view whose storage has the pad rows' room
    assert be._row_room(x_in, 128)
    groups = _groups(gc, q_block, seed=52)
    qs = [_q7(g) for g in groups]
    y, yi = be.linear_i8_cls_grouped(x_in, w_c, rs, b, xq, table, wd, EPS, _hip.ACT_NONE, qs, q_block, want_y=True)
    assert y.shape == (M, N) and yi.shape == (M, N)
    _assert_same(y, yi, _numpy_reference(p, groups, gc, q_block, _hip.ACT_NONE), 'numpy formula')


def test_argument_errors_come_before_any_device_access():
    """raw ctypes, no device (fake addresses that are never dereferenced): every refused argument is -1 with a message"""
    from quantization import _hip
    lib = _hip.load_library()
    fake = 1 << 20
    one = _hip.tq_quantizer(fake, fake, None, 8, 0, 0, 1e-8, 1, 1)
    col = lambda n, inner=1, sym=0, bits=8: _hip.tq_quantizer(fake, fake, None, bits, sym, 0, 1e-8, n, inner)

    def table(ends, reps):
        t = _hip.tq_cls_table()
        t.n_classes = len(ends)
        for c, (e, r) in enumerate(zip(ends, reps)):
            t.end[c], t.rep[c] = e, r
        return t

    def call(M=64, N=768, K=256, groups=3, qs=None, q_block=128, act=0, y=fake, y_idx=fake, cls=None, x_n_params=256, bits=8,
             w_n=1, q_null=False):
        qs = [one] * groups if qs is None else qs
        arr = (C.POINTER(_hip.tq_quantizer) * max(len(qs), 1))(*[None if q is None else C.pointer(q) for q in qs])
        cls = table([128, 256], [0, 128]) if cls is None else cls
        return lib.tq_linear_i8_cls_grouped_fwd(fake, fake, fake, None, y, y_idx, 0, M, N, K, fake, fake, x_n_params, bits, 1e-8,
                                                C.byref(cls), fake, w_n, 1e-8, act, groups,
                                                None if q_null else C.cast(arr, C.POINTER(C.POINTER(_hip.tq_quantizer))), q_block, None)

    def refused(word, **kw):
        rc = call(**kw)
        msg = lib.tq_last_error().decode()
        assert rc == -1 and msg.startswith('tq_linear_i8_cls_grouped_fwd:') and word in msg, (kw, rc, msg)
    assert call(M=0) == 0 and call(N=0) == 0                              # empty problems: no launch, no checks
    refused('groups', groups=0)
    refused('groups', groups=4, qs=[one] * 4)
    refused('groups', N=704, groups=3)                                    # N % 3
    refused('groups', N=96 * 3, groups=3)                                 # groups of 96 columns
    refused('q_block', q_block=0)
    refused('q_block', q_block=96)
    refused('q_block', q_block=192)                                       # does not divide 256
    refused('q_block', q_block=512)
    refused('activation', act=2)                                          # GELU
    refused('activation', act=3)                                          # tanh
    refused('NULL', q_null=True)
    refused('NULL', y=None, y_idx=None)
    refused('shape', M=96)
    refused('shape', K=192, cls=table([128, 192], [0, 128]))
    refused('bits', bits=9)
    refused('weight scales', w_n=5)
    refused('classes', cls=table([], []))
    refused('class 1', cls=table([128, 128], [0, 128]))
    refused('representative', cls=table([128, 256], [0, 256]))
    refused('cover', cls=table([128], [0]))
    refused('every group', qs=[one, None, one])
    refused('n_params', qs=[one, col(128), one])                          # neither 1 nor the group's 256 columns
    refused('n_params', qs=[col(768), one, one])                          # the whole N
    refused('n_params', qs=[one, one, col(256, inner=2)])
    refused('y_idx', qs=[one, col(256, sym=1), one])                      # indices of a symmetric grid
    refused('y_idx', qs=[one, col(256, bits=9), one])
