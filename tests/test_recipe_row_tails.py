"""Row tails of the class-ordered and the 16-bit integer Linear (HipBackend.PADS_RECIPE_ROWS; options.INT8_RAGGED_RECIPES): rows
of a Linear are independent, so `linear_i8_cls` and `linear_i16x8` launch a row count that is no multiple of 64 over
M_pad = 64 * ceil(M / 64) rows of buffers that have the room, and the first M rows are exact.  Neither kernel nor C entry
changed: what is tested is the binding's allocation and launch logic --

* rows [:M] bit-equal to the same binding on the operand padded by the caller with RANDOM rows (whatever the pad rows hold does
  not reach the first M), and to the CPU formulas of tests/_exact_backend.py (cls_pre, i16x8_tot, i16x8_pre, oracle_epilogue);
* outputs are [:M] views over storage with room for M_pad rows; an operand with that room is read in place, an exact-sized one
  is copied once and left untouched;
* `quantize_hilo` allocates roomy planes only while options.INT8_RAGGED is on.

Shapes: (K, N) = (128, 64) without quantizer, and BERT's FFN1 (768, 3072) with GELU + staircase, index-only (the route's form);
M = 1, 63, 65 (one row, one short of / one past a tile), 150 (three tiles, [3,50])."""
import numpy as np
import pytest
import torch

from tests import test_linear_i16x8 as X16
from tests import test_linear_i8_peg as PEG

pytestmark = pytest.mark.gpu
EPS = 1e-8
ROWS = [1, 63, 65, 150]
FORMS = [(128, 64, 'plain'), (768, 3072, 'gelu-stair')]
ENTRY = {'cls': 'tq_linear_i8_cls_fwd', 'i16x8': 'tq_linear_i16x8_fwd'}


def _m_pad(M):
    return -(-M // 64) * 64


class _Spy:
    """the backend's library handle with one entry point recorded: the arguments of every call"""

    def __init__(self, lib, name):
        self._lib, self._name, self.calls = lib, name, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._name:
            return fn

        def recorded(*a):
            self.calls.append(a)
            return fn(*a)
        return recorded


def _spied(be, name, call):
    spy, lib = _Spy(be.lib, name), be.lib
    be.lib = spy
    try:
        out = call()
    finally:
        be.lib = lib
    torch.cuda.synchronize()
    return out, spy.calls


def _launched(kernel, call):
    """(pointers of the row operands, M) of a recorded call of the kernel's entry"""
    return (call[:1], call[7]) if kernel == 'cls' else (call[:2], call[8])


def _random_rows(t, M_pad, seed):
    """t int8 [M, K] on the device -> [M_pad, K] with random bytes in the pad rows"""
    g = torch.Generator().manual_seed(seed)
    pad = torch.randint(-128, 128, (M_pad - t.shape[0], t.shape[1]), generator=g).to(torch.int8)
    return torch.cat([t, pad.to(t.device)]).contiguous()


def _case(kernel, M, K, N, form):
    """-> (row operands on the device, call(row operands) -> output, reference of the M rows, M the launch covers)"""
    from quantization import _hip
    from tests._exact_backend import oracle_epilogue, stair_header_ok
    be = _hip.backend()
    gelu = form == 'gelu-stair'
    M_pad = _m_pad(M)
    if kernel == 'cls':
        p = PEG._problem(M, N, K, 6 if K == 768 else 1, K == 768, True, 8, seed=M + N + K)
        if gelu:                                                 # pre-activations ~ N(0, 1.5^2): GELU's curved part
            p['x_delta'] = (p['x_delta'] * np.float32(1.5 / PEG._numpy_pre(p).std())).astype(np.float32)
        pre = PEG._numpy_pre(p)
        x_c, w_c, rs, b, xq, table, wd = PEG._device_operands(be, p)
        rows, n_cls = (x_c,), len(p['ends'])
        bins = be.cls_stair_bins_for(M_pad, N, K, n_cls)
        run = lambda r, **kw: be.linear_i8_cls(r[0], w_c, rs, b, xq, table, wd, EPS, *kw.pop('tail'), torch.float32, **kw)
    else:
        p = X16._problem(M, N, K, 16, seed=M + N + K)
        tot = X16._numpy_tot(p)
        if gelu:
            p['x_delta'] = np.float32(1.5 / (tot.std() * p['wd_row'].mean()))
        pre = X16._numpy_pre(p, tot, True, True)
        _, hi, lo, w, rs, b, xq, wd = X16._device(p)
        rows = (hi, lo)
        bins = be.i16x8_stair_bins_for(M_pad, N, K)
        run = lambda r, **kw: be.linear_i16x8(r[0], r[1], w, rs, b, xq, wd, EPS, *kw.pop('tail'), torch.float32, **kw)
    if not gelu:
        return be, rows, (lambda r: run(r, tail=(_hip.ACT_NONE, None))), torch.from_numpy(pre), M_pad
    q = X16._q_out(lo=-0.2, hi=3.2)           # a grid the 768-bin table holds (tests/test_linear_i16x8.py)
    assert bins in (be.STAIR_BINS, be.STAIR_BINS_BIG)
    tab = be.act_stair(_hip.ACT_GELU, q, bins)
    assert stair_header_ok(tab[0]), 'the table must be exact for this grid, or the case is vacuous'
    ref = oracle_epilogue(pre, 4, tuple(t.cpu() if torch.is_tensor(t) else t for t in q))[1]      # an accepted table: code 4
    call = lambda r: run(r, tail=(_hip.ACT_GELU, q), want_idx=True, want_y=False, stair=tab)[1]
    return be, rows, call, ref, M_pad


@pytest.mark.parametrize('K,N,form', FORMS, ids=[f[2] for f in FORMS])
@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('kernel', ['cls', 'i16x8'])
def test_row_tails(kernel, M, K, N, form):
    be, rows, call, ref, M_pad = _case(kernel, M, K, N, form)
    assert be.PADS_RECIPE_ROWS is True
    before = [r.clone() for r in rows]
    assert all(r.untyped_storage().nbytes() == M * K and not be._row_room(r, M_pad) for r in rows)
    out, calls = _spied(be, ENTRY[kernel], lambda: call(rows))
    # one launch over M_pad rows of buffers with that room: the exact-sized operands were copied, once, and left untouched
    assert len(calls) == 1
    ptrs, launched = _launched(kernel, calls[0])
    assert launched == M_pad and all(p != r.data_ptr() for p, r in zip(ptrs, rows))
    assert all(torch.equal(r, b) for r, b in zip(rows, before))
    # the output: a [:M] view over storage with room for M_pad rows
    assert out.shape == (M, N) and out.is_contiguous() and out.storage_offset() == 0
    assert out.untyped_storage().nbytes() == M_pad * N * out.element_size()
    # rows [:M] == the CPU formula
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
    assert same(out.cpu(), ref), f'{int((out.cpu() != ref).sum())} of {ref.numel()} outputs differ from the CPU formula'
    # ... == the same binding on the operand padded by the caller with random rows (a whole-tile launch, as ever)
    big_rows = tuple(_random_rows(r, M_pad, seed=11 + i) for i, r in enumerate(rows))
    big, calls = _spied(be, ENTRY[kernel], lambda: call(big_rows))
    ptrs, launched = _launched(kernel, calls[0])
    assert launched == M_pad and list(ptrs) == [r.data_ptr() for r in big_rows]
    assert big.shape == (M_pad, N) and big.untyped_storage().nbytes() == M_pad * N * big.element_size()
    assert same(out, big[:M])


@pytest.mark.parametrize('kernel', ['cls', 'i16x8'])
def test_a_roomy_operand_is_used_in_place(kernel):
    """operands from the backend's own allocator (`_rows_empty`: what every producer of the route hands on while
    options.INT8_RAGGED is on) are read where they are"""
    M, K, N = 150, 128, 64
    be, rows, call, ref, M_pad = _case(kernel, M, K, N, 'plain')
    roomy = []
    for r in rows:
        t = be._rows_empty((M, K), torch.int8, r.device, force=True)
        t.copy_(r)
        assert be._row_room(t, M_pad) and t.untyped_storage().nbytes() == M_pad * K
        roomy.append(t)
    out, calls = _spied(be, ENTRY[kernel], lambda: call(tuple(roomy)))
    ptrs, launched = _launched(kernel, calls[0])
    assert len(calls) == 1 and launched == M_pad and list(ptrs) == [t.data_ptr() for t in roomy]
    assert torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32))


def test_whole_tiles_allocate_and_launch_as_before():
    for kernel in ('cls', 'i16x8'):
        M, K, N = 128, 128, 64
        be, rows, call, ref, M_pad = _case(kernel, M, K, N, 'plain')
        out, calls = _spied(be, ENTRY[kernel], lambda: call(rows))
        ptrs, launched = _launched(kernel, calls[0])
        assert launched == M == M_pad and list(ptrs) == [r.data_ptr() for r in rows]
        assert out.untyped_storage().nbytes() == M * N * 4 and torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize('M', [150, 128])
def test_quantize_hilo_planes_are_roomy_only_with_the_ragged_switch(M, monkeypatch):
    from quantization import _hip, options
    be = _hip.backend()
    K = 128
    assert options.INT8_RAGGED is False
    q4 = (torch.tensor([3.1e-4], device='cuda'), torch.tensor([0.37 * 65535], device='cuda'), 16, EPS)
    x = ((torch.rand(M, K, generator=torch.Generator().manual_seed(M)) * 1.2 - 0.1) * 65535 - 0.37 * 65535) * 3.1e-4
    x = x.cuda()
    hi, lo = be.quantize_hilo(x, q4)
    assert [t.untyped_storage().nbytes() for t in (hi, lo)] == [M * K] * 2          # exactly their own storage
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    rhi, rlo = be.quantize_hilo(x, q4)
    assert [t.untyped_storage().nbytes() for t in (rhi, rlo)] == [_m_pad(M) * K] * 2
    assert all(t.shape == (M, K) and be._row_room(t, _m_pad(M)) for t in (rhi, rlo))
    assert torch.equal(rhi, hi) and torch.equal(rlo, lo)
    idx = be.fake_quant(x, q4[0], q4[1], None, 16, False, False, EPS, 1, 1, want_y=False, idx_dtype=torch.int32)[1]
    assert torch.equal(256 * (hi.int() + 128) + (lo.int() + 128), idx)
