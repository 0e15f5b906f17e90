"""Row tails of the tiled integer Linears (HipBackend.PADS_ROWS): rows of a Linear are independent, so `linear_i8` and
`linear_i8_grouped` launch a row count that is no multiple of the tile over M_pad = 64 * ceil(M / 64) rows of buffers that
have the room, and the first M rows are exact.  No Linear kernel changed: what is tested is the backend's allocation and
launch logic -- results `torch.equal` to oracle/tq_int_oracle.c and to the same call on the operand zero-padded to M_pad, an
operand without room copied once, one from the backend's own allocator used in place, whole tiles launched exactly as before."""
import pytest
import torch

from oracle import int_oracle as IO
from tests.test_int_oracle import _dev, _f, _gelu_q, _rand_layer, _stair_header, _xq_dev

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROWS = [1, 33, 50, 150]
K = 128


class _Spy:
    """the backend's library handle with one entry point recorded: (x pointer, M) of every call"""

    def __init__(self, lib, name):
        self._lib, self._name, self.calls = lib, name, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._name:
            return fn

        def recorded(*a):
            self.calls.append((a[0], a[7]))
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


def _m_pad(M):
    return -(-M // 64) * 64


def _zero_padded(x_idx):
    M = x_idx.shape[0]
    out = torch.zeros(_m_pad(M), x_idx.shape[1], dtype=torch.int8)
    out[:M] = x_idx
    return out


_FORMS = ['relu', 'gelu-stair', 'index-only', 'no-quantizer']


@pytest.mark.parametrize('form', _FORMS)
@pytest.mark.parametrize('M', ROWS)
def test_linear_i8_row_tails(M, form):
    from quantization import _hip
    be = _hip.backend()
    assert be.PADS_ROWS is True
    N = 64
    x_idx, w_idx, x_q, w_delta, bias, q_out = _rand_layer(M, N, K, seed=5 + M)
    act, code, stair = 1, 1, None
    if form == 'gelu-stair':
        q_out = _gelu_q(0.036, 5.0)                          # a grid the 768-bin table holds (tests/test_int_oracle.py)
        stair = be.act_stair(2, _dev(q_out), be.stair_bins_for(M, N))
        assert _stair_header(stair)[3] == 1.0
        act, code = 2, 4                                     # an accepted table evaluates the correctly rounded GELU
    if form == 'no-quantizer':
        q_out = None
    ref_y, ref_i = IO.linear_i8(x_idx, w_idx, bias, x_q, w_delta, 1e-8, code, _f(q_out))
    wi = w_idx.to(DEV)
    rest = (wi, be.rowsum_i8(wi), bias.to(DEV), _xq_dev(x_q), w_delta.to(DEV), 1e-8, act, _dev(q_out), torch.float32)
    kw = dict(want_idx=q_out is not None, want_y=form != 'index-only', stair=stair)
    out, calls = _spied(be, 'tq_linear_i8_stair_fwd', lambda: be.linear_i8(x_idx.to(DEV), *rest, **kw))
    assert [c[1] for c in calls] == [_m_pad(M)]
    big = be.linear_i8(_zero_padded(x_idx).to(DEV), *rest, **kw)       # the same call on the operand padded by the caller
    y, yi = out if q_out is not None else (out, None)
    by, bi = big if q_out is not None else (big, None)
    if form == 'index-only':
        assert y is None
    else:
        assert y.shape == (M, N) and torch.equal(y.cpu(), ref_y) and torch.equal(y, by[:M])
    if q_out is not None:
        assert yi.shape == (M, N) and torch.equal(yi.cpu(), ref_i) and torch.equal(yi, bi[:M])


@pytest.mark.parametrize('M', ROWS)
def test_linear_i8_grouped_row_tails(M):
    """three Linears sharing their input (Q | K | V), index-only and with the fp32 output"""
    from quantization import _hip
    be = _hip.backend()
    G, Ng = 3, 64
    N = G * Ng
    x_idx, w_idx, x_q, _, bias, q_out = _rand_layer(M, N, K, seed=9 + M, per_row=True)
    g = torch.Generator().manual_seed(M)
    w_rows = torch.rand(N, generator=g) * 0.002 + 0.0005
    q_outs = [(q_out[0] * s, q_out[1] + z, None, 8, False, False, 1e-8) for s, z in ((1.0, 0.0), (0.8, -9.0), (1.3, 5.0))]
    refs = [IO.linear_i8(x_idx, w_idx[s], bias[s], x_q, w_rows[s], 1e-8, 0, _f(q))
            for s, q in ((slice(i * Ng, (i + 1) * Ng), q_outs[i]) for i in range(G))]
    ref_y, ref_i = torch.cat([r[0] for r in refs], -1), torch.cat([r[1] for r in refs], -1)
    wi = w_idx.to(DEV)
    rest = (wi, be.rowsum_i8(wi), bias.to(DEV), _xq_dev(x_q), w_rows.to(DEV), 1e-8, 0, [_dev(q) for q in q_outs])
    (y, yi), calls = _spied(be, 'tq_linear_i8_grouped_fwd',
                            lambda: be.linear_i8_grouped(x_idx.to(DEV), *rest, want_y=True, want_idx=True))
    assert [c[1] for c in calls] == [_m_pad(M)]
    assert y.shape == yi.shape == (M, N) and torch.equal(yi.cpu(), ref_i) and torch.equal(y.cpu(), ref_y)
    none, yi2 = be.linear_i8_grouped(x_idx.to(DEV), *rest)             # the route's form: indices only
    assert none is None and torch.equal(yi2, yi)
    by, bi = be.linear_i8_grouped(_zero_padded(x_idx).to(DEV), *rest, want_y=True, want_idx=True)
    assert torch.equal(y, by[:M]) and torch.equal(yi, bi[:M])


def _layer(M, N=64):
    x_idx, w_idx, x_q, w_delta, bias, q_out = _rand_layer(M, N, K, seed=5 + M)
    return x_idx, w_idx, x_q, w_delta, bias, q_out


def test_operand_without_room_is_copied_once():
    from quantization import _hip
    be = _hip.backend()
    M, N = 50, 64
    x_idx, w_idx, x_q, w_delta, bias, q_out = _layer(M)
    x = x_idx.to(DEV).clone()
    assert x.untyped_storage().nbytes() == M * K and not be._row_room(x, 64)
    before = x.clone()
    wi = w_idx.to(DEV)
    (y, yi), calls = _spied(be, 'tq_linear_i8_stair_fwd', lambda: be.linear_i8(
        x, wi, be.rowsum_i8(wi), bias.to(DEV), _xq_dev(x_q), w_delta.to(DEV), 1e-8, 1, _dev(q_out), torch.float32, want_idx=True))
    assert len(calls) == 1 and calls[0][1] == 64 and calls[0][0] != x.data_ptr()       # a buffer with room, not the operand
    assert torch.equal(x, before)
    ref_y, ref_i = IO.linear_i8(x_idx, w_idx, bias, x_q, w_delta, 1e-8, 1, _f(q_out))
    assert torch.equal(y.cpu(), ref_y) and torch.equal(yi.cpu(), ref_i)


def test_operand_from_the_backends_allocator_is_used_in_place(monkeypatch):
    """with options.INT8_RAGGED on, indices produced by `quantize_to_int8` (as every producer of the route: tails, embedding
    block, attention core, the Linears themselves) have room for M_pad rows: the next Linear reads them where they are, and so
    does the one after it"""
    from quantization import _hip, options
    be = _hip.backend()
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    M, N = 50, 128
    x_idx, w_idx, x_q, w_delta, bias, q_out = _layer(M, N)
    xq = _xq_dev(x_q)
    zp = float(x_q[1])
    xf = ((x_idx.float() + 128 - zp) * x_q[0]).to(DEV)       # the values whose grid indices are x_idx
    x = be.quantize_to_int8(xf, xq[0], xq[1], None, 8, False, False, 1e-8, 1, 1, minus_128=True)
    assert torch.equal(x.cpu(), x_idx) and x.shape == (M, K)
    assert be._row_room(x, 64) and x.untyped_storage().nbytes() == 64 * K
    wi = w_idx.to(DEV)
    (y, yi), calls = _spied(be, 'tq_linear_i8_stair_fwd', lambda: be.linear_i8(
        x, wi, be.rowsum_i8(wi), bias.to(DEV), xq, w_delta.to(DEV), 1e-8, 1, _dev(q_out), torch.float32, want_idx=True))
    assert calls == [(x.data_ptr(), 64)]
    ref_y, ref_i = IO.linear_i8(x_idx, w_idx, bias, x_q, w_delta, 1e-8, 1, _f(q_out))
    assert torch.equal(y.cpu(), ref_y) and torch.equal(yi.cpu(), ref_i)
    # the indices it emitted feed the next Linear in place, too (K = 128 = N)
    assert be._row_room(yi, 64) and be._row_room(y, 64)
    _, calls = _spied(be, 'tq_linear_i8_stair_fwd', lambda: be.linear_i8(
        yi, wi, be.rowsum_i8(wi), bias.to(DEV), (q_out[0].to(DEV), q_out[1].to(DEV), 8, 1e-8), w_delta.to(DEV), 1e-8, 0, None,
        torch.float32))
    assert calls == [(yi.data_ptr(), 64)]


def test_option_off_allocates_exactly_as_before():
    """options.INT8_RAGGED off (the default): every tensor the backend returns owns exactly its own storage, whatever its row
    count -- only the outputs of a launch that is itself padded have the room the kernel writes"""
    from quantization import _hip, options
    be = _hip.backend()
    assert options.INT8_RAGGED is False
    for M in (50, 96, 32):
        x_idx, w_idx, x_q, w_delta, bias, q_out = _layer(M)
        xq = _xq_dev(x_q)
        xf = torch.randn(M, K, device=DEV)
        i8 = be.quantize_to_int8(xf, xq[0], xq[1], None, 8, False, False, 1e-8, 1, 1, minus_128=True)
        y, yi = be.fake_quant_int8(xf, xq[0], xq[1], 8, 1e-8)
        assert [t.untyped_storage().nbytes() for t in (i8, y, yi)] == [M * K, M * K * 4, M * K]
        wi = w_idx.to(DEV)
        out, oi = be.linear_i8(x_idx.to(DEV), wi, be.rowsum_i8(wi), bias.to(DEV), xq, w_delta.to(DEV), 1e-8, 1, _dev(q_out),
                               torch.float32, want_idx=True)
        rows = M if M % 32 == 0 else _m_pad(M)                  # M = 50: the launch covers 64 rows and writes them
        assert out.untyped_storage().nbytes() == rows * 64 * 4 and oi.untyped_storage().nbytes() == rows * 64
        assert out.shape == (M, 64)


def test_option_on_pads_multiples_of_32_to_the_lds_tile(monkeypatch):
    """M = 96: launched as it is by default (the register-tile kernel); with options.INT8_RAGGED on, over 128 rows -- the
    LDS-tiled kernels the rest of the route runs.  Same bits either way."""
    from quantization import _hip, options
    be = _hip.backend()
    M = 96
    x_idx, w_idx, x_q, w_delta, bias, q_out = _layer(M)
    wi = w_idx.to(DEV)
    call = lambda: be.linear_i8(x_idx.to(DEV), wi, be.rowsum_i8(wi), bias.to(DEV), _xq_dev(x_q), w_delta.to(DEV), 1e-8, 1,
                                _dev(q_out), torch.float32, want_idx=True)
    (y0, i0), calls = _spied(be, 'tq_linear_i8_stair_fwd', call)
    assert [c[1] for c in calls] == [96]
    monkeypatch.setattr(options, 'INT8_RAGGED', True)
    (y1, i1), calls = _spied(be, 'tq_linear_i8_stair_fwd', call)
    assert [c[1] for c in calls] == [128] and be.stair_bins_for(96, 64) == be.stair_bins_for(128, 64)
    ref_y, ref_i = IO.linear_i8(x_idx, w_idx, bias, x_q, w_delta, 1e-8, 1, _f(q_out))
    assert torch.equal(y1, y0) and torch.equal(i1, i0) and torch.equal(y1.cpu(), ref_y) and torch.equal(i1.cpu(), ref_i)


def test_whole_tiles_allocate_and_launch_as_before():
    from quantization import _hip
    be = _hip.backend()
    M, N = 128, 64
    x_idx, w_idx, x_q, w_delta, bias, q_out = _layer(M)
    x = x_idx.to(DEV).clone()
    wi = w_idx.to(DEV)
    (y, yi), calls = _spied(be, 'tq_linear_i8_stair_fwd', lambda: be.linear_i8(
        x, wi, be.rowsum_i8(wi), bias.to(DEV), _xq_dev(x_q), w_delta.to(DEV), 1e-8, 1, _dev(q_out), torch.float32, want_idx=True))
    assert calls == [(x.data_ptr(), M)]
    assert y.untyped_storage().nbytes() == M * N * 4 and yi.untyped_storage().nbytes() == M * N and y.storage_offset() == 0
    for rows in (32, 96):                                    # multiples of 32 are shapes the launcher tiles itself
        xs = x[:rows].clone()
        _, calls = _spied(be, 'tq_linear_i8_stair_fwd', lambda: be.linear_i8(
            xs, wi, be.rowsum_i8(wi), bias.to(DEV), _xq_dev(x_q), w_delta.to(DEV), 1e-8, 1, _dev(q_out), torch.float32,
            want_idx=True))
        assert calls == [(xs.data_ptr(), rows)]
    ref_y, ref_i = IO.linear_i8(x_idx, w_idx, bias, x_q, w_delta, 1e-8, 1, _f(q_out))
    assert torch.equal(y.cpu(), ref_y) and torch.equal(yi.cpu(), ref_i)
    w3 = torch.cat([wi, wi, wi])
    (_, gi), calls = _spied(be, 'tq_linear_i8_grouped_fwd', lambda: be.linear_i8_grouped(
        x, w3, be.rowsum_i8(w3), torch.cat([bias] * 3).to(DEV), _xq_dev(x_q), w_delta.to(DEV).expand(3 * N).contiguous(), 1e-8, 0, [_dev(q_out)] * 3))
    assert calls == [(x.data_ptr(), M)] and gi.untyped_storage().nbytes() == M * 3 * N
