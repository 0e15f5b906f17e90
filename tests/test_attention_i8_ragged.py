"""tq_attention_i8_ragged_fwd: the integer attention core for ANY sequence length 1 <= T <= 512.

Contract (include/tq_hip.h): on all B * T rows bit-identical to tq_attention_i8_strided_fwd on the batch padded to
T_pad = 64 * ceil(T / 64) rows of arbitrary content with the mask -inf at the pad keys; nothing outside the B * T rows is read
or written.  Every GPU case compares values AND int8 indices with `torch.equal` against
tests/_ragged_twin.ragged_attention_reference (the existing oracle on the padded problem); the shapes are the smallest that
reach each launch form (plain / key-split / eight-wave, register-resident and streamed K tiles, branch-free and general
softmax path), the environment switches the launcher reads per call reach the others."""
import ctypes as C
import math

import pytest
import torch

from tests._ragged_twin import ragged_attention_reference, t_pad_of

DEV = 'cuda'


def _mk(d, z, nb=8):
    return (torch.tensor(d), torch.tensor(z), None, nb, False, False, 1e-8)


def _dev(q):
    return None if q is None else (q[0].to(DEV), q[1].to(DEV), None) + tuple(q[3:])


def _f(q):
    return None if q is None else (float(q[0]), float(q[1]), None) + tuple(q[3:])


def _quantizers(D, zero_q=False, scores=True):
    """(q_q, q_k, q_v, q_scores, q_probs, q_ctx) as in tests/test_int_oracle.py; zero_q: query zero point 0 -> c_q = 128"""
    q_q = _mk(0.011, 0.0 if zero_q else 120.0)
    q_c = _mk(0.15, 8.0, 4) if D == 32 else _mk(0.012, 125.0)
    return (q_q, _mk(0.013, 131.0), _mk(0.009, 128.0), _mk(0.35, 128.0) if scores else None, _mk(1.0 / 255, 0.0), q_c)


def _inputs(B, T, H, D, masked, seed=None):
    g = torch.Generator().manual_seed(B * 1000 + T + H if seed is None else seed)
    qi, ki, vi = (torch.randint(-128, 128, (B, T, H * D), generator=g).to(torch.int8) for _ in range(3))
    mask = None
    if masked:                                   # -10000 on some VALID keys; no query row is masked completely
        mask = torch.zeros(B, T)
        if T >= 4:
            mask[0, T - T // 4:] = -10000.0
        if B > 1 and T >= 2:
            mask[1, :T // 2] = -10000.0
    return qi, ki, vi, mask


_REF = {}


def _reference(B, T, H, D, masked, zero_q=False, scores=True):
    """computed once per problem, shared by every launch form of it, never modified"""
    key = (B, T, H, D, masked, zero_q, scores)
    if key not in _REF:
        qi, ki, vi, mask = _inputs(B, T, H, D, masked)
        qs = _quantizers(D, zero_q, scores)
        _REF[key] = ragged_attention_reference(qi, ki, vi, H, mask, math.sqrt(D), *[_f(q) for q in qs])
    return _REF[key]


def _check(B, T, H, D, masked, zero_q=False, scores=True):
    from quantization import _hip
    be = _hip.backend()
    qi, ki, vi, mask = _inputs(B, T, H, D, masked)
    qs = _quantizers(D, zero_q, scores)
    ctx, ci = be.attention_i8_ragged(qi.to(DEV), ki.to(DEV), vi.to(DEV), H, None if mask is None else mask.to(DEV),
                                     math.sqrt(D), *[_dev(q) for q in qs], want_idx=True)
    ref, ri = _reference(B, T, H, D, masked, zero_q, scores)
    assert ctx.shape == (B, T, H * D) and ci.shape == (B, T, H * D)
    assert torch.equal(ci.cpu(), ri), f'{int((ci.cpu() != ri).sum())} context indices differ'
    assert torch.equal(ctx.cpu(), ref)
    assert torch.isfinite(ref).all()


# (B, T, H, D): plain form | single token | head dim 32 | T_pad = 128 | 16 key tiles | 20 key tiles, general path | last row
SHAPES = [(2, 50, 2, 64), (3, 1, 1, 64), (2, 63, 2, 32), (2, 65, 2, 64), (1, 200, 2, 64), (1, 300, 1, 64), (1, 511, 1, 64)]
_ID = lambda c: 'B%d-T%d-H%d-d%d' % c


@pytest.mark.gpu
@pytest.mark.parametrize('masked', [False, True], ids=['mask-null', 'mask-on-valid-keys'])
@pytest.mark.parametrize('cfg', SHAPES, ids=_ID)
def test_ragged_core_equals_the_padded_oracle(cfg, masked, monkeypatch):
    for v in ('TQ_ATTN_SPLIT', 'TQ_ATTN_QW', 'TQ_ATTN_FAST'):
        monkeypatch.delenv(v, raising=False)
    _check(*cfg, masked)


@pytest.mark.gpu
@pytest.mark.parametrize('env', [{'TQ_ATTN_SPLIT': '0'}, {'TQ_ATTN_SPLIT': '0', 'TQ_ATTN_QW': '2'}],
                         ids=['eight-wave', 'plain'])
@pytest.mark.parametrize('cfg', [(2, 65, 2, 64), (1, 200, 2, 64), (1, 511, 1, 64)], ids=_ID)
def test_ragged_core_other_launch_forms(cfg, env, monkeypatch):
    """T_pad % 128 == 0: the default on these small grids is the key-split form; the switches reach the other two"""
    monkeypatch.delenv('TQ_ATTN_FAST', raising=False)
    monkeypatch.delenv('TQ_ATTN_QW', raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(*cfg, True)


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', [(2, 50, 2, 64), (2, 65, 2, 64)], ids=_ID)
def test_ragged_core_guarded_element_math(cfg, monkeypatch):
    monkeypatch.setenv('TQ_ATTN_FAST', '0')
    _check(*cfg, True)


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', [(2, 50, 2, 64), (2, 65, 2, 64)], ids=_ID)
def test_ragged_core_query_zero_point_zero(cfg):
    """c_q = 128: the zero-point correction of the scores takes two MFMA passes"""
    _check(*cfg, True, zero_q=True)


@pytest.mark.gpu
def test_ragged_core_without_score_quantizer():
    _check(2, 50, 2, 64, True, scores=False)


@pytest.mark.gpu
def test_ragged_core_reads_column_blocks_of_stacked_buffers():
    """Q | K as column blocks of one [B, T, 3 H d] buffer, V a column block of another with a row stride of its own"""
    from quantization import _hip
    be = _hip.backend()
    B, T, H, D = 2, 50, 2, 64
    HD = H * D
    qi, ki, vi, mask = _inputs(B, T, H, D, True)
    g = torch.Generator().manual_seed(9)
    qk = torch.randint(-128, 128, (B, T, 3 * HD), generator=g).to(torch.int8)
    vb = torch.randint(-128, 128, (B, T, 2 * HD), generator=g).to(torch.int8)
    qk[..., :HD], qk[..., HD:2 * HD], vb[..., HD:] = qi, ki, vi
    qk, vb = qk.to(DEV), vb.to(DEV)
    q, k, v = qk[..., :HD], qk[..., HD:2 * HD], vb[..., HD:]
    assert q.stride() == k.stride() == (T * 3 * HD, 3 * HD, 1) and v.stride(1) == 2 * HD
    qs = _quantizers(D)
    seen = []
    orig = be.lib.tq_attention_i8_ragged_fwd

    class Spy:                                      # the strides the C entry point was handed: nothing was copied
        def __getattr__(self, name):
            return getattr(be.lib, name)

        def tq_attention_i8_ragged_fwd(self, *a):
            seen.append((a[0], a[1], a[2], a[9], a[10]))
            return orig(*a)
    lib = be.lib
    be.lib = Spy()
    try:
        ctx, ci = be.attention_i8_ragged(q, k, v, H, mask.to(DEV), math.sqrt(D), *[_dev(x) for x in qs], want_idx=True)
    finally:
        be.lib = lib
    assert seen == [(q.data_ptr(), k.data_ptr(), v.data_ptr(), 3 * HD, 2 * HD)]
    ref, ri = _reference(B, T, H, D, True)
    assert torch.equal(ci.cpu(), ri) and torch.equal(ctx.cpu(), ref)


# ---- memory behaviour: raw entry point on buffers the test owns ------------------------------------------------------------
def _raw_call(be, q, k, v, ctx, ci, B, T, H, D, mask, qs, stride=0):
    descs = [None if x is None else be._qdesc(*x, 1, 1) for x in qs]
    refs = [None if d is None else C.byref(d) for d in descs]
    rc = be.lib.tq_attention_i8_ragged_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ctx.data_ptr(), ci.data_ptr(), B, T, H, D,
                                           stride, stride, None if mask is None else mask.data_ptr(), float(math.sqrt(D)), *refs,
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', [(2, 50, 2, 64), (2, 65, 2, 64), (1, 300, 1, 64)], ids=_ID)
def test_ragged_core_touches_only_its_rows(cfg):
    """outputs: sentinel rows behind row B * T stay intact.  Inputs: the prefix of larger buffers -- two runs whose tails differ
    (zeros | random bytes, mask tail 0 | NaN) give identical outputs, equal to the reference."""
    from quantization import _hip
    be = _hip.backend()
    B, T, H, D = cfg
    HD, rows, extra = H * D, B * T, 64
    qi, ki, vi, mask = _inputs(B, T, H, D, True)
    qs = [_dev(x) for x in _quantizers(D)]
    ref, ri = _reference(B, T, H, D, True)
    g = torch.Generator().manual_seed(4)
    outs = []
    for tail in ('zeros', 'random'):
        bufs = []
        for t in (qi, ki, vi):
            b = torch.zeros(rows + extra, HD, dtype=torch.int8)
            if tail == 'random':
                b[rows:] = torch.randint(-128, 128, (extra, HD), generator=g).to(torch.int8)
            b[:rows] = t.reshape(rows, HD)
            bufs.append(b.to(DEV))
        m = torch.zeros(rows + extra)
        if tail == 'random':
            m[rows:] = float('nan')
        m[:rows] = mask.reshape(-1)
        m = m.to(DEV)
        ctx = torch.full((rows + extra, HD), 12345.0, device=DEV)
        ci = torch.full((rows + extra, HD), 77, dtype=torch.int8, device=DEV)
        assert _raw_call(be, *bufs, ctx, ci, B, T, H, D, m, qs) == 0, be.lib.tq_last_error()
        assert bool((ctx[rows:] == 12345.0).all()) and bool((ci[rows:] == 77).all()), 'rows behind B * T were written'
        outs.append((ctx[:rows].cpu().reshape(B, T, HD), ci[:rows].cpu().reshape(B, T, HD)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][1], ri) and torch.equal(outs[0][0], ref)


@pytest.mark.gpu
def test_ragged_core_on_exactly_sized_inputs():
    """the last sequence ends where the allocation ends: every pad-row index of it is clamped to its last valid row"""
    from quantization import _hip
    be = _hip.backend()
    B, T, H, D = 2, 50, 2, 64
    qi, ki, vi, mask = _inputs(B, T, H, D, True)
    qs = [_dev(x) for x in _quantizers(D)]
    bufs = [t.reshape(B * T, H * D).to(DEV).clone() for t in (qi, ki, vi)]
    assert all(b.untyped_storage().nbytes() == B * T * H * D for b in bufs)
    m = mask.reshape(-1).to(DEV).clone()
    ctx = torch.empty(B * T, H * D, device=DEV)
    ci = torch.empty(B * T, H * D, dtype=torch.int8, device=DEV)
    assert _raw_call(be, *bufs, ctx, ci, B, T, H, D, m, qs) == 0, be.lib.tq_last_error()
    ref, ri = _reference(B, T, H, D, True)
    assert torch.equal(ci.cpu().reshape(B, T, -1), ri) and torch.equal(ctx.cpu().reshape(B, T, -1), ref)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [64, 128])
def test_whole_tiles_forward_to_the_existing_entry_point(T):
    from quantization import _hip
    be = _hip.backend()
    B, H, D = 2, 2, 64
    qi, ki, vi, mask = _inputs(B, T, H, D, True)
    qs = [_dev(x) for x in _quantizers(D)]
    a = be.attention_i8_ragged(qi.to(DEV), ki.to(DEV), vi.to(DEV), H, mask.to(DEV), math.sqrt(D), *qs, want_idx=True)
    b = be.attention_i8(qi.to(DEV), ki.to(DEV), vi.to(DEV), H, mask.to(DEV), math.sqrt(D), *qs, want_idx=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_whole_tiles_take_a_mask_that_is_only_4_byte_aligned():
    """the contract asks 4-byte alignment of the mask at EVERY T: at T = 64 a mask 4 bytes off a 16-byte boundary runs the
    ragged form with no pad rows and gives the whole-tile entry point's bits"""
    from quantization import _hip
    be = _hip.backend()
    B, T, H, D = 2, 64, 2, 64
    qi, ki, vi, mask = _inputs(B, T, H, D, True)
    qs = [_dev(x) for x in _quantizers(D)]
    want = be.attention_i8(qi.to(DEV), ki.to(DEV), vi.to(DEV), H, mask.to(DEV), math.sqrt(D), *qs, want_idx=True)
    buf = torch.zeros(B * T + 4, device=DEV)
    m = buf[1:1 + B * T]
    m.copy_(mask.reshape(-1))
    assert m.data_ptr() % 16 == 4
    bufs = [t.reshape(B * T, H * D).to(DEV) for t in (qi, ki, vi)]
    ctx = torch.empty(B * T, H * D, device=DEV)
    ci = torch.empty(B * T, H * D, dtype=torch.int8, device=DEV)
    assert _raw_call(be, *bufs, ctx, ci, B, T, H, D, m, qs) == 0, be.lib.tq_last_error()
    assert torch.equal(ctx.reshape(B, T, -1), want[0]) and torch.equal(ci.reshape(B, T, -1), want[1])


# ---- no GPU ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_access():
    """raw ctypes, no device: T = 513 is TQ_EINVAL (the pointers are never followed), T = 0 is TQ_OK without a launch, and the
    existing entry point keeps refusing T = 96"""
    from quantization import _hip
    lib = _hip.load_library()
    q = _hip.tq_quantizer(None, None, None, 8, 0, 0, 1e-8, 1, 1)
    r = C.byref(q)
    fake = 1 << 20                                   # a non-NULL, 16-byte aligned address that is never dereferenced
    call = lambda fn, T, **kw: fn(fake, fake, fake, fake, None, kw.get('B', 2), T, kw.get('H', 2), kw.get('D', 64), 0, 0, None,
                                  8.0, r, r, r, None, r, None, None)
    assert call(lib.tq_attention_i8_ragged_fwd, 513) == -1 and b'513' in lib.tq_last_error()
    assert lib.tq_last_error().startswith(b'tq_attention_i8_ragged_fwd:')       # errors name the entry point that was called
    assert call(lib.tq_attention_i8_ragged_fwd, 0) == 0
    assert call(lib.tq_attention_i8_ragged_fwd, 50, B=0) == 0 and call(lib.tq_attention_i8_ragged_fwd, 50, H=0) == 0
    assert call(lib.tq_attention_i8_ragged_fwd, 50, D=48) == -1
    assert lib.tq_attention_i8_ragged_fwd(None, fake, fake, fake, None, 2, 50, 2, 64, 0, 0, None, 8.0, r, r, r, None, r, None,
                                          None) == -1
    assert call(lib.tq_attention_i8_strided_fwd, 96) == -1 and b'96' in lib.tq_last_error()
    assert lib.tq_last_error().startswith(b'tq_attention_i8_fwd:')


@pytest.mark.parametrize('T', [50, 1, 63, 17])
def test_reference_does_not_depend_on_pad_rows_cpu(T):
    """the padding fact the contract rests on, with the existing oracle: pad rows of zeros, random bytes or copies of the last
    valid row give identical ctx and ctx_idx on the valid rows (with -10000 on some valid keys as well)"""
    B, H, D = 2, 2, 64
    qi, ki, vi, mask = _inputs(B, T, H, D, True, seed=T)
    assert t_pad_of(T) == 64
    qs = [_f(x) for x in _quantizers(D)]
    outs = [ragged_attention_reference(qi, ki, vi, H, mask, 8.0, *qs, pad=pad, seed=T) for pad in ('zeros', 'random', 'last')]
    assert outs[0][0].shape == (B, T, H * D) and torch.isfinite(outs[0][0]).all()
    for ctx, ci in outs[1:]:
        assert torch.equal(ctx, outs[0][0]) and torch.equal(ci, outs[0][1])
    if T == 50:                                      # and the mask extension is what removes the pad keys
        from oracle import int_oracle
        pad = lambda t: torch.cat([t, t[:, :14]], 1).contiguous()
        m = torch.cat([mask, torch.zeros(B, 14)], 1)
        unmasked = int_oracle.attention_i8(pad(qi), pad(ki), pad(vi), H, m, 8.0, *qs)[1][:, :T]
        assert not torch.equal(unmasked, outs[0][1])
