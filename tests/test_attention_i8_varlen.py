"""tq_attention_i8_varlen_fwd: the integer attention core over PACKED sequences (no pad tokens).

Contract (include/tq_hip.h): sequence b owns rows seq_start[b] .. seq_start[b + 1] - 1 of the [total_rows, ...] buffers; on every
owned row ctx and ctx_idx are bit-identical to tq_attention_i8_ragged_fwd on the [B, T_cap] batch with sequence b at [b, :len_b],
arbitrary pad rows, the packed mask's values at the valid keys and -inf at the pad keys; rows nobody owns are not written and
nothing outside the total_rows rows is touched.

The first test (CPU) shows with the existing oracle that the padded problem does not depend on what its pad rows hold.  Every
GPU case then compares `attention_i8_varlen` with `attention_i8_ragged` -- the KERNEL the contract names -- on the padded batch
(pad rows of random bytes), `torch.equal` on values and int8 indices, sequence by sequence.  H = 2 throughout; the lengths are the
smallest that reach every launch form (plain, key-split, eight-wave), both early exits (32- and 128-query workgroups beyond
len_b), a sequence of the full T_cap, a single-token sequence and T_pad = 64 / 128 / 192.  seq_start is consistent in every
case: the device-side clamps are a defence to be read, not exercised."""
import ctypes as C
import math

import pytest
import torch

from tests._packed_twin import pad_packed, padded_mask, packed_attention_reference
from tests.test_attention_i8_ragged import _dev, _f, _quantizers

DEV = 'cuda'
H = 2


def _starts(lengths, first=0):
    s = [first]
    for n in lengths:
        s.append(s[-1] + n)
    return torch.tensor(s, dtype=torch.int32)


def _packed_inputs(lengths, D, masked=False, first=0, extra=0, seed=None):
    """q, k, v int8 [1, M, H * D] of random bytes (M = first + sum(lengths) + extra), seq_start, packed mask [M] or None: -10000
    and small finite addends on some valid keys, never on a sequence's first key (no query row is masked completely)"""
    s = _starts(lengths, first)
    M = int(s[-1]) + extra
    g = torch.Generator().manual_seed(sum(lengths) * 31 + len(lengths) + D if seed is None else seed)
    q, k, v = (torch.randint(-128, 128, (1, M, H * D), generator=g).to(torch.int8) for _ in range(3))
    mask = None
    if masked:
        mask = torch.randn(M, generator=g) * 0.5
        mask[torch.rand(M, generator=g) < 0.25] = -10000.0
        mask[s[:-1].long().clamp(max=M - 1)] = 0.25
    return q, k, v, s, mask


def _ragged_on_the_padded_batch(be, q, k, v, s, T_cap, mask, D, qs):
    """the reference launch: attention_i8_ragged on [B, T_cap] with random pad rows and -inf on the pad keys -> host tensors"""
    g = torch.Generator().manual_seed(77)
    qp, kp, vp = (pad_packed(t, s, T_cap, 'random', g).to(DEV) for t in (q, k, v))
    ctx, ci = be.attention_i8_ragged(qp, kp, vp, H, padded_mask(mask, s, T_cap).to(DEV), math.sqrt(D), *qs, want_idx=True)
    return ctx.cpu(), ci.cpu()


def _assert_owned_rows_equal(ctx, ci, ref, ri, s):
    """ctx / ci [M, HD] packed, ref / ri [B, T_cap, HD] padded"""
    for b in range(len(s) - 1):
        lo, hi = int(s[b]), int(s[b + 1])
        assert torch.equal(ci[lo:hi], ri[b, :hi - lo]), f'sequence {b} (rows {lo}..{hi - 1}): context indices differ'
        assert torch.equal(ctx[lo:hi], ref[b, :hi - lo]), f'sequence {b} (rows {lo}..{hi - 1}): context values differ'
        assert torch.isfinite(ctx[lo:hi]).all()


def _check(lengths, D=64, T_cap=None, masked=False, extra=0):
    from quantization import _hip
    be = _hip.backend()
    T_cap = max(lengths) if T_cap is None else T_cap
    q, k, v, s, mask = _packed_inputs(lengths, D, masked, extra=extra)
    qs = [_dev(x) for x in _quantizers(D)]
    ctx, ci = be.attention_i8_varlen(q.to(DEV), k.to(DEV), v.to(DEV), H, s.to(DEV), T_cap, None if mask is None else mask.to(DEV),
                                     math.sqrt(D), *qs, want_idx=True)
    assert ctx.shape == (1, q.shape[1], H * D) and ci.shape == ctx.shape and ci.dtype == torch.int8
    ref, ri = _ragged_on_the_padded_batch(be, q, k, v, s, T_cap, mask, D, qs)
    _assert_owned_rows_equal(ctx[0].cpu(), ci[0].cpu(), ref, ri, s)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_packed_reference_does_not_depend_on_pad_rows_cpu():
    """pad rows of zeros, of random bytes and of copies of the last valid row give the same ctx and ctx_idx on every owned row
    (oracle/int_oracle.py on the padded problem); and it is the -inf at the pad keys that makes it so"""
    lengths, D = (50, 1, 37), 64
    q, k, v, s, mask = _packed_inputs(lengths, D, masked=True)
    qs = [_f(x) for x in _quantizers(D)]
    outs = [packed_attention_reference(q, k, v, H, s, 50, mask, 8.0, *qs, pad=pad, seed=5) for pad in ('zeros', 'random', 'last')]
    assert outs[0][0].shape == (1, 88, H * D) and torch.isfinite(outs[0][0]).all()
    for ctx, ci in outs[1:]:
        assert torch.equal(ctx, outs[0][0]) and torch.equal(ci, outs[0][1])
    from oracle import int_oracle
    g = torch.Generator().manual_seed(5)
    qp, kp, vp = (pad_packed(t, s, 64, 'random', g) for t in (q, k, v))
    m = padded_mask(mask, s, 64)
    m[m == float('-inf')] = 0.0                                # pad keys visible: the short sequences change
    ci = int_oracle.attention_i8(qp, kp, vp, H, m.contiguous(), 8.0, *qs)[1]
    assert not torch.equal(ci[2, :37], outs[0][1][0, 51:88])


def test_argument_errors_come_before_any_device_access():
    """raw ctypes, no device: the added checks (seq_start, total_rows), the ragged entry's (T_cap = 513, head_dim) and the empty
    problems that return TQ_OK without a launch"""
    from quantization import _hip
    lib = _hip.load_library()
    qd = _hip.tq_quantizer(None, None, None, 8, 0, 0, 1e-8, 1, 1)
    r = C.byref(qd)
    fake = 1 << 20                                   # a non-NULL, 16-byte aligned address that is never dereferenced
    fn = lib.tq_attention_i8_varlen_fwd

    def call(seq=fake, B=3, rows=99, T=50, Hh=2, D=64):
        return fn(fake, fake, fake, fake, None, seq, B, rows, T, Hh, D, 0, 0, None, 8.0, r, r, r, None, r, None, None)
    assert call(seq=None) == -1 and lib.tq_last_error().startswith(b'tq_attention_i8_varlen_fwd:')
    assert call(seq=fake + 2) == -1 and b'seq_start' in lib.tq_last_error()
    assert call(rows=1 << 31) == -1 and b'total_rows' in lib.tq_last_error()
    assert call(T=513) == -1 and b'513' in lib.tq_last_error()
    assert call(D=48) == -1
    assert call(B=0) == 0 and call(Hh=0) == 0 and call(T=0) == 0 and call(rows=0) == 0
    assert call(B=0, seq=None) == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _clear_env(monkeypatch):
    for v in ('TQ_ATTN_SPLIT', 'TQ_ATTN_QW', 'TQ_ATTN_FAST'):
        monkeypatch.delenv(v, raising=False)


@pytest.mark.gpu
def test_varlen_core_t_pad_64(monkeypatch):
    """lengths (50, 1, 37), T_cap 50: the plain form on 4 key tiles; a single-token sequence leaves from its second workgroup"""
    _clear_env(monkeypatch)
    _check((50, 1, 37))


@pytest.mark.gpu
@pytest.mark.parametrize('env', [{'TQ_ATTN_SPLIT': '1'}, {'TQ_ATTN_SPLIT': '0', 'TQ_ATTN_QW': '8'},
                                 {'TQ_ATTN_SPLIT': '0', 'TQ_ATTN_QW': '2'}], ids=['key-split', 'eight-wave', 'plain'])
def test_varlen_core_t_pad_128_every_launch_form(env, monkeypatch):
    """lengths (128, 65, 3, 16), T_cap 128: a full-length sequence, one that spills into the third 32-query workgroup, and two
    that end inside the first -- the 32-query (key-split, plain) and 128-query (eight-wave) workgroup exits"""
    _clear_env(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check((128, 65, 3, 16))


@pytest.mark.gpu
def test_varlen_core_t_pad_192(monkeypatch):
    _clear_env(monkeypatch)
    _check((130, 64, 129))


@pytest.mark.gpu
def test_varlen_core_head_dim_32(monkeypatch):
    _clear_env(monkeypatch)
    _check((50, 1, 37), D=32)


@pytest.mark.gpu
def test_varlen_core_packed_mask_with_finite_values(monkeypatch):
    """additive mask per KEY row of the packed buffers: -10000 and small finite addends"""
    _clear_env(monkeypatch)
    _check((50, 1, 37), masked=True)
    _check((128, 65, 3, 16), masked=True)


@pytest.mark.gpu
def test_varlen_core_total_rows_beyond_the_last_sequence(monkeypatch):
    """total_rows > seq_start[B]: the rows behind the last sequence belong to nobody, and T_cap may exceed every length"""
    _clear_env(monkeypatch)
    _check((50, 1, 37), extra=29, T_cap=60, masked=True)


@pytest.mark.gpu
def test_varlen_core_reads_column_blocks_of_the_stacked_buffer(monkeypatch):
    """Q | K column blocks of one [1, M, 3 H d] buffer, V a column block of another buffer with a row stride of its own: the
    C entry point is handed the blocks in place"""
    from quantization import _hip
    _clear_env(monkeypatch)
    be = _hip.backend()
    lengths, D = (50, 1, 37), 64
    HD = H * D
    q, k, v, s, mask = _packed_inputs(lengths, D, masked=True)
    M = q.shape[1]
    g = torch.Generator().manual_seed(9)
    qk = torch.randint(-128, 128, (1, M, 3 * HD), generator=g).to(torch.int8)
    vb = torch.randint(-128, 128, (1, M, 2 * HD), generator=g).to(torch.int8)
    qk[..., :HD], qk[..., HD:2 * HD], vb[..., HD:] = q, k, v
    qk, vb = qk.to(DEV), vb.to(DEV)
    qd, kd, vd = qk[..., :HD], qk[..., HD:2 * HD], vb[..., HD:]
    qs = [_dev(x) for x in _quantizers(D)]
    seen = []
    orig = be.lib.tq_attention_i8_varlen_fwd

    class Spy:
        def __getattr__(self, name):
            return getattr(be.lib, name)

        def tq_attention_i8_varlen_fwd(self, *a):
            seen.append((a[0], a[1], a[2], a[6], a[7], a[8], a[11], a[12]))
            return orig(*a)
    lib = be.lib
    be.lib = Spy()
    try:
        ctx, ci = be.attention_i8_varlen(qd, kd, vd, H, s.to(DEV), 50, mask.to(DEV), math.sqrt(D), *qs, want_idx=True)
    finally:
        be.lib = lib
    assert seen == [(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), 3, M, 50, 3 * HD, 2 * HD)]
    ref, ri = _ragged_on_the_padded_batch(be, q, k, v, s, 50, mask, D, qs)
    _assert_owned_rows_equal(ctx[0].cpu(), ci[0].cpu(), ref, ri, s)


@pytest.mark.gpu
@pytest.mark.parametrize('lengths', [(50, 0, 1, 37), (128, 65, 3, 16)], ids=['T_pad64-with-an-empty-sequence', 'T_pad128'])
def test_varlen_core_writes_only_owned_rows(lengths, monkeypatch):
    """raw entry point on sentinel-filled ctx / ctx_idx: 3 unowned rows in front of the first sequence and 7 behind the last one
    INSIDE the total_rows rows, 8 guard rows on either side OUTSIDE them -- all keep their sentinels, every owned row is written
    with the reference's bits.  (A sequence of length 0 is consistent: it owns nothing and its workgroups leave.)"""
    from quantization import _hip
    _clear_env(monkeypatch)
    be = _hip.backend()
    D, first, extra, guard = 64, 3, 7, 8
    HD = H * D
    q, k, v, s, mask = _packed_inputs(lengths, D, masked=True, first=first, extra=extra)
    M = q.shape[1]
    assert int(s[0]) == first and int(s[-1]) == M - extra
    qs = [_dev(x) for x in _quantizers(D)]
    ctx = torch.full((guard + M + guard, HD), 12345.0, device=DEV)
    ci = torch.full((guard + M + guard, HD), 77, dtype=torch.int8, device=DEV)
    bufs = [t[0].to(DEV).contiguous() for t in (q, k, v)]
    sd, md = s.to(DEV), mask.to(DEV)
    descs = [None if x is None else be._qdesc(*x, 1, 1) for x in qs]
    refs = [None if d is None else C.byref(d) for d in descs]
    T_cap = max(lengths)
    rc = be.lib.tq_attention_i8_varlen_fwd(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ctx[guard:].data_ptr(),
                                           ci[guard:].data_ptr(), sd.data_ptr(), len(lengths), M, T_cap, H, D, 0, 0, md.data_ptr(),
                                           float(math.sqrt(D)), *refs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, be.lib.tq_last_error()
    ctx, ci = ctx.cpu(), ci.cpu()
    owned = torch.zeros(guard + M + guard, dtype=torch.bool)
    owned[guard + first:guard + M - extra] = True
    assert bool((ctx[~owned] == 12345.0).all()) and bool((ci[~owned] == 77).all()), 'a row that no sequence owns was written'
    ref, ri = _ragged_on_the_padded_batch(be, q, k, v, s, T_cap, mask, D, qs)
    _assert_owned_rows_equal(ctx[guard:guard + M], ci[guard:guard + M], ref, ri, s)
