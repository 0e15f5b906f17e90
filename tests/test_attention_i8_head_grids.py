"""The attention core with ONE GRID PER HEAD for Q, K, V and the context (include/tq_hip.h: `n_params == H * head_dim`
per-column buffers in natural column order, constant over every head's columns -- the per-embedding-group recipe without
permutation, where a group is a run of whole heads).

Contract, per head: the workgroups of head h read their parameters at column h * head_dim and everything downstream is the
per-tensor kernel's, so ctx and ctx_idx of head h are BIT-IDENTICAL to
  (a) the same entry called with H = 1 on that head's column slice (pointer offset h * head_dim, row stride H * head_dim) with
      the head's parameters as per-tensor quantizers -- whichever launch form either call takes (the forms are bit-identical
      among themselves only where the row sum's order agrees, and the oracle states that order once for all of them), and
  (b) oracle/int_oracle.py on that slice (through the padded reference of tests/_ragged_twin.py, which is the plain oracle
      call at T % 64 == 0).
B = 2, H = 4 throughout, head_dim 64 and 32; the four heads carry four distinct (delta, zero point) pairs for each of Q, K, V
and the context: a query zero point of 0 (c_q = 128: the two-pass correction) NEXT to one of 131, and one at the top of the
grid (255).  Shapes: the smallest that reach each launch form -- T = 64 plain, T = 128 key-split / eight-wave / plain through
the switches the launcher reads per call, T = 50 and 65 on the ragged entry, lengths (1, 37, 64, 20) on the packed entry, and
the strided entry once (Q | K in one stacked buffer, V in another)."""
import ctypes as C
import math

import pytest
import torch

from tests._packed_twin import packed_attention_reference
from tests._ragged_twin import ragged_attention_reference

DEV = 'cuda'
B, H = 2, 4
# (delta, zero point) of heads 0..3
Q_HEADS = [(0.011, 0.0), (0.012, 131.0), (0.0095, 255.0), (0.0105, 120.0)]
K_HEADS = [(0.013, 131.0), (0.010, 97.0), (0.0125, 140.0), (0.0115, 128.0)]
V_HEADS = [(0.009, 128.0), (0.0075, 110.0), (0.0085, 0.0), (0.0095, 255.0)]
C_HEADS = [(0.012, 125.0), (0.010, 131.0), (0.014, 118.0), (0.011, 140.0)]
SCORES, PROBS = (0.35, 128.0), (1.0 / 255, 0.0)
# (q_scores, q_ctx, mask)
USES = [(1, 1, 1), (0, 1, 1), (1, 1, 0), (1, 0, 1)]


def _t(v):
    return torch.tensor(v, dtype=torch.float32)


def _one(pair, dev):
    """per-tensor 7-tuple of a (delta, zero point) pair: device tensors for the backend, python floats for the oracle"""
    d, z = _t(pair[0]), _t(pair[1])
    return (d.to(DEV), z.to(DEV), None, 8, False, False, 1e-8) if dev else (float(d), float(z), None, 8, False, False, 1e-8)


def _wide(pairs, D):
    """per-column buffers [H * D], natural order: head h's pair over its D columns"""
    d = _t([p[0] for p in pairs]).repeat_interleave(D).to(DEV)
    z = _t([p[1] for p in pairs]).repeat_interleave(D).to(DEV)
    return (d, z, None, 8, False, False, 1e-8)


def _quantizers(D, head, dev, use_s=1, use_c=1):
    """head None: the wide set; else head h's per-tensor set"""
    pick = (lambda ps: _wide(ps, D)) if head is None else (lambda ps: _one(ps[head], dev))
    return [pick(Q_HEADS), pick(K_HEADS), pick(V_HEADS), _one(SCORES, dev) if use_s else None, _one(PROBS, dev),
            pick(C_HEADS) if use_c else None]


def _inputs(T, D, seed=0):
    g = torch.Generator().manual_seed(1000 * T + D + seed)
    qi, ki, vi = (torch.randint(-128, 128, (B, T, H * D), generator=g).to(torch.int8) for _ in range(3))
    mask = torch.zeros(B, T)
    mask[0, T - T // 4:] = -10000.0
    mask[1, 1:T // 2] = -10000.0
    return qi, ki, vi, mask


def _head(t, h, D):
    return t[..., h * D:(h + 1) * D]


_ORACLE = {}


def _oracle(T, D, h, use_s, use_c, use_m):
    """oracle/int_oracle.py on head h's slice: once per problem, shared by every launch form, never modified"""
    key = (T, D, h, use_s, use_c, use_m)
    if key not in _ORACLE:
        qi, ki, vi, mask = _inputs(T, D)
        _ORACLE[key] = ragged_attention_reference(_head(qi, h, D), _head(ki, h, D), _head(vi, h, D), 1, mask if use_m else None,
                                                  math.sqrt(D), *_quantizers(D, h, False, use_s, use_c))
    return _ORACLE[key]


def _assert_heads(D, out_wide, per_head_kernel, per_head_oracle, use_c, rows=slice(None)):
    """out_wide: (ctx, ctx_idx | None) [.., H * D] of the wide call; per_head_*: h -> (ctx, ctx_idx) [.., D]"""
    ctx, ci = out_wide
    for h in range(H):
        for what, ref in (('the H = 1 launch', per_head_kernel(h)), ('the integer oracle', per_head_oracle(h))):
            rc, ri = ref
            assert torch.equal(_head(ctx, h, D)[rows], rc[rows]), f'head {h}: context values differ from {what}'
            if use_c:
                assert torch.equal(_head(ci, h, D)[rows], ri[rows]), f'head {h}: context indices differ from {what}'
        assert torch.isfinite(_head(ctx, h, D)[rows]).all()


def _check_dense(method, T, D):
    from quantization import _hip
    be = _hip.backend()
    fn = getattr(be, method)
    qi, ki, vi, mask = _inputs(T, D)
    qd, kd, vd, md = qi.to(DEV), ki.to(DEV), vi.to(DEV), mask.to(DEV)
    for use_s, use_c, use_m in USES:
        m = md if use_m else None

        def call(q, k, v, heads, qs):
            out = fn(q, k, v, heads, m, math.sqrt(D), *qs, want_idx=bool(use_c))
            return (out[0].cpu(), out[1].cpu()) if use_c else (out.cpu(), None)
        wide = call(qd, kd, vd, H, _quantizers(D, None, True, use_s, use_c))
        assert wide[0].shape == (B, T, H * D)
        _assert_heads(D, wide,
                      lambda h: call(_head(qd, h, D), _head(kd, h, D), _head(vd, h, D), 1, _quantizers(D, h, True, use_s, use_c)),
                      lambda h: _oracle(T, D, h, use_s, use_c, use_m), use_c)


def _set_env(monkeypatch, env):
    for v in ('TQ_ATTN_SPLIT', 'TQ_ATTN_QW', 'TQ_ATTN_FAST'):
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


FORMS = [(64, {}), (128, {'TQ_ATTN_SPLIT': '1'}), (128, {'TQ_ATTN_SPLIT': '0'}), (128, {'TQ_ATTN_SPLIT': '0', 'TQ_ATTN_QW': '0'})]


@pytest.mark.gpu
@pytest.mark.parametrize('D', [64, 32])
@pytest.mark.parametrize('T,env', FORMS, ids=['T64-plain', 'T128-key-split', 'T128-eight-wave', 'T128-plain'])
def test_head_grids_equal_one_head_launches_and_the_oracle(T, env, D, monkeypatch):
    _set_env(monkeypatch, env)
    _check_dense('attention_i8', T, D)


@pytest.mark.gpu
@pytest.mark.parametrize('D', [64, 32])
@pytest.mark.parametrize('T', [50, 65])
def test_head_grids_on_the_ragged_entry(T, D, monkeypatch):
    _set_env(monkeypatch, {})
    _check_dense('attention_i8_ragged', T, D)


@pytest.mark.gpu
def test_head_grids_on_the_plain_ragged_form_at_128_keys(monkeypatch):
    """T = 100 (T_pad = 128), head_dim 64, with both switches off: the plain two-wave ragged form, the ONE instantiation that
    keeps the per-tensor parameter fetch (csrc/tq_attention_i8.hip: kRaggedPerTensorOnly) -- the wide call is launched on its
    twin attention_i8_ragged_heads_k, the H = 1 references with per-tensor grids on the kernel itself."""
    _set_env(monkeypatch, {'TQ_ATTN_SPLIT': '0', 'TQ_ATTN_QW': '0'})
    _check_dense('attention_i8_ragged', 100, 64)


def _packed_problem(D):
    lengths = (1, 37, 64, 20)
    s = torch.tensor([0, 1, 38, 102, 122], dtype=torch.int32)
    M = int(s[-1])
    g = torch.Generator().manual_seed(4242 + D)
    q, k, v = (torch.randint(-128, 128, (1, M, H * D), generator=g).to(torch.int8) for _ in range(3))
    mask = torch.randn(M, generator=g) * 0.5
    mask[torch.rand(M, generator=g) < 0.25] = -10000.0
    mask[s[:-1].long()] = 0.25                          # no query row is masked completely
    return lengths, s, M, q, k, v, mask


@pytest.mark.gpu
@pytest.mark.parametrize('D', [64, 32])
def test_head_grids_on_the_packed_entry(D, monkeypatch):
    from quantization import _hip
    _set_env(monkeypatch, {})
    be = _hip.backend()
    lengths, s, M, q, k, v, mask = _packed_problem(D)
    qd, kd, vd, sd, md = q.to(DEV), k.to(DEV), v.to(DEV), s.to(DEV), mask.to(DEV)
    owned = slice(0, M)                                  # every row belongs to a sequence here
    for use_s, use_c, use_m in USES:
        m = md if use_m else None

        def call(a, b_, c, heads, qs):
            out = be.attention_i8_varlen(a, b_, c, heads, sd, max(lengths), m, math.sqrt(D), *qs, want_idx=bool(use_c))
            return (out[0].cpu(), out[1].cpu()) if use_c else (out.cpu(), None)
        wide = call(qd, kd, vd, H, _quantizers(D, None, True, use_s, use_c))
        _assert_heads(D, wide,
                      lambda h: call(_head(qd, h, D), _head(kd, h, D), _head(vd, h, D), 1, _quantizers(D, h, True, use_s, use_c)),
                      lambda h: packed_attention_reference(_head(q, h, D), _head(k, h, D), _head(v, h, D), 1, s, max(lengths),
                                                           mask if use_m else None, math.sqrt(D),
                                                           *_quantizers(D, h, False, use_s, use_c)),
                      use_c, rows=(0, owned))


@pytest.mark.gpu
def test_head_grids_on_the_strided_entry():
    """Q | K as column blocks of one [B, T, 2 H d] buffer, V a column block of a [B, T, 3 H d] buffer: two row strides; the
    parameter index is the head's, whatever the strides of the data"""
    from quantization import _hip
    be = _hip.backend()
    T, D = 64, 64
    HD = H * D
    qi, ki, vi, mask = _inputs(T, D)
    g = torch.Generator().manual_seed(9)
    qk = torch.randint(-128, 128, (B, T, 2 * HD), generator=g).to(torch.int8)
    vb = torch.randint(-128, 128, (B, T, 3 * HD), generator=g).to(torch.int8)
    qk[..., :HD], qk[..., HD:], vb[..., 2 * HD:] = qi, ki, vi
    qk, vb = qk.to(DEV), vb.to(DEV)
    q, k, v = qk[..., :HD], qk[..., HD:], vb[..., 2 * HD:]
    assert q.stride() == k.stride() == (T * 2 * HD, 2 * HD, 1) and v.stride(1) == 3 * HD
    seen, lib = [], be.lib

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name != 'tq_attention_i8_strided_fwd':
                return fn
            return lambda *a: (seen.append(a[:3] + a[9:11]), fn(*a))[1]
    be.lib = Spy()
    try:
        ctx, ci = be.attention_i8(q, k, v, H, mask.to(DEV), math.sqrt(D), *_quantizers(D, None, True), want_idx=True)
    finally:
        be.lib = lib
    assert seen == [(q.data_ptr(), k.data_ptr(), v.data_ptr(), 2 * HD, 3 * HD)], 'the operands were copied'
    ctx, ci = ctx.cpu(), ci.cpu()
    for h in range(H):
        rc, ri = _oracle(T, D, h, 1, 1, 1)
        assert torch.equal(_head(ci, h, D), ri) and torch.equal(_head(ctx, h, D), rc), f'head {h}'


@pytest.mark.gpu
@pytest.mark.parametrize('method,T', [('attention_i8', 64), ('attention_i8', 128), ('attention_i8_ragged', 50)])
def test_wide_buffers_of_equal_heads_give_the_per_tensor_bits(method, T, monkeypatch):
    from quantization import _hip
    _set_env(monkeypatch, {})
    be = _hip.backend()
    D = 64
    qi, ki, vi, mask = _inputs(T, D, seed=3)
    args = (qi.to(DEV), ki.to(DEV), vi.to(DEV), H, mask.to(DEV), math.sqrt(D))
    pairs = (Q_HEADS[1], K_HEADS[0], V_HEADS[1], C_HEADS[0])
    wide = [_wide([p] * H, D) for p in pairs]
    one = [_one(p, True) for p in pairs]
    sp = (_one(SCORES, True), _one(PROBS, True))
    a = getattr(be, method)(*args, wide[0], wide[1], wide[2], *sp, wide[3], want_idx=True)
    b = getattr(be, method)(*args, one[0], one[1], one[2], *sp, one[3], want_idx=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and a mixed call: only the keys and the context wide
    c = getattr(be, method)(*args, one[0], wide[1], one[2], *sp, wide[3], want_idx=True)
    assert torch.equal(c[0], b[0]) and torch.equal(c[1], b[1])


def _descs(be, qs):
    descs = [None if x is None else be._qdesc(*x, x[0].numel(), 1) for x in qs]
    return descs, [None if d is None else C.byref(d) for d in descs]


@pytest.mark.gpu
def test_ragged_entry_with_head_grids_touches_only_its_rows():
    """raw entry point on sentinel-filled ctx / ctx_idx with 64 rows behind row B * T: they keep their sentinels"""
    from quantization import _hip
    be = _hip.backend()
    T, D = 50, 64
    HD, rows, extra = H * D, B * T, 64
    qi, ki, vi, mask = _inputs(T, D)
    bufs = [t.reshape(rows, HD).to(DEV) for t in (qi, ki, vi)]
    md = mask.reshape(-1).to(DEV)
    ctx = torch.full((rows + extra, HD), 12345.0, device=DEV)
    ci = torch.full((rows + extra, HD), 77, dtype=torch.int8, device=DEV)
    keep, refs = _descs(be, _quantizers(D, None, True))
    rc = be.lib.tq_attention_i8_ragged_fwd(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ctx.data_ptr(), ci.data_ptr(),
                                           B, T, H, D, 0, 0, md.data_ptr(), float(math.sqrt(D)), *refs,
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, be.lib.tq_last_error()
    assert bool((ctx[rows:] == 12345.0).all()) and bool((ci[rows:] == 77).all()), 'rows behind B * T were written'
    ctx, ci = ctx[:rows].cpu().reshape(B, T, HD), ci[:rows].cpu().reshape(B, T, HD)
    for h in range(H):
        rc_, ri = _oracle(T, D, h, 1, 1, 1)
        assert torch.equal(_head(ci, h, D), ri) and torch.equal(_head(ctx, h, D), rc_), f'head {h}'


@pytest.mark.gpu
def test_packed_entry_with_head_grids_writes_only_owned_rows():
    """3 unowned rows in front of the first sequence and 7 behind the last one inside the total_rows rows, 8 guard rows on
    either side outside them: all keep their sentinels, the owned rows hold the oracle's bits"""
    from quantization import _hip
    be = _hip.backend()
    D, first, extra, guard = 64, 3, 7, 8
    HD = H * D
    lengths, s0, M0, q0, k0, v0, mask0 = _packed_problem(D)
    M = first + M0 + extra
    s = s0 + first
    g = torch.Generator().manual_seed(5)
    bufs, host = [], []
    for t in (q0, k0, v0):
        b_ = torch.randint(-128, 128, (1, M, HD), generator=g).to(torch.int8)
        b_[0, first:first + M0] = t[0]
        host.append(b_)
        bufs.append(b_[0].to(DEV).contiguous())
    mask = torch.zeros(M)
    mask[first:first + M0] = mask0
    ctx = torch.full((guard + M + guard, HD), 12345.0, device=DEV)
    ci = torch.full((guard + M + guard, HD), 77, dtype=torch.int8, device=DEV)
    sd, md = s.to(DEV), mask.to(DEV)
    keep, refs = _descs(be, _quantizers(D, None, True))
    rc = be.lib.tq_attention_i8_varlen_fwd(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ctx[guard:].data_ptr(),
                                           ci[guard:].data_ptr(), sd.data_ptr(), len(lengths), M, max(lengths), H, D, 0, 0,
                                           md.data_ptr(), float(math.sqrt(D)), *refs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, be.lib.tq_last_error()
    ctx, ci = ctx.cpu(), ci.cpu()
    owned = torch.zeros(guard + M + guard, dtype=torch.bool)
    owned[guard + first:guard + M - extra] = True
    assert bool((ctx[~owned] == 12345.0).all()) and bool((ci[~owned] == 77).all()), 'a row that no sequence owns was written'
    for h in range(H):
        rc_, ri = packed_attention_reference(_head(host[0], h, D), _head(host[1], h, D), _head(host[2], h, D), 1, s, max(lengths),
                                             mask, math.sqrt(D), *_quantizers(D, h, False))
        got_c, got_i = _head(ctx[guard:guard + M], h, D), _head(ci[guard:guard + M], h, D)
        assert torch.equal(got_i[first:M - extra], ri[0, first:M - extra]), f'head {h}'
        assert torch.equal(got_c[first:M - extra], rc_[0, first:M - extra]), f'head {h}'


def test_argument_errors_come_before_any_device_access():
    """raw ctypes, no device (fake addresses that are never dereferenced): every refused form of a wide grid is -1 with a
    message, on all four entry points"""
    from quantization import _hip
    lib = _hip.load_library()
    Hh, D = 4, 64
    fake = 1 << 20
    mk = lambda n_params=1, inner=1, sym=0, log=0, bits=8: _hip.tq_quantizer(fake, fake, None, bits, sym, log, 1e-8,
                                                                             n_params, inner)
    one = mk()

    def entries(q_q, q_k, q_v, q_s, q_p, q_c, T=64):
        r = [None if d is None else C.byref(d) for d in (q_q, q_k, q_v, q_s, q_p, q_c)]
        yield 'fwd', lib.tq_attention_i8_fwd(fake, fake, fake, fake, None, 2, T, Hh, D, 0, None, 8.0, *r, None)
        yield 'strided', lib.tq_attention_i8_strided_fwd(fake, fake, fake, fake, None, 2, T, Hh, D, 0, 0, None, 8.0, *r, None)
        yield 'ragged', lib.tq_attention_i8_ragged_fwd(fake, fake, fake, fake, None, 2, 50, Hh, D, 0, 0, None, 8.0, *r, None)
        yield 'varlen', lib.tq_attention_i8_varlen_fwd(fake, fake, fake, fake, None, fake, 2, 100, 50, Hh, D, 0, 0, None, 8.0, *r, None)

    def refused(word, *qs):
        for name, rc in entries(*qs):
            msg = lib.tq_last_error().decode()
            assert rc == -1 and any(w in msg for w in word.split('|')), (name, rc, msg)
    for bad in (mk(7), mk(Hh * D + 64), mk(Hh * D, inner=2)):
        refused('n_params', bad, one, one, None, one, None)
        refused('n_params', one, bad, one, None, one, None)
        refused('n_params', one, one, bad, None, one, None)
        refused('n_params', one, one, one, None, one, bad)
    wide_sym, wide_log, wide9 = mk(Hh * D, sym=1), mk(Hh * D, log=1), mk(Hh * D, bits=9)
    for bad in (wide_sym, wide_log, wide9):
        refused('per-head', bad, one, one, None, one, None)
        refused('per-head', one, one, bad, None, one, None)
    refused('per-head', one, one, one, None, one, wide_sym)
    refused('per-head', one, one, one, None, one, wide_log)
    refused('per-tensor', one, one, one, None, mk(Hh * D), None)            # wide probabilities
    # wide scores: the generic quantizer checks come first, as they always did (T = 50: 2 * 4 * 50 * 50 scores are no multiple
    # of 256 parameters), then the per-tensor rule
    refused('per-tensor|n_params', one, one, one, mk(Hh * D), one, None)
