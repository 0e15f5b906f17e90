"""The integer attention cores at the ends of their zero points and of their second contraction.

tests/test_attention_i8.py sweeps the query zero point alone; c_k, c_v and c_p (c = 128 - z) enter through
q_const = c_k rsq + DH c_q c_k and p_const = c_v rsp + T c_p c_v and have only ever run at 131 / 128 / 0.  Here:

* (z_k, z_v, z_p) over {0, 255}^3 and (1, 254, 37) on every launch form of tq_attention_i8_fwd -- plain, key-split, eight
  query waves, head dim 32, and T = 384 (the guarded element chain) -- with and without the scores quantizer;
* a NON-ZERO probability zero point on the pad-key forms (tq_attention_i8_ragged_fwd, tq_attention_i8_varlen_fwd), whose
  contract rests on "a pad key's probability index is the zero point, so its term (a'_p + c_p)(a'_v + c_v) is 0" with T in
  p_const the PADDED length (header of csrc/tq_attention_i8_body.h) -- only ever run with z_p = 0; guard rows around the
  outputs stay untouched;
* the second contraction above 2^24 (its ceiling is T 255 255 = 3.3e7 at T = 512), where (float)(acc + c_p csv + p_const)
  rounds: every probability clamped to index 255, V at the ends of its grid.  The CPU test reads the oracle's probability
  indices back through one-hot V operands, restates the contraction in int64 and ties the oracle's int32 sums to it.

Reference throughout: oracle/tq_int_oracle.c (on the padded batch with -inf at the pad keys for the pad-key forms), values
and int8 indices compared with torch.equal."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import int_oracle as IO
from tests._packed_twin import packed_attention_reference
from tests._ragged_twin import ragged_attention_reference

gpu = pytest.mark.gpu

DEV = 'cuda'
ATTN_ENV = ('TQ_ATTN_SPLIT', 'TQ_ATTN_QW', 'TQ_ATTN_FAST')

# the helpers of tests/test_attention_i8.py::test_query_zero_point_extremes_equal_the_integer_oracle
mk = lambda d, z, nb=8: (torch.tensor(d), torch.tensor(z), None, nb, False, False, 1e-8)
f = lambda q: None if q is None else (float(q[0]), float(q[1]), None, q[3], False, False, q[6])
dev = lambda q: None if q is None else (q[0].to(DEV), q[1].to(DEV), None, q[3], False, False, q[6])


def _env(monkeypatch, env):
    for v in ATTN_ENV:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)               # read per call by the launcher


# ---- zero-point ends of K, V and P ---------------------------------------------------------------------------------------------
ZERO_POINTS = list(itertools.product((0, 255), repeat=3)) + [(1, 254, 37)]
# (T, head dim, switches): plain | head dim 32 (key-split by default) | one-wave rows, two query waves | key-split | eight query
# waves | T > 256: the guarded quantizer / quotient chain (key-split by default)
FORMS = {
    'T64': (64, 64, {}),
    'T128-d32': (128, 32, {}),
    'T128-plain': (128, 64, {'TQ_ATTN_SPLIT': '0', 'TQ_ATTN_QW': '2'}),
    'T128-split': (128, 64, {'TQ_ATTN_SPLIT': '1'}),
    'T128-eight-waves': (128, 64, {'TQ_ATTN_SPLIT': '0', 'TQ_ATTN_QW': '8'}),
    'T384-guarded': (384, 64, {}),
}


def _zp_quantizers(zk, zv, zp, dh, scores):
    """the grids of tests/test_int_oracle.py with the zero points under test; the probability grid is four times finer, so
    that the indices spread over it and reach its top where z_p is large"""
    q_c = mk(0.15, 8.0, 4) if dh == 32 else mk(0.012, 125.0)
    return (mk(0.011, 120.0), mk(0.013, float(zk)), mk(0.009, float(zv)), mk(0.35, 128.0) if scores else None,
            mk(1.0 / 1020, float(zp)), q_c)


def _zp_inputs(T, dh):
    B, H = 2, 2
    g = torch.Generator().manual_seed(97 * T + dh)
    qi, ki, vi = (torch.randint(-128, 128, (B, T, H * dh), generator=g).to(torch.int8) for _ in range(3))
    mask = torch.zeros(B, T)
    mask[1, T - 9:] = -10000.0
    return qi, ki, vi, H, mask


_REF = {}


def _zp_reference(T, dh, zps, scores):
    """computed once per problem, shared by the launch forms of (128, 64), never modified"""
    key = (T, dh, zps, scores)
    if key not in _REF:
        qi, ki, vi, H, mask = _zp_inputs(T, dh)
        _REF[key] = IO.attention_i8(qi, ki, vi, H, mask, math.sqrt(dh), *[f(q) for q in _zp_quantizers(*zps, dh, scores)])
    return _REF[key]


@gpu
@pytest.mark.parametrize('zps', ZERO_POINTS, ids=lambda z: 'zk%d-zv%d-zp%d' % z)
@pytest.mark.parametrize('form', list(FORMS))
def test_key_value_probability_zero_point_ends_equal_the_oracle(form, zps, monkeypatch):
    from quantization import _hip
    be = _hip.backend()
    T, dh, env = FORMS[form]
    _env(monkeypatch, env)
    qi, ki, vi, H, mask = _zp_inputs(T, dh)
    for scores in (True, False):
        qs = _zp_quantizers(*zps, dh, scores)
        ctx, ci = be.attention_i8(qi.to(DEV), ki.to(DEV), vi.to(DEV), H, mask.to(DEV), math.sqrt(dh), *[dev(q) for q in qs],
                                  want_idx=True)
        ref, ri = _zp_reference(T, dh, zps, scores)
        assert torch.isfinite(ref).all()
        assert torch.equal(ci.cpu(), ri), f'scores={scores}: {int((ci.cpu() != ri).sum())} of {ri.numel()} context indices differ'
        assert torch.equal(ctx.cpu(), ref), f'scores={scores}: context values differ'


# ---- a non-zero probability zero point on the pad-key forms ----------------------------------------------------------------------
PAD_ZERO_POINTS = list(itertools.product((37, 255), (0, 255)))          # (z_p, z_v)
H_PAD, D_PAD, GUARD = 2, 64, 8


def _pad_quantizers(zp, zv):
    return (mk(0.011, 120.0), mk(0.013, 131.0), mk(0.009, float(zv)), mk(0.35, 128.0), mk(1.0 / 1020, float(zp)), mk(0.012, 125.0))


def _guarded_outputs(rows, HD):
    """ctx / ctx_idx with GUARD sentinel rows on either side of the `rows` rows the entry point is handed"""
    ctx = torch.full((GUARD + rows + GUARD, HD), 12345.0, device=DEV)
    ci = torch.full((GUARD + rows + GUARD, HD), 77, dtype=torch.int8, device=DEV)
    return ctx, ci


def _assert_guards_untouched(ctx, ci, written):
    """written: bool [rows] -- the rows inside the guards that the launch owns"""
    own = torch.zeros(ctx.shape[0], dtype=torch.bool)
    own[GUARD:ctx.shape[0] - GUARD] = written
    assert bool((ctx[~own] == 12345.0).all()) and bool((ci[~own] == 77).all()), 'a row outside the owned rows was written'


@gpu
@pytest.mark.parametrize('zp,zv', PAD_ZERO_POINTS, ids=lambda v: str(v))
@pytest.mark.parametrize('T', [100, 1])
def test_ragged_core_with_a_nonzero_probability_zero_point(T, zp, zv, monkeypatch):
    """T = 100: T_pad = 128, 28 pad keys per sequence (the key-split form, the default on this grid); T = 1: 63 pad keys"""
    from quantization import _hip
    be = _hip.backend()
    _env(monkeypatch, {})
    B, HD = 2, H_PAD * D_PAD
    g = torch.Generator().manual_seed(1000 + T)
    qi, ki, vi = (torch.randint(-128, 128, (B, T, HD), generator=g).to(torch.int8) for _ in range(3))
    mask = torch.zeros(B, T)
    if T > 9:
        mask[1, T - 9:] = -10000.0
    qs = _pad_quantizers(zp, zv)
    ref, ri = ragged_attention_reference(qi, ki, vi, H_PAD, mask, math.sqrt(D_PAD), *[f(q) for q in qs], pad='random', seed=3)
    assert torch.isfinite(ref).all() and (zp == 255 or ri.unique().numel() > 1)
    rows = B * T
    ctx, ci = _guarded_outputs(rows, HD)
    qd = [dev(q) for q in qs]                                # (a descriptor holds the addresses of these buffers)
    descs = [be._qdesc(*q, 1, 1) for q in qd]
    bufs = [t.reshape(rows, HD).to(DEV) for t in (qi, ki, vi)]
    m = mask.reshape(-1).to(DEV)
    rc = be.lib.tq_attention_i8_ragged_fwd(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ctx[GUARD:].data_ptr(),
                                           ci[GUARD:].data_ptr(), B, T, H_PAD, D_PAD, 0, 0, m.data_ptr(), float(math.sqrt(D_PAD)),
                                           *[C.byref(d) for d in descs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, be.lib.tq_last_error()
    ctx, ci = ctx.cpu(), ci.cpu()
    _assert_guards_untouched(ctx, ci, torch.ones(rows, dtype=torch.bool))
    assert torch.equal(ci[GUARD:GUARD + rows].reshape(B, T, HD), ri), 'context indices differ'
    assert torch.equal(ctx[GUARD:GUARD + rows].reshape(B, T, HD), ref), 'context values differ'
    # and through the backend method (its own output buffers)
    c2, i2 = be.attention_i8_ragged(qi.to(DEV), ki.to(DEV), vi.to(DEV), H_PAD, mask.to(DEV), math.sqrt(D_PAD),
                                    *[dev(q) for q in qs], want_idx=True)
    assert torch.equal(i2.cpu(), ri) and torch.equal(c2.cpu(), ref)


@gpu
@pytest.mark.parametrize('zp,zv', PAD_ZERO_POINTS, ids=lambda v: str(v))
def test_varlen_core_with_a_nonzero_probability_zero_point(zp, zv, monkeypatch):
    """lengths (100, 1, 64, 17) packed, T_cap = 100 -> T_pad = 128: 28, 127, 64 and 111 pad keys; 3 unowned rows in front of the
    first sequence and 5 behind the last inside total_rows, guard rows outside"""
    from quantization import _hip
    be = _hip.backend()
    _env(monkeypatch, {})
    lengths, first, extra, HD = (100, 1, 64, 17), 3, 5, H_PAD * D_PAD
    s = torch.tensor(np.concatenate([[first], first + np.cumsum(lengths)]), dtype=torch.int32)
    M = int(s[-1]) + extra
    g = torch.Generator().manual_seed(2000)
    q, k, v = (torch.randint(-128, 128, (1, M, HD), generator=g).to(torch.int8) for _ in range(3))
    mask = torch.zeros(M)
    mask[int(s[1]) - 9:int(s[1])] = -10000.0                 # the last 9 keys of the first sequence
    qs = _pad_quantizers(zp, zv)
    ref, ri = packed_attention_reference(q, k, v, H_PAD, s, max(lengths), mask, math.sqrt(D_PAD), *[f(x) for x in qs],
                                         pad='random', seed=5)
    owned = torch.zeros(M, dtype=torch.bool)
    owned[first:M - extra] = True
    assert torch.isfinite(ref).all() and (zp == 255 or ri[0, owned].unique().numel() > 1)
    ctx, ci = _guarded_outputs(M, HD)
    qd = [dev(x) for x in qs]                                # (a descriptor holds the addresses of these buffers)
    descs = [be._qdesc(*x, 1, 1) for x in qd]
    bufs = [t[0].to(DEV).contiguous() for t in (q, k, v)]
    sd, md = s.to(DEV), mask.to(DEV)
    rc = be.lib.tq_attention_i8_varlen_fwd(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ctx[GUARD:].data_ptr(),
                                           ci[GUARD:].data_ptr(), sd.data_ptr(), len(lengths), M, max(lengths), H_PAD, D_PAD, 0, 0,
                                           md.data_ptr(), float(math.sqrt(D_PAD)), *[C.byref(d) for d in descs],
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, be.lib.tq_last_error()
    ctx, ci = ctx.cpu(), ci.cpu()
    _assert_guards_untouched(ctx, ci, owned)
    got_c, got_i = ctx[GUARD:GUARD + M], ci[GUARD:GUARD + M]
    for b in range(len(lengths)):
        lo, hi = int(s[b]), int(s[b + 1])
        assert torch.equal(got_i[lo:hi], ri[0, lo:hi]), f'sequence {b} (length {hi - lo}): context indices differ'
        assert torch.equal(got_c[lo:hi], ref[0, lo:hi]), f'sequence {b} (length {hi - lo}): context values differ'
    # and through the backend method (its own output buffers)
    c2, i2 = be.attention_i8_varlen(q.to(DEV), k.to(DEV), v.to(DEV), H_PAD, sd, max(lengths), md, math.sqrt(D_PAD),
                                    *[dev(x) for x in qs], want_idx=True)
    assert torch.equal(i2[0].cpu()[owned], ri[0, owned]) and torch.equal(c2[0].cpu()[owned], ref[0, owned])


# ---- the second contraction above 2^24 -----------------------------------------------------------------------------------------
Z_Q, D_SAT = 120, 64


def _sat_problem(T):
    """B = H = 1.  Every query sits ON its zero point (Q = 0 after dequantisation), so every score is exactly 0 whatever K
    holds and every probability 1 / T; the probability grid has delta = 1 / (255 * 8 * T) and z_p = 0, so 1 / T is 8 times
    beyond its top and every index clamps to 255.  V: index 255 on even head dims, index 0 on odd ones (z_v = 0), with ~3 % of
    every row overwritten by uniform grid values."""
    rng = np.random.default_rng(T)
    qi = torch.full((1, T, D_SAT), Z_Q - 128, dtype=torch.int8)
    ki = torch.from_numpy(rng.integers(-128, 128, (1, T, D_SAT)).astype(np.int8))
    v = np.where(np.arange(D_SAT) % 2 == 0, 127, -128).astype(np.int8)[None, :].repeat(T, 0)
    hit = rng.random(v.shape) < 0.03
    v[hit] = rng.integers(-128, 128, int(hit.sum())).astype(np.int8)
    vi = torch.from_numpy(np.ascontiguousarray(v))[None]
    qs = (mk(0.011, float(Z_Q)), mk(0.013, 131.0), mk(0.009, 0.0), mk(0.35, 128.0), mk(1.0 / (255 * 8 * T), 0.0))
    return qi, ki, vi, qs, mk(0.29 / 255, 2.0)          # T 255 255 s_pv = 0.287: the top of this context grid


def _sat_reference(T, with_ctx):
    key = ('sat', T, with_ctx)
    if key not in _REF:
        qi, ki, vi, qs, q_c = _sat_problem(T)
        _REF[key] = IO.attention_i8(qi, ki, vi, 1, None, math.sqrt(D_SAT), *[f(q) for q in qs], f(q_c) if with_ctx else None)
    return _REF[key]


@pytest.mark.parametrize('T', [512, 384])
def test_saturated_second_contraction_premise_and_int64_restatement_cpu(T):
    """The oracle's probability indices, read back through V operands that hold index z_v + 1 at (key 64 c + d, dim d) and z_v
    elsewhere (ctx[i, d] = (p[i, 64 c + d] - z_p) s_pv), are all 255; sum_k (p - z_p)(v - z_v) over them in int64 has a maximum
    above 2^24 and below 2^31; and the oracle's fp32 context without a context quantizer is fp32(that sum) * s_pv bit for bit."""
    qi, ki, vi, qs, _ = _sat_problem(T)
    s_pv = np.float32(f(qs[4])[0]) * np.float32(f(qs[2])[0])
    p = np.empty((T, T), np.int64)
    for c in range(T // D_SAT):
        probe = torch.full((1, T, D_SAT), -128, dtype=torch.int8)            # index z_v = 0
        probe[0, D_SAT * c + torch.arange(D_SAT), torch.arange(D_SAT)] = -127  # index 1
        got = IO.attention_i8(qi, ki, probe, 1, None, math.sqrt(D_SAT), *[f(q) for q in qs], None)[0][0].numpy()
        p[:, D_SAT * c:D_SAT * (c + 1)] = np.rint(got.astype(np.float64) / np.float64(s_pv)).astype(np.int64)
    assert p.min() == 255 and p.max() == 255, (p.min(), p.max())
    tot = p @ (vi[0].numpy().astype(np.int64) + 128)                         # z_p = z_v = 0: index = int8 value + 128
    print(f'T = {T}: second contraction in [{tot.min()}, {tot.max()}], 2^{np.log2(tot.max()):.2f}')
    assert tot.max() > 2 ** 24 and tot.max() < 2 ** 31 and (tot[:, 0::2] > 2 ** 24).all() and tot.min() >= 0
    assert len(np.unique(tot[0])) > 8
    want = (tot.astype(np.float32) * s_pv).astype(np.float32)
    ref = _sat_reference(T, False)[0][0].numpy()
    assert np.array_equal(ref.view(np.uint32), want.view(np.uint32))


@gpu
@pytest.mark.parametrize('fast', ['1', '0'], ids=['branch-free', 'guarded'])
@pytest.mark.parametrize('T', [512, 384])
def test_saturated_second_contraction_equals_the_oracle(T, fast, monkeypatch):
    """with and without the context quantizer; TQ_ATTN_FAST=0 keeps the guarded element chain"""
    from quantization import _hip
    be = _hip.backend()
    _env(monkeypatch, {'TQ_ATTN_FAST': fast})
    qi, ki, vi, qs, q_c = _sat_problem(T)
    args = (qi.to(DEV), ki.to(DEV), vi.to(DEV), 1, None, math.sqrt(D_SAT)) + tuple(dev(q) for q in qs)
    ref, ri = _sat_reference(T, True)
    ctx, ci = be.attention_i8(*args, dev(q_c), want_idx=True)
    assert ri.unique().numel() > 8
    assert torch.equal(ci.cpu(), ri), f'{int((ci.cpu() != ri).sum())} of {ri.numel()} context indices differ'
    assert torch.equal(ctx.cpu(), ref)
    raw = be.attention_i8(*args, None)
    assert torch.equal(raw.cpu().view(torch.int32), _sat_reference(T, False)[0].view(torch.int32))
