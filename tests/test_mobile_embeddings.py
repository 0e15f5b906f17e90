"""MobileBERT's embedding block as ONE exact integer launch (tq_mobile_embeddings_nonorm_quant_fwd) against the reference
built here: a numpy gather of the int8 word rows into the trigram, an int64 contraction and the CPU element functions of the
other exact tests (tests/_mobile_embeddings_twin.mobile_embeddings_chain).  Exact integers and single IEEE fp32 operations on
both sides: every comparison is torch.equal.  Shapes around the kernel's chunk of R = 16 tokens."""
import numpy as np
import pytest
import torch

from tests._exact_backend import _p
from tests._mobile_embeddings_twin import mobile_embeddings_chain

pytestmark = pytest.mark.gpu

R, VOCAB, E, N, POSITIONS, TYPES = 16, 100, 128, 512, 64, 2
EPS = 1e-8


def _grid(v, n_bits):
    """an asymmetric per-tensor 7-tuple that clips a little of v at both ends"""
    lo, hi = float(v.min()), float(v.max())
    delta = np.float32(0.9 * (hi - lo) / (2 ** n_bits - 1))
    return (torch.tensor(delta), torch.tensor(np.float32(-0.95 * lo / delta)), None, n_bits, False, False, EPS)


def _case(B, T, bits, per_channel, use=(True, True, True, True), seed=0):
    """operands (CPU) and the quantizers of the sites in `use`"""
    g = np.random.default_rng(seed)
    half = 2 ** (bits - 1)
    o = dict(e_idx=g.integers(-half, half, (VOCAB, E)).astype(np.int8), w_idx=g.integers(-half, half, (N, 3 * E)).astype(np.int8),
             ids=g.integers(0, VOCAB, (B, T)), e_delta=np.float32(0.013),
             w_delta=(g.uniform(0.004, 0.012, N) if per_channel else g.uniform(0.004, 0.012, 1)).astype(np.float32),
             bias=g.normal(0, 0.5, N).astype(np.float32), pos=torch.from_numpy(g.normal(0, 1, (POSITIONS, N)).astype(np.float32)),
             typ=torch.from_numpy(g.normal(0, 1, (TYPES, N)).astype(np.float32)),
             nn_w=torch.from_numpy(g.normal(1, 0.3, N).astype(np.float32)), nn_b=torch.from_numpy(g.normal(0, 0.3, N).astype(np.float32)),
             pos_ids=torch.arange(T).repeat(B), type_ids=torch.from_numpy(g.integers(0, TYPES, B * T)))
    free = _reference(o, [None] * 4)[0]      # every site's range from the un-quantized chain's output (the widest of the four)
    return o, [_grid(free, bits) if on else None for on in use]


def _reference(o, qs):
    return mobile_embeddings_chain(o['e_idx'], o['ids'], o['e_delta'], EPS, o['w_idx'], o['w_delta'], EPS, o['bias'], o['pos'],
                                   o['pos_ids'], o['typ'], o['type_ids'], o['nn_w'], o['nn_b'], *[_p(q) for q in qs])


def _dev(q):
    return None if q is None else tuple(t.cuda() if torch.is_tensor(t) else t for t in q)


def _launch(be, o, qs, want_idx, ids=None, pos_ids=None, type_ids=None):
    c = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).cuda()
    return be.mobile_embeddings_nonorm_quant(
        c(o['e_idx']), c(o['e_delta']).reshape(1), EPS, c(o['ids'] if ids is None else ids), c(o['w_idx']), c(o['w_delta']), EPS,
        c(o['bias']), c(o['pos']), c(o['pos_ids'] if pos_ids is None else pos_ids), c(o['typ']),
        c(o['type_ids'] if type_ids is None else type_ids), c(o['nn_w']), c(o['nn_b']), *[_dev(q) for q in qs], want_idx=want_idx)


def _chained(be, o, qs, tri):
    """the launches the block replaces, on the explicitly built trigram: tq_linear_i8_fwd (input zero point 128; the backend
    pads the rows to its tile rule), the two adds, tq_fake_quant_fwd twice, tq_affine_fake_quant_fwd"""
    c = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).cuda()
    w_idx = c(o['w_idx'])
    x_q = (c(o['e_delta']).reshape(1), torch.tensor([128.0], device='cuda'), 8, EPS)
    a = be.linear_i8(c(tri), w_idx, be.rowsum_i8(w_idx), c(o['bias']), x_q, c(o['w_delta']), EPS, 0, _dev(qs[0]), torch.float32)
    a = a + c(o['pos'])[c(o['pos_ids'])]
    if qs[1] is not None:
        a = be.fake_quant(a, *_dev(qs[1]), 1, 1)[0]
    a = a + c(o['typ'])[c(o['type_ids'])]
    if qs[2] is not None:
        a = be.fake_quant(a, *_dev(qs[2]), 1, 1)[0]
    if qs[3] is None:
        return a * c(o['nn_w']) + c(o['nn_b']), None
    return be.affine_fake_quant(a, c(o['nn_w']), c(o['nn_b']), *_dev(qs[3]), want_idx=True)


ALL = (True, True, True, True)


@pytest.mark.parametrize('B,T,bits,per_channel,want_idx,use', [
    (1, 1, 8, True, True, ALL),                                     # both halos zero
    (2, 3, 4, False, False, ALL),                                   # T < R, two sequences
    (2, R, 8, False, True, (False, True, True, True)),              # a full chunk; Q_t absent
    (2, R + 1, 4, True, True, (True, False, True, True)),           # halo from the neighbouring chunk + a one-token chunk; Q_1 absent
    (3, 50, 4, False, True, (True, True, False, True)),             # a partial last chunk; Q_2 absent
    (3, 50, 8, True, False, (True, True, True, False)),             # Q_3 absent (no indices)
])
def test_block_equals_reference_and_chained_launches(B, T, bits, per_channel, want_idx, use):
    from quantization import _hip
    be = _hip.backend()
    o, qs = _case(B, T, bits, per_channel, use)
    ref_y, ref_idx, tri = _reference(o, qs)
    out = _launch(be, o, qs, want_idx)
    y, idx = out if want_idx else (out, None)
    assert y.shape == (B * T, N) and torch.isfinite(y).all()
    assert torch.equal(y.cpu(), ref_y)
    if want_idx:
        assert torch.equal(idx.cpu(), (ref_idx - 128).to(torch.int8))
    ch_y, ch_idx = _chained(be, o, qs, tri)
    assert torch.equal(y, ch_y)
    if want_idx:
        assert torch.equal(idx, ch_idx)


def test_a_chunk_never_sees_the_next_sequence():
    """the second sequence differs from the first only in its first token: the last row of sequence 0 keeps its bits"""
    from quantization import _hip
    be = _hip.backend()
    o, qs = _case(2, R, 8, False)
    same = np.stack([o['ids'][0], o['ids'][0]])
    other = same.copy()
    other[1, 0] = (other[1, 0] + 1) % VOCAB
    y_same, y_other = (_launch(be, o, qs, False, ids=i).cpu().view(2, R, N) for i in (same, other))
    assert torch.equal(y_same[0], y_other[0])
    assert not torch.equal(y_other[1, 0], y_same[1, 0]) and not torch.equal(y_other[1, 1], y_same[1, 1])
    assert torch.equal(y_other[1, 2:], y_same[1, 2:])
    assert torch.equal(y_other.view(-1, N), _reference(dict(o, ids=other), qs)[0])


@pytest.mark.parametrize('table,b,t', [('word', 0, 0), ('word', 1, R), ('word', 2, 19), ('pos', 1, 5), ('type', 0, 19)])
def test_out_of_range_ids_make_nan_rows_and_raise_the_flag(table, b, t):
    """a word id outside the table: rows t-1, t, t+1 of its sequence (the trigrams that touch it) are NaN as a whole, every
    other row keeps its bits; a position / token-type id: its own row.  The flag becomes the deferred IndexError."""
    from quantization import _hip
    be = _hip.backend()
    B, T = 3, 20
    o, qs = _case(B, T, 8, False)
    y_ok, i_ok = _launch(be, o, qs, True)
    bad = {k: torch.as_tensor(o[k]).clone() for k in ('ids', 'pos_ids', 'type_ids')}
    if table == 'word':
        bad['ids'][b, t] = VOCAB if t else -1
        rows = [b * T + s for s in (t - 1, t, t + 1) if 0 <= s < T]
    else:
        bad['pos_ids' if table == 'pos' else 'type_ids'][b * T + t] = POSITIONS if table == 'pos' else -2
        rows = [b * T + t]
    y_bad, i_bad = _launch(be, o, qs, True, ids=bad['ids'], pos_ids=bad['pos_ids'], type_ids=bad['type_ids'])
    torch.cuda.synchronize()
    assert int(be._bad_ids_flag()[0]) == 1
    with pytest.raises(IndexError):
        be.raise_deferred()
    nan_rows = torch.isnan(y_bad).all(1).cpu()
    assert nan_rows.nonzero().flatten().tolist() == rows and not torch.isnan(y_bad[~nan_rows.cuda()]).any()
    keep = ~nan_rows.cuda()
    assert torch.equal(y_bad[keep], y_ok[keep]) and torch.equal(i_bad[keep], i_ok[keep])
