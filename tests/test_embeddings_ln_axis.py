"""BERT's embedding block as ONE launch behind PER-COLUMN quantizers (tq_embeddings_layernorm_quant_axis_fwd): what the
per-embedding / per-embedding-group (PEG) recipes put on the three activation sites of the block.  Two references, each
matched bit for bit, on y and on y_idx + 128:

    tests._exact_backend.embeddings_chain                   the CPU oracle chain (statistics in the kernel's order)
    residual_layernorm_quant_axis(word[ids] + type[tok], pos[pid], ...)   the GPU's own per-column tail on the gathered rows

Tables: a vocabulary of 97 rows, 2 token types, 40 positions; ids [3, 13] with repeats.  The argument checks at the end need
no GPU."""
import ctypes as C
import itertools

import pytest
import torch

from tests.test_fused_ln_axis import F32_D, _k, _quantizers

EPS = 1e-12
VOCAB, TYPES, POSITIONS = 97, 2, 40
B, T = 3, 13


def _tables(d, seed=0):
    """word + type ~ N(0, 2), pos ~ N(0, 1.5) with one wide column: the sites' ranges of tests/test_fused_ln_axis.py clip
    some columns at both ends and leave others alone"""
    g = torch.Generator().manual_seed(1000 * seed + d + 11)
    word = torch.randn(VOCAB, d, generator=g) * 1.6
    typ = torch.randn(TYPES, d, generator=g) * 1.2
    pos = torch.randn(POSITIONS, d, generator=g) * 1.5
    pos[:, 5] *= 12
    w = 1 + 0.1 * torch.randn(d, generator=g)
    b = 0.05 * torch.randn(d, generator=g)
    return g, word, typ, pos, w, b


def _ids(g, shape=(B, T)):
    ids = torch.randint(0, VOCAB, shape, generator=g)
    ids.view(-1)[:4] = ids.view(-1)[0]                      # repeats
    ids.view(-1)[-1] = ids.view(-1)[5]
    tok = torch.randint(0, TYPES, shape, generator=g)
    pid = torch.randint(0, POSITIONS, shape, generator=g)
    pid.view(-1)[:T] = torch.arange(T)
    return ids, tok, pid


def _spec(p):
    return None if p is None else (p[0], p[1], 8, False, False)


def _chain(word, ids, typ, tok, pos, pid, p1, p2, w, b, p3):
    from tests._exact_backend import embeddings_chain
    y, idx, _ = embeddings_chain(word, ids.reshape(-1), typ, tok.reshape(-1), pos, pid.reshape(-1), _spec(p1), _spec(p2), w, b,
                                 EPS, _spec(p3))
    return y, idx


def _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3, method='embeddings_layernorm_quant_axis'):
    """-> (y, y_idx or None) on the GPU"""
    out = getattr(be, method)(word.cuda(), ids.cuda(), typ.cuda(), tok.cuda(), pos.cuda(), pid.cuda(), _k(p1), _k(p2), w.cuda(),
                              b.cuda(), EPS, _k(p3), want_idx=p3 is not None)
    return (out, None) if p3 is None else out


def _tail(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3):
    """the GPU's per-column tail on the gathered rows (one fp32 addition in front, as in the block) -> (y, y_idx or None)"""
    d = word.shape[-1]
    wc, tc, pc = word.cuda(), typ.cuda(), pos.cuda()
    a = (wc[ids.cuda().reshape(-1)] + tc[tok.cuda().reshape(-1)]).reshape(-1, d)
    r = pc[pid.cuda().reshape(-1)].reshape(-1, d)
    out = be.residual_layernorm_quant_axis(a, r, _k(p1), _k(p2), w.cuda(), b.cuda(), EPS, _k(p3), want_idx=p3 is not None)
    return (out, None) if p3 is None else out


def _same_bits(got, want, what):
    """(y, idx) pairs on one device: the same NaN elements, the same bit patterns everywhere else, the same indices there"""
    y, idx = got
    ry, ridx = want
    assert torch.equal(torch.isnan(y), torch.isnan(ry)), what
    ok = ~torch.isnan(ry)
    assert torch.equal(y.view(torch.int32)[ok], ry.view(torch.int32)[ok]), (what, float((y[ok] - ry[ok]).abs().max()))
    if ridx is not None:
        assert torch.equal(idx[ok], ridx[ok]), what


def _check(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3, what):
    ref, ref_idx = _chain(word, ids, typ, tok, pos, pid, p1, p2, w, b, p3)
    y, idx = _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3)
    assert y.dtype == torch.float32 and tuple(y.shape) == (ids.numel(), word.shape[-1])
    assert torch.equal(y.cpu(), ref), (what, float((y.cpu() - ref).abs().max()))
    if p3 is not None:
        assert torch.equal(idx.cpu().float() + 128, ref_idx), what
    _same_bits((y, idx), _tail(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3), what)
    return y, idx


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['contig6', 'scatter6', 'embd'])
@pytest.mark.parametrize('d', F32_D)
def test_block_equals_chain_and_axis_tail(d, layout):
    """every width the entry is built for x {six contiguous groups, six scattered groups, per-embedding}"""
    from quantization import _hip
    be = _hip.backend()
    g, word, typ, pos, w, b = _tables(d)
    ids, tok, pid = _ids(g)
    ps = _quantizers(g, d, (layout,) * 3)
    assert all(p[0].numel() == d for p in ps)
    _check(be, word, ids, typ, tok, pos, pid, *ps[:2], w, b, ps[2], (d, layout))


def test_ranges_clip_at_both_ends():
    """the drawn ranges do what the cases need: the output indices of the chain reach 0 and 255"""
    g, word, typ, pos, w, b = _tables(768)
    ids, tok, pid = _ids(g)
    ps = _quantizers(g, 768, ('scatter6',) * 3)
    _, idx = _chain(word, ids, typ, tok, pos, pid, *ps[:2], w, b, ps[2])
    assert int((idx == 0).sum()) > 0 and int((idx == 255).sum()) > 0


MIXES = list(itertools.product(('tensor', 'scatter6'), repeat=3))


@pytest.mark.gpu
@pytest.mark.parametrize('mix', MIXES)
def test_site_mixes(mix):
    """each of the eight per-tensor / per-column mixes of the three sites at d = 768; three per-tensor sites give the
    per-tensor launch's bits"""
    from quantization import _hip
    be = _hip.backend()
    g, word, typ, pos, w, b = _tables(768, seed=1)
    ids, tok, pid = _ids(g)
    p1, p2, p3 = _quantizers(g, 768, mix)
    got = _check(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3, mix)
    if mix == ('tensor',) * 3:
        _same_bits(got, _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3, method='embeddings_layernorm_quant'), mix)


@pytest.mark.gpu
@pytest.mark.parametrize('use', [(1, 1, 1), (0, 1, 1), (1, 1, 0), (0, 0, 0), (1, 0, 1), (1, 0, 0)])
@pytest.mark.parametrize('layout', ['scatter6', 'tensor'])
def test_absent_sites(use, layout):
    """sites switched off, the others per-column (or per-tensor: with an absent site the per-tensor launch's bits too)"""
    from quantization import _hip
    be = _hip.backend()
    g, word, typ, pos, w, b = _tables(768, seed=2)
    ids, tok, pid = _ids(g)
    p1, p2, p3 = (p if u else None for p, u in zip(_quantizers(g, 768, (layout,) * 3), use))
    got = _check(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3, (use, layout))
    if layout == 'tensor':
        _same_bits(got, _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3, method='embeddings_layernorm_quant'), use)


@pytest.mark.gpu
@pytest.mark.parametrize('d,rows', [(768, 8197), (64, 32785)])
def test_second_trip_of_the_row_loop(d, rows):
    """more rows than 2048 blocks take in one trip (iters == 2; a partial last block and an odd tail): the GPU's axis tail on
    all rows, the chain on the first and the last 64 (rows are independent: the chain runs on those ids alone)"""
    from quantization import _hip
    be = _hip.backend()
    g, word, typ, pos, w, b = _tables(d, seed=3)
    ids, tok, pid = _ids(g, (rows,))
    p1, p2, p3 = _quantizers(g, d, ('scatter6',) * 3)
    y, idx = _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3)
    assert tuple(y.shape) == (rows, d)
    _same_bits((y, idx), _tail(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3), (d, rows))
    for part in (slice(0, 64), slice(rows - 64, rows)):
        ref, ref_idx = _chain(word, ids[part], typ, tok[part], pos, pid[part], p1, p2, w, b, p3)
        assert torch.equal(y[part].cpu(), ref), (d, rows, part)
        assert torch.equal(idx[part].cpu().float() + 128, ref_idx), (d, rows, part)


@pytest.mark.gpu
@pytest.mark.parametrize('site', [0, 1, 2])
def test_division_path(site):
    """one column whose scale lies outside [2^-100, 2^100], at each site in turn: the block vote sends the whole launch down
    the division path -- the axis tail's bits (and the chain's), a NaN row included"""
    from quantization import _hip
    be = _hip.backend()
    d = 768
    g, word, typ, pos, w, b = _tables(d, seed=4)
    ids, tok, pid = _ids(g)
    ps = [list(p) for p in _quantizers(g, d, ('scatter6',) * 3)]
    ps[site][0] = ps[site][0].clone()
    ps[site][0][301] = 2.0e30
    word[int(ids.view(-1)[7]), 9] = float('nan')
    nan_rows = ids.view(-1) == ids.view(-1)[7]
    for use in ((1, 1, 1), (1, 1, 0) if site < 2 else (0, 1, 1)):
        p1, p2, p3 = (tuple(p) if u else None for p, u in zip(ps, use))
        got = _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3)
        assert torch.equal(torch.isnan(got[0]).all(1).cpu(), nan_rows) and torch.equal(torch.isnan(got[0]).any(1).cpu(), nan_rows)
        _same_bits(got, _tail(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3), (site, use))
        ref, ref_idx = _chain(word, ids, typ, tok, pos, pid, p1, p2, w, b, p3)
        ref_idx = None if ref_idx is None else (ref_idx - 128).to(torch.int8)
        _same_bits((got[0].cpu(), None if got[1] is None else got[1].cpu()), (ref, ref_idx), (site, use, 'chain'))


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['scatter6', 'embd'])
@pytest.mark.parametrize('table', ['word', 'type', 'pos'])
def test_special_values(table, layout):
    """NaN and +-inf entries in each of the three tables: a NaN anywhere in a gathered row makes the whole output row NaN,
    +-inf clamps to the column's grid ends; the bit patterns (the sign of zero included) are the axis tail's on the gathered
    rows, with and without the output quantizer"""
    from quantization import _hip
    be = _hip.backend()
    d = 768
    g, word, typ, pos, w, b = _tables(d, seed=5)
    ids, tok, pid = _ids(g)
    p1, p2, p3 = _quantizers(g, d, (layout,) * 3)
    flat = lambda t: t.reshape(-1)
    if table == 'word':
        tab, used = word, flat(ids)
    elif table == 'type':
        tab, used = typ, flat(tok)
    else:
        tab, used = pos, flat(pid)
    word[int(flat(ids)[10])] = -0.0                          # a row of negative zeros through the one addition in front
    typ[:, 40:48] = -0.0
    nan_id = int(used[3])
    others = [int(i) for i in used.unique() if int(i) != nan_id]
    tab[nan_id, 17] = float('nan')
    tab[others[0], 5] = float('inf')
    tab[others[0], 700] = -float('inf')
    tab[others[-1], 6] = -float('inf')
    nan_rows = used == nan_id
    assert bool(nan_rows.any()) and not bool(nan_rows.all())
    for q3 in (p3, None):
        got = _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, q3)
        nan = torch.isnan(got[0]).cpu()
        assert torch.equal(nan.all(1), nan_rows) and torch.equal(nan.any(1), nan_rows), (table, layout)
        _same_bits(got, _tail(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, q3), (table, layout, q3 is None))
    ref, ref_idx = _chain(word, ids, typ, tok, pos, pid, p1, p2, w, b, p3)
    got = _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3)
    _same_bits((got[0].cpu(), got[1].cpu()), (ref, (ref_idx - 128).to(torch.int8)), (table, layout, 'chain'))


@pytest.mark.gpu
def test_out_of_range_ids():
    """word ids 97 + 5 and -3, a position id 40, a token-type id 2 (torch's CPU F.embedding raises IndexError): the kernel
    reads a clamped row, exactly the rows that carry such an id are NaN in y, every other row of y and y_idx is bit-identical
    to the clean call, and the IndexError surfaces once -- at raise_deferred(sync=True), or at the next call"""
    from quantization import _hip
    be = _hip.backend()
    d = 768
    g, word, typ, pos, w, b = _tables(d, seed=6)
    ids, tok, pid = _ids(g)
    p1, p2, p3 = _quantizers(g, d, ('scatter6',) * 3)
    be.raise_deferred(sync=True)
    y_ok, i_ok = (t.cpu().view(B, T, d) for t in _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3))
    be.raise_deferred(sync=True)                             # a clean call reports nothing
    bad_ids, bad_tok, bad_pid = ids.clone(), tok.clone(), pid.clone()
    bad_ids[1, 1], bad_ids[2, 2] = VOCAB + 5, -3
    bad_pid[0, 4] = POSITIONS
    bad_tok[2, 12] = TYPES
    hit = torch.zeros(B, T, dtype=torch.bool)
    hit[1, 1] = hit[2, 2] = hit[0, 4] = hit[2, 12] = True
    y_bad, i_bad = (t.cpu().view(B, T, d) for t in _emb(be, word, bad_ids, typ, bad_tok, pos, bad_pid, p1, p2, w, b, p3))
    assert torch.equal(torch.isnan(y_bad).all(-1), hit) and torch.equal(torch.isnan(y_bad).any(-1), hit)
    assert torch.equal(y_bad[~hit].view(torch.int32), y_ok[~hit].view(torch.int32)) and torch.equal(i_bad[~hit], i_ok[~hit])
    with pytest.raises(IndexError):
        be.raise_deferred(sync=True)
    be.raise_deferred(sync=True)                             # reported once
    for one in ((bad_ids, tok, pid), (ids, bad_tok, pid), (ids, tok, bad_pid)):       # each table is checked on its own
        y = _emb(be, word, one[0], typ, one[1], pos, one[2], p1, p2, w, b, None)[0]
        assert bool(torch.isnan(y).any())
        with pytest.raises(IndexError):                      # without an explicit check: at the next call
            torch.cuda.synchronize()
            _emb(be, word, ids, typ, tok, pos, pid, p1, p2, w, b, p3)
    be.raise_deferred(sync=True)


def test_argument_errors_without_gpu():
    """NULL pointers, an empty table, misaligned pointers, d % 4 != 0, n_params neither 1 nor d, y_idx with a 16-bit output
    grid -> TQ_EINVAL; a row length without instantiation -> TQ_EUNSUPPORTED; all before anything is launched (the pointers are
    never dereferenced)."""
    from quantization import _hip
    lib = _hip.load_library()
    buf = 1 << 20                                    # an aligned address nobody reads
    d = 768
    mk = lambda n_params=d, inner=1, sym=0, bits=8, delta=buf: _hip.tq_quantizer(delta, None if sym else buf, None, bits, sym, 0,
                                                                                1e-8, n_params, inner)

    def call(q1=None, q2=None, q3=None, word=buf, typ=buf, pos=buf, ids=buf, tok=buf, pid=buf, y=buf, yi=None, d_=d, rows=4,
             n_word=VOCAB, n_typ=TYPES, n_pos=POSITIONS, w=buf, bad=None):
        ref = lambda q: None if q is None else C.byref(q)
        return lib.tq_embeddings_layernorm_quant_axis_fwd(word, n_word, ids, typ, n_typ, tok, pos, n_pos, pid, y, yi, rows, d_,
                                                          ref(q1), ref(q2), w, buf, 1e-12, ref(q3), bad, None)
    err = lambda: lib.tq_last_error().decode()
    assert call(mk(), mk(1), mk(), rows=0) == 0                                   # empty problem: no-op
    for name in ('word', 'typ', 'pos', 'ids', 'tok', 'pid', 'y', 'w'):
        assert call(q1=mk(), **{name: None}) == -1 and 'NULL' in err(), name
    for name in ('n_word', 'n_typ', 'n_pos'):
        assert call(q1=mk(), **{name: 0}) == -1 and 'empty table' in err(), name
    for name in ('word', 'typ', 'pos', 'y'):
        assert call(q1=mk(), **{name: buf + 4}) == -1 and 'alignment' in err(), name
    assert call(q1=mk(), bad=buf + 2) == -1 and 'bad_ids' in err()
    assert call(q1=mk(delta=buf + 2)) == -1 and 'aligned' in err()
    for bad_d in (770, 766, 63):
        assert call(q1=mk(n_params=bad_d), d_=bad_d) == -1 and '16-byte vectors' in err(), bad_d
    assert call(q1=mk(n_params=6)) == -1 and 'n_params' in err()
    assert call(q2=mk(n_params=2 * d)) == -1 and 'n_params' in err()
    assert call(q3=mk(inner=2)) == -1
    assert call(q3=mk(bits=16), yi=buf) == -1 and 'y_idx' in err()
    assert call(q3=mk(n_params=1, bits=16), yi=buf) == -1 and 'y_idx' in err()
    assert call(q3=mk(sym=1), yi=buf) == -1 and 'y_idx' in err()
    assert call(q3=None, yi=buf) == -1 and 'y_idx' in err()
    assert call(q3=mk(), yi=buf + 4) == -1 and 'y_idx' in err()
    assert call(q1=mk(bits=25)) == -1
    for bad_d in (1028, 2048, 1536, 3072, 100):
        assert call(q1=mk(n_params=bad_d), d_=bad_d) == -4, bad_d
        assert 'row length' in err()
    # the per-tensor entry keeps refusing per-column parameters
    assert lib.tq_embeddings_layernorm_quant_fwd(buf, VOCAB, buf, buf, TYPES, buf, buf, POSITIONS, buf, buf, None, 4, d,
                                                 C.byref(mk()), None, buf, buf, 1e-12, None, None, None) == -1
    assert 'per-tensor' in err()
