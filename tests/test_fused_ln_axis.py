"""Fused residual + LayerNorm tail with PER-COLUMN quantizer parameters (tq_residual_layernorm_quant_axis_fwd): what the
per-embedding / per-embedding-group (PEG) activation quantizers need.  Contract: bit for bit the oracle chain

    O.fake_quant([d] parameters) -> + residual -> O.fake_quant -> oracle.ln_sum.layer_norm_kernel_order -> O.fake_quant

(the LayerNorm statistics in the kernel's summation order, exactly as for the per-tensor kernel: tests/test_fused_ln.py),
for y and for the int8 indices.  The argument checks at the end need no GPU."""
import ctypes as C
import itertools

import pytest
import torch

from oracle import tq_oracle as O

EPS = 1e-12
F32_D = (64, 128, 256, 384, 512, 768, 1024)       # every row length the entry point is built for
BF16_D = (128, 256, 512, 768, 1024)


def _data(d, dtype, rows=515, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + d + 7)
    a = (torch.randn(rows, d, generator=g) * 2).to(dtype)
    r = (torch.randn(rows, d, generator=g) * 1.5).to(dtype)
    r[:, 5] *= 12
    w = 1 + 0.1 * torch.randn(d, generator=g)
    b = 0.05 * torch.randn(d, generator=g)
    return g, a, r, w, b


def _per_column(g, d, layout, lo_range, hi_range):
    """(delta [d], zero_float [d]) of an 8-bit asymmetric quantizer: one range per group, drawn from lo_range / hi_range (the
    narrow ones clip the data at both ends, the wide ones do not).  'contig6': 6 runs of columns; 'scatter6': 6 groups over a
    random column permutation (PEG with permutation); 'embd': d distinct ranges; 'tensor': one range, scalar tensors."""
    n = {'contig6': 6, 'scatter6': 6, 'embd': d, 'tensor': 1}[layout]
    lo = lo_range[0] + (lo_range[1] - lo_range[0]) * torch.rand(n, generator=g)
    hi = hi_range[0] + (hi_range[1] - hi_range[0]) * torch.rand(n, generator=g)
    if layout == 'tensor':
        return O.asym_params_from_range(lo[0], hi[0], 8)
    group = (torch.arange(d) * n) // d
    if layout == 'scatter6':
        group = group[torch.randperm(d, generator=g)]
    dl, zf = O.asym_params_from_range(lo[group], hi[group], 8)
    return dl.contiguous(), zf.contiguous()


# ranges of the three sites: a ~ N(0, 2), a + r ~ N(0, 2.5) with one wide column, LayerNorm output ~ N(0, 1)
SITE_RANGES = (((-7.0, -1.0), (1.0, 7.5)), ((-20.0, -2.0), (2.0, 22.0)), ((-6.0, -0.5), (0.5, 11.0)))


def _quantizers(g, d, layouts):
    return [_per_column(g, d, lay, *rng) for lay, rng in zip(layouts, SITE_RANGES)]


def _chain(a, r, p1, p2, w, b, p3, kernel_order=True):
    """(y, indices of y or None) of the oracle chain (tests/_exact_backend.py: the whole-model CPU twin uses it too)"""
    from tests._exact_backend import ln_tail_chain
    spec = lambda p: None if p is None else (p[0], p[1], 8, False)
    y, idx, _ = ln_tail_chain(a, r, spec(p1), spec(p2), w, b, EPS, spec(p3), kernel_order=kernel_order)
    return y, idx


def _k(p):
    return None if p is None else (p[0].cuda(), p[1].cuda(), None, 8, False, False, 1e-8)


def _run(be, a, r, p1, p2, w, b, p3, method='residual_layernorm_quant_axis'):
    out = getattr(be, method)(a.cuda(), r.cuda(), _k(p1), _k(p2), w.cuda(), b.cuda(), EPS, _k(p3), want_idx=p3 is not None)
    if p3 is None:
        return out.cpu(), None
    return out[0].cpu(), out[1].cpu()


def _check(be, a, r, p1, p2, w, b, p3, what):
    ref, ref_idx = _chain(a, r, p1, p2, w, b, p3)
    y, idx = _run(be, a, r, p1, p2, w, b, p3)
    ref = ref.to(a.dtype)
    assert y.dtype == a.dtype
    assert torch.equal(y, ref), (what, float((y.float() - ref.float()).abs().max()), float((y != ref).float().mean()))
    if p3 is not None:
        assert torch.equal(idx.float() + 128, ref_idx), what


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['contig6', 'scatter6', 'embd'])
@pytest.mark.parametrize('dtype,d', [(torch.float32, d) for d in F32_D] + [(torch.bfloat16, d) for d in BF16_D])
def test_axis_tail_equals_kernel_order_oracle(dtype, d, layout):
    """Every supported width, three per-column layouts, all sites per-column, sites switched off as in
    tests/test_fused_ln.py; rows = 515 is not a multiple of the rows a block handles."""
    from quantization import _hip
    be = _hip.backend()
    g, a, r, w, b = _data(d, dtype)
    ps = _quantizers(g, d, (layout,) * 3)
    for p in ps:                                # the drawn ranges clip some columns at both ends and leave others alone
        assert p[0].numel() == d
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 0), (0, 0, 0), (1, 1, 0)):
        p1, p2, p3 = (p if u else None for p, u in zip(ps, use))
        _check(be, a, r, p1, p2, w, b, p3, (str(dtype), d, layout, use))


def test_axis_tail_clips_at_both_ends():
    """the ranges drawn above do what the cases need: under Q_dense some columns reach index 0 AND index 255, others
    neither"""
    g, a, r, w, b = _data(768, torch.float32)
    p1 = _quantizers(g, 768, ('contig6',) * 3)[0]
    idx = O.fake_quant(a, p1[0], p1[1], 8, False)[0]
    both = ((idx == 0).any(0) & (idx == 255).any(0))
    assert bool(both.any()) and not bool(both.all())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('mix', list(itertools.product(('tensor', 'scatter6'), repeat=3)))
def test_axis_tail_site_mixes(dtype, mix):
    """each of the eight per-tensor / per-column mixes of the three sites at d = 768"""
    from quantization import _hip
    be = _hip.backend()
    g, a, r, w, b = _data(768, dtype, seed=1)
    p1, p2, p3 = _quantizers(g, 768, mix)
    _check(be, a, r, p1, p2, w, b, p3, (str(dtype), mix))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('d', [512, 768, 1024])
def test_equal_columns_give_the_per_tensor_kernels_bits(dtype, d):
    """per-column arrays whose entries are all equal == tq_residual_layernorm_quant_fwd on the same inputs"""
    from quantization import _hip
    be = _hip.backend()
    g, a, r, w, b = _data(d, dtype, seed=2)
    ps = _quantizers(g, d, ('tensor',) * 3)
    wide = [(p[0].reshape(1).expand(d).contiguous(), p[1].reshape(1).expand(d).contiguous()) for p in ps]
    for use in ((1, 1, 1), (0, 1, 1), (1, 1, 0)):
        sel = lambda qs: [q if u else None for q, u in zip(qs, use)]
        y0, i0 = _run(be, a, r, *sel(ps)[:2], w, b, sel(ps)[2], method='residual_layernorm_quant')
        y1, i1 = _run(be, a, r, *sel(wide)[:2], w, b, sel(wide)[2])
        assert torch.equal(y0.view(torch.int32 if dtype == torch.float32 else torch.int16),
                           y1.view(torch.int32 if dtype == torch.float32 else torch.int16)), (d, use)
        if i0 is not None:
            assert torch.equal(i0, i1)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('layout', ['scatter6', 'embd'])
def test_axis_tail_special_values(dtype, layout):
    """NaN / +-Inf / -0.0 / rounding ties: a NaN anywhere in a row makes the whole row NaN, +-Inf clamps to the column's
    grid ends, no -0.0 where the reference produces +0.0 -- and every other row still equals the oracle chain bit for bit."""
    from quantization import _hip
    be = _hip.backend()
    d = 768
    g, a, r, w, b = _data(d, dtype, rows=64, seed=3)
    p1, p2, p3 = _quantizers(g, d, (layout,) * 3)
    a[3, 17] = float('nan')
    r[7, 700] = float('nan')
    a[9, 5] = float('inf')
    r[11, 6] = -float('inf')
    a[13, :] = -0.0
    r[13, :] = -0.0
    # rounding ties of Q_dense: (k + 1/2) * scale of the column, k around the zero point
    s1 = torch.clamp_min(p1[0], 1e-8)
    a[15, :] = ((torch.arange(d) % 7 - 3).float() + 0.5) * s1
    a[16, :] = -((torch.arange(d) % 5).float() + 0.5) * s1
    a = a.to(dtype)
    ref, ref_idx = _chain(a, r, p1, p2, w, b, p3)
    ref = ref.to(dtype)
    y, idx = _run(be, a, r, p1, p2, w, b, p3)
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    assert torch.isnan(y[3]).all() and torch.isnan(y[7]).all() and int(torch.isnan(y).sum()) == 2 * d
    ok = ~torch.isnan(ref)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(y.view(bits)[ok], ref.view(bits)[ok])                    # bit patterns, incl. the sign of zero
    assert torch.equal((idx.float() + 128)[ok], ref_idx[ok])
    # ... and without the output quantizer the NaN rows are NaN as a whole, too
    y2, _ = _run(be, a, r, p1, p2, w, b, None)
    assert torch.isnan(y2[3]).all() and torch.isnan(y2[7]).all() and int(torch.isnan(y2).sum()) == 2 * d


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('site', [0, 1, 2])
def test_axis_tail_division_path(dtype, site):
    """One column whose scale lies outside the exact path's domain [2^-100, 2^100] sends the WHOLE launch down the
    division path: same bits (the chain above), NaN rows included."""
    from quantization import _hip
    be = _hip.backend()
    d = 768
    g, a, r, w, b = _data(d, dtype, rows=131, seed=4)
    ps = [list(p) for p in _quantizers(g, d, ('scatter6',) * 3)]
    ps[site][0] = ps[site][0].clone()
    ps[site][0][301] = 2.0e30                          # > 2^100: guarded_rcp refuses it
    a[5, 9] = float('nan')
    for use in ((1, 1, 1), (1, 1, 0) if site < 2 else (0, 1, 1)):
        p1, p2, p3 = (tuple(p) if u else None for p, u in zip(ps, use))
        ref, ref_idx = _chain(a, r, p1, p2, w, b, p3)
        ref = ref.to(dtype)
        y, idx = _run(be, a, r, p1, p2, w, b, p3)
        assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.isnan(y[5]).all()
        ok = ~torch.isnan(ref)
        assert torch.equal(y[ok], ref[ok]), (site, use)
        if p3 is not None:
            assert torch.equal((idx.float() + 128)[ok], ref_idx[ok])


@pytest.mark.gpu
def test_axis_tail_is_close_to_torch_layer_norm():
    """the project's contract for a fused tail vs F.layer_norm (tests/test_fused_ln.py): >= 99.9 % identical, the rest one
    step of the column's grid away"""
    from quantization import _hip
    be = _hip.backend()
    d = 768
    g, a, r, w, b = _data(d, torch.float32, rows=1024, seed=5)
    p1, p2, p3 = _quantizers(g, d, ('scatter6',) * 3)
    ref, _ = _chain(a, r, p1, p2, w, b, p3, kernel_order=False)
    y, _ = _run(be, a, r, p1, p2, w, b, p3)
    diff = (y - ref).abs()
    assert float((diff == 0).float().mean()) >= 0.999
    assert bool((diff <= torch.clamp_min(p3[0], 1e-8) * 1.01).all())


def test_axis_tail_argument_errors_without_gpu():
    """n_params neither 1 nor d, inner != 1, misaligned pointers, y_idx with a symmetric q_out -> TQ_EINVAL; a row length
    without instantiation -> TQ_EUNSUPPORTED; all before anything is launched (the pointers are never dereferenced)."""
    from quantization import _hip
    lib = _hip.load_library()
    buf = 1 << 20                                    # an aligned address nobody reads
    d = 768
    mk = lambda n_params=d, inner=1, sym=0, bits=8, delta=buf: _hip.tq_quantizer(delta, None if sym else buf, None, bits, sym, 0,
                                                                                1e-8, n_params, inner)

    def call(q1=None, q2=None, q3=None, a=buf, y=buf, yi=None, d_=d, rows=4, dtype=0, w=buf):
        ref = lambda q: None if q is None else C.byref(q)
        return lib.tq_residual_layernorm_quant_axis_fwd(a, buf, y, yi, rows, d_, dtype, ref(q1), ref(q2), w, buf, 1e-12, ref(q3),
                                                        None)
    err = lambda: lib.tq_last_error().decode()
    assert call(mk(), mk(1), mk(), rows=0) == 0                                   # empty problem: no-op
    assert call(q1=mk(n_params=6)) == -1 and 'n_params' in err()
    assert call(q2=mk(n_params=2 * d)) == -1
    assert call(q3=mk(inner=2)) == -1
    assert call(q3=mk(n_params=d, inner=4)) == -1
    assert call(q1=mk(), a=buf + 4) == -1 and 'alignment' in err()
    assert call(q1=mk(), y=buf + 8) == -1 and 'alignment' in err()
    assert call(q1=mk(delta=buf + 2)) == -1 and 'aligned' in err()
    assert call(q3=mk(sym=1), yi=buf) == -1 and 'y_idx' in err()
    assert call(q3=None, yi=buf) == -1 and 'y_idx' in err()
    assert call(q3=mk(), yi=buf + 4) == -1 and 'y_idx' in err()
    assert call(q1=mk(), w=None) == -1 and 'NULL' in err()
    assert call(q1=mk(), dtype=7) == -1 and 'dtype' in err()
    assert call(q1=mk(bits=25)) == -1
    for bad_d, dtype in ((3072, 0), (1536, 0), (2048, 1), (1536, 1), (100, 0), (770, 0), (64, 1)):
        assert call(q1=mk(n_params=bad_d), d_=bad_d, dtype=dtype) == -4, (bad_d, dtype)
        assert 'row length' in err()
    # the per-tensor entry point keeps refusing per-column parameters
    assert lib.tq_residual_layernorm_quant_fwd(buf, buf, buf, None, 4, d, 0, C.byref(mk()), None, buf, buf, 1e-12, None,
                                               None) == -1 and 'per-tensor' in err()


def test_tail_row_lengths_match_exactly_without_gpu():
    """A row length that is no whole number of 16-byte vectors, or a whole number of them that no kernel is built for,
    is TQ_EUNSUPPORTED in every per-tensor tail entry, before anything is launched: d = 770 must not select the d = 768
    kernel through a floor division (770 / 4 == 192 vectors).  The pointers are never dereferenced."""
    from quantization import _hip
    lib = _hip.load_library()
    buf = 1 << 20                                    # an aligned address nobody reads
    rows = 4
    q = _hip.tq_quantizer(buf, buf, None, 8, 0, 0, 1e-8, 1, 1)
    q16 = _hip.tq_quantizer(buf, buf, None, 16, 0, 0, 1e-8, 1, 1)
    Q, Q16 = C.byref(q), C.byref(q16)
    calls = {
        'layernorm fp32 770': lambda: lib.tq_residual_layernorm_quant_fwd(buf, buf, buf, None, rows, 770, 0, Q, Q, buf, buf, 1e-12, Q, None),
        'layernorm fp32 769': lambda: lib.tq_residual_layernorm_quant_fwd(buf, buf, buf, None, rows, 769, 0, Q, Q, buf, buf, 1e-12, Q, None),
        'layernorm bf16 772': lambda: lib.tq_residual_layernorm_quant_fwd(buf, buf, buf, None, rows, 772, 1, Q, Q, buf, buf, 1e-12, Q, None),
        'layernorm f16 100': lambda: lib.tq_residual_layernorm_quant_fwd(buf, buf, buf, None, rows, 100, 2, Q, Q, buf, buf, 1e-12, Q, None),
        'nonorm fp32 770': lambda: lib.tq_residual_nonorm_quant_fwd(buf, buf, buf, None, rows, 770, 0, Q, Q, buf, buf, Q, None),
        'ires 770': lambda: lib.tq_residual_layernorm_quant_ires_fwd(buf, None, buf, Q, None, buf, buf, buf, rows, 770, Q, Q, buf, buf,
                                                                    1e-12, Q, None),
        'planes 770': lambda: lib.tq_residual_layernorm_quant_planes_fwd(buf, buf, buf, buf, buf, rows, 770, Q, Q, buf, buf, 1e-12,
                                                                        Q16, None),
        'pres 770 (planes out)': lambda: lib.tq_residual_layernorm_quant_pres_fwd(buf, None, buf, None, None, Q, None, None, None, buf,
                                                                                   buf, buf, rows, 770, Q, Q, buf, buf, 1e-12, Q16,
                                                                                   None),
        'pres 770 (planes in)': lambda: lib.tq_residual_layernorm_quant_pres_fwd(buf, None, None, buf, buf, Q16, None, buf, buf, None,
                                                                                  None, buf, rows, 770, Q, Q, buf, buf, 1e-12, Q,
                                                                                  None),
    }
    for name, call in calls.items():
        assert call() == -4, (name, lib.tq_last_error().decode())
        assert 'row length' in lib.tq_last_error().decode(), name
