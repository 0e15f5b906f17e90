"""Parameter gradients of `tq_fake_quant_bwd` (learn_ranges(): d loss / d _delta, d loss / d _zero_float) in every launch
form, against the float64 reference `oracle.tq_oracle.ste_param_grad_terms`.

The reference computes the integer index, the clamp mask and x_int in fp32 exactly as the forward does and everything
after that in float64 (see its docstring); `test_float64_reference_agrees_with_autograd` (CPU) holds it against fp32
autograd through the reference's op chain so that it cannot be wrong on its own.

TOLERANCE (derived, not measured).  The kernels add fp32 terms along a chain of at most
    L = ceil(elements per block / 256) + 10
additions (the thread's loop, 6 wave-shuffle steps, 4 waves), then in float64.  A term carries a few roundings of its own
(g * (x_int - zp): 1; (g * s * x) / (s * s): 4; their difference: 1; the cast of the float64 sum to fp32: 1; the chain
factor: 1-3).  With A = sum(|t1| + |t2|) resp. sum(|tz|) from the reference,
    |got - ref64| <= (L + 16) * 2^-24 * A * |chain factor|                                    (`_bound`)
and 4 more ulps in the log domain, where the device's expf may sit in the last bit next to the host's exp.  `elements per
block` follows from the launch plan, restated below: per-tensor vectorised form 2 * 256 * V, scalar form ceil(n / grid),
vector parameters chunk * inner.

That bound sees one missing element only while a block holds a few thousand of them.  ONE-HOT PROBES are the sharp part:
every case runs again with grad_y == 0 except ONE element (value 1.25) at a position where a kernel could drop or
double-count -- first / last element, the ends of the first and of the last non-empty slice, every element of the n % V
tail, the first element of the second block / grid-stride round.  The sums then consist of that single term: the same
formula with L = 0 (a few ulps) for its parameter, EXACTLY 0 for every other parameter.  x at the probed positions is
set three and a bit grid steps outside the clamp, on the side further from the zero point, where both gradients are large
(|t1| = 1.25 * |x_int - zp|, |tz| = 1.25 * scale), and each probe asserts that its expected value is at least 1000 bounds
away from 0.

Linear-domain inputs carry exact rounding ties and values exactly on lo / hi.  Log-domain inputs are built as
x = scale * (k + u), k integer, |u| <= 0.4, so no index or mask can flip when the device's scale differs in the last bit;
their grad_x reference uses the scale read back from the device (the forward's y of an element with index zp + 1), which
must lie within 2 ulps of the correctly rounded exp(float64(delta)).
"""
import ctypes as C

import pytest
import torch

from oracle import tq_oracle as O

gpu = pytest.mark.gpu
DEV = 'cuda'
EPS = 1e-8
U24 = 2.0 ** -24
PROBE_G = 1.25                       # exact in fp32, bf16 and fp16

# ------------------------------------------------------------------------------------------------------------------
# The launch plan of `launch_bwd`, restated once.  Mirrors:
#   K_BLOCK, MAX_GRID    csrc/tq_device.h: `constexpr int kBlock = 256`, `constexpr int kMaxGrid = 256 * 8`
#   BWD_U, VEC_GRID_CAP  csrc/tq_fake_quant.hip, launch_bwd: `constexpr int U = 2`, `pgrad ? 65536 : kMaxTiles`
#   NT_MIN_BYTES         launch_bwd: `const bool nt = (n * elem_size(DT)) >= ((uint64_t)64 << 20)`
#   SLICE_ELEMS          bwd_param_slices: `uint64_t s = per_param / 4096`
#   MAX_SLICES           `constexpr unsigned kBwdSlices = 64`
#   FINAL_BLOCK          launch of fq_bwd_params_final_k: `dim3((unsigned)ceil_div(q.n_params, 256)), dim3(256)`
# ------------------------------------------------------------------------------------------------------------------
K_BLOCK = 256
MAX_GRID = 2048
BWD_U = 2
VEC_GRID_CAP = 65536
NT_MIN_BYTES = 64 << 20
SLICE_ELEMS = 4096
MAX_SLICES = 64
FINAL_BLOCK = 256


def _ceil_div(a, b):
    return -(-a // b)


def _vec(dtype):
    return 4 if dtype == torch.float32 else 8


def slices_of(outer, inner):
    """bwd_param_slices"""
    return min(max(outer * inner // SLICE_ELEMS, 1), MAX_SLICES, outer)


def tensor_form(n, dtype, aligned):
    """(form, elements per block, grid, streaming) of a per-tensor launch with parameter gradients"""
    V = _vec(dtype)
    nt = n * (4 if dtype == torch.float32 else 2) >= NT_MIN_BYTES
    if aligned:
        tiles = max(_ceil_div(n // V, K_BLOCK * BWD_U), 1)
        assert tiles <= VEC_GRID_CAP, 'the grid is capped: blocks take more than one tile, re-derive elements per block'
        return 'vector', K_BLOCK * BWD_U * V, tiles, nt
    grid = min(max(_ceil_div(n, K_BLOCK), 1), MAX_GRID)
    return 'scalar', _ceil_div(n, grid), grid, nt


def _chain(elements_per_block):
    return _ceil_div(elements_per_block, K_BLOCK) + 10


def _bound(A, chain_factor, L, log):
    return (L + 16 + (4 if log else 0)) * U24 * A * chain_factor.abs()


# ------------------------------------------------------------------------------------------------------------------
# quantizers, inputs, reference
# ------------------------------------------------------------------------------------------------------------------
class Quant:
    """A quantizer whose parameters live on the host (reference) and, lazily, on the device (kernel)."""

    def __init__(self, delta, zero_float, n_bits, symmetric=False, signed=False, log=False, eps=EPS, inner=1):
        self.delta = delta.detach().float().reshape(-1).contiguous()
        self.zf = None if zero_float is None else zero_float.detach().float().reshape(-1).contiguous()
        self.n_bits, self.symmetric, self.signed, self.log, self.eps, self.inner = n_bits, symmetric, bool(signed), log, eps, inner
        self.P = self.delta.numel()
        self.lo, self.hi = O.grid_limits(n_bits, symmetric, self.signed)
        self._dev = None

    @property
    def domain(self):
        return 'log' if self.log else 'linear'

    def scale(self):
        """fp32 scale per parameter: clamp(delta, eps), or the correctly rounded exp(float64(delta))"""
        if self.log:
            return torch.exp(self.delta.double()).float()
        return torch.clamp(self.delta, min=self.eps)

    def zp(self):
        return torch.zeros(self.P) if self.symmetric else torch.clamp(torch.round(self.zf), self.lo, self.hi)

    def dev(self):
        if self._dev is None:
            self._dev = (self.delta.to(DEV), None if self.zf is None else self.zf.to(DEV),
                         torch.tensor(self.signed).to(DEV) if self.symmetric else None)
        return self._dev

    def one(self, p):
        """parameter p as a per-tensor quantizer"""
        return Quant(self.delta[p:p + 1], None if self.zf is None else self.zf[p:p + 1], self.n_bits, self.symmetric,
                     self.signed, self.log, self.eps)


def _quant_from_data(x3, n_bits, symmetric=False, log=False):
    """ranges clipped to 0.7 x min / max per parameter, so that both branches of the clamp mask are populated"""
    P = x3.shape[1]
    rows = x3.float().permute(1, 0, 2).reshape(P, -1)
    mn, mx = rows.min(1)[0] * 0.7, rows.max(1)[0] * 0.7
    if P == 1:
        mn, mx = mn[0], mx[0]
    dom = 'log' if log else 'linear'
    if symmetric:
        delta, signed = O.sym_params_from_range(mn, mx, n_bits, EPS, dom)
        return Quant(delta, None, n_bits, True, bool(signed), log, inner=x3.shape[2])
    delta, zf = O.asym_params_from_range(mn, mx, n_bits, EPS, dom)
    return Quant(delta, zf, n_bits, log=log, inner=x3.shape[2])


def _inputs(outer, P, inner, dtype, seed, nonneg=False):
    """x ~ randn * 3 * (per-parameter amplitude in [0.5, 3]), grad_y ~ randn, as [outer, P, inner]"""
    g = torch.Generator().manual_seed(seed)
    amp = torch.linspace(0.5, 3.0, P).view(1, P, 1)
    x = torch.randn(outer, P, inner, generator=g) * 3 * amp
    if nonneg:
        x = x.abs()
    gy = torch.randn(outer, P, inner, generator=g)
    return x.to(dtype), gy.to(dtype)


def _on_grid_inputs(x3, q, seed):
    """log domain: x = scale * (k + u), k integer with k + zp up to 4 steps outside [lo, hi], |u| <= 0.4 (fp32)"""
    g = torch.Generator().manual_seed(seed)
    outer, P, inner = x3.shape
    s, zp = q.scale().view(1, P, 1), q.zp().view(1, P, 1)
    span = int(q.hi - q.lo) + 9
    k = torch.randint(0, span, x3.shape, generator=g).float() + (q.lo - 4) - zp
    u = (torch.rand(x3.shape, generator=g) - 0.5) * 0.8
    return (s * (k + u)).float()


def _plant_edges(x3, q):
    """linear domain: exact rounding ties and values exactly on lo / hi (and half a step outside) among parameter 0"""
    outer, P, inner = x3.shape
    s, zp = float(q.scale()[0]), float(q.zp()[0])
    vals = torch.tensor([s * 1.5, s * 2.5, s * (q.lo - zp), s * (q.hi - zp), s * (q.hi - zp + 0.5), s * (q.lo - zp - 0.5)])
    if inner >= 8:
        x3[0, 0, 1:7] = vals.to(x3.dtype)
    elif outer >= 8:
        x3[1:7, 0, 0] = vals.to(x3.dtype)


def _plant_probes(x3, q, probes):
    """x three and a bit steps outside the clamp at every probed position, on the side that lies further from the zero
    point: |t1| = g * |x_int - zp| >= g * (hi - lo) / 2 and tz = -g * scale, both far from 0"""
    outer, P, inner = x3.shape
    s, zp = q.scale(), q.zp()
    flat = x3.view(-1)
    for pos in probes:
        p = (pos // inner) % P
        k = q.hi - zp[p] + 3.3 if q.hi - zp[p] >= zp[p] - q.lo else q.lo - zp[p] - 3.3
        flat[pos] = (s[p] * k).to(x3.dtype)


def _reference(x3, g3, q, chunk=1 << 22):
    """per-parameter float64 sums of the oracle's terms (in slabs of `outer`, so that 2^24 elements stay cheap)"""
    outer, P, inner = x3.shape
    rows = max(1, chunk // (P * inner))
    keys = ('d_scale', 'd_zp', 'A_d', 'A_z')
    tot = None
    for o0 in range(0, outer, rows):
        xs, gs = x3[o0:o0 + rows], g3[o0:o0 + rows]
        if P == 1:
            xs, gs = xs.reshape(-1), gs.reshape(-1)
        r = O.ste_param_grad_terms(xs, gs, q.delta, q.zf, q.n_bits, q.symmetric, q.signed, q.eps,
                                   axis=None if P == 1 else 1, scale_domain=q.domain)
        if tot is None:
            tot = {k: r[k].clone() for k in keys}
            tot['chain_delta'], tot['chain_zero_float'] = r['chain_delta'], r['chain_zero_float']
        else:
            for k in keys:
                tot[k] += r[k]
    tot['d_delta'] = tot['d_scale'] * tot['chain_delta']
    tot['d_zero_float'] = tot['d_zp'] * tot['chain_zero_float']
    return tot


def _bwd(be, xd, gd, q, param_grads):
    d, z, s = q.dev()
    return be.fake_quant_bwd(xd, gd, d, z, s, q.n_bits, q.symmetric, q.log, q.eps, q.P, q.inner, param_grads=param_grads)


def _device_scale(be, q):
    """the scale the kernels derive from delta, read from the forward: y of x = scale has index zp + 1, y = scale * 1"""
    want = q.scale()
    assert bool((q.zp() + 1 <= q.hi).all())
    d, z, s = q.dev()
    y, _ = be.fake_quant(want.view(1, q.P, 1).to(DEV), d, z, s, q.n_bits, q.symmetric, q.log, q.eps, q.P, 1)
    got = y.cpu().reshape(-1)
    two_ulps = 2 * (torch.nextafter(want, want * 2) - want)
    assert bool(((got - want).abs() <= two_ulps).all()), ('device exp(delta) further than 2 ulps from the correctly rounded value',
                                                          got, want)
    return got


def _ref_dx(be, x3, g3, q):
    """grad_x: fp32 autograd through the reference's op chain (tests/test_fuzz_parity.py::test_ste_backward_fuzz)"""
    P = x3.shape[1]
    if not q.log:
        dx = O.fake_quant_with_grads(x3.float(), q.delta if P > 1 else q.delta.reshape(()),
                                     None if q.zf is None else (q.zf if P > 1 else q.zf.reshape(())),
                                     q.n_bits, q.symmetric, q.signed, q.eps, grad_out=g3.float(),
                                     axis=1 if P > 1 else None)[1]
        return dx.to(x3.dtype)
    # log domain: what autograd computes, ((g * scale) * mask) / scale, with the device's own scale (the mask cannot flip)
    s = _device_scale(be, q).view(1, P, 1)
    mask = O.ste_param_grad_terms(x3, g3, q.delta, q.zf, q.n_bits, q.symmetric, q.signed, q.eps, axis=None if P == 1 else 1,
                                  scale_domain='log')['mask']
    gf = g3.float()
    return torch.where(mask, (gf * s) / s, torch.zeros_like(gf)).to(x3.dtype)


def _to_device(t, aligned):
    if aligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)          # base pointer off by one element: scalar kernels
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _assert_sums(gd, gz, ref, q, L, tag):
    for name, got, want, A, chain in (('d_delta', gd, ref['d_delta'], ref['A_d'], ref['chain_delta']),
                                      ('d_zero_float', gz, ref['d_zero_float'], ref['A_z'], ref['chain_zero_float'])):
        got = got.cpu().double().reshape(-1)
        if name == 'd_zero_float' and q.symmetric:
            assert int(torch.count_nonzero(got)) == 0, (tag, 'symmetric: d_zero_float must stay zero', got)
            continue
        bound = _bound(A, chain, L, q.log)
        err = (got - want).abs()
        closed = chain == 0
        assert int(torch.count_nonzero(got[closed])) == 0, (tag, name, 'closed gate: exactly 0 expected', got)
        worst = int(torch.argmax(err - bound))
        assert bool((err <= bound).all()), (tag, name, 'parameter', worst, 'got', float(got[worst]), 'ref', float(want[worst]),
                                            'err', float(err[worst]), 'bound', float(bound[worst]), 'L', L)


def _probe(be, xd, x3, q, pos, tag):
    """grad_y == 0 except PROBE_G at flat position `pos`: the sums are that single term"""
    outer, P, inner = x3.shape
    p = (pos // inner) % P
    gd1 = torch.zeros(x3.shape, dtype=x3.dtype, device=DEV)
    gd1.view(-1)[pos] = PROBE_G
    gx, gd, gz = _bwd(be, xd, gd1, q, True)
    q1 = q.one(p)
    r = O.ste_param_grad_terms(x3.view(-1)[pos:pos + 1], torch.tensor([PROBE_G]), q1.delta, q1.zf, q1.n_bits, q1.symmetric,
                               q1.signed, q1.eps, scale_domain=q1.domain)
    for name, got, want, A, chain in (('d_delta', gd, r['d_delta'], r['A_d'], r['chain_delta']),
                                      ('d_zero_float', gz, r['d_zero_float'], r['A_z'], r['chain_zero_float'])):
        got = got.cpu().double().reshape(-1)
        others = torch.cat([got[:p], got[p + 1:]])
        assert int(torch.count_nonzero(others)) == 0, (tag, 'probe', pos, name, 'leaked into another parameter', got)
        if name == 'd_zero_float' and q.symmetric:
            assert float(got[p]) == 0.0, (tag, 'probe', pos, name)
            continue
        bound = float(_bound(A, chain, 0, q.log))
        assert abs(float(want)) >= 1000 * bound > 0, (tag, 'probe', pos, name, 'the probed element is not sharp', float(want), bound)
        assert abs(float(got[p]) - float(want)) <= bound, (tag, 'probe', pos, name, 'parameter', p, 'got', float(got[p]),
                                                           'ref', float(want), 'bound', bound)


def _run_case(x3, g3, q, elements_per_block, probes, aligned=True, twice=False, dx_reference=True, tag=None):
    from quantization import _hip
    be = _hip.backend()
    n = x3.numel()
    probes = sorted({p for p in probes if 0 <= p < n})
    xd, gd_ = _to_device(x3, aligned), g3.to(DEV)
    ref = _reference(x3, g3, q)
    gx, gd, gz = _bwd(be, xd, gd_, q, True)
    _assert_sums(gd, gz, ref, q, _chain(elements_per_block), tag)
    gx0, none_d, none_z = _bwd(be, xd, gd_, q, False)
    assert none_d is None and none_z is None
    assert torch.equal(gx, gx0), (tag, 'grad_x differs between param_grads=True and False')
    if dx_reference:
        assert torch.equal(gx.cpu().reshape(x3.shape), _ref_dx(be, x3, g3, q)), (tag, 'grad_x differs from autograd')
    if twice:
        _, gd2, gz2 = _bwd(be, xd, gd_, q, True)
        assert torch.equal(gd, gd2) and torch.equal(gz, gz2), (tag, 'two calls on the same inputs differ')
    for pos in probes:
        _probe(be, xd, x3, q, pos, tag)


# ------------------------------------------------------------------------------------------------------------------
# the float64 reference against fp32 autograd (CPU)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout,symmetric,log', [('tensor', False, False), ('tensor', True, False), ('channel', False, False),
                                                  ('channel', True, True), ('embd', False, False), ('embd', False, True)])
def test_float64_reference_agrees_with_autograd(layout, symmetric, log):
    """`ste_param_grad_terms` against `fake_quant_with_grads` (fp32 autograd through the reference's op chain with the STE
    round) within 1e-4 relative, on six small cases: asymmetric / symmetric, per tensor / per channel / per embedding,
    linear / log.  fp32 autograd carries up to ~1e-6 of A = sum(|terms|) (a pairwise sum of a few hundred terms with a few
    roundings each), so 1e-4 of the VALUE is above autograd's own error only where the sum does not cancel: grad_out is
    positive and x is shifted so that one side of the clamp dominates, and the test asserts |sum| >= 1e-2 A first."""
    g = torch.Generator().manual_seed(12)
    if layout == 'tensor':
        x = torch.randn(7, 41, generator=g) * 3 + 6
        axis, per_channel, P, mn, mx = None, False, 1, x.min(), x.max()
    elif layout == 'channel':
        x = (torch.randn(6, 150, generator=g) * 3 + 6) * torch.linspace(0.5, 3, 6)[:, None]
        axis, per_channel, P, mn, mx = None, True, 6, x.min(1)[0], x.max(1)[0]
    else:
        x = (torch.randn(5, 30, 12, generator=g) * 3 + 6) * torch.linspace(0.5, 3, 12)
        axis, per_channel, P = 2, False, 12
        mn, mx = x.reshape(-1, 12).min(0)[0], x.reshape(-1, 12).max(0)[0]
    gy = torch.randn(x.shape, generator=g).abs() + 0.5
    dom = 'log' if log else 'linear'
    n_bits = 4
    if symmetric:
        delta, signed = O.sym_params_from_range(mn * 0.7, mx * 0.7, n_bits, EPS, dom)
        zf, sgn = None, bool(signed)
    else:
        delta, zf = O.asym_params_from_range(mn * 0.7, mx * 0.7, n_bits, EPS, dom)
        sgn = False
    ref = O.ste_param_grad_terms(x, gy, delta, zf, n_bits, symmetric, sgn, EPS, axis=axis, per_channel=per_channel,
                                 scale_domain=dom)
    ag_axis = 0 if per_channel else axis
    _, _, dd, dz = O.fake_quant_with_grads(x, delta, zf, n_bits, symmetric, sgn, EPS, grad_out=gy, axis=ag_axis,
                                           scale_domain=dom)
    assert ref['d_delta'].shape == (P,) and ref['mask'].shape == x.shape
    assert 0 < int(ref['mask'].sum()) < x.numel()                       # both branches of the clamp are populated
    pairs = [('d_delta', dd, ref['A_d'] * ref['chain_delta'])]
    if not symmetric:
        pairs.append(('d_zero_float', dz, ref['A_z'] * ref['chain_zero_float']))
    else:
        assert int(torch.count_nonzero(ref['d_zero_float'])) == 0
    for name, ag, mag in pairs:
        want, got = ag.double().reshape(-1), ref[name]
        assert bool((want.abs() >= 1e-2 * mag).all()), (name, 'the sum cancels: autograd is no reference at 1e-4 here', want, mag)
        assert bool(((got - want).abs() <= 1e-4 * want.abs()).all()), (name, got, want)


# ------------------------------------------------------------------------------------------------------------------
# per tensor
# ------------------------------------------------------------------------------------------------------------------
def _tensor_sizes(dtype):
    V = _vec(dtype)
    tile = K_BLOCK * BWD_U * V
    return [1, V - 1, V, tile, tile + 1, 3 * tile + V + 3]


def _tensor_case(n, dtype, n_bits, seed, aligned, symmetric=False):
    x3, g3 = _inputs(n, 1, 1, dtype, seed)
    q = _quant_from_data(x3, n_bits, symmetric)
    if n >= 8:
        _plant_edges(x3, q)
    return x3, g3, q


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('k', range(6))
def test_per_tensor_vectorised_form(dtype, k):
    """fq_bwd_tensor<DT, true, false, 2>: n = 1 and V - 1 (no whole vector), V, one full tile, one tile + 1 (a tail of one
    behind a full tile), three tiles + one vector + a tail of three (four blocks, the last with one vector)."""
    n = _tensor_sizes(dtype)[k]
    V = _vec(dtype)
    form, epb, grid, nt = tensor_form(n, dtype, aligned=True)
    assert (form, nt) == ('vector', False)
    x3, g3, q = _tensor_case(n, dtype, 4 if k % 2 else 8, 100 + k, True, symmetric=(k == 3))
    tail0 = n // V * V
    probes = [0, n - 1, tail0 - 1, epb - 1, epb, 3 * epb] + list(range(tail0, n))
    probes = [p for p in probes if 0 <= p < n]
    _plant_probes(x3, q, probes)
    _run_case(x3, g3, q, epb, probes, tag=('vectorised', str(dtype), n))


@gpu
def test_per_tensor_streaming_form_and_determinism():
    """fq_bwd_tensor<TQ_F32, true, true, 2>: the non-temporal instantiation from 64 MiB, n = 2^24 + 5 (8193 blocks, a tail
    of one).  grad_x is compared with the param_grads=False launch only (its values are those of the cached form, which
    the small cases compare with autograd).  Two calls return bit-identical gradients."""
    n, dtype = (1 << 24) + 5, torch.float32
    form, epb, grid, nt = tensor_form(n, dtype, aligned=True)
    assert (form, nt, grid, n % 4) == ('vector', True, 8193, 1)
    assert tensor_form(n - 8, dtype, aligned=True)[3] is False           # the smallest size of the table that streams
    x3, g3, q = _tensor_case(n, dtype, 8, 7, True)
    probes = [0, n - 1, n - 2, epb * 4096 - 1, epb * 4096, epb * (grid - 1)]
    _plant_probes(x3, q, probes)
    _run_case(x3, g3, q, epb, probes, twice=True, dx_reference=False, tag=('streaming', n))


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('n', [7, 4097, 600001])
def test_per_tensor_scalar_form(dtype, n):
    """fq_bwd<DT, true>: base pointer off by one element.  600001 elements are 2344 blocks' worth: the grid is capped at
    2048 and the first 75713 threads take a second grid-stride round."""
    form, epb, grid, nt = tensor_form(n, dtype, aligned=False)
    assert form == 'scalar' and not nt
    second_round = MAX_GRID * K_BLOCK
    assert (n > second_round) == (n == 600001) and (grid == MAX_GRID) == (n == 600001)
    x3, g3, q = _tensor_case(n, dtype, 4 if n == 4097 else 8, 200 + n % 97, False)
    probes = [p for p in (0, n - 1, K_BLOCK - 1, K_BLOCK, second_round - 1, second_round, second_round + K_BLOCK) if p < n]
    _plant_probes(x3, q, probes)
    _run_case(x3, g3, q, epb, probes, aligned=False, tag=('scalar', str(dtype), n))


# ------------------------------------------------------------------------------------------------------------------
# vector parameters: x viewed as [outer, P, inner]
# ------------------------------------------------------------------------------------------------------------------
#            id                          outer    P   inner  dtype           bits sym    nonneg log    slices
VECTOR_CASES = [
    ('d-embd-8191-1slice',                8191,   8,     1, torch.float32,    8, False, False, False, 1),
    ('d-embd-8192-2slices',               8192,   8,     1, torch.float32,    4, False, False, False, 2),
    ('d-embd-12289-3slices-short-last',  12289,   8,     1, torch.float32,    8, False, False, False, 3),
    ('d-embd-262145-64slices-short-last', 262145, 8,     1, torch.float32,    4, False, False, False, 64),
    ('e-64slices-31-empty',                 65,   2,  4096, torch.float32,    8, False, False, False, 64),
    ('f-middle-axis-4slices',               20,   5,  1000, torch.float32,    4, False, False, False, 4),
    ('g-channel-outer1-clamp',               1,   3, 10000, torch.float32,    8, False, False, False, 1),
    ('h-257-params-second-final-block',   8192, 257,     1, torch.float32,    4, False, False, False, 2),
    ('i-embd-12289-bf16',                12289,   8,     1, torch.bfloat16,   8, False, False, False, 3),
    ('i-embd-12289-fp16',                12289,   8,     1, torch.float16,    4, False, False, False, 3),
    ('i-middle-axis-bf16',                  20,   5,  1000, torch.bfloat16,   4, False, False, False, 4),
    ('i-middle-axis-fp16',                  20,   5,  1000, torch.float16,    8, False, False, False, 4),
    ('j-channel-symmetric-signed',           1,   6,  9000, torch.float32,    4, True,  False, False, 1),
    ('j-channel-symmetric-unsigned',         1,   6,  9000, torch.float32,    8, True,  True,  False, 1),
    ('j-embd-log-domain',                12289,   8,     1, torch.float32,    8, False, False, True,  3),
]


def _slice_probes(outer, P, inner, slices):
    """flat positions: first / last element of the tensor, last element of the first slice, first and last element of the
    last NON-EMPTY slice (each with another parameter), first element of the second slice"""
    chunk = _ceil_div(outer, slices)
    last = _ceil_div(outer, chunk) - 1                    # index of the last non-empty slice
    at = lambda o, p, i: (o * P + p) * inner + i
    pos = [at(0, 0, 0), at(outer - 1, P - 1, inner - 1), at(min(chunk, outer) - 1, 1 % P, inner - 1),
           at(last * chunk, 2 % P, 0), at(outer - 1, 3 % P, inner - 1), at(outer - 1, 0, 0)]
    if slices > 1:
        pos.append(at(chunk, P - 1, 0))
    return pos, chunk, last


@gpu
@pytest.mark.parametrize('case', VECTOR_CASES, ids=[c[0] for c in VECTOR_CASES])
def test_vector_parameters(case):
    """fq_bwd_params_k + fq_bwd_params_final_k: slice counts 1, 2, 3, 4 and 64, short and empty last slices, the
    `s > outer` clamp, parameters 256.. of the final kernel, 16-bit inputs, symmetric and log-domain quantizers.  The
    workspace size the library reports pins the slice count, so a plan change fails here first.  grad_x is bit-equal to the
    param_grads=False launch and to autograd; the 64-slice per-embedding case is also run twice (determinism)."""
    from quantization import _hip
    name, outer, P, inner, dtype, n_bits, symmetric, nonneg, log, want_slices = case
    slices = slices_of(outer, inner)
    assert slices == want_slices, ('bwd_param_slices no longer gives this shape the slice count it was picked for', slices)
    lib = _hip.backend().lib
    assert lib.tq_fake_quant_bwd_params_workspace_bytes(outer * P * inner, P, inner) == P * slices * 8
    if name.startswith('h-'):
        assert P > FINAL_BLOCK
    x3, g3 = _inputs(outer, P, inner, dtype, 300 + len(name), nonneg)
    q = _quant_from_data(x3, n_bits, symmetric, log)
    if symmetric:
        assert q.signed == (not nonneg)
    if log:
        x3 = _on_grid_inputs(x3, q, 17)
    else:
        _plant_edges(x3, q)
    probes, chunk, last = _slice_probes(outer, P, inner, slices)
    if name.startswith('e-'):
        assert (chunk, last) == (2, 32)                                   # slices 33..63 are empty
    if 'short-last' in name:
        assert 0 < outer - last * chunk < chunk and last == slices - 1
    if name.startswith('h-'):
        probes += [(0 * P + 255) * inner, (0 * P + 256) * inner, ((outer - 1) * P + 256) * inner]
    _plant_probes(x3, q, probes)
    _run_case(x3, g3, q, chunk * inner, probes, twice=(slices == 64 and inner == 1), tag=name)


# ------------------------------------------------------------------------------------------------------------------
# the two gates of the final kernels
# ------------------------------------------------------------------------------------------------------------------
GATE_EPS = 2.0 ** -5


def _gate_inputs(outer, P, inner, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(outer, P, inner, generator=g) * 0.6, torch.randn(outer, P, inner, generator=g)


@gpu
@pytest.mark.parametrize('n_bits', [4, 8])
def test_gates_per_tensor(n_bits):
    """fq_bwd_final: delta < eps closes d_delta (scale = clamp(delta, eps) is flat there), rint(zero_float) outside
    [lo, hi] closes d_zero_float (the clamp of the zero point is flat there); exactly 0 then, the full sum otherwise."""
    hi = 2.0 ** n_bits - 1
    x3, g3 = _gate_inputs(1000, 1, 1, 5)
    epb = tensor_form(1000, torch.float32, True)[1]
    seen = []
    for delta, zf in [(GATE_EPS / 2, 3.0), (GATE_EPS, 3.0), (2 * GATE_EPS, 3.0),
                      (0.1, -0.6), (0.1, -0.4), (0.1, hi + 0.4), (0.1, hi + 0.6)]:
        q = Quant(torch.tensor([delta]), torch.tensor([zf]), n_bits, eps=GATE_EPS)
        ref = _reference(x3, g3, q)
        seen.append((float(ref['chain_delta']), float(ref['chain_zero_float'])))
        assert float(ref['d_scale'].abs()) > 0 and float(ref['d_zp'].abs()) > 0      # an open gate lets something through
        _run_case(x3, g3, q, epb, [], tag=('gate', delta, zf))
    assert seen == [(0.0, 1.0), (1.0, 1.0), (1.0, 1.0), (1.0, 0.0), (1.0, 1.0), (1.0, 1.0), (1.0, 0.0)]


@gpu
@pytest.mark.parametrize('n_bits', [4, 8])
def test_gates_mixed_across_a_parameter_vector(n_bits):
    """fq_bwd_params_final_k with open and closed gates side by side (P = 6)"""
    hi = 2.0 ** n_bits - 1
    x3, g3 = _gate_inputs(50, 6, 7, 6)
    delta = torch.tensor([GATE_EPS / 2, GATE_EPS, 2 * GATE_EPS, 0.1, 0.1, 0.1])
    zf = torch.tensor([3.0, -0.6, -0.4, hi + 0.4, hi + 0.6, 3.0])
    q = Quant(delta, zf, n_bits, eps=GATE_EPS, inner=7)
    ref = _reference(x3, g3, q)
    assert ref['chain_delta'].tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert ref['chain_zero_float'].tolist() == [1.0, 0.0, 1.0, 1.0, 0.0, 1.0]
    assert bool((ref['d_scale'].abs() > 0).all()) and bool((ref['d_zp'].abs() > 0).all())
    _run_case(x3, g3, q, _ceil_div(50, slices_of(50, 7)) * 7, [], tag=('gates', n_bits))


@gpu
def test_symmetric_per_tensor_returns_zero_zero_point_gradient():
    x3, g3 = _inputs(5000, 1, 1, torch.float32, 9)
    q = _quant_from_data(x3, 4, symmetric=True)
    assert q.signed
    _run_case(x3, g3, q, tensor_form(5000, torch.float32, True)[1], [0, 4999], tag='symmetric per tensor')


# ------------------------------------------------------------------------------------------------------------------
# workspace
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_workspace_one_float_short_is_refused_before_any_launch():
    """TQ_EWORKSPACE (-3) for a workspace one float short of P * slices * 8 bytes, vector and per-tensor parameters; no
    output buffer is touched."""
    from quantization import _hip
    be = _hip.backend()
    lib = be.lib
    st = torch.cuda.current_stream().cuda_stream
    for outer, P, inner in [(12289, 8, 1), (65, 2, 4096), (600, 1, 1)]:
        n = outer * P * inner
        x = torch.randn(n, device=DEV)
        gy = torch.randn(n, device=DEV)
        gx = torch.full((n,), 7.0, device=DEV)
        gd = torch.full((P,), 7.0, device=DEV)
        gz = torch.full((P,), 7.0, device=DEV)
        d = torch.full((P,), 0.1, device=DEV)
        z = torch.full((P,), 3.0, device=DEV)
        q = _hip.tq_quantizer(d.data_ptr(), z.data_ptr(), None, 8, 0, 0, 1e-8, P, inner)
        if P > 1:
            need = P * slices_of(outer, inner) * 8
            assert lib.tq_fake_quant_bwd_params_workspace_bytes(n, P, inner) == need
        else:
            need = tensor_form(n, torch.float32, True)[2] * 8          # one (d, z) pair per block
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        call = lambda nbytes: lib.tq_fake_quant_bwd(x.data_ptr(), gy.data_ptr(), gx.data_ptr(), gd.data_ptr(), gz.data_ptr(), n,
                                                    0, C.byref(q), ws.data_ptr(), nbytes, st)
        assert call(need - 4) == -3 and 'workspace' in lib.tq_last_error().decode()
        torch.cuda.synchronize()
        assert bool((gx == 7.0).all()) and bool((gd == 7.0).all()) and bool((gz == 7.0).all())
        assert call(need) == 0
        torch.cuda.synchronize()
        assert not bool((gd == 7.0).any())
