"""The tiled integer Linears at the ENDS of their operand range, against int64 sums.

Every other test of tq_linear_i8_fwd & co draws uniform operands with mid-grid zero points: the accumulators stay near
sqrt(K) 74 74 < 2^20.  Here the operands are saturated -- x at the top (index 255, z_x = 0 or 1) or the bottom (index 0,
z_x = 255) of its grid, w rows alternating +127 / -128 by output feature -- with a seeded ~3 % of every x and w row overwritten
by uniform grid values, so that every output has a sum of its own (a kernel that reads the wrong K slab, row or column cannot
pass by constancy).  That reaches what the header of csrc/tq_linear_i8.hip promises and nothing else runs:

    |tot| up to 255 * 128 * K = 5.3e8 at K = 16384 (int32; the largest sum any operands can give -- just under 2^29)
    (float)(acc + rs) above 2^24, where the int -> float conversion rounds (from K = 768 on)
    shift = 128 - z_x at its ends 128 and -127 (and their neighbour 127) times w_rowsum in int32;  w = -128

Reference.  oracle/tq_int_oracle.c accumulates in int32 like the kernels, so on its own it could not tell a wrapped sum from a
right one: the CPU tests first tie it, bit for bit, to

    tot = x.int64 @ w.int64.T + (128 - z) * w.int64.sum(1)          pre = fp32(fp32(tot) * fp32(s_x * s_w[n]) + b[n])

(the formula of tests/test_linear_i8_skinny.py) and assert the premises -- conditions on the INPUTS, checked on the reference
alone: |tot| > 2^24 on every output from K = 768 on, both signs; the largest |tot| above 0.94 of the ceiling 255 * 128 * K for
K >= 16256 (the overwrite takes 3 % / 2 + 3 % = 4.5 % off the saturated sum in expectation; 2^29 itself is out of reach:
255 * 128 * 16384 = 534 773 760 < 536 870 912); |tot|, |x @ w.T| and |(128 - z) rowsum| below 2^31.  The GPU tests then hold
every launch form of `launch_linear_t`, the staircase epilogue, the grouped launch, the NoNorm tails, the class-ordered kernel
and the fused feed-forward block to the oracle at ZERO tolerance (uint32 views of fp32, torch.equal of bf16 and int8), in four
output variants: fp32 and bf16 y without a quantizer, y + y_idx behind an 8-bit asymmetric quantizer (none / ReLU), index-only.

Scales: per-tensor, and per-channel log-spaced over the columns (s_x s_w from 1e-10 to 1e-5; the lowest columns sit on the eps
floor of the weight scale), so that under ONE output quantizer some columns land inside the grid, some clamp at the top and some
at the bottom."""
import numpy as np
import pytest
import torch

from oracle import int_oracle as IO

gpu = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-8
X_DELTA = np.float32(0.02)
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
PATTERNS = {'plus': (127, 0), 'minus': (-128, 255), 'one': (127, 1)}      # saturated x (index - 128), z_x
I8_ENV = ('TQ_I8_LDS', 'TQ_I8_BIG_MIN', 'TQ_I8_RING_MIN_K', 'TQ_I8_RING_MAX_GRID', 'TQ_I8_SMALL_MAX_GRID', 'TQ_I8_FAST_EPI',
          'TQ_I8_STAIR', 'TQ_I8_LDS_PAD', 'TQ_FFN_BM')

# launch forms of launch_linear_t (csrc/tq_linear_i8.hip): the smallest shape that selects each, and the switches that do
FORMS = {
    # M % 64 != 0 -> linear_i8_k<32, 32> (LDS-free, 32 x 32 wave tiles), the longest K
    'lds-free-M32': ((32, 32, 16384), {}),
    # K % 128 == 64 -> linear_i8_k<32, 32>; M, N no multiples of 64 either, more than one block
    'lds-free-K832': ((96, 160, 832), {}),
    # K % 256 != 0 (no ring), grid 1 <= 256 -> linear_i8_lds_k<16> (32 x 32 block tiles, double buffer)
    'tiles32': ((64, 64, 16256), {}),
    # K % 256 == 0, K >= 1024, grid 1 <= 256 -> linear_i8_lds_k<32, ..., 8> (64 x 64 tiles, 8-stage ring)
    'ring': ((64, 64, 16384), {}),
    # ring and 32 x 32 tiles switched off -> linear_i8_lds_k<32> (64 x 64 tiles, double buffer)
    'tiles64': ((64, 64, 16384), {'TQ_I8_RING_MAX_GRID': '0', 'TQ_I8_SMALL_MAX_GRID': '0'}),
    # one 128 x 128 tile, K >= 512, tiles128 >= TQ_I8_BIG_MIN -> linear_i8_lds_k<64> (128 x 128 tiles)
    'tiles128': ((128, 128, 16384), {'TQ_I8_BIG_MIN': '1'}),
    # the ring kernel with the generic epilogue (one scalar conversion per accumulator instead of the packed pairs)
    'generic-epilogue': ((64, 64, 16384), {'TQ_I8_FAST_EPI': '0'}),
    # BERT's K, sums above 2^24 only: K = 768 < 1024 -> linear_i8_lds_k<16> (32 x 32 tiles); K = 3072 -> the ring
    'bert-K768': ((64, 64, 768), {}),
    'bert-K3072': ((64, 64, 3072), {}),
}
# (and the shapes of the grouped launch and of the NoNorm tails below: every problem of this file is tied to int64 on the CPU)
SHAPES = sorted({shape for shape, _ in FORMS.values()} | {(64, 192, 16384), (64, 128, 16384)})


# ---- operands and references -------------------------------------------------------------------------------------------------
def _overwrite(a, rng, share=0.03):
    """uniform grid values on a seeded ~3 % of the positions of every row"""
    hit = rng.random(a.shape) < share
    a[hit] = rng.integers(-128, 128, int(hit.sum())).astype(np.int8)
    return a


def _saturated_w(N, K, rng):
    """rows alternating +127 / -128 by output feature (the signed grid's two ends), ~3 % overwritten"""
    w = np.where(np.arange(N) % 2 == 0, 127, -128).astype(np.int8)[:, None].repeat(K, 1)
    return _overwrite(np.ascontiguousarray(w), rng)


def _problem(M, N, K, pattern):
    xv, z = PATTERNS[pattern]
    rng = np.random.default_rng(1000 * M + 10 * N + K + 7 * z)
    x = _overwrite(np.full((M, K), xv, np.int8), rng)
    w = _saturated_w(N, K, rng)
    top = 255.0 * 127.5 * K                                       # size of a saturated sum
    # one output grid for every scale below: 128 steps reach the pre-activation of the column 3 / 4 up the log-spaced scales
    q_delta = np.float32(top * 10.0 ** -6.25 / 128)
    return dict(x=x, w=w, z=z, x_zf=np.float32(z),
                wd_one=np.array([3e-7], np.float32) / X_DELTA,
                wd_row=(np.logspace(-10, -5, N) / X_DELTA).astype(np.float32),
                bias=(rng.standard_normal(N) * 6.0 * q_delta).astype(np.float32),
                q_out=(float(q_delta), 121.0, None, 8, False, False, EPS))


def _tot(x, w, z):
    """(tot, x @ w.T, (128 - z) rowsum) in int64"""
    w64 = w.astype(np.int64)
    acc = x.astype(np.int64) @ w64.T
    corr = (128 - int(z)) * w64.sum(1)[None, :]
    return acc + corr, acc, corr


def _pre64(tot, x_delta, w_delta, bias):
    """pre = fp32(fp32(tot) * fp32(s_x * s_w[n]) + b[n]): every fp32 operation rounded on its own"""
    sw = np.maximum(np.asarray(w_delta, np.float32), np.float32(EPS)).astype(np.float32)
    sx = np.float32(max(np.float32(x_delta), np.float32(EPS)))
    pre = tot.astype(np.float32) * (sx * np.broadcast_to(sw, (tot.shape[1],))).astype(np.float32)[None, :]
    if bias is not None:
        pre = (pre + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
    return pre.astype(np.float32)


def _bits_equal(a, b):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32)
    b = np.ascontiguousarray(b.cpu().numpy() if torch.is_tensor(b) else b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


_REF = {}


def _oracle_pre(shape, pattern, per_channel, with_bias):
    """IO.linear_i8 without activation and quantizer: computed once per problem, shared by every launch form, never modified"""
    key = (shape, pattern, per_channel, with_bias)
    if key not in _REF:
        p = _problem(*shape, pattern)
        _REF[key] = IO.linear_i8(_t(p['x']), _t(p['w']), _t(p['bias']) if with_bias else None, (X_DELTA, p['x_zf'], 8, EPS),
                                 _t(p['wd_row'] if per_channel else p['wd_one']), EPS, ACT_NONE, None)[0]
    return _REF[key]


def _clear_env(monkeypatch, env=None):
    for v in I8_ENV:
        monkeypatch.delenv(v, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)               # read per call by the launchers (csrc/tq_host.h)


def _q_dev(q):
    return None if q is None else (torch.tensor([q[0]], dtype=torch.float32, device=DEV),
                                   torch.tensor([q[1]], dtype=torch.float32, device=DEV), None) + tuple(q[3:])


def _xq_dev(zf, delta=X_DELTA):
    return (torch.tensor([delta], dtype=torch.float32, device=DEV), torch.tensor([zf], dtype=torch.float32, device=DEV), 8, EPS)


# ---- CPU: the oracle is tied to int64, the premises hold ---------------------------------------------------------------------
@pytest.mark.parametrize('pattern', list(PATTERNS))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_oracle_equals_the_int64_sums_and_the_premises_hold_cpu(shape, pattern):
    M, N, K = shape
    p = _problem(M, N, K, pattern)
    tot, acc, corr = _tot(p['x'], p['w'], p['z'])
    a = np.abs(tot)
    print(f'{shape} {pattern}: |tot| in [{a.min()}, {a.max()}] = [2^{np.log2(a.min()):.2f}, 2^{np.log2(a.max()):.2f}], '
          f'|acc| <= {np.abs(acc).max()}, |corr| <= {np.abs(corr).max()}')
    assert a.max() < 2 ** 31 and np.abs(acc).max() < 2 ** 31 and np.abs(corr).max() < 2 ** 31
    assert (p['w'] == -128).any() and (p['w'] == 127).any()
    if K >= 768:
        assert a.min() > 2 ** 24, a.min()
        assert (tot > 0).any() and (tot < 0).any()
    if K >= 16256:
        assert a.max() > 0.94 * 255 * 128 * K and a.max() > 1.85 * 2 ** 28, a.max()
    for per_channel in (False, True):
        for with_bias in (False, True):
            want = _pre64(tot, X_DELTA, p['wd_row'] if per_channel else p['wd_one'], p['bias'] if with_bias else None)
            assert _bits_equal(_oracle_pre(shape, pattern, per_channel, with_bias), want), (per_channel, with_bias)
    # one output quantizer over the log-spaced columns: inside the grid, clamped at the top, clamped at the bottom
    _, idx = IO.epilogue(_oracle_pre(shape, pattern, True, True), ACT_NONE, p['q_out'])
    assert (idx == 127).any() and (idx == -128).any() and idx.unique().numel() > N // 4, idx.unique().numel()


# ---- GPU: every launch form of launch_linear_t -------------------------------------------------------------------------------
def _check_four_variants(call, pre, q, what):
    """call(activation, q_out on the device or None, dtype, want_idx, want_y) against the oracle's epilogue on `pre`"""
    assert _bits_equal(call(ACT_NONE, None, torch.float32, False, True), pre), f'{what}: fp32 pre-activation'
    assert torch.equal(call(ACT_NONE, None, torch.bfloat16, False, True).cpu(), pre.to(torch.bfloat16)), f'{what}: bf16'
    for act in (ACT_NONE, ACT_RELU):
        ry, ri = IO.epilogue(pre, act, q)
        y, yi = call(act, _q_dev(q), torch.float32, True, True)
        assert torch.equal(yi.cpu(), ri), f'{what}: act {act}, {int((yi.cpu() != ri).sum())} indices differ'
        assert _bits_equal(y, ry), f'{what}: act {act}, values'
        none, only = call(act, _q_dev(q), torch.float32, True, False)
        assert none is None and torch.equal(only.cpu(), ri), f'{what}: act {act}, index-only'


@gpu
@pytest.mark.parametrize('pattern', list(PATTERNS))
@pytest.mark.parametrize('form', list(FORMS))
def test_every_launch_form_equals_the_oracle(form, pattern, monkeypatch):
    from quantization import _hip
    be = _hip.backend()
    shape, env = FORMS[form]
    _clear_env(monkeypatch, env)
    p = _problem(*shape, pattern)
    x, w = _t(p['x']).to(DEV), _t(p['w']).to(DEV)
    rs = be.rowsum_i8(w)
    assert torch.equal(rs.cpu().long(), _t(p['w'].astype(np.int64).sum(1)))
    xq = _xq_dev(p['x_zf'])
    for per_channel in (False, True):
        wd = _t(p['wd_row'] if per_channel else p['wd_one']).to(DEV)
        for with_bias in (False, True):
            b = _t(p['bias']).to(DEV) if with_bias else None
            pre = _oracle_pre(shape, pattern, per_channel, with_bias)

            def call(act, q, dtype, want_idx, want_y):
                return be.linear_i8(x, w, rs, b, xq, wd, EPS, act, q, dtype, want_idx=want_idx, want_y=want_y)
            _check_four_variants(call, pre, p['q_out'], f'{form} {pattern} per_channel={per_channel} bias={with_bias}')


@gpu
@pytest.mark.parametrize('pattern', ['plus', 'minus'])
def test_staircase_epilogue_reads_both_ends_of_its_table(pattern, monkeypatch):
    """(64, 64, 16384) on linear_i8_lds_k<32> (64 x 64 tiles, double buffer: a table excludes the ring and the 32 x 32 tiles):
    GELU + quantizer through the staircase table, log-spaced per-channel scales -- pre-activations from a fraction of a grid
    step to far beyond both ends of the table's bins -- against the oracle's correctly rounded GELU (code 4)"""
    from quantization import _hip
    from tests._exact_backend import stair_header_ok
    be = _hip.backend()
    shape = (64, 64, 16384)
    _clear_env(monkeypatch, {'TQ_I8_RING_MAX_GRID': '0', 'TQ_I8_SMALL_MAX_GRID': '0'})
    p = _problem(*shape, pattern)
    x, w = _t(p['x']).to(DEV), _t(p['w']).to(DEV)
    rs, wd, b, q = be.rowsum_i8(w), _t(p['wd_row']).to(DEV), _t(p['bias']).to(DEV), p['q_out']
    stair = be.act_stair(ACT_GELU, _q_dev(q), be.stair_bins_for(shape[0], shape[1]))
    assert stair_header_ok(stair[0]), 'the builder declined the table: pick a coarser output grid'
    pre = _oracle_pre(shape, pattern, True, True)
    ry, ri = IO.epilogue(pre, 4, q)
    assert float(pre.min()) < -100 * q[0] and float(pre.max()) > 300 * q[0] and ri.unique().numel() > 10
    args = (x, w, rs, b, _xq_dev(p['x_zf']), wd, EPS, ACT_GELU, _q_dev(q))
    y, yi = be.linear_i8(*args, torch.float32, want_idx=True, stair=stair)
    assert torch.equal(yi.cpu(), ri) and _bits_equal(y, ry)
    yb, yib = be.linear_i8(*args, torch.bfloat16, want_idx=True, stair=stair)
    assert torch.equal(yb.cpu(), ry.to(torch.bfloat16)) and torch.equal(yib.cpu(), ri)
    none, only = be.linear_i8(*args, torch.float32, want_idx=True, want_y=False, stair=stair)
    assert none is None and torch.equal(only.cpu(), ri)


@gpu
@pytest.mark.parametrize('pattern', ['plus', 'minus'])
def test_grouped_launch_equals_the_oracle_group_by_group(pattern, monkeypatch):
    """(64, 192, 16384), three groups of 64 columns with an output quantizer each (one of them 4-bit): grid 3 -> the ring
    kernel; every group equals IO.linear_i8 of its slice"""
    from quantization import _hip
    be = _hip.backend()
    _clear_env(monkeypatch)
    M, N, K = 64, 192, 16384
    p = _problem(M, N, K, pattern)
    d = p['q_out'][0]
    q_outs = [p['q_out'], (d * 0.01, 3.0, None, 8, False, False, EPS), (d * 9.0, 7.0, None, 4, False, False, EPS)]
    x, w = _t(p['x']).to(DEV), _t(p['w']).to(DEV)
    rs, wd, b = be.rowsum_i8(w), _t(p['wd_row']).to(DEV), _t(p['bias']).to(DEV)
    for act in (ACT_NONE, ACT_RELU):
        y, yi = be.linear_i8_grouped(x, w, rs, b, _xq_dev(p['x_zf']), wd, EPS, act, [_q_dev(q) for q in q_outs], want_y=True,
                                     want_idx=True)
        for g, q in enumerate(q_outs):
            sl = slice(64 * g, 64 * (g + 1))
            ry, ri = IO.linear_i8(_t(p['x']), _t(p['w'][sl]), _t(p['bias'][sl]), (X_DELTA, p['x_zf'], 8, EPS), _t(p['wd_row'][sl]),
                                  EPS, act, q)
            assert torch.equal(yi[:, sl].cpu(), ri), f'group {g}, act {act}: indices'
            assert _bits_equal(y[:, sl], ry), f'group {g}, act {act}: values'
            assert ri.unique().numel() > (3 if g == 2 else 8)


def _tail(N, q_delta, seed):
    """NoNorm operands and the quantizers behind Q_dense, sized to its grid of 256 steps of q_delta"""
    rng = np.random.default_rng(seed)
    nn_w = (rng.random(N) + 0.5).astype(np.float32)
    nn_b = (rng.standard_normal(N) * 10 * q_delta).astype(np.float32)
    q_sum = (q_delta * 1.3, 119.0, None, 8, False, False, EPS)
    q_fin = (q_delta * 24.0, 7.0, None, 4, False, False, EPS)
    return nn_w, nn_b, q_sum, q_fin


@gpu
@pytest.mark.parametrize('pattern', ['plus', 'minus'])
@pytest.mark.parametrize('with_residual', [False, True], ids=['bottleneck', 'residual'])
@pytest.mark.parametrize('shape', [(96, 160, 832), (64, 128, 16384)], ids=lambda s: 'x'.join(map(str, s)))
def test_nonorm_tails_equal_the_oracle(shape, with_residual, pattern, monkeypatch):
    """tq_linear_i8_nonorm_fwd (tail 1 / 2 behind the saturated contraction): (96, 160, 832) -> linear_i8_k<32, 32, ., true>,
    (64, 128, 16384) -> the ring kernel with the tail"""
    from quantization import _hip
    be = _hip.backend()
    _clear_env(monkeypatch)
    M, N, K = shape
    p = _problem(M, N, K, pattern)
    q_dense = p['q_out']
    nn_w, nn_b, q_sum, q_fin = _tail(N, q_dense[0], seed=N + K)
    res = (np.random.default_rng(M).standard_normal((M, N)) * 40 * q_dense[0]).astype(np.float32) if with_residual else None
    x, w = _t(p['x']).to(DEV), _t(p['w']).to(DEV)
    rs = be.rowsum_i8(w)
    for per_channel in (False, True):
        wd = p['wd_row'] if per_channel else p['wd_one']
        ry, ri = IO.linear_i8(_t(p['x']), _t(p['w']), _t(p['bias']), (X_DELTA, p['x_zf'], 8, EPS), _t(wd), EPS, ACT_NONE, q_dense,
                              tail=2 if with_residual else 1, residual=_t(res), nn_w=_t(nn_w), nn_b=_t(nn_b),
                              q_t1=q_sum if with_residual else None, q_t2=q_fin)
        assert ri.unique().numel() > 8
        for dtype in (torch.float32, torch.bfloat16):
            y, yi = be.linear_i8_nonorm(x, w, rs, _t(p['bias']).to(DEV), None if res is None else _t(res).to(DEV),
                                        _t(nn_w).to(DEV), _t(nn_b).to(DEV), _xq_dev(p['x_zf']), _t(wd).to(DEV), EPS,
                                        _q_dev(q_dense), _q_dev(q_sum) if with_residual else None, _q_dev(q_fin), dtype,
                                        want_idx=True)
            assert torch.equal(yi.cpu(), ri), f'per_channel={per_channel} {dtype}: {int((yi.cpu() != ri).sum())} indices differ'
            assert torch.equal(y.cpu(), ry.to(dtype)) and (dtype != torch.float32 or _bits_equal(y, ry))


# ---- class-ordered input grid (tq_linear_i8_cls_fwd) ----------------------------------------------------------------------------
CLS_CASES = {
    'C2-0-255': ((64, 64, 16384), (0, 255)),
    'C2-255-0': ((64, 64, 16384), (255, 0)),
    'C6': ((64, 64, 3072), (0, 255, 1, 254, 0, 255)),
}


def _cls_problem(case):
    """operands as tests/test_linear_i8_peg.py::_problem builds them, classes in contiguous runs of K / C columns (natural order
    = class order): class c is saturated at the end of the grid its zero point z_c is farthest from, every class has a scale of
    its own, w as above.  One conversion per class, then an fp32 sum of class terms of OPPOSITE signs (z = 0 against z = 255)."""
    (M, N, K), zs = CLS_CASES[case]
    C = len(zs)
    rng = np.random.default_rng(K + 31 * C + zs[0])
    cls_of_col = np.repeat(np.arange(C), K // C)
    zc = np.array(zs, np.float32)
    dc = (X_DELTA * (1.0 + 0.37 * np.arange(C))).astype(np.float32)
    x = np.where(zc[cls_of_col] < 128, 127, -128).astype(np.int8)[None, :].repeat(M, 0)
    x = _overwrite(np.ascontiguousarray(x), rng)
    w = _saturated_w(N, K, rng)
    ends = np.cumsum(np.bincount(cls_of_col))
    reps = np.concatenate([[0], ends[:-1]])
    top = 255.0 * 127.5 * K / C
    q_delta = np.float32(top * 10.0 ** -6.25 / 128)
    return dict(x=x, w=w, zs=zs, x_delta=dc[cls_of_col], x_zf=zc[cls_of_col], ends=ends, reps=reps,
                wd_one=np.array([3e-7], np.float32) / X_DELTA, wd_row=(np.logspace(-10, -5, N) / X_DELTA).astype(np.float32),
                bias=(rng.standard_normal(N) * 6.0 * q_delta).astype(np.float32),
                q_out=(float(q_delta), 121.0, None, 8, False, False, EPS))


def _cls_pre(p, per_channel, with_bias):
    from tests._exact_backend import cls_pre
    return cls_pre(p['x'], p['w'], p['ends'], p['reps'], p['x_delta'], p['x_zf'], 8, EPS, p['wd_row'] if per_channel else p['wd_one'],
                   EPS, p['bias'] if with_bias else None)


@pytest.mark.parametrize('case', list(CLS_CASES))
def test_cls_reference_equals_its_int64_restatement_cpu(case):
    """tests/_exact_backend.cls_pre (float64 matrix products) against int64 class sums: per class fp32(tot_c) * fp32 scale, summed
    in class order in fp32, plus bias.  Premise for C = 2: every class sum of every output exceeds 2^24."""
    p = _cls_problem(case)
    N = p['w'].shape[0]
    for per_channel in (False, True):
        sw = np.broadcast_to(np.maximum(p['wd_row'] if per_channel else p['wd_one'], np.float32(EPS)).astype(np.float32), (N,))
        acc, s = None, 0
        for c, e in enumerate(p['ends']):
            tot_c = _tot(p['x'][:, s:e], p['w'][:, s:e], p['zs'][c])[0]
            assert np.abs(tot_c).max() < 2 ** 31
            if len(p['zs']) == 2:
                assert np.abs(tot_c).min() > 2 ** 24, (c, np.abs(tot_c).min())
            term = tot_c.astype(np.float32) * (np.float32(max(p['x_delta'][p['reps'][c]], np.float32(EPS))) * sw).astype(np.float32)[None, :]
            acc = term if acc is None else (acc + term).astype(np.float32)
            s = e
        assert _bits_equal(_cls_pre(p, per_channel, False), acc)
        assert _bits_equal(_cls_pre(p, per_channel, True), (acc + p['bias'][None, :]).astype(np.float32))


@gpu
@pytest.mark.parametrize('case', list(CLS_CASES))
def test_class_ordered_kernel_equals_its_reference(case, monkeypatch):
    """linear_i8_cls_k<32> (64 x 64 tiles) at class zero points 0 / 255 / 1 / 254, fast and generic epilogue"""
    from quantization import _hip
    be = _hip.backend()
    p = _cls_problem(case)
    x, w = _t(p['x']).to(DEV), _t(p['w']).to(DEV)
    starts = np.concatenate([[0], p['ends'][:-1]])
    rs = torch.stack([be.rowsum_i8(w[:, s:e].contiguous()) for s, e in zip(starts, p['ends'])]).contiguous()
    xq = (_t(p['x_delta']).to(DEV), _t(p['x_zf']).to(DEV), 8, EPS)
    table = be.cls_table(p['ends'], p['reps'])
    for fast in ('1', '0'):
        _clear_env(monkeypatch, {'TQ_I8_FAST_EPI': fast})
        for per_channel, with_bias in ((False, True), (True, False), (True, True)):
            wd = _t(p['wd_row'] if per_channel else p['wd_one']).to(DEV)
            b = _t(p['bias']).to(DEV) if with_bias else None
            pre = _t(_cls_pre(p, per_channel, with_bias))

            def call(act, q, dtype, want_idx, want_y):
                return be.linear_i8_cls(x, w, rs, b, xq, table, wd, EPS, act, q, dtype, want_idx=want_idx, want_y=want_y)
            _check_four_variants(call, pre, p['q_out'], f'{case} fast_epi={fast} per_channel={per_channel} bias={with_bias}')


# ---- fused feed-forward block (tq_ffn_i8_nonorm_fwd) -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('mid', ['clamped', 'graded'])
@pytest.mark.parametrize('pattern', ['plus', 'minus'])
@pytest.mark.parametrize('bm', ['16', '32'])
def test_fused_ffn_equals_the_oracle(bm, pattern, mid, monkeypatch):
    """M = 32, (K1, N1, N2) = (128, 512, 128), both block forms.  x saturated (z_x = 0 / 255), w1 = +127 / -128 by row, a bias
    that lifts every intermediate above zero, q_mid with zero point 0: 'clamped' -- a delta so small that the WHOLE intermediate
    sits at index 255, the second contraction is 512 * 255 * w2; 'graded' -- the intermediate spread over q_mid's grid, so that
    the first contraction decides it"""
    from quantization import _hip
    be = _hip.backend()
    _clear_env(monkeypatch, {'TQ_FFN_BM': bm})
    M, K1, N1, N2 = 32, 128, 512, 128
    xv, z = PATTERNS[pattern]
    rng = np.random.default_rng(5 + z)
    x = _overwrite(np.full((M, K1), xv, np.int8), rng)
    w1, w2 = _saturated_w(N1, K1, rng), _saturated_w(N2, N1, rng)
    w1d, w2d = np.array([1e-4], np.float32), (np.logspace(-9, -5, N2) / np.float32(0.001)).astype(np.float32)
    tot1 = _tot(x, w1, z)[0]
    peak = float(np.abs(tot1).max()) * float(X_DELTA) * 1e-4                 # largest |pre-activation| of the first Linear
    b1 = np.full(N1, 1.5 * peak, np.float32)
    q_mid = (peak / 1e4 if mid == 'clamped' else 2.6 * peak / 255, 0.0, None, 8, False, False, EPS)
    x_q = (X_DELTA, np.float32(z), 8, EPS)
    _, mid_idx = IO.linear_i8(_t(x), _t(w1), _t(b1), x_q, _t(w1d), EPS, ACT_RELU, q_mid)
    if mid == 'clamped':
        assert bool((mid_idx == 127).all())
        tot2 = _tot(mid_idx.numpy(), w2, 0)[0]
        assert np.array_equal(tot2, 255 * w2.astype(np.int64).sum(1)[None, :].repeat(M, 0)) and np.abs(tot2).max() > 2 ** 23.9
    else:
        assert mid_idx.unique().numel() > 20 and int(mid_idx.max()) < 127     # two clusters (the sign of w1's row), none clamped
    sat = 255.0 * 127.5 * N1 * float(q_mid[0])                              # a saturated second sum times the input scale
    q_dense = (sat * 10.0 ** -6.0 / 128, 121.0, None, 8, False, False, EPS)
    nn_w, nn_b, q_sum, q_fin = _tail(N2, q_dense[0], seed=11)
    b2 = (rng.standard_normal(N2) * 6 * q_dense[0]).astype(np.float32)
    res = (rng.standard_normal((M, N2)) * 40 * q_dense[0]).astype(np.float32)
    ry, ri = IO.ffn_i8(_t(x), x_q, _t(w1), _t(b1), _t(w1d), EPS, q_mid, _t(w2), _t(b2), _t(w2d), EPS, _t(res), _t(nn_w), _t(nn_b),
                       q_dense, q_sum, q_fin)
    assert ri.unique().numel() > 8
    w1g, w2g = _t(w1).to(DEV), _t(w2).to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        y, yi = be.ffn_i8_nonorm(_t(x).to(DEV), _xq_dev(np.float32(z)), w1g, be.rowsum_i8(w1g), _t(b1).to(DEV), _t(w1d).to(DEV), EPS,
                                 _q_dev(q_mid), w2g, be.rowsum_i8(w2g), _t(b2).to(DEV), _t(w2d).to(DEV), EPS, _t(res).to(DEV),
                                 _t(nn_w).to(DEV), _t(nn_b).to(DEV), _q_dev(q_dense), _q_dev(q_sum), _q_dev(q_fin), dtype,
                                 want_idx=True)
        assert torch.equal(yi.cpu(), ri), f'{dtype}: {int((yi.cpu() != ri).sum())} indices differ'
        assert torch.equal(y.cpu(), ry.to(dtype)) and (dtype != torch.float32 or _bits_equal(y, ry))


# ---- the generic epilogue of the kernels that hand it fp32 sums ------------------------------------------------------------------
@gpu
def test_generic_epilogue_of_the_16_bit_kernel_equals_its_reference(monkeypatch):
    """tq_linear_i16x8_fwd hands the epilogue fp32 pre-activations as the class-ordered kernel does.  Its generic epilogue
    (TQ_I8_FAST_EPI=0, Tanh, or an output grid the branch-free quantizer declines) gave all four columns of a lane the sum of
    the first one -- found by test_class_ordered_kernel_equals_its_reference; (64, 64, 128) on a 16-bit grid, uniform operands"""
    from tests import test_linear_i16x8 as X
    p = X._problem(64, 64, 128, 16, seed=5)
    tot = X._numpy_tot(p)
    q = (0.02, 121.0, None, 8, False, False, EPS)
    for fast in ('1', '0'):
        _clear_env(monkeypatch, {'TQ_I8_FAST_EPI': fast})
        be, hi, lo, w, rs, b, xq, wd = X._device(p, True, True)
        pre = _t(X._numpy_pre(p, tot, True, True))

        def call(act, q_out, dtype, want_idx, want_y):
            return be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, act, q_out, dtype, want_idx=want_idx, want_y=want_y)
        _check_four_variants(call, pre, q, f'16-bit input grid, fast_epi={fast}')
