"""The range-search kernels of csrc/tq_search.hip, called directly: `tq_argmin_select`, `tq_xent_candidates`,
`tq_mse_candidates` / `tq_mse_candidates_grouped`.  Every MSE / cross-entropy estimator and AdaRound's weight-range init end
in them; the estimator traces reach them only at the shapes of the golden file.

argmin_select   np.argmin semantics, compared exactly (first minimum wins, first NaN wins).  The kernel is a strided scan
                (candidate c belongs to thread c % 256) and a 256-way merge by thread 0, so the cases put ties and NaNs in
                one thread, in neighbouring threads, and with the LOWER index in the LATER thread.
xent_candidates float64 -softmax(x) * log_softmax(y), y dequantised from the fp32-exact index.  Tolerance per candidate,
                first order, device expf / logf assumed within 2 ulps (`xent_reference`):
                  2^-22 * sum over rows [(2 cols + 8) sum_j p_j |logq_j| + sum_j p_j |y_j - max y| + cols + 4 + |log sum exp|]
                The CPU test holds torch's fp32 evaluation (the `_oracle_backend` twin) and a sequential fp32 emulation of
                the kernel's order against the same bound.
mse_candidates  reference and bar of tests/test_fuzz_parity.py::test_mse_candidates_fuzz (float64 sum of the oracle's
                per-element error, 1e-5 |ref| + 1e-12), at the forms that test never reaches: 16 elements per lane, the
                grid-stride loop over tiles, candidate tiles halved down to 16, the segmented scalar and the ragged
                segmented vector path.  One-hot probe per case: x == 0 except the last element of the last tile; 0
                quantises exactly, so every candidate's loss is that element's single squared error, to 4 fp32 ulps.
"""
import numpy as np
import pytest
import torch

from tests._oracle_backend import OracleBackend

gpu = pytest.mark.gpu
DEV = 'cuda'

# ------------------------------------------------------------------------------------------------------------------
# Plan constants, mirrored once from csrc/tq_search.hip:
#   K_BLOCK           csrc/tq_device.h `constexpr int kBlock = 256` (argmin_select_k and mse_cand_k run 256 threads)
#   XENT_BLOCK        tq_xent_candidates: `dim3((unsigned)ceil_div(n_cand, 64)), dim3(64)`
#   plan_mse          `p.e = row_len <= 2048 ? 4 : 16`, `row_len < (uint64_t)kBlock * 16 * 256` -> 8,
#                     `constexpr int kCandTile = 128`, `while (p.cand_tile > 16 && tiles * rows * ceil_div(...) < 2048)`,
#                     `budget = max(1, 4096 / max(1, gy * rows))`
# ------------------------------------------------------------------------------------------------------------------
K_BLOCK = 256
XENT_BLOCK = 64
MSE_SMALL_ROW = 2048
MSE_E16_MIN_ROW = K_BLOCK * 16 * 256          # 1 048 576
CAND_TILE, CAND_TILE_MIN = 128, 16
MSE_FILL_BLOCKS, MSE_BLOCK_BUDGET = 2048, 4096


def _ceil_div(a, b):
    return -(-a // b)


def plan_mse(rows, row_len, n_cand):
    """plan_mse of csrc/tq_search.hip -> (E, tiles, cand_tile, gx, gy)"""
    e = 4 if row_len <= MSE_SMALL_ROW else (8 if row_len < MSE_E16_MIN_ROW else 16)
    tiles = _ceil_div(row_len, K_BLOCK * e)
    ct = CAND_TILE
    while ct > CAND_TILE_MIN and tiles * rows * _ceil_div(n_cand, ct) < MSE_FILL_BLOCKS:
        ct //= 2
    gy = _ceil_div(n_cand, ct)
    gx = max(1, min(tiles, max(1, MSE_BLOCK_BUDGET // max(1, gy * rows))))
    return e, tiles, ct, gx, gy


def _backend():
    from quantization import _hip
    return _hip.backend()


# ------------------------------------------------------------------------------------------------------------------
# argmin_select
# ------------------------------------------------------------------------------------------------------------------
def _distinct(rows, n, seed):
    return np.random.RandomState(seed).permutation(rows * n).reshape(rows, n).astype(np.float64) * 0.37 - 11.0


def _with(base, row, pairs):
    a = base.copy()
    for idx, v in pairs:
        a[row, idx] = v
    return a


def _argmin_cases():
    nan, inf = float('nan'), float('inf')
    cases = []
    for n in (1, 2, 255, 256, 257, 1000):
        for rows in (1, 3):
            cases.append(('distinct-%dx%d' % (rows, n), _distinct(rows, n, 10 * n + rows)))
    b1, b3 = _distinct(1, 1000, 1), _distinct(3, 1000, 2)
    lo = -1e6                                                        # below every random loss
    cases += [
        ('all-equal-1x1000', np.full((1, 1000), 2.5)),
        ('all-equal-3x257', np.full((3, 257), -7.0)),
        ('tie-same-thread-100-356', _with(b1, 0, [(100, lo), (356, lo)])),
        ('tie-neighbour-threads-100-101', _with(b1, 0, [(100, lo), (101, lo)])),
        ('tie-threads-255-0-at-255-256', _with(b1, 0, [(255, lo), (256, lo)])),
        ('tie-5-700', _with(b1, 0, [(5, lo), (700, lo)])),
        ('tie-700-5-written-in-reverse', _with(b1, 0, [(700, lo), (5, lo)])),
        ('tie-lower-index-in-later-thread-300-517', _with(b1, 0, [(517, lo), (300, lo)])),   # threads 5 and 44
        ('tie-three-rows', _with(_with(_with(b3, 0, [(5, lo), (700, lo)]), 1, [(300, lo), (517, lo)]), 2, [(999, lo), (743, lo)])),
        ('all-plus-inf-1x1000', np.full((1, 1000), inf)),
        ('all-plus-inf-3x2', np.full((3, 2), inf)),
        ('one-minus-inf-at-613', _with(b1, 0, [(613, -inf)])),
        ('minus-inf-twice-613-101', _with(b1, 0, [(613, -inf), (101, -inf)])),
        ('plus-inf-but-one', _with(np.full((1, 1000), inf), 0, [(777, 3.0)])),
        ('nan-alone-at-0', _with(b1, 0, [(0, nan)])),
        ('nan-alone-at-last', _with(b1, 0, [(999, nan)])),
        ('nan-at-600-minimum-at-3', _with(b1, 0, [(600, nan), (3, lo)])),
        ('nans-at-300-and-40', _with(b1, 0, [(300, nan), (40, nan)])),
        ('nans-lower-index-in-later-thread-517-300', _with(b1, 0, [(517, nan), (300, nan)])),
        ('nans-same-thread-40-296', _with(b1, 0, [(296, nan), (40, nan), (3, lo)])),
        ('nan-and-minus-inf', _with(b1, 0, [(600, nan), (3, -inf)])),
        ('all-nan', np.full((1, 300), nan)),
        ('nan-in-one-row-of-three', _with(_with(b3, 1, [(600, nan), (3, lo)]), 2, [(8, lo)])),
        ('single-candidate-nan', np.full((3, 1), nan)),
    ]
    return cases


ARGMIN_CASES = _argmin_cases()


def _thresholds(n):
    k = np.arange(n, dtype=np.float32)
    return -0.5 * k - 1.0, 0.25 * k + 1.0              # distinct per candidate, exact in fp32 up to n = 1000


def test_argmin_cases_mean_what_their_names_say():
    """np.argmin on the case tables (CPU): ties take the first index, a NaN beats every number, the first NaN wins."""
    want = {'tie-5-700': [5], 'tie-700-5-written-in-reverse': [5], 'tie-lower-index-in-later-thread-300-517': [300],
            'tie-same-thread-100-356': [100], 'tie-threads-255-0-at-255-256': [255], 'tie-three-rows': [5, 300, 743],
            'all-equal-3x257': [0, 0, 0], 'all-plus-inf-1x1000': [0], 'one-minus-inf-at-613': [613],
            'minus-inf-twice-613-101': [101], 'plus-inf-but-one': [777], 'nan-alone-at-0': [0], 'nan-alone-at-last': [999],
            'nan-at-600-minimum-at-3': [600], 'nans-at-300-and-40': [40], 'nans-lower-index-in-later-thread-517-300': [300],
            'nans-same-thread-40-296': [40], 'nan-and-minus-inf': [600], 'all-nan': [0], 'nan-in-one-row-of-three': None,
            'single-candidate-nan': [0, 0, 0]}
    table = dict(ARGMIN_CASES)
    for name, idx in want.items():
        got = np.argmin(table[name], axis=1).tolist()
        if idx is None:
            assert got[1:] == [600, 8] and got[0] not in (3, 8, 600)
        else:
            assert got == idx, name
    assert 517 % K_BLOCK < 300 % K_BLOCK and 5 % K_BLOCK < 700 % K_BLOCK          # which thread the merge visits first


@gpu
@pytest.mark.parametrize('name,loss', ARGMIN_CASES, ids=[c[0] for c in ARGMIN_CASES])
def test_argmin_select(name, loss):
    be = _backend()
    rows, n = loss.shape
    tmin, tmax = _thresholds(n)
    ref = np.argmin(loss, axis=1)
    cur_min, cur_max, best = be.argmin_select(torch.from_numpy(loss).to(DEV), torch.from_numpy(tmin).to(DEV),
                                              torch.from_numpy(tmax).to(DEV))
    assert best.dtype == torch.int64 and best.cpu().numpy().tolist() == ref.tolist(), name
    assert np.array_equal(cur_min.cpu().numpy(), tmin[ref]) and np.array_equal(cur_max.cpu().numpy(), tmax[ref]), name
    twin = OracleBackend().argmin_select(torch.from_numpy(loss), torch.from_numpy(tmin), torch.from_numpy(tmax))
    assert torch.equal(best.cpu(), twin[2]) and torch.equal(cur_min.cpu(), twin[0]) and torch.equal(cur_max.cpu(), twin[1]), name


# ------------------------------------------------------------------------------------------------------------------
# xent_candidates
# ------------------------------------------------------------------------------------------------------------------
XENT_SHAPES = [(1, 1), (1, 2), (7, 3), (32, 3), (33, 64), (128, 2)]
XENT_CANDS = [1, XENT_BLOCK - 1, XENT_BLOCK, XENT_BLOCK + 1, 200]
SATURATING_SCALE = 2.0 ** -100            # every logit clamps to lo or hi; y = scale * k is 0 to 1e-27: a uniform softmax


def _xent_inputs(rows, cols, n_cand, seed):
    """logits ~ randn * 3; candidates (scale, zp, lo, hi) cycling through fine (8-bit), coarse (4-bit, 2-bit) and
    saturating grids"""
    rs = np.random.RandomState(seed)
    x = (rs.randn(rows, cols) * 3).astype(np.float32)
    span = float(np.abs(x).max()) * 2 + 1.0
    tab = np.zeros((n_cand, 4), np.float32)
    kinds = []
    for c in range(n_cand):
        kind = ('fine', 'coarse4', 'saturating', 'coarse2')[c % 4] if n_cand > 1 else 'fine'
        top = {'fine': 255.0, 'coarse4': 15.0, 'coarse2': 3.0, 'saturating': 255.0}[kind]
        scale = SATURATING_SCALE if kind == 'saturating' else span / top * rs.uniform(0.3, 1.2)
        tab[c] = (scale, np.round(rs.uniform(0, top)), 0.0, top)
        kinds.append(kind)
    return x, tab, kinds


def xent_reference(x, tab):
    """-> (loss[C], bound[C]) in float64.  The index is the fp32 one (IEEE division, as q_index computes it); from there on
    float64: y = scale * (index - zp), p = softmax(x), logq = log_softmax(y), loss = sum over rows and columns of -p logq.
    bound: see the module docstring."""
    s, zp, lo, hi = (tab[:, k].reshape(-1, 1, 1) for k in range(4))
    idx = np.clip(np.rint((x[None] / s).astype(np.float32)) + zp, lo, hi)
    assert idx.dtype == np.float32
    y = s.astype(np.float64) * (idx.astype(np.float64) - zp.astype(np.float64))
    x64 = x.astype(np.float64)[None]
    ex = np.exp(x64 - x64.max(-1, keepdims=True))
    p = ex / ex.sum(-1, keepdims=True)
    ymax = y.max(-1, keepdims=True)
    lse = np.log(np.exp(y - ymax).sum(-1, keepdims=True))
    logq = (y - ymax) - lse
    loss = (-(p * logq)).sum((-1, -2))
    cols = x.shape[1]
    per_row = ((2 * cols + 8) * (p * np.abs(logq)).sum(-1) + (p * np.abs(y - ymax)).sum(-1) + cols + 4 + np.abs(lse[..., 0]))
    return loss, 2.0 ** -22 * per_row.sum(-1)


def _kernel_order_fp32(x, tab):
    """xent_cand_k's arithmetic, operation by operation in fp32 and in its order (sequential sums over the columns, row
    losses added in float64), with numpy's fp32 exp / log in place of the device's"""
    f = np.float32
    C, (rows, cols) = tab.shape[0], x.shape
    s, zp, lo, hi = (tab[:, k].reshape(-1, 1, 1) for k in range(4))
    y = (s * (np.clip(np.rint(x[None] / s) + zp, lo, hi) - zp)).astype(f)
    xs, qs = np.zeros((1, rows), f), np.zeros((C, rows), f)
    xm, qm = x.max(-1)[None], y.max(-1)
    for j in range(cols):
        xs = (xs + np.exp((x[None, :, j] - xm).astype(f))).astype(f)
        qs = (qs + np.exp((y[:, :, j] - qm).astype(f))).astype(f)
    lqs = np.log(qs).astype(f)
    row_loss = np.zeros((C, rows), f)
    for j in range(cols):
        prob = (np.exp((x[None, :, j] - xm).astype(f)) / xs).astype(f)
        logq = ((y[:, :, j] - qm).astype(f) - lqs).astype(f)
        row_loss = (row_loss + (-prob * logq).astype(f)).astype(f)
    return row_loss.astype(np.float64).sum(-1)


def _xent_premises(x, tab, kinds, ref):
    rows, cols = x.shape
    if cols == 1:
        assert np.all(ref == 0.0)
    for c, kind in enumerate(kinds):
        if kind == 'saturating':
            assert abs(ref[c] - rows * np.log(cols)) <= 1e-12 * max(1.0, rows * np.log(cols)), (c, ref[c])


@pytest.mark.parametrize('rows,cols', XENT_SHAPES)
def test_xent_bound_holds_for_fp32_evaluations_on_the_cpu(rows, cols):
    """Two fp32 evaluations that share nothing with the kernel but the formula stay inside the derived bound: torch's
    (softmax / log_softmax of the `_oracle_backend` twin) and a sequential emulation of the kernel's order."""
    for n_cand in XENT_CANDS:
        x, tab, kinds = _xent_inputs(rows, cols, n_cand, 100 * rows + cols)
        ref, bound = xent_reference(x, tab)
        _xent_premises(x, tab, kinds, ref)
        twin = OracleBackend().xent_candidates(torch.from_numpy(x), torch.from_numpy(tab),
                                               torch.zeros((1, n_cand), dtype=torch.float64)).numpy()[0]
        emu = _kernel_order_fp32(x, tab)
        for name, got in (('torch fp32', twin), ('kernel order fp32', emu)):
            err = np.abs(got - ref)
            worst = int(np.argmax(err - bound))
            assert np.all(err <= bound), (name, rows, cols, n_cand, worst, kinds[worst], got[worst], ref[worst], err[worst], bound[worst])


@gpu
@pytest.mark.parametrize('rows,cols', XENT_SHAPES)
def test_xent_candidates(rows, cols):
    """Every candidate count around the 64-thread block (1, 63, 64, 65, 200); fine, coarse and saturating grids in one
    table (a saturating grid gives rows * log(cols)); cols = 1 gives exactly 0; a second call on the same buffer doubles
    it exactly (+=)."""
    be = _backend()
    for n_cand in XENT_CANDS:
        x, tab, kinds = _xent_inputs(rows, cols, n_cand, 100 * rows + cols)
        ref, bound = xent_reference(x, tab)
        _xent_premises(x, tab, kinds, ref)
        loss = be.zeros_f64((1, n_cand), DEV)
        xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(tab).to(DEV)
        be.xent_candidates(xd, td, loss)
        got = loss.cpu().numpy()[0].copy()
        err = np.abs(got - ref)
        worst = int(np.argmax(err - bound))
        assert np.all(err <= bound), (rows, cols, n_cand, worst, kinds[worst], got[worst], ref[worst], err[worst], bound[worst])
        if cols == 1:
            assert np.all(got == 0.0), got
        be.xent_candidates(xd, td, loss)
        assert np.array_equal(loss.cpu().numpy()[0], 2.0 * got), (rows, cols, n_cand, 'the second call must add the same sums')


@gpu
def test_xent_on_float64_input_stays_refused():
    from quantization._hip import TQError
    be = _backend()
    x = torch.randn(4, 3, dtype=torch.float64, device=DEV)
    tab = torch.tensor([[0.1, 3.0, 0.0, 255.0]], device=DEV)
    loss = be.zeros_f64((1, 1), DEV)
    with pytest.raises(TQError, match='the cross-entropy range search is fp32 only'):
        be.xent_candidates(x, tab, loss)
    assert float(loss.cpu()) == 0.0


# ------------------------------------------------------------------------------------------------------------------
# mse_candidates / mse_candidates_grouped
# ------------------------------------------------------------------------------------------------------------------
PROBE_X = 1.703125                      # exact in fp32, bf16 and fp16


def _mse_table(C, n_bits, rs):
    """candidates sampled as tests/test_fuzz_parity.py::test_mse_candidates_fuzz samples them"""
    top = 2.0 ** n_bits - 1
    scales = np.exp(rs.uniform(-5, 0, C)).astype(np.float32)
    zps = np.round(rs.uniform(0, top, C)).astype(np.float32)
    return np.stack([scales, zps, np.zeros(C, np.float32), np.full(C, top, np.float32)], 1)


def _mse_ref(xr, cand):
    """float64 sum of the oracle's per-element error of one row (fp32 tensor) under one candidate"""
    s_, z_, lo, hi = (float(v) for v in cand)
    xi = torch.clamp(torch.round(xr / s_) + z_, lo, hi)
    return float(((xr - s_ * (xi - z_)).double() ** 2).sum())


def _assert_mse(got, ref, tag):
    assert abs(got - ref) <= 1e-5 * abs(ref) + 1e-12, tag + (got, ref)


def _check_mse(x, tab, check_rows, grouped=None, tag=()):
    """x: [rows, L] (contiguous rows) or, grouped = n_groups, [tokens, d].  The reference for the rows in check_rows and
    every candidate; then the one-hot probe."""
    be = _backend()
    C = tab.shape[0]
    td = torch.from_numpy(tab).to(DEV)
    if grouped:
        ng, d = grouped, x.shape[-1]
        row_of = lambda t, r: t.float().reshape(-1, ng, d // ng)[:, r, :].reshape(-1)
        launch = lambda xd, loss: be.mse_candidates_grouped(xd, ng, td, loss)
        n_rows = ng
    else:
        row_of = lambda t, r: t.float()[r]
        launch = lambda xd, loss: be.mse_candidates(xd, x.shape[0], td, loss)
        n_rows = x.shape[0]
    loss = be.zeros_f64((n_rows, C), DEV)
    launch(x.to(DEV), loss)
    got = loss.cpu().numpy()
    for r in check_rows:
        xr = row_of(x, r)
        for c in range(C):
            _assert_mse(got[r, c], _mse_ref(xr, tab[c]), tag + (r, c))
    # one-hot: the last element of the last tile of the last row / group, everything else 0
    hot = torch.zeros(x.shape, dtype=x.dtype, device=DEV)
    hot.view(-1)[-1] = PROBE_X
    loss = be.zeros_f64((n_rows, C), DEV)
    launch(hot, loss)
    got = loss.cpu().numpy()
    assert np.all(got[:-1] == 0.0), tag + ('rows of zeros must give exactly 0',)
    one = torch.tensor([PROBE_X])
    for c in range(C):
        ref = _mse_ref(one, tab[c])
        assert abs(got[-1, c] - ref) <= 4 * 2.0 ** -23 * ref, tag + ('one-hot', c, got[-1, c], ref)
    assert max(_mse_ref(one, tab[c]) for c in range(C)) > 0


def _mse_plan_is(rows, row_len, C, want):
    """the case still reaches the form it was picked for, and the library plans the same number of x blocks"""
    plan = plan_mse(rows, row_len, C)
    assert plan == want, ('plan_mse no longer gives this shape the form the case was picked for', plan, want)
    assert _backend().lib.tq_mse_workspace_bytes(rows, row_len, C) == rows * plan[3] * C * 8


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_mse_sixteen_elements_per_lane(dtype):
    """E = 16 from row_len = 1 048 576 (a 768 x 3072 weight takes it): 257 tiles of 4096, the last with 3 elements"""
    L, C = (1 << 20) + 3, 7
    _mse_plan_is(1, L, C, (16, 257, 16, 257, 1))
    assert plan_mse(1, MSE_E16_MIN_ROW - 1, C)[0] == 8
    rs = np.random.RandomState(61)
    x = (torch.randn(1, L, generator=torch.Generator().manual_seed(61)) * 2).to(dtype)
    _check_mse(x, _mse_table(C, 8, rs), [0], tag=('E16', str(dtype)))


@gpu
def test_mse_grid_stride_over_tiles():
    """rows * gy eats the 4096-block budget: gx = 1 block walks the 3 tiles of a row"""
    rows, L, C = 3000, 5000, 16
    _mse_plan_is(rows, L, C, (8, 3, 128, 1, 1))
    rs = np.random.RandomState(62)
    x = torch.randn(rows, L, generator=torch.Generator().manual_seed(62)) * 2
    _check_mse(x, _mse_table(C, 4, rs), [0, 1499, 2999], tag=('grid-stride',))


@gpu
@pytest.mark.parametrize('C,gy', [(16, 1), (17, 2), (33, 3), (129, 9)])
def test_mse_candidate_tile_halved_to_16(C, gy):
    """one small row: the candidate tile halves down to 16, the candidates spread over gy blocks (the last one ragged)"""
    _mse_plan_is(1, 300, C, (4, 1, 16, 1, gy))
    rs = np.random.RandomState(63 + C)
    x = torch.randn(1, 300, generator=torch.Generator().manual_seed(C)) * 2
    _check_mse(x, _mse_table(C, 8, rs), [0], tag=('cand-tile', C))


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=['fp32', 'fp16'])
def test_mse_grouped_scalar_segmented_path(dtype):
    """d = 18 in 6 groups: segments of 3 elements are no whole 16-byte vectors"""
    tokens, d, ng, C = 257, 18, 6, 20
    assert (d // ng) % (4 if dtype == torch.float32 else 8) != 0
    _mse_plan_is(ng, tokens * (d // ng), C, (4, 1, 16, 1, 2))
    rs = np.random.RandomState(64)
    x = (torch.randn(tokens, d, generator=torch.Generator().manual_seed(64)) * 2).to(dtype)
    _check_mse(x, _mse_table(C, 4, rs), range(ng), grouped=ng, tag=('grouped-scalar', str(dtype)))


@gpu
def test_mse_grouped_vector_path_with_ragged_last_tile():
    """d = 48 in 6 groups, bf16: segments of one 16-byte vector; 1031 tokens are 8248 elements per group, 5 tiles of 2048,
    the last with 56"""
    tokens, d, ng, C = 1031, 48, 6, 20
    assert (d // ng) % 8 == 0 and d % 8 == 0 and (tokens * (d // ng)) % 2048 == 56
    _mse_plan_is(ng, tokens * (d // ng), C, (8, 5, 16, 5, 2))
    rs = np.random.RandomState(65)
    x = (torch.randn(tokens, d, generator=torch.Generator().manual_seed(65)) * 2).to(torch.bfloat16)
    _check_mse(x, _mse_table(C, 8, rs), range(ng), grouped=ng, tag=('grouped-vector',))
