"""Integer Linear for 16-bit activation inputs (mixed precision W8A16): tq_linear_i16x8_fwd and tq_quantize_hilo_fwd.

The grid index of a per-tensor asymmetric input quantizer of up to 16 bits is split into two int8 byte planes; the kernel
contracts each plane exactly on the i8 matrix cores and combines the sums in 64 bits (include/tq_hip.h):

    tot = 256 A_hi + A_lo + (32896 - z_x) rowsum        pre = RN32(tot) * (max(x_delta, eps) * s_w) + b

Bars: `pre` bit-exact against a numpy restatement (int64 tot, tot.astype(float32), separate fp32 multiply and add), also
where |tot| > 2^31; grids of <= 8 bits bit-identical to tq_linear_i8_stair_fwd; GELU + 8-bit output quantizer through the
staircase equal to the oracle's correctly rounded activation (code 4) at zero tolerance; the byte planes equal to
tq_fake_quant_fwd's int32 indices; `pre` within 1e-5 of the row scale of the reference's fp32 simulation."""
import ctypes as C

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

EPS = 1e-8


def _problem(M, N, K, n_bits, seed):
    rng = np.random.default_rng(seed)
    top = 2 ** n_bits - 1
    return dict(idx=rng.integers(0, top + 1, (M, K)).astype(np.int32),
                w=rng.integers(-127, 128, (N, K)).astype(np.int8),
                x_delta=np.float32(rng.uniform(1e-5, 4e-5) * 2.0 ** (16 - n_bits)), x_zf=np.float32(rng.uniform(0, top)),
                wd_row=rng.uniform(0.001, 0.01, N).astype(np.float32), wd_one=rng.uniform(0.001, 0.01, 1).astype(np.float32),
                bias=(rng.standard_normal(N) * 0.1).astype(np.float32), n_bits=n_bits)


def _planes(idx):
    return ((idx >> 8) - 128).astype(np.int8), ((idx & 255) - 128).astype(np.int8)


def _zero_point(p):
    return int(np.clip(np.rint(p['x_zf']), 0, 2 ** p['n_bits'] - 1))


def _numpy_tot(p, by_planes=False):
    """tot of include/tq_hip.h as int64.  float64 matmuls of integers are exact here: every partial sum is an integer below
    65535 * 127 * 16384 < 2^38.  (The one-matmul form lives in tests/_exact_backend.py, shared with the whole-model twin.)"""
    from tests._exact_backend import i16x8_tot
    z = _zero_point(p)
    if by_planes:
        w = torch.from_numpy(p['w']).double()
        rs = p['w'].astype(np.int64).sum(1)
        hi, lo = _planes(p['idx'])
        a_hi = (torch.from_numpy(hi).double() @ w.T).numpy().astype(np.int64)
        a_lo = (torch.from_numpy(lo).double() @ w.T).numpy().astype(np.int64)
        return 256 * a_hi + a_lo + (32896 - z) * rs[None, :]
    return i16x8_tot(p['idx'], p['w'], z)                                 # = 256 A_hi + A_lo + (32896 - z) rowsum


def _numpy_pre(p, tot, per_channel, with_bias):
    from tests._exact_backend import i16x8_pre
    return i16x8_pre(tot, p['x_delta'], EPS, p['wd_row'] if per_channel else p['wd_one'], EPS, p['bias'] if with_bias else None)


def _device(p, per_channel=True, with_bias=True, dev='cuda'):
    from quantization import _hip
    be = _hip.backend()
    hi, lo = _planes(p['idx'])
    w = torch.from_numpy(p['w']).to(dev)
    xq = (torch.tensor([p['x_delta']], device=dev), torch.tensor([p['x_zf']], device=dev), p['n_bits'], EPS)
    wd = torch.from_numpy(p['wd_row'] if per_channel else p['wd_one']).to(dev)
    b = torch.from_numpy(p['bias']).to(dev) if with_bias else None
    return be, torch.from_numpy(hi).to(dev), torch.from_numpy(lo).to(dev), w, be.rowsum_i8(w), b, xq, wd


def _q_out(dev='cuda', lo=-0.2, hi=3.0, n_bits=8):
    top = 2 ** n_bits - 1
    delta = torch.tensor([(hi - lo) / top], dtype=torch.float32, device=dev)
    zf = torch.tensor([-lo / ((hi - lo) / top)], dtype=torch.float32, device=dev)
    return (delta, zf, None, n_bits, False, False, EPS)


def _assert_bits(got, ref):
    got, ref = got.cpu().numpy(), np.ascontiguousarray(ref)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
        f'{np.count_nonzero(got != ref)} of {got.size} outputs differ (max {np.abs(got - ref).max()})'


def test_plane_identity_of_the_restatement():
    """256 A_hi + A_lo + 32896 rowsum == sum_k index w: the one-matmul form of `_numpy_tot` is the formula's"""
    for n_bits in (16, 12, 9, 8):
        p = _problem(64, 64, 128, n_bits, seed=n_bits)
        assert np.array_equal(_numpy_tot(p), _numpy_tot(p, by_planes=True))


@gpu
@pytest.mark.parametrize('shape', [(1024, 3072, 768), (1024, 768, 3072), (64, 64, 128), (16384, 3072, 768)])
@pytest.mark.parametrize('n_bits', [16, 12, 9])
def test_pre_bit_exact_vs_numpy(shape, n_bits):
    """per-tensor and per-channel w_delta x with and without bias x fp32 and bf16 y, on one integer problem per case"""
    from quantization import _hip
    M, N, K = shape
    p = _problem(M, N, K, n_bits, seed=M + N + K + n_bits)
    tot = _numpy_tot(p)
    for per_channel in (False, True):
        for with_bias in (False, True):
            be, hi, lo, w, rs, b, xq, wd = _device(p, per_channel, with_bias)
            ref = _numpy_pre(p, tot, per_channel, with_bias)
            y = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_NONE, None, torch.float32)
            _assert_bits(y, ref)
            yb = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_NONE, None, torch.bfloat16)
            assert torch.equal(yb.cpu(), torch.from_numpy(ref).to(torch.bfloat16)), (per_channel, with_bias)


@gpu
@pytest.mark.parametrize('K', [3072, 16384])
@pytest.mark.parametrize('weights', ['plus', 'minus', 'alternating'])
def test_sums_beyond_32_bits(K, weights):
    """All indices 65535, z_x = 0, weights +-127: |tot| is ~2.5e10 (K = 3072) / ~1.4e11 (K = 16384), which a 32-bit combine
    of the two plane sums gets wrong.  'alternating': +127 and -127 by output feature, both signs in one launch."""
    from quantization import _hip
    M = N = 64
    p = _problem(M, N, K, 16, seed=K)
    p['idx'][:] = 65535
    p['x_zf'] = np.float32(0.0)
    sign = {'plus': np.ones(N), 'minus': -np.ones(N), 'alternating': np.where(np.arange(N) % 2 == 0, 1, -1)}[weights]
    p['w'] = (127 * sign[:, None] * np.ones((1, K))).astype(np.int8)
    tot = _numpy_tot(p)
    assert np.abs(tot).min() > 2 ** 31, 'the case must leave the 32-bit range'
    assert np.array_equal(tot, _numpy_tot(p, by_planes=True))
    for per_channel in (False, True):
        be, hi, lo, w, rs, b, xq, wd = _device(p, per_channel, True)
        y = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_NONE, None, torch.float32)
        _assert_bits(y, _numpy_pre(p, tot, per_channel, True))


@gpu
@pytest.mark.parametrize('shape', [(1024, 3072, 768), (1024, 768, 3072), (64, 64, 128)])
@pytest.mark.parametrize('n_bits', [8, 4])
def test_grids_of_at_most_8_bits_equal_the_8_bit_kernel(shape, n_bits):
    """hi plane constantly -128: tq_linear_i8_stair_fwd on index - 128 bit for bit -- pre, GELU + quantizer with indices,
    index-only and staircase outputs"""
    from quantization import _hip
    M, N, K = shape
    p = _problem(M, N, K, n_bits, seed=M + K + n_bits)
    be, hi, lo, w, rs, b, xq, wd = _device(p)
    assert int(hi.max()) == int(hi.min()) == -128
    a = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_NONE, None, torch.float32)
    r = be.linear_i8(lo, w, rs, b, xq, wd, EPS, _hip.ACT_NONE, None, torch.float32)
    assert torch.equal(a.view(torch.int32), r.view(torch.int32))
    pre = _numpy_pre(p, _numpy_tot(p), True, True)
    q = _q_out(lo=float(np.minimum(pre.min(), -0.17)), hi=float(pre.max()))
    for stair in (False, True):
        t16 = be.act_stair(_hip.ACT_GELU, q, be.i16x8_stair_bins_for(M, N, K)) if stair else None
        t8 = be.act_stair(_hip.ACT_GELU, q, be.stair_bins_for(M, N)) if stair else None
        a_y, a_i = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, stair=t16)
        r_y, r_i = be.linear_i8(lo, w, rs, b, xq, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, stair=t8)
        assert torch.equal(a_i, r_i) and torch.equal(a_y.view(torch.int32), r_y.view(torch.int32)), stair
        _, o_i = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, want_y=False,
                                 stair=t16)
        assert torch.equal(o_i, r_i), stair


def _oracle_epilogue(pre, activation, q):
    """The C oracle's epilogue on given pre-activations (oracle/tq_int_oracle.c: tq_io_epilogue)"""
    from tests._exact_backend import oracle_epilogue
    return oracle_epilogue(pre, activation, q)


def _epilogue_through_a_linear(pre, activation, q):
    """The same epilogue reached through tq_io_linear_i8: a Linear whose integer part is zero (x on its zero point) and
    whose bias is `pre` -- 0.0f * scale + b == b exactly -- in chunks of 65536 outputs."""
    from oracle import int_oracle
    flat = torch.from_numpy(np.ascontiguousarray(pre).reshape(-1))
    x0 = torch.full((1, 64), 3 - 128, dtype=torch.int8)
    w0 = torch.zeros((65536, 64), dtype=torch.int8)
    q7 = None if q is None else (float(q[0]), float(q[1]), None, q[3], q[4], q[5], q[6])
    ys, idxs = [], []
    for s in range(0, flat.numel(), 65536):
        b = flat[s:s + 65536]
        y, yi = int_oracle.linear_i8(x0, w0[:b.numel()], b, (0.1, 3.0, 8, EPS), torch.ones(1), EPS, activation, q7)
        ys.append(y.reshape(-1))
        idxs.append(yi.reshape(-1))
    return torch.cat(ys).reshape(pre.shape), torch.cat(idxs).reshape(pre.shape)


@pytest.mark.parametrize('activation', [0, 1, 2, 4])
def test_exported_epilogue_is_the_integer_linears(activation):
    """tq_io_epilogue == the epilogue inside tq_io_linear_i8, bit for bit, for every activation code the integer Linears
    use, with and without an output quantizer; grid ends and rounding ties included"""
    rng = np.random.default_rng(activation)
    pre = (rng.standard_normal((300, 257)) * 1.7).astype(np.float32)
    pre[0, :6] = [0.0, 1e-30, 40.0, -40.0, 3.2, -0.2]
    q = _q_out(dev='cpu', lo=-0.2, hi=3.2)
    pre[1, :256] = ((np.arange(256) - np.rint(float(q[1])) + 0.5) * float(q[0])).astype(np.float32)     # rounding ties
    for qq in (q, None):
        y, yi = _oracle_epilogue(pre, activation, qq)
        ry, ryi = _epilogue_through_a_linear(pre, activation, qq)
        assert torch.equal(y.view(torch.int32), ry.view(torch.int32))
        if qq is not None:
            assert torch.equal(yi, ryi)


@gpu
@pytest.mark.parametrize('shape', [(1024, 3072, 768), (64, 64, 128)])
@pytest.mark.parametrize('n_bits', [16, 12])
def test_gelu_and_output_quantizer(shape, n_bits):
    from oracle import tq_oracle as O
    from quantization import _hip
    M, N, K = shape
    p = _problem(M, N, K, n_bits, seed=K + n_bits)
    tot = _numpy_tot(p)
    p['x_delta'] = np.float32(1.5 / (tot.std() * p['wd_row'].mean()))       # pre-activations ~ N(0, 1.5^2): GELU's curved part
    pre = _numpy_pre(p, tot, True, True)
    be, hi, lo, w, rs, b, xq, wd = _device(p)
    g = torch.nn.functional.gelu(torch.from_numpy(pre).double()).float()
    q = _q_out(lo=-0.2, hi=3.2)           # a grid the 768-bin table holds (step 0.0133); larger activations saturate it
    bins = be.i16x8_stair_bins_for(M, N, K)
    assert bins in (be.STAIR_BINS, be.STAIR_BINS_BIG)
    tab = be.act_stair(_hip.ACT_GELU, q, bins)
    assert float(tab[0][:16].view(torch.float32)[3]) == 1.0, 'the table must be exact for this grid, or the case is vacuous'
    # staircase: the oracle's correctly rounded GELU + quantizer, zero tolerance
    y_s, i_s = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, stair=tab)
    y_o, i_o = _oracle_epilogue(pre, 4, q)
    assert torch.equal(i_s.cpu(), i_o)
    assert torch.equal(y_s.cpu().view(torch.int32), y_o.view(torch.int32))
    # index-only output == the indices of the full call, with and without the table
    _, i_only = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, want_y=False,
                                stair=tab)
    assert torch.equal(i_only, i_s)
    y_a, i_a = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True)
    _, i_a_only = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, want_y=False)
    assert torch.equal(i_a_only, i_a)
    # arithmetic GELU epilogue: the bar tests/test_linear_i8.py holds activation code 2 to
    _, ref = O.fake_quant(g, q[0].cpu().reshape(()), q[1].cpu().reshape(()), 8, False)
    diff = (y_a.cpu() - ref).abs()
    assert (diff == 0).float().mean().item() >= 0.999, (diff == 0).float().mean().item()
    assert diff.max().item() <= float(q[0]) * 1.001


def _hilo_input(n, delta, zf, n_bits, seed):
    rng = np.random.default_rng(seed)
    top = 2 ** n_bits - 1
    x = (rng.uniform(-0.2, 1.2, n) * top - zf) * delta                       # 20 % beyond either grid end
    k = rng.integers(0, top, n // 4)
    x[:n // 4] = (k + 0.5 - np.rint(zf)) * delta                             # rounding ties of the quotient
    x[n // 4:n // 4 + 7] = [np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, np.nan]
    return x.astype(np.float32)


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('n_bits', [9, 10, 11, 12, 13, 14, 15, 16])
def test_quantize_hilo_equals_fake_quant_indices(dtype, n_bits):
    from quantization import _hip
    be = _hip.backend()
    delta, zf = np.float32(3.1e-4 * 2.0 ** (16 - n_bits)), np.float32(0.37 * (2 ** n_bits - 1))
    for n in (1024 * 768, 4099, 7):                          # whole vectors, a ragged end, less than one group
        x = torch.from_numpy(_hilo_input(max(n, 64), delta, zf, n_bits, seed=n + n_bits))[:n].to(dtype).cuda()
        d, z = torch.tensor([delta], device='cuda'), torch.tensor([zf], device='cuda')
        hi, lo = be.quantize_hilo(x, (d, z, n_bits, EPS))
        _, ref = be.fake_quant(x, d, z, None, n_bits, False, False, EPS, 1, 1, want_y=False, idx_dtype=torch.int32)
        assert hi.dtype == lo.dtype == torch.int8 and hi.shape == lo.shape == x.shape
        got = 256 * (hi.int() + 128) + (lo.int() + 128)
        assert torch.equal(got, ref), (n, int((got != ref).sum()))
        if n >= 4096:
            assert int(ref.min()) == 0 and int(ref.max()) == 2 ** n_bits - 1              # both grid ends are reached
    # a view that is not 16-byte aligned takes the element-wise kernel
    buf = x.new_zeros(4100)
    buf += 0.01
    xs = buf[1:]
    assert xs.data_ptr() % 16 != 0
    hi, lo = be.quantize_hilo(xs, (d, z, n_bits, EPS))
    _, ref = be.fake_quant(xs, d, z, None, n_bits, False, False, EPS, 1, 1, want_y=False, idx_dtype=torch.int32)
    assert torch.equal(256 * (hi.int() + 128) + (lo.int() + 128), ref)


def _simulation(p):
    z = np.float32(_zero_point(p))
    xq_f = torch.from_numpy(((p['idx'].astype(np.float32) - z) * p['x_delta']).astype(np.float32))
    wq_f = torch.from_numpy((p['w'].astype(np.float32) * p['wd_row'].reshape(-1, 1)).astype(np.float32))
    sim = torch.nn.functional.linear(xq_f, wq_f, torch.from_numpy(p['bias']))
    scale = (xq_f.abs() @ wq_f.abs().T).amax(1, keepdim=True) + 1e-12
    return sim, scale


SIM_CASES = [((1024, 3072, 768), 16), ((1024, 768, 3072), 16), ((1024, 3072, 768), 12), ((4096, 3072, 768), 9)]


@pytest.mark.parametrize('shape,n_bits', SIM_CASES)
def test_numpy_restatement_meets_the_fp32_simulation_bar(shape, n_bits):
    """The bar of tests/test_linear_i8_peg.py::test_pre_quantizer_output_vs_fp32_simulation (1e-5 of the row scale), for the
    restatement alone and the seeds of the GPU test below: what the kernel is then held to bit for bit can meet it."""
    M, N, K = shape
    p = _problem(M, N, K, n_bits, seed=3 + n_bits)
    pre = torch.from_numpy(_numpy_pre(p, _numpy_tot(p), True, True))
    sim, scale = _simulation(p)
    err = float(((pre - sim).abs() / scale).max())
    print('restatement vs fp32 simulation: %.3e of the row scale' % err)
    assert err <= 1e-5


@gpu
@pytest.mark.parametrize('shape,n_bits', SIM_CASES)
def test_pre_vs_fp32_simulation(shape, n_bits):
    from quantization import _hip
    M, N, K = shape
    p = _problem(M, N, K, n_bits, seed=3 + n_bits)
    be, hi, lo, w, rs, b, xq, wd = _device(p)
    y = be.linear_i16x8(hi, lo, w, rs, b, xq, wd, EPS, _hip.ACT_NONE, None, torch.float32).cpu()
    sim, scale = _simulation(p)
    err = float(((y - sim).abs() / scale).max())
    print('kernel vs fp32 simulation: %.3e of the row scale' % err)
    assert err <= 1e-5


def test_argument_errors_without_gpu():
    """Bad shapes, a NULL plane and x_n_bits = 17 come back as TQ_EINVAL with a message before any HIP call (the pointers
    below are never dereferenced)."""
    from quantization import _hip
    lib = _hip.load_library()
    P = 0x10000                                               # any non-NULL 16-byte aligned address
    err = lambda: lib.tq_last_error().decode()

    def lin(**kw):
        return lib.tq_linear_i16x8_fwd(kw.get('hi', P), kw.get('lo', P), P, P, None, kw.get('y', P), None, 0, kw.get('M', 64),
                                       kw.get('N', 64), kw.get('K', 128), P, P, kw.get('bits', 16), EPS, P, kw.get('wn', 64), EPS,
                                       kw.get('act', 0), None, kw.get('stair', None), kw.get('nb', 0), None)
    assert lin(M=0) == 0                                       # empty problem: no-op
    for bad in (dict(M=96), dict(M=32), dict(N=96), dict(K=64), dict(K=192), dict(K=16384 + 128)):
        assert lin(**bad) == -1 and 'unsupported shape' in err() and 'tq_linear_i16x8_fwd' in err(), bad
    assert lin(lo=None) == -1 and 'NULL' in err()
    assert lin(hi=None) == -1 and 'NULL' in err()
    assert lin(y=None) == -1 and 'NULL' in err()              # neither y nor y_idx
    assert lin(bits=17) == -1 and '16 bits' in err()
    assert lin(bits=0) == -1 and '16 bits' in err()
    assert lin(lo=P + 4) == -1 and 'alignment' in err()
    assert lin(wn=7) == -1 and 'weight scales' in err()
    assert lin(act=9) == -1 and 'activation' in err()
    assert lin(stair=P, nb=768) == -1 and 'staircase' in err()            # a table needs an output quantizer
    q = _hip.tq_quantizer(P, P, None, 16, 0, 0, EPS, 1, 1)
    hilo = lambda **kw: lib.tq_quantize_hilo_fwd(kw.get('x', P), kw.get('hi', P), kw.get('lo', P), kw.get('n', 64), kw.get('dt', 0),
                                                 kw.get('q', C.byref(q)), None)
    assert hilo(n=0) == 0
    assert hilo(x=None) == -1 and 'NULL' in err()
    assert hilo(lo=None) == -1 and 'NULL' in err()
    assert hilo(dt=7) == -1 and 'dtype' in err()
    q17 = _hip.tq_quantizer(P, P, None, 17, 0, 0, EPS, 1, 1)
    assert hilo(q=C.byref(q17)) == -1 and '16 bits' in err()
    qsym = _hip.tq_quantizer(P, None, P, 16, 1, 0, EPS, 1, 1)
    assert hilo(q=C.byref(qsym)) == -1 and 'asymmetric' in err()
    # the table-size query: no device either
    assert lib.tq_linear_i16x8_stair_bins(1024, 3072, 768) == 768 == lib.tq_linear_i16x8_stair_bins(16384, 3072, 768)
