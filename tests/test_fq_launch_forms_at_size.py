"""The fake-quant forward's at-size launch forms against the CPU oracle, over the whole tensor, bit for bit.

`launch_fq` (csrc/tq_fake_quant.hip) picks its kernel form by size: U = 4 (or U = 2 on 1024-lane blocks) vectors per
lane once the tensor has 2 097 152 vectors (`big`), streaming loads / stores from 64 MiB (`nt`), several consecutive
tiles per block (`tpb`) from a few thousand tiles, and two tiles per block for 16-bit index-only launches that are both.
The tuning variables of these forms are read once per process, so a test reaches a form by SIZE only: every case below
uses the smallest size that reaches its form, asserts that premise with `launch_form` -- a restatement of the
launcher's arithmetic -- before it runs, and then compares EVERY element of every output with
`oracle.tq_oracle.fake_quant_lowp` evaluated on the CPU (in row chunks).  If a threshold moves, the premise fails
first and says which size has to be re-picked.

Inputs are seeded `randn * 3` (per-embedding: times a per-column ramp 0.5 .. 4, two columns 20-fold), with NaN, +-inf
and values one ulp either side of a rounding tie planted in the first tile, in the LAST vector slot of a lane in a middle
tile, at both ends of the ragged last tile and -- per-tensor -- in the tail of fewer than V elements.  A NaN has no
integer index; the kernels' integer outputs hold 0 there (tests/test_hip_parity.py::
test_byte_index_outputs_equal_the_float_indices), and so does the reference used here.

Cases (n_vec = 16-byte vectors; "ragged" = vectors in the last tile, "partial" = tiles in the last block):

  per tensor (fq_tensor), n = n_vec * V + r
   1  fp32          n_vec 2 097 152 + 5 420   U=4            y + int32   (+ symmetric signed 4-bit, + 16-bit grid)
   2  fp32          n_vec 4 194 304 + 3 772   U=4 streaming  y + uint8, uint8 alone
   3  bf16, fp16    n_vec 2 097 152 + 5 420   U=4            y + int32
   4  bf16          n_vec 4 194 304 + 3 772   U=4 streaming  y + int8(index - 128)
   5  bf16, fp16    n_vec 4 194 304 + 2 348   U=4 streaming, two tiles per block, 4099 tiles (last block: one ragged tile)
                    n_vec 4 194 304 + 1 324   the same, 4098 tiles (the ragged tile is the second of its pair)
                                              uint8 alone, int8(index - 128) alone
  per embedding (n_params = d, inner = 1), x = [rows, d]
   6  fq_axis_reg fp32 d=768   rows 10 925  bs=192 U=4             y + int32   (+ symmetric signed 4-bit, + 16-bit grid)
                               rows 21 849  streaming; y + uint8: tpb=1; uint8 alone: tpb=2, 5463 tiles
   7  fq_axis_reg fp32 d=3072  rows 2 733   bs=768 (1024-lane form) U=2;  rows 5 463: streaming
   8  fq_axis_reg bf16 + y     d=3072: rows 5 463 (bs=384, U=2), rows 10 925 (streaming, tpb=2, 5463 tiles)
                               d=768:  rows 21 849 (bs=192, U=4), rows 65 573 (streaming, tpb=4, 8197 tiles, ~100 MB)
   9  fq_axis bf16 index-only  d=768: rows 21 849 (U=4, tpb=1; + symmetric signed 4-bit, + 16-bit grid),
                               rows 43 713 (streaming, tpb=2, 4099 tiles)
  10  the width rule at 37 rows: fp32 d=4096 (last register width), 4100 and 5440 (LDS table), 5444 (fq_scalar);
      bf16 d=5440 (registers with y, LDS table index-only) and 5448 (registers)
  11  quantize_hilo, bf16, 67 108 864 + 4 805 elements: the second trip of its capped grid-stride loop

Where a case has an output, the launch WITHOUT an index output (a template instantiation of its own) is compared too.
Cases 1, 5, 6 and 9 also run through the C entry point into buffers 4096 elements longer than n, pre-filled with a
sentinel: an overrun of a ragged tile would land in the caching allocator's rounding otherwise.

Measured once on an MI355X box (pytest --durations=0 within the whole GPU suite; seconds of the slowest case of each
test function, input generation and CPU reference included; the 32 cases together take under 6 s):
  test_fq_tensor_fp32_four_vectors_per_lane                     0.18    (case 1)
  test_fq_tensor_fp32_streaming                                 0.13    (case 2)
  test_fq_tensor_16bit_four_vectors_per_lane                    0.12    (case 3)
  test_fq_tensor_bf16_streaming_with_int8_operand               0.22    (case 4)
  test_fq_tensor_16bit_index_only_two_tiles_per_block           0.29    (case 5)
  test_fq_axis_reg_fp32_d768_four_vectors_per_lane              0.08    (case 6)
  test_fq_axis_reg_fp32_d768_streaming_and_two_tiles_per_block  0.11    (case 6)
  test_fq_axis_reg_fp32_d3072_1024_lane_blocks                  0.12    (case 7)
  test_fq_axis_reg_bf16_with_output                             0.48    (case 8; the ~100 MB tpb = 4 case, whole tensor)
  test_fq_axis_bf16_index_only_four_vectors_per_lane            0.13    (case 9)
  test_fq_axis_bf16_index_only_two_tiles_per_block              0.25    (case 9)
  test_width_rule_edges                                         0.02    (case 10)
  test_quantize_hilo_second_grid_stride_trip                    0.26    (case 11)
No case stands out, so none is reduced to slabs.
"""
import collections
import ctypes as C

import pytest
import torch

from oracle import tq_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-8

# ------------------------------------------------------------------------------------------------------------------
# launch_fq's arithmetic, restated.  Mirrors csrc/tq_fake_quant.hip, `launch_fq`:
#   nt / big                         the lines `const bool nt = ...` and `const bool big = ...`
#   per tensor                       TQ_LAUNCH_TENSOR and the `HAS_IDX && DT != TQ_F32 && y == nullptr && big && nt` branch
#   lds_ok / reg_ok / prefer_reg     the three lines of those names
#   fq_axis_reg: bs, U, rule, tpb    `const uint32_t bs = ...`, TQ_LAUNCH_AXIS_REG and its `if (bs <= kBlock)` ladder
#   fq_axis: U, want, tpb            TQ_LAUNCH_AXIS
# (kBlock: csrc/tq_device.h; 16-byte alignment of every pointer and the default tuning variables are assumed.)
# ------------------------------------------------------------------------------------------------------------------
K_BLOCK = 256
BIG_MIN_VECS = K_BLOCK * 4 * 2048            # 2 097 152
NT_MIN_BYTES = 64 << 20
LDS_MAX_COLS = 5440
REG_MAX_VPR = 1024

Form = collections.namedtuple('Form', 'kernel V n_vec tail big nt bs U tile n_tiles tpb ragged partial')


def _ceil_div(a, b):
    return -(-a // b)


def launch_form(n, dtype, d=1, want_y=True, want_idx=True):
    """The form `launch_fq` gives a contiguous tensor of n elements with n_params = d, inner = 1."""
    fp32 = dtype == torch.float32
    V = 4 if fp32 else 8
    n_vec = n // V
    big = n_vec >= BIG_MIN_VECS
    nt = n * (4 if fp32 else 2) >= NT_MIN_BYTES

    def form(kernel, bs, U, tpb, tail=0):
        tile = bs * U
        n_tiles = max(_ceil_div(n_vec, tile), 1)
        if callable(tpb):
            tpb = tpb(n_tiles)
        return Form(kernel, V, n_vec, tail, big, nt, bs, U, tile, n_tiles, tpb, n_vec % tile, n_tiles % tpb)

    if d == 1:
        two = want_idx and not fp32 and not want_y and big and nt
        return form('fq_tensor', K_BLOCK, 4 if big else 1, 2 if two else 1, tail=n % V)
    lds_ok = d % V == 0 and d <= LDS_MAX_COLS
    reg_ok = d % V == 0 and d // V <= REG_MAX_VPR
    prefer_reg = fp32 or (want_y and (d >= 2048 or big))
    if reg_ok and (prefer_reg or not lds_ok):
        vpr = d // V
        bs = vpr * (K_BLOCK // vpr) if vpr <= K_BLOCK else vpr
        U = (4 if big else 1) if bs <= K_BLOCK else (2 if big else 1)
        rule = (4 if fp32 else 16) // U * (1 if want_y else 2)
        return form('fq_axis_reg', bs, U, lambda n_tiles: max(min(rule, n_tiles // 2048), 1))
    if lds_ok:
        want = 8 if d > 2048 else (4 if d > 1024 else 2)
        return form('fq_axis', K_BLOCK, 4 if big else 1,
                    lambda n_tiles: want if n_tiles >= 2048 * want else (2 if n_tiles >= 4096 else 1))
    # fq_scalar: one element per lane, grid-stride; described as tiles of one block for the planted positions
    return Form('fq_scalar', 1, n, 0, big, False, K_BLOCK, 1, K_BLOCK, max(_ceil_div(n, K_BLOCK), 1), 1, n % K_BLOCK, 0)


def _premise(form, **want):
    """The case's size still reaches the form it was picked for."""
    got = {k: getattr(form, k) for k in want}
    assert got == want, ('launch_fq no longer gives this size the form the case was picked for: re-pick the size with '
                         'launch_form()', want, form)


# ------------------------------------------------------------------------------------------------------------------
# quantizers, inputs, reference
# ------------------------------------------------------------------------------------------------------------------
Quant = collections.namedtuple('Quant', 'delta zf signed n_bits symmetric sgn')
GRIDS = {'asym8': (8, False), 'sym4': (4, True), 'asym16': (16, False)}
IDX_DTYPE = {None: None, 'i32': torch.int32, 'u8': torch.uint8, 'i8': torch.int8}


def _col_scale(d):
    """Standard deviation of every column of the per-embedding inputs: 3 x ramp, two columns 20-fold."""
    s = 3.0 * torch.linspace(0.5, 4, d)
    s[2 * d // 5 + 1] *= 20
    s[d // 2 - 3] *= 20
    return s


def _quantizer(grid, d):
    """Per tensor (d == 1): the range [-7, 9] (16 bits: [-9, 9]) under inputs of deviation 3; per embedding: column c
    gets [-2.5, 3.5] deviations of ITS inputs, so every column has its own scale and zero point and clips at both ends."""
    n_bits, symmetric = GRIDS[grid]
    if d == 1:
        lo, hi = (-9.0, 9.0) if n_bits == 16 else (-7.0, 9.0)
    else:
        s = _col_scale(d)
        lo, hi = -2.5 * s, 3.5 * s
    if symmetric:
        delta, signed = O.sym_params_from_range(lo, hi, n_bits)
        assert bool(signed)
        return Quant(delta, None, signed, n_bits, True, True)
    delta, zf = O.asym_params_from_range(lo, hi, n_bits)
    return Quant(delta, zf, None, n_bits, False, False)


def _ulp(v, up):
    """The neighbour of a positive finite value in its own format."""
    if v.dtype == torch.float32:
        return torch.nextafter(v, torch.tensor(float('inf') if up else 0.0))
    return (v.view(torch.int16) + (1 if up else -1)).view(v.dtype)


def _plant(x, form, q, d):
    """NaN, +-inf and tie-adjacent values at the places a launch form can go wrong (flat element positions)."""
    n, V = x.numel(), form.V
    last_tile = (form.n_tiles - 1) * form.tile
    at = [(5 * V, 8),                                                                       # first tile
          (((form.n_tiles // 2) * form.tile + 37 + (form.U - 1) * form.bs) * V, 8),       # last slot of a lane, middle tile
          (last_tile * V, 8),                                                               # ragged last tile: first lane ...
          ((form.n_vec - 1) * V, V)]                                                        # ... and its last vector
    if form.tail:
        at.append((form.n_vec * V, form.tail))                                              # elements after the last vector
    scale = torch.clamp(q.delta.reshape(-1), min=EPS)
    for e0, count in at:
        for j in range(min(count, n - e0)):
            e = e0 + j
            tie = ((1 + e % 5 + 0.5) * scale[e % d].double()).float().to(x.dtype)
            x[e] = [_ulp(tie, False), torch.tensor(float('nan')), _ulp(tie, True), torch.tensor(float('inf')),
                    torch.tensor(-float('inf')), tie, -_ulp(tie, True), -_ulp(tie, False)][j % 8]


def _oracle(x, q, per_column, chunk=1 << 22):
    """(int32 indices, dequantised values) of the whole tensor from oracle.tq_oracle.fake_quant_lowp, in chunks of rows."""
    ref_idx = torch.empty(x.shape, dtype=torch.int32)
    ref_y = torch.empty_like(x)
    step = max(chunk // (x.shape[1] if x.dim() == 2 else 1), 1)
    for r0 in range(0, x.shape[0], step):
        xi, y = O.fake_quant_lowp(x[r0:r0 + step], q.delta, q.zf, q.n_bits, q.symmetric, q.sgn,
                                  axis=1 if per_column else None)
        ref_idx[r0:r0 + step] = torch.nan_to_num(xi, nan=0.0).to(torch.int32)
        ref_y[r0:r0 + step] = y
    return ref_idx, ref_y


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16) if t.is_floating_point() else t


def _assert_same(got, ref, form, d, what):
    """Every element equal (floats: bit patterns; a NaN equals a NaN), with the launch coordinates of the first miss."""
    got, ref = got.reshape(-1), ref.reshape(-1)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = _bits(got) != _bits(ref)
    if got.is_floating_point():
        bad &= ~(torch.isnan(got) & torch.isnan(ref))
    n_bad = int(bad.sum())
    if n_bad:
        e = int(torch.argmax(bad.to(torch.uint8)))
        v = e // form.V
        where = dict(element=e, column=e % d, vector=v, tile=v // form.tile, of_tiles=form.n_tiles,
                     slot=(v % form.tile) // form.bs, lane=(v % form.tile) % form.bs,
                     in_tail=v >= form.n_vec, got=got[e].item(), want=ref[e].item())
        raise AssertionError('%s: %d of %d elements differ from the oracle; first: %r; %r' % (what, n_bad, got.numel(), where, form))


class _Case:
    """One input tensor, its quantizer and its whole-tensor reference; `check` runs one launch form against it."""

    def __init__(self, dtype, grid='asym8', n=None, rows=None, d=1, plant_for_y=True):
        self.dtype, self.d, self.q = dtype, d, _quantizer(grid, d)
        g = torch.Generator().manual_seed(1000 + (n if d == 1 else rows + d))
        if d == 1:
            x = torch.randn(n, generator=g).mul_(3)
        else:
            x = torch.randn(rows, d, generator=g).mul_(_col_scale(d))
        x = x.to(dtype)
        _plant(x.view(-1), launch_form(x.numel(), dtype, d, want_y=plant_for_y), self.q, d)
        self.x = x
        self.xd = x.to(DEV)
        ref_idx, ref_y = _oracle(x, self.q, d > 1)
        self.ref_idx, self.ref_y = ref_idx.to(DEV), ref_y.to(DEV)
        q = self.q
        self.qargs = (q.delta.to(DEV), None if q.zf is None else q.zf.to(DEV), None if q.signed is None else q.signed.to(DEV),
                      q.n_bits, q.symmetric, False, EPS)

    def form(self, want_y):
        return launch_form(self.x.numel(), self.dtype, self.d, want_y=want_y)

    def check(self, be, want_y, idx_kind, **premise):
        """One launch: y (if asked for) and the indices as int32 / uint8 / int8, as int8(index - 128) ('m128'), or none."""
        form = launch_form(self.x.numel(), self.dtype, self.d, want_y=want_y, want_idx=idx_kind is not None)
        _premise(form, **premise)
        if idx_kind == 'm128' and want_y:
            y, idx = be.fake_quant_int8(self.xd, self.qargs[0], self.qargs[1], self.q.n_bits, EPS)
        elif idx_kind == 'm128':
            y, idx = None, be.quantize_to_int8(self.xd, *self.qargs, self.d, 1, True)
        else:
            y, idx = be.fake_quant(self.xd, *self.qargs, self.d, 1, want_y=want_y, idx_dtype=IDX_DTYPE[idx_kind])
        torch.cuda.synchronize()
        what = '%s %s d=%d %s%s' % (form.kernel, self.dtype, self.d, 'y + ' if want_y else '', idx_kind)
        assert (y is not None) == want_y and (idx is not None) == (idx_kind is not None)
        if want_y:
            _assert_same(y, self.ref_y, form, self.d, what + ': y')
        if idx is not None:
            _assert_same(idx.to(torch.int32) + (128 if idx_kind == 'm128' else 0), self.ref_idx, form, self.d, what + ': indices')
        return y, idx

    def check_no_overrun(self, be, want_y, idx_kind, y, idx, pad=4096):
        """The same launch through the C entry point into buffers this test owns, `pad` elements longer than n and
        pre-filled with a sentinel: the first n elements are `check`'s outputs, the pad is untouched."""
        from quantization import _hip
        n = self.x.numel()
        code, idt = (_hip.IDX_I8_M128, torch.int8) if idx_kind == 'm128' else (_hip._IDX_DTYPES[IDX_DTYPE[idx_kind]], IDX_DTYPE[idx_kind])
        y2 = torch.full((n + pad,), -1.5, dtype=self.dtype, device=DEV) if want_y else None
        idx2 = torch.full((n + pad,), 90, dtype=idt, device=DEV)
        q = be._qdesc(*self.qargs, self.d, 1)
        rc = be.lib.tq_fake_quant_fwd(_hip._ptr(self.xd), _hip._ptr(y2), _hip._ptr(idx2), code, n,
                                      _hip._dtype_code(self.xd, 'fake_quant'), C.byref(q), _hip._stream())
        _hip._check(rc, be.lib)
        torch.cuda.synchronize()
        form = self.form(want_y)
        if want_y:
            _assert_same(y2[:n], y.reshape(-1), form, self.d, 'own buffers: y')
            assert bool((y2[n:] == -1.5).all()), ('y written past n', int((y2[n:] != -1.5).sum()), form)
        _assert_same(idx2[:n], idx.reshape(-1), form, self.d, 'own buffers: indices')
        assert bool((idx2[n:] == 90).all()), ('indices written past n', int((idx2[n:] != 90).sum()), form)


@pytest.fixture(scope='module')
def be():
    from quantization import _hip
    b = _hip.backend()
    assert b.name == 'hip'
    yield b
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------
# per tensor
# ------------------------------------------------------------------------------------------------------------------
N_VEC_BIG = BIG_MIN_VECS + 5 * 1024 + 300                 # 2053 full tiles of 1024 vectors + 300
N_VEC_STREAM = 2 * BIG_MIN_VECS + 3 * 1024 + 700


@pytest.mark.parametrize('grid', ['asym8', 'sym4', 'asym16'])
def test_fq_tensor_fp32_four_vectors_per_lane(be, grid):
    """Case 1: fp32, U = 4, ordinary loads and stores; ragged last tile, tail of 3 elements."""
    c = _Case(torch.float32, grid, n=N_VEC_BIG * 4 + 3)
    form = dict(kernel='fq_tensor', U=4, nt=False, tpb=1, n_tiles=2054, ragged=300, tail=3)
    y, idx = c.check(be, True, 'i32', **form)
    if grid == 'asym8':
        c.check_no_overrun(be, True, 'i32', y, idx)
        c.check(be, True, None, **form)
    if grid == 'sym4':
        c.check(be, False, 'i8', **form)


def test_fq_tensor_fp32_streaming(be):
    """Case 2: fp32, U = 4 with streaming loads and stores; with y and index-only (fp32 keeps one tile per block)."""
    c = _Case(torch.float32, n=N_VEC_STREAM * 4 + 3)
    form = dict(kernel='fq_tensor', U=4, nt=True, tpb=1, n_tiles=4100, ragged=700, tail=3)
    c.check(be, True, 'u8', **form)
    c.check(be, True, None, **form)
    c.check(be, False, 'u8', **form)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
def test_fq_tensor_16bit_four_vectors_per_lane(be, dtype):
    """Case 3: 16-bit storage, U = 4, ordinary loads and stores, with y."""
    c = _Case(dtype, n=N_VEC_BIG * 8 + 5)
    form = dict(kernel='fq_tensor', U=4, nt=False, tpb=1, n_tiles=2054, ragged=300, tail=5)
    c.check(be, True, 'i32', **form)
    c.check(be, True, None, **form)


def test_fq_tensor_bf16_streaming_with_int8_operand(be):
    """Case 4: bf16, U = 4, streaming, y and int8(index - 128) from one launch (fake_quant_int8)."""
    c = _Case(torch.bfloat16, n=N_VEC_STREAM * 8 + 5)
    form = dict(kernel='fq_tensor', U=4, nt=True, tpb=1, n_tiles=4100, ragged=700, tail=5)
    c.check(be, True, 'm128', **form)
    c.check(be, True, None, **form)             # output only: the instantiation without an index store


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'fp16'])
@pytest.mark.parametrize('n_vec,n_tiles,partial', [(2 * BIG_MIN_VECS + 2 * 1024 + 300, 4099, 1),
                                                   (2 * BIG_MIN_VECS + 1024 + 300, 4098, 0)],
                         ids=['last-block-one-ragged-tile', 'ragged-tile-second-of-its-pair'])
def test_fq_tensor_16bit_index_only_two_tiles_per_block(be, dtype, n_vec, n_tiles, partial):
    """Case 5: the TPB = 2 form (16-bit, index-only, big and streaming)."""
    c = _Case(dtype, n=n_vec * 8 + 7, plant_for_y=False)
    form = dict(kernel='fq_tensor', U=4, nt=True, tpb=2, n_tiles=n_tiles, partial=partial, ragged=300, tail=7)
    _, idx = c.check(be, False, 'u8', **form)
    c.check_no_overrun(be, False, 'u8', None, idx)
    _, idx = c.check(be, False, 'm128', **form)
    c.check_no_overrun(be, False, 'm128', None, idx)


# ------------------------------------------------------------------------------------------------------------------
# per embedding: register-resident parameters
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', ['asym8', 'sym4', 'asym16'])
def test_fq_axis_reg_fp32_d768_four_vectors_per_lane(be, grid):
    """Case 6, rows = 10925: 192-lane blocks, U = 4, one tile per block, the last tile holds 192 of 768 vectors."""
    c = _Case(torch.float32, grid, rows=10925, d=768)
    form = dict(kernel='fq_axis_reg', bs=192, U=4, nt=False, tpb=1, n_tiles=2732, ragged=192)
    y, idx = c.check(be, True, 'i32', **form)
    if grid == 'asym8':
        c.check_no_overrun(be, True, 'i32', y, idx)
    if grid == 'sym4':
        c.check(be, False, 'i8', **form)


def test_fq_axis_reg_fp32_d768_streaming_and_two_tiles_per_block(be):
    """Case 6, rows = 21849: streaming; with y one tile per block, index-only two (5463 tiles: the last block holds one)."""
    c = _Case(torch.float32, rows=21849, d=768)
    form = dict(kernel='fq_axis_reg', bs=192, U=4, nt=True, n_tiles=5463, ragged=192)
    c.check(be, True, 'u8', tpb=1, **form)
    _, idx = c.check(be, False, 'u8', tpb=2, partial=1, **form)
    c.check_no_overrun(be, False, 'u8', None, idx)


@pytest.mark.parametrize('rows,nt,n_tiles', [(2733, False, 1367), (5463, True, 2732)], ids=['2733', '5463-streaming'])
def test_fq_axis_reg_fp32_d3072_1024_lane_blocks(be, rows, nt, n_tiles):
    """Case 7: rows of 768 vectors -> 768-lane blocks (the 1024-lane form), U = 2, half a tile at the end."""
    c = _Case(torch.float32, rows=rows, d=3072)
    form = dict(kernel='fq_axis_reg', bs=768, U=2, nt=nt, tpb=1, n_tiles=n_tiles, ragged=768)
    c.check(be, True, 'i32', **form)
    c.check(be, True, None, **form)


@pytest.mark.parametrize('d,rows,form', [
    (3072, 5463, dict(bs=384, U=2, nt=False, tpb=1, n_tiles=2732, ragged=384, partial=0)),
    (3072, 10925, dict(bs=384, U=2, nt=True, tpb=2, n_tiles=5463, ragged=384, partial=1)),
    (768, 21849, dict(bs=192, U=4, nt=False, tpb=1, n_tiles=2732, ragged=96, partial=0)),
    (768, 65573, dict(bs=192, U=4, nt=True, tpb=4, n_tiles=8197, ragged=480, partial=1)),
], ids=['d3072-U2', 'd3072-U2-streaming-tpb2', 'd768-U4', 'd768-U4-streaming-tpb4'])
def test_fq_axis_reg_bf16_with_output(be, d, rows, form):
    """Case 8: bf16 with y takes the register form on wide rows and on big launches; tpb of 2 and of 4 (whole tensor
    against the oracle in every case, the ~100 MB one included)."""
    c = _Case(torch.bfloat16, rows=rows, d=d)
    c.check(be, True, 'u8', kernel='fq_axis_reg', **form)
    c.check(be, True, None, kernel='fq_axis_reg', **form)


# ------------------------------------------------------------------------------------------------------------------
# per embedding: LDS table
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid,idx_kind', [('asym8', 'u8'), ('sym4', 'i8'), ('asym16', 'i32')])
def test_fq_axis_bf16_index_only_four_vectors_per_lane(be, grid, idx_kind):
    """Case 9, rows = 21849: TILE = 1024 vectors over rows of 96 (the column bookkeeping cv / tile_mod / blk_mod)."""
    c = _Case(torch.bfloat16, grid, rows=21849, d=768, plant_for_y=False)
    _, idx = c.check(be, False, idx_kind, kernel='fq_axis', U=4, nt=False, tpb=1, n_tiles=2049, ragged=352)
    if grid == 'asym8':
        c.check_no_overrun(be, False, 'u8', None, idx)


def test_fq_axis_bf16_index_only_two_tiles_per_block(be):
    """Case 9, rows = 43713: 4099 tiles -> two per block, streaming; the last block holds one ragged tile."""
    c = _Case(torch.bfloat16, rows=43713, d=768, plant_for_y=False)
    form = dict(kernel='fq_axis', U=4, nt=True, tpb=2, n_tiles=4099, partial=1, ragged=96)
    _, idx = c.check(be, False, 'u8', **form)
    c.check_no_overrun(be, False, 'u8', None, idx)
    c.check(be, False, 'm128', **form)


@pytest.mark.parametrize('dtype,d,with_y,index_only', [
    (torch.float32, 4096, dict(kernel='fq_axis_reg', bs=1024, U=1), dict(kernel='fq_axis_reg', bs=1024, U=1)),
    (torch.float32, 4100, dict(kernel='fq_axis', U=1, ragged=37 * 1025 % 256), dict(kernel='fq_axis', U=1)),
    (torch.float32, 5440, dict(kernel='fq_axis', U=1, ragged=37 * 1360 % 256), dict(kernel='fq_axis', U=1)),
    (torch.float32, 5444, dict(kernel='fq_scalar'), dict(kernel='fq_scalar')),
    (torch.bfloat16, 5440, dict(kernel='fq_axis_reg', bs=680, U=1), dict(kernel='fq_axis', U=1, ragged=37 * 680 % 256)),
    (torch.bfloat16, 5448, dict(kernel='fq_axis_reg', bs=681, U=1), dict(kernel='fq_axis_reg', bs=681, U=1)),
], ids=['fp32-4096', 'fp32-4100', 'fp32-5440', 'fp32-5444', 'bf16-5440', 'bf16-5448'])
def test_width_rule_edges(be, dtype, d, with_y, index_only):
    """Case 10: the widths at which the launcher changes kernel, at 37 rows."""
    c = _Case(dtype, rows=37, d=d)
    c.check(be, True, 'i32', nt=False, tpb=1, **with_y)
    c.check(be, False, 'i32', nt=False, tpb=1, **index_only)


# ------------------------------------------------------------------------------------------------------------------
# quantize_hilo past its grid cap
# ------------------------------------------------------------------------------------------------------------------
def test_quantize_hilo_second_grid_stride_trip(be):
    """Case 11.  quantize_hilo_k (csrc/tq_quantize_hilo.hip, launch_hilo) runs at most kMaxGrid * 8 = 16384 blocks of 256
    lanes, 16 elements per lane: beyond 67 108 864 elements a lane makes a second trip.  256 (hi + 128) + (lo + 128) equals
    the int32 indices of the index-only fake-quant launch over the whole tensor (case 5 holds that launch to the oracle),
    and three slabs equal the oracle directly."""
    cap = 16384 * K_BLOCK * 16
    n = cap + 16 * 300 + 5
    assert min(max(_ceil_div(_ceil_div(n, 16), K_BLOCK), 1), 2048 * 8) * K_BLOCK < n // 16 and n % 16, \
        'quantize_hilo_k no longer makes a second trip at this size: re-pick it'
    _premise(launch_form(n, torch.bfloat16, want_y=False), kernel='fq_tensor', U=4, nt=True, tpb=2)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, generator=g).mul_(3).to(torch.bfloat16)
    slabs = [0, cap - 32768, n - 65536]
    for s in slabs:
        x[s + 32768 - 3:s + 32768 + 3] = torch.tensor([float('nan'), float('inf'), -float('inf'), 0.0, -0.0, float('nan')]).to(x.dtype)
    x[n - 3:] = torch.tensor([float('inf'), float('nan'), -1.0]).to(x.dtype)
    delta, zf = O.asym_params_from_range(-9.0, 9.0, 16)
    xd, dd, zd = x.to(DEV), delta.to(DEV), zf.to(DEV)
    hi, lo = be.quantize_hilo(xd, (dd, zd, 16, EPS))
    _, idx = be.fake_quant(xd, dd, zd, None, 16, False, False, EPS, 1, 1, want_y=False, idx_dtype=torch.int32)
    torch.cuda.synchronize()
    assert hi.dtype == torch.int8 and lo.dtype == torch.int8
    step = 1 << 24
    for s in range(0, n, step):
        joined = (hi[s:s + step].to(torch.int32) + 128) * 256 + (lo[s:s + step].to(torch.int32) + 128)
        bad = joined != idx[s:s + step]
        assert not bool(bad.any()), ('hi / lo planes differ from the fake-quant indices', s + int(torch.argmax(bad.to(torch.uint8))),
                                     int(bad.sum()))
    for s in slabs:
        ref_idx, _ = O.fake_quant_lowp(x[s:s + 65536], delta, zf, 16, False)
        ref = torch.nan_to_num(ref_idx, nan=0.0).to(torch.int32)
        got = ((hi[s:s + 65536].to(torch.int32) + 128) * 256 + (lo[s:s + 65536].to(torch.int32) + 128)).cpu()
        assert torch.equal(got, ref), ('slab at %d differs from the oracle' % s, int((got != ref).sum()))
