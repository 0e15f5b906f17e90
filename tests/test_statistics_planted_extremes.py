"""The min / max statistics kernels with planted extremes at every edge of their launch forms, bit for bit.

Every other statistics test feeds `randn` data: a reduction that skips part of its input still gets the right answer
unless the one extreme element sits in the skipped part.  Here the data is uniform in [-1, 1] (rounded to the storage
dtype, no zeros: the sign of a +-0 tie is unspecified), one value is PLANTED at one position, the kernel runs, the base
value is put back.  The statistic of the planted tensor is known by construction -- min(base min, planted), max(base
max, planted), the base's own amin / amax computed once on the CPU on the fp32 upcast -- and exact, so every assertion
is bit equality.  For one probe per case the planted tensor is downloaded and its torch.amin / torch.amax on the CPU must
equal that expectation: the construction is anchored to the reference, not to itself.

Planted values.  Per tensor: +3 / -3, +inf / -inf, and one ulp (of the storage dtype) above the base maximum / below the
base minimum -- a compare in reduced precision or on a truncated value misses the last.  A launch carries one probe for
the maximum and one for the minimum at two different positions (two independent accumulators: neither can hide the
other); after the sweep every position of the set has been the maximum and the minimum once for each value.  NaN is a
probe of its own: minimum and maximum both NaN -- and, with several parameters, every other parameter's bits unchanged.

Per parameter (sections 3, 4), with L elements per parameter.  Launch k of a sweep plants, in EVERY parameter p at once, a
maximum at per-parameter position k and a minimum at position (k + L/2) % L.  What is planted goes by k % 4:
  k % 4 == 0      +-(3 + frac(p))
  k % 4 == 2      +-(2 + frac(p))
  k odd           one ulp (of the storage dtype) beyond parameter p's OWN base maximum / minimum
frac(p) = (p % M) / M with M = n_params for fp32 / fp64, min(n_params, 64) for bf16, min(n_params, 512) for fp16: after
rounding to the format still different for neighbouring parameters (asserted), so a parameter that reads its neighbour's data is caught on every
launch (the one-ulp values are each parameter's own as well).  Plain 3 + p / n_params on every launch would leave two
things unseen that the alternation shows: an output that is not written (the expectation changes from launch to launch)
and a compare in reduced precision (the one-ulp launches).
Positions: L <= 2048: all L launches, so every (parameter, position) pair has been maximum and minimum.  Larger L: the
edge positions plus every 61st.  The edge positions are, in EVERY row of the outer index, the first and last two vectors
and vectors 64 m - 1, 64 m, 64 m + 1 of the row -- slots 0 and V - 1 of each, all V slots of the row's first and last
vector; rows of up to 8 vectors are taken whole.  NaN probes run at the edge positions (L <= 2048: every (L / 256)-th
position and both ends), one parameter at a time -- the edge parameters in turn.

Guard bands.  The tensor under test is a view into a larger device buffer: >= 64 elements before it (the view stays
16-byte aligned; the unaligned cases shift it by one element), 4096 after it, filled +big, -big, NaN, NaN, ... (big =
1e30; 6e4 in fp16): an over-read changes the statistic, and the guard bytes are compared after the launches.

Premises.  `plan_minmax`, `mm_final`'s block shape, the ticket limits and the one-pass MAXV rule are restated below from
csrc/tq_stats.hip / csrc/tq_fake_quant.hip and asserted before each case: when a threshold moves, the premise fails first
and names the case to re-pick.  fp32 per-tensor cases also anchor the restated gx to the library
(tq_minmax_workspace_bytes(n, 1, 1) == 8 gx).

What reaches what (pb = per_block = 256 V 8 elements: 8192 fp32, 16384 16-bit; t = block, gx blocks):

 1 per tensor, tq_minmax (test_per_tensor_minmax)
     n = 5                    mm_rows<!VEC>, one block, fewer elements than lanes
     n = 3 pb                 mm_rows<VEC> gx = 3: the U = 4 loop (i + 768 < n_vec), chunk ends.  A chunk of k pb / gx = 2048
                              vectors is exactly two 4-vector rounds: the one-vector remainder loop does not run here (nor
                              at 2100 pb, 4200 pb), so:
     n = 2 pb + 1075 vectors  mm_rows<VEC> gx = 3, chunks of 1724 / 1723 vectors: one 4-vector round, then 3 (lanes 0 .. 187)
                              or 2 one-vector steps: a chunk's last vectors belong to the remainder loop
     n = 3 pb + 3             mm_rows<!VEC> by n % V, gx = 4, grid-stride
     n = 3 pb, shifted        mm_rows<!VEC> by misalignment
     n = 2100 pb              P = 2100 > sy = 1024: mm_final's plain loop wraps (p, p + 1024, p + 2048 < P)
     n = 4200 pb              P >= 4 sy: mm_final's 4-record loop once per lane and its remainder (records 4096 .. 4199)
   probe positions (the edge set): blocks {0, 1, gx/2, gx-2, gx-1, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096}
   that exist; in each, vectors j in {0, 1, 63, 64, 255, 256, 767, 768, 1023, 1024, len-2, len-1} of the block's chunk, slots
   0 and V-1, all V slots of the chunk's first and last vector (scalar kernels: the same j counted in elements of the
   block's grid-stride order); elements 0 and n-1; every element of the ragged tail; 64 seeded random positions.
 2 one range, tq_calibrate_tensor / tq_calibrate_stats + tq_calibrate_apply (test_single_range_calibration_step)
     ticket      calib_tensor_k<VEC> + ragged tail   n = pb + 3 (gx 2), 511 pb + 23 (gx = 512 = kTicketMaxBlocks; last-block
                                                     fold: its remainder loop, two records per lane)
     ticket-1    calib_tensor_k<!VEC>                n = 3 pb shifted by one element
     free        calib_partials_k + fq_tensor_calib  n = pb + 3, 512 pb + 7 (gx 513), 2047 pb + 7 (gx = 2048 =
                                                     kTicketFreeMaxBlocks: the `t += kBlock` fold, 8 pairs per lane)
     four        mm_rows + mm_final + calib_update_k + fq_tensor    n = 2048 pb + 7 (gx 2049)
     stats       calib_tensor_k, [-min, max] layout  n = pb + 3, 511 pb + 23; then tq_calibrate_apply with fresh buffers
                                                     (fq_tensor_calib from statistics) and in-place state (calib_update_k)
   checked: cur_min / cur_max (EST_CURRENT) == planted statistic, delta / zero_float == oracle.asym_params_from_range of
   it, on a few probes the symmetric recipe, an EST_ALL and an EST_RUNNING step against the fp32 update evaluated by hand,
   y == oracle.fake_quant_lowp on the CPU for a slab around the probe and for the last 64 elements; the ticket word is 0
   after every ticket launch; NaN probe -> NaN state and parameters.
   NOT reachable: the 4-record unrolled loop of calib_tensor_k's last-block fold needs b + 768 < gridDim.x, i.e. more than
   768 blocks, and the ticket form stops at 512.  The kernel is left as it is.
 3 per parameter, tq_minmax (test_per_parameter_minmax)
     mm_cols       (700, 24)       gy > 1; the U = 4 row loop and its remainder
                   (300, 768)      two column chunks, 19 row blocks
                   (37, 1032)      fp32: vpr = 258 -> gx = 3, dead lanes (live = cx < vpr) in the last column chunk
     mm_rows_wave  (9, 4096, 16)   two slices, 4-row batch + remainder;  (70, 128, 64);  (3, 7, 8) rows shorter than a wave
                   (19, 33, 1000)  vpr = 250 / 125: one row per wave (S = outer), the remainder loop over a long row
                   (9, 4096, 520)  vpr = 130 / 65 (> 64, not a multiple): the FLAT U-row index space, one full U S batch and
                                   a remainder (slice 0).  It is here because at (19, 33, 1000) S = min(ceil(8192 / 33),
                                   19) = 19 = outer: no wave ever owns U = 4 rows there and the flat loop does not run.
                   (131, 500, 136) S = 17, batches + remainder
                   (2100, 2, 8)    P = 2100, sy = 512: mm_final's 4-record loop and its remainder on a 134 KB tensor; rows
                                   of one or two vectors, so the edge set is every element: all 16 800 launches
     mm_rows       (4, 6, 4104)    block per row, rows longer than 512 vectors;  (3, 5, 33) inner % V != 0 (scalar);
                   (8, 16, 24) shifted by one element (scalar)
 4 calib_rows_onepass_k (test_onepass_dynamic_step): total = outer vpr = 512 | 513, 1024 | 1025, 2047, 2048 (MAXV 2 | 4 | 8)
   and 2049 (falls back to the layered launches); cur_min / cur_max against the planted values and delta / zero_float
   against the oracle on every launch, delta / zero_float / the whole y against tq_minmax -> tq_set_range_asym ->
   tq_fake_quant_fwd on every 16th (an on-device comparison), and the whole y against oracle.fake_quant_lowp on the CPU on
   the first, a middle and the last launch.  tq_minmax_f64 (test_float64_minmax): mm_f64_rows_k (5, 7, 24) and per tensor 20 011 (4 slices),
   mm_f64_cols_k (300, 40), mm_f64_final_k behind both; the one-ulp probes are one DOUBLE ulp.

Measured once on an MI355X (pytest --durations=0 of this module, seconds of the slowest case of each test function, input
generation, CPU reference and downloads included; the 90 cases together take 17 s):
  test_per_tensor_minmax                 0.43    (4200 pb, fp16: 134 MB, 2416 launches)
  test_single_range_calibration_step     0.26    (ticket-free, 2047 pb + 7, bf16: 67 MB)
  test_per_parameter_minmax              1.40    ((2100, 2, 8) fp32: 16 800 sweep launches and 16 800 NaN probes)
  test_onepass_dynamic_step              0.81    (total 2049, bf16: 16 392 launches of the layered fallback)
  test_float64_minmax                    0.78    (per tensor, 20 011 launches)
No case stands out, so no sample is thinned.
"""
import collections
import itertools

import pytest
import torch

from oracle import tq_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-8
NAN, INF = float('nan'), float('inf')

# ------------------------------------------------------------------------------------------------------------------
# the launchers' arithmetic, restated
#   plan_minmax, launch_minmax (cx, sy), kTicketMaxBlocks, kTicketFreeMaxBlocks     csrc/tq_stats.hip
#   launch_calib_rows_onepass (MAXV)                                                csrc/tq_fake_quant.hip
#   kBlock, kWave, kMaxGrid: csrc/tq_device.h; kWaveRowMaxVec, kWaveRowTarget: csrc/tq_host.h
# ------------------------------------------------------------------------------------------------------------------
K_BLOCK, K_WAVE, K_MAX_GRID = 256, 64, 2048
WAVE_ROW_MAX_VEC, WAVE_ROW_TARGET = 512, 8192
MM_MAX_BLOCKS = 16384
TICKET_MAX_BLOCKS, TICKET_FREE_MAX_BLOCKS = 512, 2048

Plan = collections.namedtuple('Plan', 'kernel vec bx by gx gy P S cx sy')


def _ceil_div(a, b):
    return -(-a // b)


def _V(dtype):
    return 4 if dtype == torch.float32 else 8


def plan_minmax(n, n_params, inner, V, aligned=True):
    """The launch `launch_minmax` gives n elements viewed as [n / (n_params inner), n_params, inner]."""
    def final(P):
        cx = min(n_params, 64)
        return cx, max(1, min(1024 // cx, max(1, P)))

    if n_params > 1 and inner == 1 and n_params % V == 0 and aligned:
        vpr, rows = n_params // V, n // n_params
        bx = min(vpr, 128)
        by = max(1, 256 // bx)
        gx = _ceil_div(vpr, bx)
        want = max(1, K_MAX_GRID // 2 // gx)
        gy = max(1, min(want, _ceil_div(rows, by * 8)))
        return Plan('mm_cols', True, bx, by, gx, gy, gy, 0, *final(gy))
    if (n_params > 1 and inner > 1 and inner % V == 0 and aligned and inner // V <= WAVE_ROW_MAX_VEC and n_params <= 1 << 24
            and n % (n_params * inner) == 0):
        outer = n // (n_params * inner)
        S = max(1, min(_ceil_div(WAVE_ROW_TARGET, n_params), outer))
        return Plan('mm_rows_wave', True, K_BLOCK, 1, _ceil_div(n_params * S, K_BLOCK // K_WAVE), 1, S, S, *final(S))
    eff_inner = n if n_params == 1 else inner
    n_rows = 1 if n_params == 1 else n // inner
    per_block = K_BLOCK * V * 4 * 2
    gy = min(n_rows, 65535)
    max_gx = max(1, MM_MAX_BLOCKS // max(1, min(n_rows, MM_MAX_BLOCKS)))
    gx = max(1, min(_ceil_div(eff_inner, per_block), max_gx))
    outer = 1 if n_params == 1 else n_rows // n_params
    return Plan('mm_rows', aligned and eff_inner % V == 0, K_BLOCK, 1, gx, gy, outer * gx, 0, *final(outer * gx))


def calibrate_tensor_form(n, V, aligned, want_y):
    """tq_calibrate_tensor: 'free' (calib_partials_k + fq_tensor_calib), 'ticket' (calib_tensor_k) or 'four' launches."""
    gx = plan_minmax(n, 1, 1, V, aligned).gx
    free_ok = want_y and aligned and gx <= TICKET_FREE_MAX_BLOCKS
    if gx > TICKET_MAX_BLOCKS and not free_ok:
        return 'four', gx
    return ('free' if free_ok else 'ticket'), gx


def onepass_maxv(outer, n_params, inner, V):
    """launch_calib_rows_onepass: registers per lane (2 / 4 / 8 vectors), or None when the shape falls back."""
    if n_params < 2 or inner < 2 or inner % V or n_params > 1 << 20:
        return None
    total = outer * (inner // V)
    if total > K_BLOCK * 8 or outer > 0xffff:
        return None
    return 2 if total <= K_BLOCK * 2 else (4 if total <= K_BLOCK * 4 else 8)


def _premise(got, **want):
    have = {k: getattr(got, k) for k in want}
    assert have == want, ('the launcher no longer gives this case the form it was picked for: re-pick its size', want, got)


# ------------------------------------------------------------------------------------------------------------------
# base tensors, guard bands, probes
# ------------------------------------------------------------------------------------------------------------------
def _base(n, dtype, seed):
    """Seeded uniform [-1, 1] rounded to `dtype`, no zeros (flat, CPU)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, generator=g, dtype=torch.float64 if dtype == torch.float64 else torch.float32).mul_(2).sub_(1).to(dtype)
    x[x == 0] = 0.5
    return x


def _int_view(t):
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _ulp_out(v):
    """One ulp of v's own dtype away from zero (v != 0, finite)."""
    return (_int_view(v.clone()) + 1).view(v.dtype)


def _wide(t):
    """The values as the kernels' result type holds them (fp32; fp64 for the double entry): exact."""
    return t.double() if t.dtype == torch.float64 else t.float()


def _assert_bits(got, want, what, probe=None):
    """Bit equality of two tensors of the result type (compared on the CPU); a NaN equals a NaN.  probe(k) describes the
    probe behind row k of the first miss."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (_int_view(got) != _int_view(want)) & ~(torch.isnan(got) & torch.isnan(want))
    if bool(bad.any()):
        first = bad.nonzero()[0].tolist()
        raise AssertionError('%s: %d of %d values differ; first at %r%s: got %r, want %r' % (
            what, int(bad.sum()), bad.numel(), first, '' if probe is None or not first else ' (%s)' % (probe(first[0]),),
            got[tuple(first)].item(), want[tuple(first)].item()))


class _Guarded:
    """A flat base tensor as a view into a device buffer with guard bands on both sides."""
    BACK = 4096

    def __init__(self, base, shift=0):
        n, dtype = base.numel(), base.dtype
        self.n, self.front = n, 64 + shift
        big = 6e4 if dtype == torch.float16 else 1e30
        self.buf = torch.empty(self.front + n + self.BACK, dtype=dtype, device=DEV)
        pattern = torch.tensor([big, -big, NAN, NAN], dtype=dtype, device=DEV)
        self.buf[:self.front] = pattern.repeat(self.front // 4 + 1)[-self.front:]          # +-big, NaN next to the tensor
        self.buf[self.front + n:] = pattern.repeat(self.BACK // 4)
        self.x = self.buf[self.front:self.front + n]
        self.x.copy_(base)
        assert (self.x.data_ptr() % 16 == 0) == (shift == 0)
        self.base = base
        self.base_bits = _int_view(self.x).clone()
        self.guards = self._guard_bits()

    def _guard_bits(self):
        b = _int_view(self.buf)
        return torch.cat([b[:self.front], b[self.front + self.n:]]).clone()

    def sweep(self, idx, val, launch):
        """For every row k of idx / val ([K, m], CPU): plant val[k] at the flat positions idx[k], launch(k), put the base
        values back.  -> the list of what launch(k) returned (small device tensors; nothing is synchronised)."""
        idx_d, val_d = idx.to(DEV), val.to(self.x.dtype).to(DEV)
        keep = self.x[idx_d]
        outs = []
        for k, (i, v, b) in enumerate(zip(idx_d.unbind(0), val_d.unbind(0), keep.unbind(0))):
            self.x.index_put_((i,), v)
            outs.append(launch(k))
            self.x.index_put_((i,), b)
        return outs

    def planted_on_cpu(self, idx_row, val_row):
        """The tensor with one probe planted, downloaded (the device tensor is restored)."""
        i, v = idx_row.to(DEV), val_row.to(self.x.dtype).to(DEV)
        keep = self.x[i]
        self.x.index_put_((i,), v)
        host = self.x.to('cpu', copy=True)
        self.x.index_put_((i,), keep)
        return host

    def check_untouched(self, what):
        torch.cuda.synchronize()
        assert torch.equal(self._guard_bits(), self.guards), what + ': guard bytes changed'
        assert torch.equal(_int_view(self.x), self.base_bits), what + ': the tensor was not restored / was written to'


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
# 1 / 2: one range
# ------------------------------------------------------------------------------------------------------------------
EDGE_BLOCKS = (255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096)
EDGE_J = (0, 1, 63, 64, 255, 256, 767, 768, 1023, 1024)


def tensor_edge_positions(n, V, gx, vec, seed):
    """The edge set of section 1 (sorted flat element positions) and the ragged tail's positions."""
    pos = {0, n - 1}
    blocks = sorted({t for t in (0, 1, gx // 2, gx - 2, gx - 1) + EDGE_BLOCKS if 0 <= t < gx})
    tail = []
    if vec:
        n_all = n // V
        chunk = _ceil_div(n_all, gx)
        for t in blocks:
            v0, v1 = t * chunk, min(n_all, (t + 1) * chunk)
            ln = v1 - v0
            for j in EDGE_J + (ln - 2, ln - 1):
                if 0 <= j < ln:
                    pos.update((v0 + j) * V + s for s in (range(V) if j in (0, ln - 1) else (0, V - 1)))
        tail = list(range(n_all * V, n))
        pos.update(tail)
    else:
        stride = gx * K_BLOCK                                # block t, trip k, lane l reads t 256 + l + k stride
        for t in blocks:
            if t * K_BLOCK >= n:
                continue
            trips = _ceil_div(n - t * K_BLOCK, stride)
            ln = (trips - 1) * K_BLOCK + min(K_BLOCK, n - t * K_BLOCK - (trips - 1) * stride)
            for j in EDGE_J + (ln - 2, ln - 1):
                if 0 <= j < ln:
                    pos.add(t * K_BLOCK + j % K_BLOCK + (j // K_BLOCK) * stride)
    g = torch.Generator().manual_seed(seed)
    pos.update(torch.randint(0, n, (64,), generator=g).tolist())
    assert all(0 <= p < n for p in pos)
    return sorted(pos), tail


KINDS = ('three', 'inf', 'ulp')


def tensor_probes(base, positions):
    """-> idx [K', 2], val [K', 2] (fp32 / storage-exact), want [K', 2] = (min, max), kinds [K'].  Three value kinds per
    position pair (maximum at positions[k], minimum at positions[(k + K/2) % K]) and one NaN probe per position."""
    K = len(positions)
    wide = _wide(base)
    bmin, bmax = torch.amin(wide), torch.amax(wide)
    assert bmin < 0 < bmax
    up = _wide(_ulp_out(bmax.to(base.dtype)))
    down = _wide(_ulp_out(bmin.to(base.dtype)))
    assert up > bmax and down < bmin
    p_max = torch.tensor(positions)
    p_min = p_max.roll(-(K // 2))
    assert K > 1 and bool((p_max != p_min).all())
    at = torch.stack([p_max, p_min], 1)
    rows_v, rows_w, kinds = [], [], []
    for kind, (hi, lo) in zip(KINDS, ((3.0, -3.0), (INF, -INF), (up.item(), down.item()))):
        rows_v.append(torch.tensor([hi, lo], dtype=wide.dtype).repeat(K, 1))
        rows_w.append(torch.tensor([lo, hi], dtype=wide.dtype).repeat(K, 1))
        kinds += [kind] * K
    # NaN: alone (the second slot re-plants the base value that is there anyway)
    rows_v.append(torch.stack([torch.full((K,), NAN, dtype=wide.dtype), wide[p_min]], 1))
    rows_w.append(torch.full((K, 2), NAN, dtype=wide.dtype))
    kinds += ['nan'] * K
    return at.repeat(4, 1), torch.cat(rows_v), torch.cat(rows_w), kinds, (bmin, bmax)


def _describe(idx, kinds):
    return lambda k: '%s probe: maximum / NaN at element %d, minimum at element %d' % (kinds[k], idx[k, 0], idx[k, -1])


def _anchor_tensor(gd, idx, val, want, k):
    """Probe k's expectation equals torch.amin / torch.amax of the downloaded planted tensor."""
    host = _wide(gd.planted_on_cpu(idx[k], val[k]))
    _assert_bits(torch.stack([torch.amin(host), torch.amax(host)]), want[k], 'construction vs torch.amin / amax, probe %d' % k)


TENSOR_CASES = {                 # blocks of per_block elements, extra elements, shift -> kernel arm, gx
    '5': (0, 5, 0, dict(vec=False, gx=1)),
    '3pb': (3, 0, 0, dict(vec=True, gx=3)),
    '2pb+1075v': (2, ('vectors', 1075), 0, dict(vec=True, gx=3)),
    '3pb+3': (3, 3, 0, dict(vec=False, gx=4)),
    '3pb-shifted': (3, 0, 1, dict(vec=False, gx=3)),
    '2100pb': (2100, 0, 0, dict(vec=True, gx=2100, sy=1024)),
    '4200pb': (4200, 0, 0, dict(vec=True, gx=4200, sy=1024)),
}


@pytest.mark.parametrize('case,dtype', [(c, d) for d in (torch.float32, torch.bfloat16) for c in TENSOR_CASES] +
                         [(c, torch.float16) for c in TENSOR_CASES],
                         ids=lambda v: str(v).replace('torch.', ''))
def test_per_tensor_minmax(be, case, dtype):
    """Section 1: tq_minmax with one range -- mm_rows<VEC>, mm_rows<!VEC>, mm_final."""
    blocks, extra, shift, premise = TENSOR_CASES[case]
    V = _V(dtype)
    n = blocks * K_BLOCK * V * 8 + (extra[1] * V if isinstance(extra, tuple) else extra)
    pl = plan_minmax(n, 1, 1, V, aligned=shift == 0)
    _premise(pl, kernel='mm_rows', cx=1, P=premise['gx'], **premise)
    if case == '2pb+1075v':
        chunk = _ceil_div(n // V, pl.gx)
        assert 4 * K_BLOCK < chunk and 0 < chunk % (4 * K_BLOCK) <= 3 * K_BLOCK and chunk % K_BLOCK, \
            'mm_rows<VEC>: the last vectors of a chunk belong to the one-vector loop, and its last trip is ragged'
    if case == '2100pb':
        assert pl.sy < pl.P < 4 * pl.sy, 'mm_final: the plain loop alone, more than one trip'
    if case == '4200pb':
        assert pl.P >= 4 * pl.sy and pl.P % (4 * pl.sy), 'mm_final: the 4-record loop and a remainder'
    if dtype == torch.float32:       # (the library reports the larger of its plans over vector widths: that is fp32's)
        assert be.lib.tq_minmax_workspace_bytes(n, 1, 1) == 8 * pl.gx
    base = _base(n, dtype, 100 + n % 1009)
    gd = _Guarded(base, shift)
    positions, _ = tensor_edge_positions(n, V, pl.gx, pl.vec, seed=n)
    idx, val, want, kinds, _ = tensor_probes(base, positions)
    _anchor_tensor(gd, idx, val, want, kinds.index('ulp'))
    outs = gd.sweep(idx, val, lambda k: be.minmax(gd.x, 1, 1))
    got = torch.stack([t for o in outs for t in o]).view(-1, 2)
    gd.check_untouched(case)
    _assert_bits(got, want.float(), 'tq_minmax %s %s' % (case, dtype), _describe(idx, kinds))


# ---- 2 -------------------------------------------------------------------------------------------------------------
CALIB_CASES = {                  # form, blocks, extra (fp32; 16-bit: extra stays below its own V), shift, want_y, gx
    'ticket-pb+3': ('ticket', 1, 3, 0, False, 2),
    'ticket-511pb+23': ('ticket', 511, 23, 0, False, 512),
    'ticket-scalar-3pb-shifted': ('ticket', 3, 0, 1, False, 3),
    'free-pb+3': ('free', 1, 3, 0, True, 2),
    'free-512pb+7': ('free', 512, 7, 0, True, 513),
    'free-2047pb+7': ('free', 2047, 7, 0, True, 2048),
    'four-2048pb+7': ('four', 2048, 7, 0, True, 2049),
    'four-2048pb+7-no-y': ('four', 2048, 7, 0, False, 2049),
    'stats-pb+3': ('stats', 1, 3, 0, False, 2),
    'stats-511pb+23': ('stats', 511, 23, 0, False, 512),
}


def _asym(lo, hi):
    return O.asym_params_from_range(lo.float(), hi.float(), 8, EPS)


def _some(kinds, positions_of_probe, tail, count=3):
    """A handful of probe indices per finite kind: spread over the sweep, plus those whose maximum sits in the tail."""
    pick = []
    for kind in ('three', 'ulp'):
        ks = [k for k, v in enumerate(kinds) if v == kind]
        pick += [ks[(len(ks) - 1) * j // max(count - 1, 1)] for j in range(count)]
        pick += [k for k in ks if positions_of_probe[k] in tail][:count]
    return sorted(set(pick))


@pytest.mark.parametrize('case,dtype', [(c, torch.float32) for c in CALIB_CASES] +
                         [(c, torch.bfloat16) for c in CALIB_CASES] +
                         [('ticket-pb+3', torch.float16), ('free-pb+3', torch.float16), ('stats-pb+3', torch.float16)],
                         ids=lambda v: str(v).replace('torch.', ''))
def test_single_range_calibration_step(be, case, dtype):
    """Section 2: the one-range calibration step in its four forms, and the stats-only ticket form."""
    from quantization import _hip
    form, blocks, extra, shift, want_y, gx_want = CALIB_CASES[case]
    V = _V(dtype)
    n = blocks * K_BLOCK * V * 8 + extra
    aligned = shift == 0
    got_form, gx = calibrate_tensor_form(n, V, aligned, want_y)
    assert (got_form, gx) == ('ticket' if form == 'stats' else form, gx_want), \
        ('tq_calibrate_tensor no longer gives this size the form the case was picked for', case, got_form, gx)
    assert extra == 0 or n % V, 'every aligned size here has a ragged tail'
    base = _base(n, dtype, 200 + blocks + extra)
    gd = _Guarded(base, shift)
    x = gd.x
    # the kernels that see a ragged tail walk whole vectors + tail; the four-launch form is tq_minmax on n % V != 0: scalar
    vec = aligned and (form != 'four' or n % V == 0)
    positions, tail = tensor_edge_positions(n, V, gx, vec, seed=n)
    if not vec:
        tail = list(range(n - n % V, n))
        positions = sorted(set(positions) | set(tail))
    idx, val, want, kinds, _ = tensor_probes(base, positions)
    describe = _describe(idx, kinds)
    _anchor_tensor(gd, idx, val, want, kinds.index('ulp'))
    want = want.float()
    want_delta, want_zf = _asym(want[:, 0], want[:, 1])
    counter = lambda: be._counters[(torch.cuda.current_device(), _hip._stream())]      # noqa: E731
    few = _some(kinds, idx[:, 0].tolist(), set(tail))
    tickets, slabs = [], {}

    def slab_of(k):
        p = int(idx[k, 0])
        lo = max(0, min(p - 512, n - 1024))
        return lo, min(n, lo + 1024)

    def keep_slabs(k, y):
        """x and y around probe k and at the end of the tensor, while the probe is planted (y itself is not kept)."""
        lo, hi = slab_of(k)
        y = y.reshape(-1)
        slabs[k] = (x[lo:hi].clone(), y[lo:hi].clone(), x[n - 64:].clone(), y[n - 64:].clone())

    def check_slabs():
        for k, (xs, ys, xt, yt) in slabs.items():
            for xi, yi, where in ((xs, ys, 'around the probe'), (xt, yt, 'last 64 elements')):
                ref = O.fake_quant_lowp(xi.cpu(), want_delta[k], want_zf[k], 8, False)[1]
                assert torch.equal(_int_view(yi.cpu()), _int_view(ref)), (case, 'y differs from the oracle', where, describe(k))

    def step(mode, prev, symmetric=False):
        def launch(k):
            r = be.calibrate_minmax(x, 1, 1, mode, prev[0], prev[1], 0.9, 0, None, 8, symmetric, EPS, False, want_y=want_y)
            assert (r[5] is not None) == want_y
            if form == 'ticket':
                tickets.append(counter().clone())
            if want_y and mode == _hip.EST_CURRENT and not symmetric and k in few:
                keep_slabs(k, r[5])
            return torch.stack([r[0], r[1], r[2], r[4].float() if symmetric else r[3]])
        return launch

    if form != 'stats':
        got = torch.stack(gd.sweep(idx, val, step(_hip.EST_CURRENT, (None, None))))
        _assert_bits(got[:, :2], want, case + ': cur_min / cur_max', describe)
        _assert_bits(got[:, 2], want_delta, case + ': delta', describe)
        _assert_bits(got[:, 3], want_zf, case + ': zero_float', describe)
        assert len(slabs) == (len(few) if want_y else 0)
        check_slabs()
        # EST_ALL / EST_RUNNING from a previous state, and the symmetric recipe, on the handful
        om, mom = torch.tensor(1.0 - 0.9, dtype=torch.float64).float(), torch.tensor(0.9, dtype=torch.float64).float()
        wf = want[few]
        for prev in ((-2.0, 5.0), (-5.0, 0.25)):
            pa, pb = torch.tensor(prev[0]), torch.tensor(prev[1])
            for mode, (a, b) in ((_hip.EST_ALL, (torch.minimum(pa, wf[:, 0]), torch.maximum(pb, wf[:, 1]))),
                                 (_hip.EST_RUNNING, (om * wf[:, 0] + mom * pa, om * wf[:, 1] + mom * pb))):
                got = torch.stack(gd.sweep(idx[few], val[few], step(mode, (pa.to(DEV), pb.to(DEV)))))
                _assert_bits(got, torch.stack([a, b, *_asym(a, b)], 1), '%s: mode %d from state %r' % (case, mode, prev),
                             lambda j: describe(few[j]))
        got = torch.stack(gd.sweep(idx[few], val[few], step(_hip.EST_CURRENT, (None, None), symmetric=True)))
        sym = [O.sym_params_from_range(lo, hi, 8, EPS) for lo, hi in wf]
        _assert_bits(got, torch.stack([wf[:, 0], wf[:, 1], torch.stack([d.reshape(()) for d, _ in sym]),
                                       torch.stack([s.reshape(()).float() for _, s in sym])], 1), case + ': symmetric recipe',
                     lambda j: describe(few[j]))
        if form == 'ticket':
            assert int(torch.stack(tickets).abs().sum()) == 0, case + ': the ticket word is not 0 after a launch'
    else:
        applied = {}

        def stats_then_apply(k):
            stats = be.calibrate_stats(x, 1, 1)
            tickets.append(counter().clone())
            if k in few:
                r = be.calibrate_apply(stats, x, 1, 1, _hip.EST_CURRENT, None, None, 0.9, 0, None, 8, False, EPS, False)
                applied[k] = torch.stack(list(r[:4]))
                keep_slabs(k, r[5])
            return stats

        got = torch.stack(gd.sweep(idx, val, stats_then_apply))
        _assert_bits(got, torch.stack([-want[:, 0], want[:, 1]], 1), case + ': [-min, max]', describe)
        assert int(torch.stack(tickets).abs().sum()) == 0, case + ': the ticket word is not 0 after a launch'
        for k, par in applied.items():
            _assert_bits(par, torch.stack([want[k, 0], want[k, 1], want_delta[k], want_zf[k]]),
                         '%s: apply into fresh buffers, %s' % (case, describe(k)))
        check_slabs()
        # in-place state through EST_ALL: the state is the running extreme of the probes so far
        state = tuple(torch.tensor(v, device=DEV) for v in (-2.0, 2.0, 0.0, 0.0))

        def apply_in_place(k):
            r = be.calibrate_apply(be.calibrate_stats(x, 1, 1), x, 1, 1, _hip.EST_ALL, state[0], state[1], 0.9, 0, None, 8, False,
                                   EPS, False, want_y=False, out=state + (None,))
            return torch.stack(list(r[:4]))

        got = torch.stack(gd.sweep(idx[few], val[few], apply_in_place))
        a = torch.cummin(torch.cat([torch.tensor([-2.0]), want[few, 0]]), 0)[0][1:]
        b = torch.cummax(torch.cat([torch.tensor([2.0]), want[few, 1]]), 0)[0][1:]
        _assert_bits(got, torch.stack([a, b, *_asym(a, b)], 1), case + ': apply, in-place state', lambda j: describe(few[j]))
    # NaN probes: state and parameters NaN -- part of the sweeps above (`want` is NaN there); nothing around x was touched
    assert kinds.count('nan') == len(positions)
    gd.check_untouched(case)


# ------------------------------------------------------------------------------------------------------------------
# 3 / 4: one range per parameter
# ------------------------------------------------------------------------------------------------------------------
def _edge_in_row(inner, V):
    """Element offsets in a row of `inner` elements: first / last two vectors, vectors 64 m - 1, 64 m, 64 m + 1."""
    vpr = _ceil_div(inner, V)
    if vpr <= 8:
        return list(range(inner))
    vecs = {0, 1, vpr - 2, vpr - 1}
    for m in range(64, vpr, 64):
        vecs.update((m - 1, m, m + 1))
    out = set()
    for v in vecs:
        if 0 <= v < vpr:
            out.update(v * V + s for s in (range(V) if v in (0, vpr - 1) else (0, V - 1)))
    return sorted(e for e in out if e < inner)


def parameter_positions(outer, inner, V):
    """-> (sweep, edge): per-parameter positions k = o inner + i.  sweep: all L = outer inner of them up to 2048, else the
    edge set plus every 61st; edge: the edge set, in every row (L <= 2048: every L // 256-th position and both ends)."""
    L = outer * inner
    if L <= 2048:
        return list(range(L)), sorted(set(range(0, L, max(L // 256, 1))) | {L - 1})
    edge = sorted({o * inner + i for o in range(outer) for i in _edge_in_row(inner, V)})
    return sorted(set(edge) | set(range(0, L, 61))), edge


class _PerParameter:
    """[outer, n_params, inner] base tensor, its per-parameter extremes, and the planted sweeps."""

    def __init__(self, shape, dtype, shift=0, seed=0):
        self.outer, self.P, self.inner = (shape[0], shape[1], 1) if len(shape) == 2 else shape
        self.shape, self.dtype, self.V = shape, dtype, (2 if dtype == torch.float64 else _V(dtype))
        self.L = self.outer * self.inner
        base = _base(self.outer * self.P * self.inner, dtype, 300 + seed + sum(shape))
        self.gd = _Guarded(base, shift)
        self.x = self.gd.x.view(*shape)
        self.bmin, self.bmax = self.per_parameter(base)
        assert bool((self.bmin < 0).all()) and bool((self.bmax > 0).all())
        steps = {torch.float32: self.P, torch.float64: self.P, torch.bfloat16: min(self.P, 64), torch.float16: min(self.P, 512)}[dtype]
        frac = (torch.arange(self.P) % steps).double() / steps
        self.mags = [_wide((m + frac).to(dtype)) for m in (3.0, 2.0)]          # both in [2, 4): one ulp of the format throughout
        assert all(bool((m[1:] != m[:-1]).all()) for m in self.mags), 'neighbouring parameters plant different magnitudes'
        self.up = _wide(_ulp_out(self.bmax.to(dtype)))
        self.down = _wide(_ulp_out(self.bmin.to(dtype)))
        assert bool((self.up > self.bmax).all()) and bool((self.down < self.bmin).all())

    def per_parameter(self, flat):
        w = _wide(flat).view(self.outer, self.P, self.inner).permute(1, 0, 2).reshape(self.P, -1)
        return torch.amin(w, 1), torch.amax(w, 1)

    def flat(self, k, p):
        """Flat element positions of per-parameter positions k ([K] or scalar) of parameters p."""
        return ((k // self.inner) * self.P + p) * self.inner + k % self.inner

    def sweep_plan(self, positions):
        """-> idx [K, 2 P], val [K, 2 P], want [K, 2, P]: launch j plants every parameter's maximum at positions[j] and
        its minimum at (positions[j] + L / 2) % L; even launches +-(3 | 2 + frac(p)), odd launches one ulp out."""
        k = torch.tensor(positions)
        p = torch.arange(self.P)
        i_max = self.flat(k[:, None], p[None, :])
        i_min = self.flat(((k + self.L // 2) % self.L)[:, None], p[None, :])
        K = len(positions)
        hi = torch.empty(K, self.P, dtype=self.bmax.dtype)
        j = torch.arange(K)
        hi[j % 4 == 0] = self.mags[0]
        hi[j % 4 == 2] = self.mags[1]
        lo = -hi
        hi[j % 2 == 1] = self.up
        lo[j % 2 == 1] = self.down
        assert self.L >= 2
        return torch.cat([i_max, i_min], 1), torch.cat([hi, lo], 1), torch.stack([lo, hi], 1)

    def nan_plan(self, positions):
        """-> idx [K, 1], val [K, 1], want [K, 2, P]: NaN at positions[j] of ONE parameter (the edge parameters in turn)."""
        V, P = self.V, self.P
        edge_p = sorted({q for q in (0, 1, V - 1, V, P // 2, P - V - 1, P - V, P - 2, P - 1, 128 * V - 1, 128 * V, 256 * V - 1,
                                     256 * V, 63, 64, 65) if 0 <= q < P})
        prm = torch.tensor(list(itertools.islice(itertools.cycle(edge_p), len(positions))))
        k = torch.tensor(positions)
        want = torch.stack([self.bmin, self.bmax]).repeat(len(positions), 1, 1)
        want[torch.arange(len(positions)), :, prm] = NAN
        return self.flat(k, prm)[:, None], torch.full((len(positions), 1), NAN, dtype=self.bmax.dtype), want

    def anchor(self, idx, val, want, k):
        host = self.gd.planted_on_cpu(idx[k], val[k])
        _assert_bits(torch.stack(self.per_parameter(host)), want[k], 'construction vs torch.amin / amax, launch %d' % k)


PARAMETER_CASES = {
    # mm_cols
    'cols-700x24': ((700, 24), 0, {torch.float32: dict(kernel='mm_cols', gx=1, gy=3, by=42), torch.bfloat16: dict(kernel='mm_cols', gx=1, gy=2, by=85)}),
    'cols-300x768': ((300, 768), 0, {torch.float32: dict(kernel='mm_cols', gx=2, gy=19, bx=128), torch.bfloat16: dict(kernel='mm_cols', gx=1, gy=19, bx=96)}),
    'cols-37x1032': ((37, 1032), 0, {torch.float32: dict(kernel='mm_cols', gx=3, gy=3, bx=128), torch.bfloat16: dict(kernel='mm_cols', gx=2, gy=3, bx=128),
                                      torch.float16: dict(kernel='mm_cols', gx=2, gy=3, bx=128)}),
    # mm_rows_wave
    'wave-9x4096x16': ((9, 4096, 16), 0, {d: dict(kernel='mm_rows_wave', S=2) for d in (torch.float32, torch.bfloat16, torch.float16)}),
    'wave-70x128x64': ((70, 128, 64), 0, {d: dict(kernel='mm_rows_wave', S=64) for d in (torch.float32, torch.bfloat16)}),
    'wave-3x7x8': ((3, 7, 8), 0, {d: dict(kernel='mm_rows_wave', S=3) for d in (torch.float32, torch.bfloat16)}),
    'wave-19x33x1000': ((19, 33, 1000), 0, {d: dict(kernel='mm_rows_wave', S=19) for d in (torch.float32, torch.bfloat16)}),
    'wave-flat-9x4096x520': ((9, 4096, 520), 0, {d: dict(kernel='mm_rows_wave', S=2) for d in (torch.float32, torch.bfloat16)}),
    'wave-131x500x136': ((131, 500, 136), 0, {d: dict(kernel='mm_rows_wave', S=17) for d in (torch.float32, torch.bfloat16)}),
    'wave-2100x2x8': ((2100, 2, 8), 0, {d: dict(kernel='mm_rows_wave', S=2100, P=2100, cx=2, sy=512) for d in (torch.float32, torch.bfloat16)}),
    # mm_rows, one block per row
    'rows-4x6x4104': ((4, 6, 4104), 0, {d: dict(kernel='mm_rows', vec=True, gx=1, gy=24) for d in (torch.float32, torch.bfloat16, torch.float16)}),
    'rows-3x5x33': ((3, 5, 33), 0, {d: dict(kernel='mm_rows', vec=False, gx=1, gy=15) for d in (torch.float32, torch.bfloat16)}),
    'rows-8x16x24-shifted': ((8, 16, 24), 1, {d: dict(kernel='mm_rows', vec=False, gx=1, gy=128) for d in (torch.float32, torch.bfloat16)}),
}


def _shape_premise(case, pc, pl):
    """What the case was picked for beyond the kernel choice."""
    outer, inner, V = pc.outer, pc.inner, pc.V
    if case == 'cols-700x24':
        chunk = _ceil_div(outer, pl.gy)
        assert pl.gy > 1 and chunk // pl.by >= 4 and chunk % (4 * pl.by), 'mm_cols: a full U = 4 trip and a remainder per lane'
    if case == 'cols-37x1032' and pc.dtype == torch.float32:
        assert pc.P // V == 258 and pl.gx * pl.bx > pc.P // V, 'mm_cols: dead lanes in the last column chunk'
    if case == 'wave-9x4096x16':
        assert outer >= 4 * pl.S and (outer - 4 * pl.S) % (4 * pl.S) and inner // V <= K_WAVE, 'a 4-row batch and a remainder'
    if case == 'wave-19x33x1000':
        vpr = inner // V
        assert vpr > K_WAVE and vpr % K_WAVE and outer < 4 * pl.S, 'long ragged rows through the remainder loop (one row per wave)'
    if case == 'wave-flat-9x4096x520':
        vpr = inner // V
        assert vpr > K_WAVE and vpr % K_WAVE, 'the flat U-row index space needs vpr > 64, vpr % 64 != 0'
        assert outer >= 4 * pl.S and 0 < outer - 4 * pl.S < 4 * pl.S, 'one full U S batch and a non-empty remainder'
    if case == 'wave-2100x2x8':
        assert pl.P >= 4 * pl.sy and pl.P % (4 * pl.sy), "mm_final's 4-record loop and its remainder"
    if case == 'rows-4x6x4104':
        assert inner // V > WAVE_ROW_MAX_VEC
    if case == 'rows-3x5x33':
        assert inner % V


@pytest.mark.parametrize('case,dtype', [(c, d) for c, v in PARAMETER_CASES.items() for d in v[2]],
                         ids=lambda v: str(v).replace('torch.', ''))
def test_per_parameter_minmax(be, case, dtype):
    """Section 3: tq_minmax with one range per parameter -- mm_cols, mm_rows_wave, mm_rows (block per row), mm_final."""
    shape, shift, premises = PARAMETER_CASES[case]
    pc = _PerParameter(shape, dtype, shift)
    pl = plan_minmax(pc.x.numel(), pc.P, pc.inner, pc.V, aligned=shift == 0)
    _premise(pl, **premises[dtype])
    _shape_premise(case, pc, pl)
    positions, edge = parameter_positions(pc.outer, pc.inner, pc.V)
    if case == 'wave-2100x2x8':
        assert len(edge) == pc.L, 'rows of one or two vectors: every element of every row is an edge position'
    idx, val, want = pc.sweep_plan(positions)
    pc.anchor(idx, val, want, 1)
    launch = lambda k: torch.stack(be.minmax(pc.x, pc.P, pc.inner))          # noqa: E731
    got = torch.stack(pc.gd.sweep(idx, val, launch))
    _assert_bits(got, want.float(), '%s %s: planted extremes (launch, min | max, parameter)' % (case, dtype),
                 lambda j: 'maxima at per-parameter position %d' % positions[j])
    idx, val, want = pc.nan_plan(edge)
    pc.anchor(idx, val, want, len(edge) - 1)
    got = torch.stack(pc.gd.sweep(idx, val, launch))
    _assert_bits(got, want.float(), '%s %s: NaN probes (launch, min | max, parameter)' % (case, dtype),
                 lambda j: 'NaN at element %d' % idx[j, 0])
    pc.gd.check_untouched(case)


# ---- 4 -------------------------------------------------------------------------------------------------------------
ONEPASS_CASES = {                # fp32 shape (16-bit: inner doubled), total = outer * vpr, MAXV
    '512': ((2, 5, 1024), 512, 2), '513': ((3, 5, 684), 513, 4), '1024': ((4, 5, 1024), 1024, 4), '1025': ((5, 5, 820), 1025, 8),
    '2047': ((23, 5, 356), 2047, 8), '2048': ((8, 5, 1024), 2048, 8), '2049-falls-back': ((3, 5, 2732), 2049, None),
}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', list(ONEPASS_CASES))
def test_onepass_dynamic_step(be, case, dtype):
    """Section 4: calib_rows_onepass_k at both sides of its MAXV steps; every element of every parameter is the maximum
    once and the minimum once."""
    from quantization import _hip
    shape, total, maxv = ONEPASS_CASES[case]
    V = _V(dtype)
    shape = (shape[0], shape[1], shape[2] * V // 4)
    assert shape[0] * (shape[2] // V) == total and onepass_maxv(*shape, V) == maxv, (case, shape, onepass_maxv(*shape, V))
    pc = _PerParameter(shape, dtype, seed=7)
    positions = list(range(pc.L))
    idx, val, want = pc.sweep_plan(positions)
    pc.anchor(idx, val, want, 1)
    want = want.float()
    ks = [k for k in positions if k % 16 == 0 or k == pc.L - 1]
    chained, on_cpu = [], {}

    def step(k, chain=True):
        r = be.calibrate_minmax(pc.x, pc.P, pc.inner, _hip.EST_CURRENT, None, None, 0.9, 0, None, 8, False, EPS, False, want_y=True)
        if chain and k in (0, pc.L // 2 + 1, pc.L - 1):          # the whole x and y of three launches, for the CPU oracle
            on_cpu[k] = (pc.x.clone(), r[5].clone())
        if chain and (k % 16 == 0 or k == pc.L - 1):
            mn, mx = be.minmax(pc.x, pc.P, pc.inner)
            d, z = be.set_range_asym(mn, mx, 8, EPS, False)
            y, _ = be.fake_quant(pc.x, d, z, None, 8, False, False, EPS, pc.P, pc.inner)
            same_y = (_int_view(y) == _int_view(r[5])).all()
            chained.append(torch.cat([torch.stack([mn, mx, d, z]).reshape(-1), same_y.float().reshape(1)]))
        return torch.stack(r[:4])                      # (y is not kept)

    got = torch.stack(pc.gd.sweep(idx, val, step)).cpu()
    at = lambda j: 'maxima at per-parameter position %d' % j          # noqa: E731
    _assert_bits(got[:, :2], want, case + ': cur_min / cur_max', at)
    d, z = _asym(want[:, 0], want[:, 1])
    _assert_bits(got[:, 2], d, case + ': delta vs the oracle', at)
    _assert_bits(got[:, 3], z, case + ': zero_float vs the oracle', at)
    chained = torch.stack(chained).cpu()
    _assert_bits(chained[:, :-1].reshape(len(ks), 4, pc.P), got[ks], case + ': state and parameters vs the layered chain',
                 lambda j: at(ks[j]))
    assert bool((chained[:, -1] == 1).all()), (case, 'y differs from tq_fake_quant_fwd of the layered chain',
                                              [k for k, same in zip(ks, chained[:, -1].tolist()) if not same])
    assert len(on_cpu) == 3
    for k, (xk, yk) in on_cpu.items():
        ref = O.fake_quant_lowp(xk.cpu(), d[k], z[k], 8, False, axis=1)[1]
        assert torch.equal(_int_view(yk.cpu()), _int_view(ref)), (case, 'y differs from the oracle', at(k))
    # NaN in one parameter: that parameter's state and parameters NaN, the others' bits as without it
    nan_at = sorted({0, 1, pc.inner - 1, pc.inner, pc.L // 2, pc.L - pc.inner, pc.L - 2, pc.L - 1})
    idx, val, want = pc.nan_plan(nan_at)
    pc.anchor(idx, val, want, 0)
    want = want.float()
    got = torch.stack(pc.gd.sweep(idx, val, lambda k: step(k, chain=False))).cpu()
    d, z = _asym(want[:, 0], want[:, 1])
    _assert_bits(got, torch.stack([want[:, 0], want[:, 1], d, z], 1), case + ': NaN probes', lambda j: 'NaN at element %d' % idx[j, 0])
    pc.gd.check_untouched(case)


@pytest.mark.parametrize('shape', [(5, 7, 24), (300, 40), (20011, 1, 1)], ids=['rows-5x7x24', 'cols-300x40', 'tensor-20011'])
def test_float64_minmax(be, shape):
    """Section 4: tq_minmax_f64 -- mm_f64_rows_k, mm_f64_cols_k (inner == 1, n_params >= 32), mm_f64_final_k; full sweeps."""
    pc = _PerParameter(shape, torch.float64, seed=11)
    cols = pc.inner == 1 and pc.P >= 32                                       # mm_plan_f64 (csrc/tq_double.hip)
    assert cols == (shape == (300, 40))
    bx = _ceil_div(pc.P, 32) if cols else pc.P
    slices = max(1, min(max(1, 2048 // max(1, min(bx, 2048))), max(1, pc.outer * pc.inner * (32 if cols else 1) // 4096), pc.outer, 1024))
    assert slices == {(5, 7, 24): 1, (300, 40): 2, (20011, 1, 1): 4}[shape], slices
    assert be.lib.tq_minmax_f64_workspace_bytes(pc.x.numel(), pc.P, pc.inner) == pc.P * slices * 16
    positions = list(range(pc.L))
    idx, val, want = pc.sweep_plan(positions)
    pc.anchor(idx, val, want, 1)

    def launch(k):
        mn, mx = be.minmax(pc.x, pc.P, pc.inner)
        return torch.stack([mn.reshape(-1), mx.reshape(-1)])

    got = torch.stack(pc.gd.sweep(idx, val, launch))
    assert got.dtype == torch.float64
    _assert_bits(got, want, '%r: planted extremes (launch, min | max, parameter)' % (shape,))
    idx, val, want = pc.nan_plan([pc.L - 1])
    pc.anchor(idx, val, want, 0)
    got = torch.stack(pc.gd.sweep(idx, val, launch))
    _assert_bits(got, want, '%r: NaN probe' % (shape,))
    pc.gd.check_untouched(str(shape))
