"""Vocabulary of the integer route's host code (quantization/fused.py, QuantLinear._int8_* in autoquant_utils.py): what a
helper decides on and what it hands to the backend, as named values.  No torch modules and no launches live here.

Everything is a `typing.NamedTuple`: the backend and its test doubles keep splatting and indexing these values
(`self._qdesc(*q, 1, 1)`, `q[0].numel()`, `x_q[2]`).  An encoder layer builds ~30 per eager forward (cProfile), so every
hot constructor goes to `tuple.__new__`: 0.24 us against 0.40 us through NamedTuple's own `__new__` (timeit, CPython 3.10)."""
from typing import Any, NamedTuple

from quantization import provenance

_new = tuple.__new__


class QSpec(NamedTuple):
    """A fixed quantizer as the backend takes it, in the parameter order of `HipBackend._qdesc`.  delta / zero_float: the
    quantizer's own buffers -- one element, or one per column of a row (flattened; `zero_float` None for a symmetric one)."""
    delta: Any
    zero_float: Any
    signed: Any
    n_bits: int
    symmetric: bool
    log_domain: bool
    eps: float

    @classmethod
    def of(cls, q):
        return _new(cls, (q._delta, q._zero_float, getattr(q, '_signed', None), q.n_bits, q.symmetric, q.scale_domain == 'log',
                          q.eps))

    @classmethod
    def index_grid(cls, q):
        """the grid of a quantizer already known to be asymmetric and in the linear domain (see `emits_int8`)"""
        return _new(cls, (q._delta, q._zero_float, None, q.n_bits, False, False, q.eps))

    @property
    def fits_int8(self):
        """asymmetric, linear domain, at most 8 bits: the grid whose indices fit int8"""
        return not (self.symmetric or self.log_domain or self.n_bits > 8)


class XGrid(NamedTuple):
    """The grid under the int8 indices an integer Linear reads (asymmetric, linear domain)."""
    delta: Any
    zero_float: Any
    n_bits: int
    eps: float

    @classmethod
    def of(cls, q):
        return _new(cls, (q._delta, q._zero_float, q.n_bits, q.eps))

    @classmethod
    def of_spec(cls, spec):
        return _new(cls, (spec.delta, spec.zero_float, spec.n_bits, spec.eps))


# kinds of integer plan: which kernel evaluates the Linear (compared by identity)
TILED = 'tiled'    # per-tensor input grid of <= 8 bits, the tiled MFMA kernel (row tails padded by the backend: options.INT8_RAGGED)
PEG = 'peg'        # input on a per-embedding-group grid: the class-ordered kernel; the plan carries the class layout
MP16 = 'mp16'      # input on a per-tensor grid of 9..16 bits: two byte planes, tq_linear_i16x8_fwd
                   # (PEG and MP16: row tails padded by the backend under options.INT8_RAGGED_RECIPES)
SKINNY = 'skinny'  # a shape no tile covers (options.INT8_HEAD: tq_linear_i16x8_skinny_fwd; tq_linear_i8_skinny_fwd is that entry
                   # without planes and without a row table)


class IntPlan(NamedTuple):
    """How one QuantLinear is evaluated on the integer route: the quantizer that produced its input, its activation code,
    its output quantizer (None: pre-quantizer output) and the kernel.  Every kind but TILED is inference-only."""
    src: Any
    act: int
    q_out: Any                 # QSpec or None
    kind: str = TILED
    layout: Any = None         # class layout of a PEG plan


class IntOperands(NamedTuple):
    """Kernel operands of an integer Linear.  x_idx: int8 indices of the input -- of a 16-bit plan their high byte plane,
    with the low plane in x_lo; of a PEG plan in class order, like w_idx's columns and the per-class rowsum."""
    x_idx: Any
    x_lo: Any
    w_idx: Any
    rowsum: Any
    bias: Any
    x_q: XGrid
    w_delta: Any
    w_eps: float
    layout: Any = None

    @property
    def rows(self):
        return self.x_idx.numel() // self.w_idx.shape[-1]


def emits_int8(q):
    """Does a fixed per-tensor quantizer's output come with int8 indices?  (asymmetric, <= 8 bit; callers that consume the
    indices as a GRID add the linear scale domain themselves.)  q: a quantizer, or None for a site that is switched off."""
    return q is not None and not q.symmetric and q.n_bits <= 8


def emits_planes(q):
    """Does a fixed per-tensor quantizer's output lie on a grid whose indices a skinny launch can write as two byte planes?
    (asymmetric, linear domain, 9..16 bits: what the <= 8-bit grids of `emits_int8` leave to the 16-bit sites)"""
    return q is not None and not q.symmetric and 8 < q.n_bits <= 16 and q.scale_domain == 'linear'


def tagged(out, quantizer, want_idx, want_planes=False):
    """The end of a fused launch: `out` is (y, idx) with want_idx, (y, (hi, lo)) with want_planes, else y; y leaves with the
    record of the quantizer that produced it (None: the site is switched off, no record)."""
    y, idx = out if (want_idx or want_planes) else (out, None)
    if quantizer is not None:
        if want_planes:
            provenance.tag(y, quantizer, None, planes=idx)
        else:
            provenance.tag(y, quantizer, idx)
    return y
