"""Which quantizer produced this tensor -- and, if the producing kernel emitted them, its int8 grid indices.

The integer fast paths (MFMA Linear, integer attention core, fused tails; `options.INT8_LINEAR`) consume activations as
int8 grid indices.  A consumer may only do so if it KNOWS the tensor lies on a fixed per-tensor grid: that knowledge is
recorded here by the producer (`tag`) and looked up by the consumer (`of`), in one explicit table instead of ad-hoc
tensor attributes:

    record = (quantizer, idx)      quantizer: the fixed-range quantizer whose grid the values lie on
                                   idx: int8(index - 128) of the same shape, or None (the consumer re-derives them
                                        exactly with one tq_fake_quant_fwd index-only launch)
    (+ row_nan)                    optional uint8, one per row (all dimensions but the last): 1 where the row is NaN as a
                                   whole -- its idx bytes mean nothing -- and 0 elsewhere; None: no flags known.  Only a
                                   consumer that reads the INDICES in place of the values needs them (`row_nan_of`;
                                   options.INT8_INDEX_RESIDUALS), `of` keeps answering (quantizer, idx).
    (+ planes)                     optional (hi, lo): the two int8 byte planes of the indices of a 9..16-bit grid, 256 (hi + 128)
                                   + (lo + 128) == index, where the producing launch wrote them (the skinny pooler under
                                   options.INT8_HEAD); read with `planes_of`.  idx stays None for such a tensor.

Records are keyed by tensor OBJECT identity and die with the tensor (weak references).  Anything that makes a new
tensor object -- a view, `.contiguous()`, dropout, an arithmetic op -- has no record, and the consumer takes the
layered path (always correct, only slower).  That is the intended safety property, not an accident: values are trusted
to be on-grid only for the very object the quantizer kernel returned -- and only while that object is UNCHANGED: a
record also carries the tensor's version counter (any in-place op: `add_`, in-place dropout, `copy_`) and the range
state of the producing quantizer (a range re-set between producer and consumer), and is ignored once either moved.
"""
import weakref

import torch

_records = {}


def version_of(tensor):
    """The tensor's in-place modification counter, or None where torch does not keep one (inference tensors)."""
    try:
        return tensor._version
    except RuntimeError:
        return None


def tag(tensor, quantizer, idx=None, row_nan=None, planes=None):
    """Record that `tensor` was produced by `quantizer` (fixed range); returns the tensor.  row_nan: the NaN flags of its rows,
    planes: the byte planes of its wide indices, where the producing launch wrote them.  A tensor without a version
    counter (created under torch.inference_mode()) gets NO record: an in-place change could not be detected later, so its
    consumers take the layered path."""
    key = id(tensor)
    if version_of(tensor) is None:
        _records.pop(key, None)
        return tensor

    def _drop(_ref, key=key):
        _records.pop(key, None)
    _records[key] = (weakref.ref(tensor, _drop), quantizer, idx, tensor._version, _range_state(quantizer), row_nan, planes)
    return tensor


def forget(tensor):
    """Drop the record of `tensor`, if any: its consumers take the layered path (always correct).  Returns the tensor."""
    _records.pop(id(tensor), None)
    return tensor


def _range_state(quantizer):
    key = getattr(quantizer, 'range_state_key', None)
    return key() if key is not None else None


def of(tensor):
    """(quantizer, idx | None) recorded for this tensor object, or None (no record, or a stale one)."""
    rec = _records.get(id(tensor))
    if rec is None or rec[0]() is not tensor:
        return None
    if version_of(tensor) != rec[3] or _range_state(rec[1]) != rec[4]:
        return None                          # modified in place / producer's grid changed since the record was made
    return rec[1], rec[2]


def quantizer_of(tensor):
    rec = of(tensor)
    return None if rec is None else rec[0]


def indices_of(tensor):
    rec = of(tensor)
    return None if rec is None else rec[1]


def row_nan_of(tensor):
    """uint8 NaN flags of the tensor's rows as its producer wrote them, or None: no (valid) record, or one without flags --
    "no flags known", which is not "no NaN rows"."""
    rec = _records.get(id(tensor))
    if rec is None or of(tensor) is None:
        return None
    return rec[5]


def planes_of(tensor):
    """(hi, lo) int8 byte planes of the tensor's indices as its producer wrote them, or None: no (valid) record, or one
    without planes."""
    rec = _records.get(id(tensor))
    if rec is None or of(tensor) is None:
        return None
    return rec[6]


def planes_like(tensor):
    """`planes_of(tensor)` where it holds two contiguous int8 tensors of the tensor's own shape (what a consumer reads in
    place of the values, element for element), else None."""
    planes = planes_of(tensor)
    if planes is None or len(planes) != 2:
        return None
    for p in planes:
        if p is None or p.dtype != torch.int8 or p.shape != tensor.shape or not p.is_contiguous():
            return None
    return planes
