"""Class layout of a per-embedding-group (PEG) activation grid for the integer Linear (tq_linear_i8_cls_fwd).

A PEG quantizer on a [.., d] activation holds per-column buffers _delta[d] / _zero_float[d] that take only a few distinct
value pairs (contiguous runs of columns without permutation, scattered columns with it).  A CLASS is the set of columns
that share one raw (delta, zero_float) pair.  The classes are derived from the quantizer's own buffers, not from its
estimator: the route is then correct whatever set the range, and two groups that happen to get equal parameters form one
class (merging them changes nothing in the arithmetic).

This module is the one place that owns the layout: the column order (class by class, each class's columns ascending),
the class boundaries in that order and one representative column per class.  It is derived with ONE device-to-host read
per range state of the quantizer and cached on it.  Layouts the kernel does not take -- a class whose size is not a
multiple of 128 columns, more than CLS_MAX classes (per-embedding grids have d of them) -- are None.

Column order of indices, by design: indices recorded on a tensor (quantization/provenance.py) are always in NATURAL
column order -- every producer writes them so -- and class-ordered indices are never recorded.  The consumer,
QuantLinear._int8_cls_operands, reorders the natural-order indices into a temporary that never leaves the call, so no
tag is needed to tell the two orders apart: a class-ordered tensor cannot reach another consumer.
"""
import numpy as np
import torch

CLS_MULTIPLE = 128       # K slab of the LDS-tiled integer Linear: a class flush happens between slabs
CLS_MAX = 24             # TQ_CLS_MAX of include/tq_hip.h


class ClassLayout:
    """order: natural-order column of every class-ordered column (int64 numpy); ends: class-ordered column one past each
    class; reps: one natural-order column per class; key: the range state it was derived for."""
    __slots__ = ('key', 'order', 'ends', 'reps', '_dev', '_table')

    def __init__(self, key, order, ends, reps):
        self.key, self.order, self.ends, self.reps = key, order, tuple(ends), tuple(reps)
        self._dev, self._table = {}, None

    @property
    def n_classes(self):
        return len(self.ends)

    @property
    def identity(self):
        return bool(np.array_equal(self.order, np.arange(self.order.size)))

    def order_on(self, device):
        """The column order as an int64 tensor on `device` (cached per device)."""
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = torch.from_numpy(self.order).to(device)
        return t

    def table(self, be):
        """The backend's host table of this layout (built once)."""
        if self._table is None:
            self._table = be.cls_table(self.ends, self.reps)
        return self._table


def layout_key(q):
    """Cache key of a quantizer's class layout: its range state plus the version of `_zero_float` (an in-place change of
    the zero point moves neither `_range_gen` nor `_delta._version`) and eps."""
    zf = q._buffers.get('_zero_float') if hasattr(q, '_buffers') else None
    return (q.range_state_key(), None if zf is None else zf._version, q.eps)


def classes_from_params(delta, zero_float, multiple=CLS_MULTIPLE, max_classes=CLS_MAX):
    """(order, ends, reps) of the classes of raw per-column parameter arrays, or None when the layout is unsupported.
    Classes are numbered in the order of their first column; equality is on the fp32 bit patterns."""
    d = np.ascontiguousarray(np.asarray(delta, dtype=np.float32).reshape(-1)).view(np.uint32)
    z = np.ascontiguousarray(np.asarray(zero_float, dtype=np.float32).reshape(-1)).view(np.uint32)
    if d.size != z.size or d.size == 0:
        return None
    pairs = (d.astype(np.uint64) << np.uint64(32)) | z.astype(np.uint64)
    _, first, inverse = np.unique(pairs, return_index=True, return_inverse=True)
    if first.size > max_classes:
        return None
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(first.size)       # class number = order of first appearance
    cls_of_col = rank[inverse.reshape(-1)]
    order = np.argsort(cls_of_col, kind='stable').astype(np.int64)
    sizes = np.bincount(cls_of_col, minlength=first.size)
    if np.any(sizes % multiple):
        return None
    ends = np.cumsum(sizes)
    reps = np.sort(first)
    return order, [int(e) for e in ends], [int(r) for r in reps]


def class_layout(q, d):
    """ClassLayout of the asymmetric per-column quantizer `q` for activations of row length `d`, or None (per-tensor,
    not along the last dimension, unsupported class sizes or count).  One host read per range state, cached on `q`."""
    delta = getattr(q, '_delta', None)
    zf = q._buffers.get('_zero_float') if hasattr(q, '_buffers') else None
    if delta is None or zf is None or delta.numel() != d or d <= 1 or zf.numel() != d or delta.shape[-1] != d:
        return None
    key = layout_key(q)
    cached = q.__dict__.get('_peg_layout')
    if cached is not None and cached[0] == key:
        return cached[1]
    host = torch.stack([delta.detach().reshape(-1).float(), zf.detach().reshape(-1).float()]).cpu().numpy()
    found = classes_from_params(host[0], host[1])
    layout = None if found is None else ClassLayout(key, *found)
    q.__dict__['_peg_layout'] = (key, layout)
    return layout
