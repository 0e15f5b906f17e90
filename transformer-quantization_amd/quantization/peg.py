"""Class layout of a per-embedding-group (PEG) activation grid for the integer Linear (tq_linear_i8_cls_fwd).

A PEG quantizer on a [.., d] activation holds per-column buffers _delta[d] / _zero_float[d] that take only a few distinct
value pairs (contiguous runs of columns without permutation, scattered columns with it).  A CLASS is the set of columns
that share one raw (delta, zero_float) pair.  The classes are derived from the quantizer's own buffers, not from its
estimator: the route is then correct whatever set the range, and two groups that happen to get equal parameters form one
class (merging them changes nothing in the arithmetic).

This module is the one place that owns the layout: the column order (class by class, each class's columns ascending),
the class boundaries in that order and one representative column per class.  It is derived with ONE device-to-host read
per range state of the quantizer and cached on it.  Layouts the kernel does not take -- a class whose size is not a
multiple of 128 columns, more than CLS_MAX classes (per-embedding grids have d of them) -- are None from `class_layout`;
`padded_class_layout` answers the first kind with every class padded to whole 128-column slabs (PaddedClassLayout).

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


class PaddedClassLayout(ClassLayout):
    """A class layout whose classes were padded to whole K slabs: `order` has one entry per class-ordered column of the PADDED
    operands (a pad column repeats its class's representative column), `pad` marks the pad columns.  The consumer zeroes the
    weight indices of the pad columns, so whatever index the input holds there contributes 0 to the class's integer sum and to
    its row sum: the class sums, and with them every fp32 operation behind them, are those of the unpadded classes."""
    __slots__ = ('pad',)

    def __init__(self, key, order, ends, reps, pad):
        super().__init__(key, order, ends, reps)
        self.pad = pad

    @property
    def identity(self):
        return False

    def pad_on(self, device):
        t = self._dev.get(('pad', device))
        if t is None:
            t = self._dev[('pad', device)] = torch.from_numpy(self.pad).to(device)
        return t


def padded_classes_from_params(delta, zero_float, multiple=CLS_MULTIPLE, max_classes=CLS_MAX):
    """(order, ends, reps, pad) of the classes of raw per-column parameter arrays with every class padded up to a multiple of
    `multiple` columns, or None (more than max_classes classes)."""
    found = classes_from_params(delta, zero_float, multiple=1, max_classes=max_classes)
    if found is None:
        return None
    order, ends, reps = found
    new_order, pad, new_ends, s = [], [], [], 0
    for e, r in zip(ends, reps):
        n = e - s
        m = -(-n // multiple) * multiple
        new_order += [order[s:e], np.full(m - n, r, dtype=np.int64)]
        pad += [np.zeros(n, dtype=bool), np.ones(m - n, dtype=bool)]
        new_ends.append((new_ends[-1] if new_ends else 0) + m)
        s = e
    return np.concatenate(new_order), new_ends, reps, np.concatenate(pad)


def padded_class_layout(q, d):
    """`class_layout` for grids whose classes are no multiple of 128 columns (64- or 192-column groups): the classes padded to
    whole K slabs (PaddedClassLayout), or None.  The plain layout where it exists.  Cached on `q` like the class layout."""
    layout = class_layout(q, d)
    if layout is not None:
        return layout
    delta = getattr(q, '_delta', None)
    zf = q._buffers.get('_zero_float') if hasattr(q, '_buffers') else None
    if delta is None or zf is None or delta.numel() != d or d <= 1 or zf.numel() != d or delta.shape[-1] != d:
        return None
    key = layout_key(q)
    cached = q.__dict__.get('_peg_padded_layout')
    if cached is not None and cached[0] == key:
        return cached[1]
    host = torch.stack([delta.detach().reshape(-1).float(), zf.detach().reshape(-1).float()]).cpu().numpy()
    found = padded_classes_from_params(host[0], host[1])
    layout = None if found is None else PaddedClassLayout(key, *found)
    q.__dict__['_peg_padded_layout'] = (key, layout)
    return layout


# ---- block-constant output grids (tq_linear_i8_cls_grouped_fwd, per-head grids of the attention core) --------------------
BLOCK_WIDTHS = (128, 64)     # tile widths of the integer Linear: a q_block is the widest of these the buffers allow


def widest_constant_block(delta, zero_float, widths=BLOCK_WIDTHS):
    """The widest w in `widths` such that the raw per-column parameter arrays are constant (fp32 bit patterns) over every
    ALIGNED block of w columns -- columns [j w, (j + 1) w) --, or None (also when w does not divide the column count)."""
    d = np.ascontiguousarray(np.asarray(delta, dtype=np.float32).reshape(-1)).view(np.uint32)
    z = np.ascontiguousarray(np.asarray(zero_float, dtype=np.float32).reshape(-1)).view(np.uint32)
    if d.size != z.size or d.size == 0:
        return None
    for w in sorted(widths, reverse=True):
        if d.size % w:
            continue
        db, zb = d.reshape(-1, w), z.reshape(-1, w)
        if np.array_equal(db, np.broadcast_to(db[:, :1], db.shape)) and np.array_equal(zb, np.broadcast_to(zb[:, :1], zb.shape)):
            return w
    return None


def constant_over(delta, zero_float, w):
    """Whether the raw per-column parameter arrays are constant over every aligned block of w columns (a head of the
    attention core: w = head_dim)"""
    return widest_constant_block(delta, zero_float, widths=(int(w),)) == int(w)


class BlockLayout:
    """block: the widest of BLOCK_WIDTHS over whose aligned blocks the quantizer's per-column buffers are constant, or None;
    `constant_over(w)` answers the same for another width (memoised); key: the range state it was derived for."""
    __slots__ = ('key', 'block', '_host', '_over')

    def __init__(self, key, host):
        self.key, self._host, self._over = key, host, {}
        self.block = widest_constant_block(host[0], host[1])

    def constant_over(self, w):
        w = int(w)
        if w not in self._over:
            self._over[w] = constant_over(self._host[0], self._host[1], w)
        return self._over[w]


def block_layout(q, d):
    """BlockLayout of the asymmetric per-column quantizer `q` for activations of row length `d`, or None (per-tensor, not
    along the last dimension).  One host read per range state, cached on `q` under `layout_key` like the class layout."""
    delta = getattr(q, '_delta', None)
    zf = q._buffers.get('_zero_float') if hasattr(q, '_buffers') else None
    if delta is None or zf is None or delta.numel() != d or d <= 1 or zf.numel() != d or delta.shape[-1] != d:
        return None
    key = layout_key(q)
    cached = q.__dict__.get('_peg_blocks')
    if cached is not None and cached[0] == key:
        return cached[1]
    host = torch.stack([delta.detach().reshape(-1).float(), zf.detach().reshape(-1).float()]).cpu().numpy()
    layout = BlockLayout(key, host)
    q.__dict__['_peg_blocks'] = (key, layout)
    return layout
