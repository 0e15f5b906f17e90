"""Class layout of per-embedding-group activation grids (quantization/peg.py): host logic, no GPU."""
import numpy as np
import torch

from quantization import peg


def test_contiguous_groups():
    d = np.repeat(np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6]), 128)
    z = np.repeat(np.float32([1, 2, 3, 4, 5, 6]), 128)
    order, ends, reps = peg.classes_from_params(d, z)
    assert np.array_equal(order, np.arange(768))
    assert ends == [128, 256, 384, 512, 640, 768]
    assert reps == [0, 128, 256, 384, 512, 640]


def test_permuted_groups():
    rng = np.random.default_rng(0)
    cls = rng.permutation(np.repeat(np.arange(6), 128))
    d = np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])[cls]
    z = np.float32([9, 8, 7, 6, 5, 4])[cls]
    order, ends, reps = peg.classes_from_params(d, z)
    assert ends == [128, 256, 384, 512, 640, 768]
    # class c = c-th class by first column; its columns ascending, the representative its first column
    firsts = sorted({int(np.flatnonzero(cls == k)[0]) for k in range(6)})
    assert reps == firsts
    for c, (s, e) in enumerate(zip([0] + ends[:-1], ends)):
        cols = order[s:e]
        assert np.all(np.diff(cols) > 0) and cols[0] == reps[c]
        assert len({(float(d[k]), float(z[k])) for k in cols}) == 1
    assert sorted(order.tolist()) == list(range(768))


def test_equal_groups_merge():
    d = np.repeat(np.float32([0.1, 0.2, 0.1, 0.3, 0.2, 0.3]), 128)
    z = np.repeat(np.float32([1, 2, 1, 3, 2, 3]), 128)
    order, ends, reps = peg.classes_from_params(d, z)
    assert ends == [256, 512, 768] and reps == [0, 128, 384]
    assert np.array_equal(order[:256], np.r_[0:128, 256:384])


def test_same_delta_other_zero_point_is_another_class():
    d = np.full(256, 0.1, np.float32)
    z = np.repeat(np.float32([1, 2]), 128)
    assert peg.classes_from_params(d, z)[1] == [128, 256]


def test_per_embedding_grid_declines():
    d = np.linspace(0.01, 0.5, 768).astype(np.float32)
    z = np.zeros(768, np.float32)
    assert peg.classes_from_params(d, z) is None


def test_class_size_not_a_multiple_of_128_declines():
    d = np.repeat(np.float32([0.1, 0.2, 0.3]), 256)
    d[:64] = 0.4                                     # 64 + 192 + 256 + 256
    z = np.zeros(768, np.float32)
    assert peg.classes_from_params(d, z) is None
    d = np.repeat(np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]), 96)     # PEG 8 on 768: 96 per group
    assert peg.classes_from_params(d, np.zeros(768, np.float32)) is None


class _Q(torch.nn.Module):
    """the parts of an asymmetric quantizer class_layout reads"""

    def __init__(self, d, z):
        super().__init__()
        self.register_buffer('_delta', torch.tensor(d).reshape(1, 1, -1))
        self.register_buffer('_zero_float', torch.tensor(z).reshape(1, 1, -1))
        self._range_gen = 0
        self.n_bits = 8
        self.eps = 1e-8

    def range_state_key(self):
        return (self._range_gen, self._delta._version, self.n_bits)


def test_layout_is_cached_and_follows_range_changes():
    d = np.repeat(np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6]), 128)
    z = np.repeat(np.float32([1, 2, 3, 4, 5, 6]), 128)
    q = _Q(d, z)
    a = peg.class_layout(q, 768)
    assert a is not None and a.n_classes == 6 and a.identity
    assert peg.class_layout(q, 768) is a                         # cached: no second host read
    assert peg.class_layout(q, 512) is None                      # another row length
    with torch.no_grad():
        q._delta[..., 128:256] = 0.1                             # in-place range change: classes 0 and 1 merge
    b = peg.class_layout(q, 768)
    assert b is not a and b.n_classes == 6                       # zero points still differ
    with torch.no_grad():
        q._zero_float[..., 128:256] = 1.0                        # only the zero point moves: still noticed
    c = peg.class_layout(q, 768)
    assert c is not b and c.n_classes == 5 and c.ends[0] == 256
    q._delta = torch.linspace(0.01, 0.5, 768).reshape(1, 1, -1)  # rebinding to a per-embedding grid
    q._range_gen += 1
    assert peg.class_layout(q, 768) is None


def test_per_tensor_quantizer_has_no_layout():
    q = _Q(np.float32([0.1]), np.float32([3]))
    assert peg.class_layout(q, 768) is None
