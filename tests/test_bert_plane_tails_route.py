"""options.INT8_PLANE_TAILS on the GPU: a 3-layer BERT under the mixed-precision recipe {'x': 16, 'h': 16, 'y': 16} whose
attention-output tails write the byte planes of site x (tq_residual_layernorm_quant_planes_fwd) equals the exact CPU twin
(tests/_planes_twin.PlanesTwin) at zero tolerance -- the embedding block's output, site x and the hidden state of every layer,
with the int8 index records of the 8-bit tensors and the plane records of x -- eager and as a hipGraph replay, with the same
launches on both sides; and it equals the same model with the switch off.  With a 16-bit last hidden state (site z of the
last layer) and options.INT8_HEAD the pooler reads the first-token rows of the planes and the LOGITS equal the twin's, also
through `forward_packed`.  One run with options.INT8_INDEX_RESIDUALS on as well equals the run with every switch off."""
import pytest
import torch

from tests.test_bert_exact_route import _HIP_CENSUS, _calibrate, _expected_census, _ids, _twin_of

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]

LAYERS = 3
ENCODER = {'x': 16, 'h': 16, 'y': 16}
RECIPES = {'mp16': ENCODER, 'head': dict(ENCODER, **{'z%d' % (LAYERS - 1): 16, 'P': 16, 'C': 16})}
NEW, HILO, TAIL, SKINNY16 = 'residual_layernorm_quant_planes', 'quantize_hilo', 'residual_layernorm_quant', 'linear_i16x8_skinny'
_GPU = {}


def _gpu_model(recipe, B, T):
    from quantization import options
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    if (recipe, B, T) not in _GPU:
        assert not (options.INT8_PLANE_TAILS or options.INT8_HEAD or options.INT8_RAGGED or options.INT8_INDEX_RESIDUALS)
        qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
                  weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
        model, _ = build_bert_base(seed=1000, num_layers=LAYERS, **qp)
        apply_quant_dict(model, RECIPES[recipe])
        _GPU[(recipe, B, T)] = _calibrate(model.to('cuda').eval(), 'mp16', [_ids(10, B, T).cuda(), _ids(11, B, T).cuda()])
    return _GPU[(recipe, B, T)]


def _mask(B, T):
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return am


class _Sites:
    """the embedding block's output, site x and the hidden state of every layer of every forward while installed, each with
    the int8 indices and the byte planes its record holds (instance-level wrappers: a module hook would be an observer)"""

    def __init__(self, model):
        self.model, self.runs = model, []

    def _wrap(self, mod, key):
        from quantization import provenance
        f = type(mod).forward

        def forward(*a, **k):
            y = f(mod, *a, **k)
            self.runs[-1].setdefault(key, []).append((y, provenance.indices_of(y), provenance.planes_of(y)))
            return y
        mod.forward = forward

    def __enter__(self):
        m = self.model
        self._mods = [m.embeddings] + [L.attention_output for L in m.layers] + list(m.layers) + [m]
        self._wrap(m.embeddings, 'emb')
        for L in m.layers:
            self._wrap(L.attention_output, 'x')
            self._wrap(L, 'h')
        top = type(m).forward

        def whole(*a, **k):
            self.runs.append({})
            return top(m, *a, **k)
        m.forward = whole
        return self

    def __exit__(self, *exc):
        for mod in self._mods:
            del mod.forward
        return False


def _host(run):
    cp = lambda t: None if t is None else t.detach().cpu().clone()
    return {k: [(cp(y), cp(i), None if p is None else tuple(cp(t) for t in p)) for y, i, p in v] for k, v in run.items()}


def _hip_log(monkeypatch):
    """launches of the HIP backend in the form the twins record their own"""
    from quantization import _hip
    from tests._skinny16_twin import count_hip_launches
    log = count_hip_launches(monkeypatch)
    info = dict(_HIP_CENSUS)
    info[NEW] = lambda a, k: (tuple(a[0].shape), int(a[7][3]))
    for name, fn in info.items():
        orig = getattr(_hip.HipBackend, name)

        def counted(self, *a, _o=orig, _n=name, _i=fn, **k):
            log.append((_n,) + _i(a, k))
            return _o(self, *a, **k)
        monkeypatch.setattr(_hip.HipBackend, name, counted)
    return log


def _twin_backend(rules):
    from tests._packed_twin import PackedTwin
    from tests._planes_twin import PlanesTwin

    class PackedPlanesTwin(PackedTwin, PlanesTwin):
        name = 'exact-twin-packed-planes'
    return PackedPlanesTwin(rules=rules)


def _on_twin(twin, be, call, sites=True):
    """call(twin) under the CPU backend `be`, no grad -> (logits, sites record or None, census)"""
    from quantization import _hip
    prev = _hip.set_backend(be)
    try:
        del be.census[:]
        with torch.no_grad():
            if sites:
                with _Sites(twin) as cap:
                    logits = call(twin)
                rec = _host(cap.runs[-1])
            else:
                logits, rec = call(twin), None
        return logits.detach().clone(), rec, list(be.census)
    finally:
        _hip.set_backend(prev)


def _assert_tables_accepted(model):
    """premise of a zero-tolerance comparison behind a GELU launch (tests/test_bert_exact_route.py): every feed-forward launch
    evaluates the correctly rounded GELU through an accepted staircase table"""
    from quantization.autoquant_utils import int8_stair_status
    status = int8_stair_status(model)
    for l in range(LAYERS):
        tables = status.get(f'layers.{l}.intermediate.0', {})
        assert tables and all(tables.values()), f'layer {l}: GELU table declined or absent ({tables}): no exact statement possible'


def _equal_sites(got, want, what):
    for where in ('emb', 'x', 'h'):
        assert len(got[where]) == len(want[where]) == (1 if where == 'emb' else LAYERS)
        for l, ((y, i, p), (ty, ti, tp)) in enumerate(zip(got[where], want[where])):
            at = f'{what}: {where} {l}'
            assert torch.equal(y.view(torch.int32), ty.view(torch.int32)), f'{at}: values differ ({int((y != ty).sum())} elements)'
            assert (i is None) == (ti is None) and (i is None or torch.equal(i, ti)), f'{at}: int8 index records differ'
            assert (p is None) == (tp is None), f'{at}: one side has a plane record, the other has none'
            if p is not None:
                keep = ~torch.isnan(ty).any(-1)
                assert torch.equal(p[0][keep], tp[0][keep]) and torch.equal(p[1][keep], tp[1][keep]), f'{at}: plane records differ'


def _census_on(B, T, stair):
    out = []
    for c in _expected_census('mp16', LAYERS, B, T, stair=stair):
        if c[0] == HILO:
            continue
        out.append((NEW, c[1], 16) if c[0] == TAIL and c[2] is False else c)
    return out


@pytest.mark.parametrize('B,T', [(3, 64), (8, 128)])
def test_encoder_equals_the_twin_eager_and_replayed(B, T, monkeypatch):
    from quantization import _hip, options
    from quantization.graphs import GraphedForward
    assert options.INT8_LINEAR == 'auto' and options.INT8_PLANE_TAILS is False
    model = _gpu_model('mp16', B, T)
    ids, am = _ids(3, B, T), _mask(B, T)
    args = (ids.cuda(), am.cuda())
    twin = _twin_of(model)
    log = _hip_log(monkeypatch)
    with torch.no_grad(), _Sites(model) as cap:
        off_logits = model(*args).clone()
        torch.cuda.synchronize()
        off, off_census = _host(cap.runs[-1]), list(log)
        del log[:]
        monkeypatch.setattr(options, 'INT8_PLANE_TAILS', True)
        on_logits = model(*args).clone()
        torch.cuda.synchronize()
        on, census = _host(cap.runs[-1]), list(log)
        del log[:]
        g = GraphedForward(model, *args)
        static = cap.runs[-1]                                   # the capture pass: the graph's own tensors
        graph_census = list(log)
        replay_logits = g(*args).clone()
        torch.cuda.synchronize()
        replay = _host(static)
    _assert_tables_accepted(model)
    stair = [c[-1] for c in census if c[0] == 'linear_i16x8']
    assert len(stair) == LAYERS and len(set(stair)) == 1
    # the launches: today's with the switch off; with it on no quantize_hilo, one plane tail and one 16-bit Linear per layer
    assert off_census == _expected_census('mp16', LAYERS, B, T, stair=stair[0]), off_census
    assert census == _census_on(B, T, stair[0]), census
    names = [c[0] for c in census]
    assert names.count(HILO) == 0 and names.count(NEW) == names.count('linear_i16x8') == LAYERS
    assert len(graph_census) % len(census) == 0 and graph_census == census * (len(graph_census) // len(census)), \
        'the launches of the graph\'s warm-up / capture passes differ from the eager forward\'s'
    # switch on == switch off on the GPU (records aside: x carries planes only with the switch on)
    assert torch.equal(on_logits, off_logits)
    for where in ('emb', 'x', 'h'):
        for l, (a, b) in enumerate(zip(on[where], off[where])):
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), f'switch on != switch off: {where} {l}'
            assert (a[1] is None) == (b[1] is None) and (a[1] is None or torch.equal(a[1], b[1]))
    assert all(p is not None and i is None for _, i, p in on['x']) and all(p is None for _, _, p in off['x'])
    # GPU == twin, eager and replayed
    be = _twin_backend(_hip.backend())
    _, chained, twin_census = _on_twin(twin, be, lambda m: m(ids, am))
    assert twin_census == census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    _equal_sites(on, chained, f'[{B},{T}] eager')
    _equal_sites(replay, chained, f'[{B},{T}] hipGraph replay')
    assert torch.equal(replay_logits, on_logits)
    assert all(torch.isfinite(y).all() for y, _, _ in on['h'])
    # the planes of x are its index: 256 (hi + 128) + (lo + 128) on the 16-bit grid, beyond what an int8 tensor holds
    hi, lo = on['x'][0][2]
    assert int((256 * (hi.int() + 128) + lo.int() + 128).max()) > 255


def test_with_index_residuals_on_as_well_equals_every_switch_off(monkeypatch):
    from quantization import options
    B, T = 3, 64
    model = _gpu_model('mp16', B, T)
    args = (_ids(3, B, T).cuda(), _mask(B, T).cuda())
    log = _hip_log(monkeypatch)
    with torch.no_grad(), _Sites(model) as cap:
        ref_logits = model(*args).clone()
        ref = _host(cap.runs[-1])
        del log[:]
        monkeypatch.setattr(options, 'INT8_PLANE_TAILS', True)
        monkeypatch.setattr(options, 'INT8_INDEX_RESIDUALS', True)
        logits = model(*args).clone()
        torch.cuda.synchronize()
        got = _host(cap.runs[-1])
    assert [c[0] for c in log].count(NEW) == LAYERS and HILO not in [c[0] for c in log]
    assert torch.equal(logits, ref_logits)
    for where in ('emb', 'x', 'h'):
        assert all(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) for a, b in zip(got[where], ref[where])), where


LENGTHS = (64, 40, 24)            # B = 3, T = 64; 128 packed rows: every Linear keeps whole tiles in both forms


def test_head_logits_equal_the_twin_padded_and_packed(monkeypatch):
    """site z of the last layer at 16 bits, 'P' and 'C' at 16 bits, options.INT8_HEAD: the last feed-forward tail writes the
    planes of the hidden state and the pooler reads its first-token rows -- strided views of a padded batch, a row table of a
    packed one"""
    from harness.bert import pack_batch
    from quantization import _hip, options
    from tests.test_bert_packed_route import _batch
    B, T, D = len(LENGTHS), max(LENGTHS), 768
    model = _gpu_model('head', B, T)
    ids, am = _batch(LENGTHS)
    p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
    p_args = tuple(t.cuda() for t in (p_ids, p_pos, seq_start))
    twin = _twin_of(model)
    log = _hip_log(monkeypatch)
    monkeypatch.setattr(options, 'INT8_HEAD', True)
    with torch.no_grad():
        layered = model(ids.cuda(), am.cuda()).cpu().clone()              # the tail switch off: the head stays layered
        assert not any(c[0] == SKINNY16 for c in log)
        del log[:]
        monkeypatch.setattr(options, 'INT8_PLANE_TAILS', True)
        logits = model(ids.cuda(), am.cuda()).cpu().clone()
        torch.cuda.synchronize()
        census = list(log)
        del log[:]
        monkeypatch.setattr(options, 'INT8_RAGGED', True)
        padded = model(ids.cuda(), am.cuda()).cpu().clone()
        del log[:]
        packed = model.forward_packed(*p_args, max_len).cpu().clone()
        torch.cuda.synchronize()
        packed_census = list(log)
    _assert_tables_accepted(model)
    head = [(SKINNY16, B, D, D, 3, (T * D, 1), True, False, True, 'planes', True), (SKINNY16, B, 2, D, 0, (D, 1), True, False, True, 'y', True)]
    assert census[-2:] == head and [c[0] for c in census].count(NEW) == LAYERS + 1 and HILO not in [c[0] for c in census]
    assert packed_census[-2:] == [(SKINNY16, B, D, D, 3, (D, 1), True, True, True, 'planes', True), head[1]], packed_census[-2:]
    be = _twin_backend(_hip.backend())
    monkeypatch.setattr(options, 'INT8_RAGGED', False)                    # the switches of the forward `census` was taken from
    t_logits, _, t_census = _on_twin(twin, be, lambda m: m(ids, am), sites=False)
    assert t_census == census, [(i, a, b) for i, (a, b) in enumerate(zip(census, t_census)) if a != b][:4]
    assert torch.equal(logits, t_logits), f'logits differ from the twin\'s: {(logits - t_logits).abs().max()}'
    assert torch.equal(padded, logits), 'the padded logits moved with INT8_RAGGED'
    assert torch.equal(packed, padded), f'packed logits differ from the padded forward\'s: {(packed - padded).abs().max()}'
    assert logits.shape == (B, 2) and torch.isfinite(logits).all() and torch.isfinite(layered).all()
