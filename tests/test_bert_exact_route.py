"""Whole-model exactness: BERT's default route (options.INT8_LINEAR = 'auto') on the GPU equals a CPU twin at ZERO tolerance.

The twin is the SAME host code (quantization/fused.py, autoquant_utils.py) on a deep copy of the calibrated model, with
tests/_exact_backend.ExactBackend installed: every entry point the route calls is answered by the specification its
kernel-level GPU test uses as reference (oracle/tq_int_oracle.c, oracle/tq_ln_oracle.c, the formulas of include/tq_hip.h).
What is compared per recipe the README advertises:

* chained: the twin runs from `input_ids` on its own; the embedding block's output and the hidden state after every encoder
  layer -- values and the int8 index tensors they carry -- are `torch.equal`;
* teacher-forced: each twin layer runs on the GPU's input to that layer (re-tagged through the producing quantizer, which is
  idempotent on its own grid) and is compared on its own: the localiser, whose message names the first differing layer.

Both sides must take the same launches (`INT8_STATS['kernel_calls']` and a per-method census), or the comparison says nothing.

OUTSIDE the claim: the logits.  The pooler and classifier see M = B rows, which no integer kernel tiles: they are fp32 GEMMs
(hipBLASLt on the GPU, ATen on the CPU) and differ by accumulation round-off; tests/test_bert_e2e.py bounds them.

GELU: a feed-forward launch whose staircase table the device builder ACCEPTED (header `ok`) evaluates the correctly rounded
GELU, which the twin evaluates directly (oracle activation code 4) -- exact.  A launch whose table was declined, or for which no
table fits, keeps the arithmetic epilogue; its specification (code 2) and the kernel differ in the hardware exp2 (<= 1 ulp), the
project's one documented exception (quantization/options.py INT8_ACT_STAIR, tests/test_int_oracle.py): for such a layer only
the teacher-forced comparison is kept, the attention block stays `torch.equal` and the layer's output indices may be at most 1
step apart on at most 2e-5 of its outputs.  Those layers are printed; no other tolerance exists in this file.

Twin cost, measured on the CPU (one thread runs the C oracle; torch threads only help the float64 matmuls of the
class-ordered / 16-bit Linears): see `test_twelve_layer_twin_forward_fits_the_suite_cpu`."""
import copy
import time

import pytest
import torch

from oracle import tq_oracle as O

GELU_FALLBACK_MAX_STEPS = 1          # options.py (INT8_ACT_STAIR note), tests/test_int_oracle.py: arithmetic epilogue vs code 2
GELU_FALLBACK_MAX_SHARE = 2e-5

RECIPES = {
    'w8a8': {},
    'peg': {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'},
    'peg_permuted': {'x': 'ngp6', 'h': 'ngp6', 'y': 'ngp6'},
    'mp16': {'x': 16, 'h': 16, 'y': 16},
}


# ---- models -----------------------------------------------------------------------------------------------------------------
def _model(recipe, num_layers, device):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests.harness_bert import apply_quant_dict, build_bert_base
    permuted = recipe == 'peg_permuted'
    # (range-sorted groups are collected by the current-min-max estimator only, as in the reference)
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax,
              act_range_method=RangeEstimators.current_minmax if permuted else RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=num_layers, **qp)
    apply_quant_dict(model, RECIPES[recipe])
    return model.to(device).eval()


def _calibrate(model, recipe, batches):
    from harness.bert import estimate_permutation_ranges
    from utils.utils import pass_data_for_range_estimation
    with torch.no_grad():
        if recipe == 'peg_permuted':
            estimate_permutation_ranges(model, [(b,) for b in batches])
        pass_data_for_range_estimation([(b,) for b in batches], model, act_quant=True, weight_quant=True,
                                       max_num_batches=len(batches))
        model.fix_ranges()
    return model


def _ids(seed, B=8, T=128):
    return torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(seed))


def _padded_mask(B, T):
    am = torch.ones(B, T, dtype=torch.long)
    am[1, 100:] = 0                                          # one padded sample
    return am


# ---- capture ----------------------------------------------------------------------------------------------------------------
class _Capture:
    """Output of the embedding block, of every layer's attention block and of every layer -- with the int8 indices each
    tensor carries -- through instance-level `forward` wrappers (module hooks would send the hooked blocks down the layered
    route).  Every forward while installed appends one record."""

    def __init__(self, model):
        self.model, self.runs = model, []

    def _wrap(self, mod, key):
        from quantization import provenance
        fwd = type(mod).forward

        def wrapped(*a, _m=mod, **k):
            y = fwd(_m, *a, **k)
            self.runs[-1].setdefault(key, []).append((y, provenance.indices_of(y)))
            return y
        mod.forward = wrapped

    def __enter__(self):
        m = self.model
        self._mods = [m.embeddings] + [L.attention_output for L in m.layers] + list(m.layers)
        self._wrap(m.embeddings, 'emb')
        for L in m.layers:
            self._wrap(L.attention_output, 'attn')
            self._wrap(L, 'h')
        top = type(m).forward

        def whole(*a, _m=m, **k):
            self.runs.append({})
            return top(_m, *a, **k)
        m.forward = whole
        self._mods.append(m)
        return self

    def __exit__(self, *exc):
        for mod in self._mods:
            del mod.forward
        return False


def _host(run):
    """a capture record as host tensors: {'emb' | 'attn' | 'h': [(values, indices)]}"""
    cp = lambda t: None if t is None else t.detach().cpu().clone()
    return {k: [(cp(y), cp(i)) for y, i in v] for k, v in run.items()}


# ---- launch census of the HIP backend, in the form ExactBackend records its own ------------------------------------------
_HIP_CENSUS = {
    'embeddings_layernorm_quant': lambda a, k: (tuple(a[1].shape), k.get('want_idx', False)),
    'linear_i8_grouped': lambda a, k: (tuple(a[0].shape), a[1].shape[0]),
    'attention_i8': lambda a, k: (tuple(a[0].shape),),
    'linear_i8': lambda a, k: (tuple(a[0].shape), a[1].shape[0], k.get('want_y', True), k.get('stair') is not None),
    'linear_i8_cls': lambda a, k: (tuple(a[0].shape), a[1].shape[0], k.get('want_y', True), k.get('stair') is not None),
    'linear_i16x8': lambda a, k: (tuple(a[0].shape), a[2].shape[0], k.get('want_y', True), k.get('stair') is not None),
    'quantize_hilo': lambda a, k: (tuple(a[0].shape),),
    'residual_layernorm_quant': lambda a, k: (tuple(a[0].shape), k.get('want_idx', False)),
    'residual_layernorm_quant_axis': lambda a, k: (tuple(a[0].shape), tuple(None if q is None else q[0].numel()
                                                                            for q in (a[2], a[3], a[7])), k.get('want_idx', False)),
}


def _hip_census(monkeypatch):
    from quantization import _hip
    log = []
    for name, info in _HIP_CENSUS.items():
        orig = getattr(_hip.HipBackend, name)

        def counted(self, *a, _o=orig, _n=name, _i=info, **k):
            log.append((_n,) + _i(a, k))
            return _o(self, *a, **k)
        monkeypatch.setattr(_hip.HipBackend, name, counted)
    return log


def _expected_census(recipe, layers, B, T, stair=True):
    """the launches of the default route per recipe (counts: tests/test_bert_e2e.py::test_bert_merged_launches_host_logic_cpu,
    tests/test_peg_tail_host.py, tests/test_mp16_route_host.py), in call order"""
    d, s = 768, (B, T, 768)
    out = [('embeddings_layernorm_quant', (B, T), True)]
    for _ in range(layers):
        out += [('linear_i8_grouped', s, 3 * d), ('attention_i8', s), ('linear_i8', s, d, True, False)]
        if recipe == 'w8a8':
            out += [('residual_layernorm_quant', s, True), ('linear_i8', s, 4 * d, False, stair)]
        elif recipe == 'mp16':
            out += [('residual_layernorm_quant', s, False), ('quantize_hilo', s), ('linear_i16x8', s, 4 * d, False, stair)]
        else:
            out += [('residual_layernorm_quant_axis', s, (1, 1, d), True), ('linear_i8_cls', s, 4 * d, False, stair)]
        out += [('linear_i8', (B, T, 4 * d), d, True, False)]
        out += [('residual_layernorm_quant_axis', s, (d, d, 1), True)] if recipe.startswith('peg') else \
               [('residual_layernorm_quant', s, True)]
    return out


# ---- the twin's forwards -----------------------------------------------------------------------------------------------------
def _twin_of(model):
    return copy.deepcopy(model).cpu()


def _twin_chained(twin, be, ids, attention_mask):
    from quantization import _hip
    from quantization.autoquant_utils import INT8_STATS
    prev = _hip.set_backend(be)
    try:
        del be.census[:]
        k0 = INT8_STATS['kernel_calls']
        t0 = time.perf_counter()
        with torch.no_grad(), _Capture(twin) as cap:
            twin(ids) if attention_mask is None else twin(ids, attention_mask)
        return _host(cap.runs[-1]), INT8_STATS['kernel_calls'] - k0, list(be.census), time.perf_counter() - t0
    finally:
        _hip.set_backend(prev)


def _additive_mask(attention_mask, B, T):
    if attention_mask is None:
        return torch.zeros(B, 1, 1, T)
    return (1.0 - attention_mask[:, None, None, :].float()) * -10000.0


def _twin_layer(twin, be, l, h_in, mask):
    """layer l of the twin on the given input: (attention block output, layer output), each (values, indices)"""
    from quantization import _hip, provenance
    producer = twin.embeddings.LayerNorm if l == 0 else twin.layers[l - 1].output.LayerNorm
    prev = _hip.set_backend(be)
    try:
        with torch.no_grad():
            x = producer.activation_quantizer(h_in.clone())          # idempotent on its own grid; tags x with its indices
            assert torch.equal(x, h_in), f'input of layer {l} does not lie on the grid of its producer'
            L, rec = twin.layers[l], {}
            block, fwd = L.attention_output, type(L.attention_output).forward

            def wrapped(*a, **k):
                rec['a'] = fwd(block, *a, **k)
                return rec['a']
            block.forward = wrapped
            try:
                y = L(x, mask)
            finally:
                del block.forward
            return (rec['a'], provenance.indices_of(rec['a'])), (y, provenance.indices_of(y))
    finally:
        _hip.set_backend(prev)


# ---- comparison --------------------------------------------------------------------------------------------------------------
def _grid_index(model_cpu, where, l, values):
    """grid indices of a hidden state from the quantizer that produced it (for tensors that carry no int8 tag: > 8 bits,
    per-column grids)"""
    mod = {'emb': model_cpu.embeddings.LayerNorm, 'attn': None if l is None else model_cpu.layers[l].attention_output.LayerNorm,
           'h': None if l is None else model_cpu.layers[l].output.LayerNorm}[where]
    q = mod.activation_quantizer.quantizer
    zf = q._zero_float
    n = q._delta.numel()
    flat = lambda t: t.detach().float().reshape(()) if n == 1 else t.detach().float().reshape(-1)
    return O.fake_quant(values.float(), flat(q._delta), flat(zf), q.n_bits, False, False, q.eps)[0]


def _report(what, got, want, got_idx, want_idx):
    """None when equal, else the localiser's message: differing elements, largest index distance, rows / columns affected"""
    same_v = torch.equal(got[0], want[0])
    same_i = (got[1] is None and want[1] is None) or (got[1] is not None and want[1] is not None and torch.equal(got[1], want[1]))
    if same_v and same_i:
        return None
    d = want[0].shape[-1]
    neq = (got[0] != want[0]).reshape(-1, d)
    dist = (got_idx - want_idx).abs().reshape(-1, d)
    return ('%s: %d of %d elements differ (%d int8 index tags differ), largest index distance %d, %.4f of the rows and %.4f of '
            'the columns affected' % (what, int(neq.sum()), neq.numel(),
                                      -1 if got[1] is None or want[1] is None else int((got[1] != want[1]).sum()),
                                      int(dist.max()), float(neq.any(1).float().mean()), float(neq.any(0).float().mean())))


def _compare(case, model, twin, be, gpu, chained, attention_mask, layers):
    """gpu / chained: host capture records of the two forwards.  -> summary dict; raises AssertionError naming the layer."""
    from quantization.autoquant_utils import int8_stair_status
    B, T = gpu['emb'][0][0].shape[:2]
    status = int8_stair_status(model)
    declined, accepted = [], []
    for l in range(layers):
        tables = status.get(f'layers.{l}.intermediate.0', {})
        (accepted if tables and all(tables.values()) else declined).append(l)
        if l in declined:
            print(f'[{case}] layer {l}: GELU launch keeps the arithmetic epilogue (tables {tables or "none fits"}) -> '
                  f'teacher-forced bar only')
    print(f'[{case}] GELU tables accepted in layers {accepted}, declined / absent in {declined}')
    first_declined = declined[0] if declined else layers
    idx_of = lambda where, l, rec: _grid_index(twin, where, l, rec[0])

    # chained: exact up to (not including) the first layer whose GELU launch has no accepted table
    msg = _report(f'[{case}] chained, embedding block', gpu['emb'][0], chained['emb'][0], idx_of('emb', 0, gpu['emb'][0]),
                  idx_of('emb', 0, chained['emb'][0]))
    assert msg is None, msg
    assert gpu['emb'][0][1] is not None, 'the embedding block emitted no int8 indices'
    chained_exact = 0
    for l in range(first_declined):
        for where in ('attn', 'h'):
            if _report('', gpu[where][l], chained[where][l], idx_of(where, l, gpu[where][l]),
                       idx_of(where, l, chained[where][l])) is not None:
                break
        else:
            chained_exact += 1
            continue
        break
    # teacher-forced: every layer on the GPU's own input; the first failure is the message
    mask = _additive_mask(attention_mask, B, T)
    fallback = []
    for l in range(layers):
        g_in = gpu['emb'][0] if l == 0 else gpu['h'][l - 1]
        c_in = chained['emb'][0] if l == 0 else chained['h'][l - 1]
        if torch.equal(g_in[0], c_in[0]):
            a_rec, h_rec = chained['attn'][l], chained['h'][l]       # same function on the same input: the chained run IS it
        else:
            a_rec, h_rec = _twin_layer(twin, be, l, g_in[0], mask)
        msg = _report(f'[{case}] teacher-forced, layer {l}, attention block', gpu['attn'][l], a_rec,
                      idx_of('attn', l, gpu['attn'][l]), idx_of('attn', l, a_rec))
        assert msg is None, msg
        gi, ti = idx_of('h', l, gpu['h'][l]), idx_of('h', l, h_rec)
        msg = _report(f'[{case}] teacher-forced, layer {l}, feed-forward block', gpu['h'][l], h_rec, gi, ti)
        if l in declined:
            dist = (gi - ti).abs()
            share = float((dist > 0).float().mean())
            print(f'[{case}] layer {l} (arithmetic GELU epilogue): max index distance {int(dist.max())}, share {share:.3e}')
            assert int(dist.max()) <= GELU_FALLBACK_MAX_STEPS and share <= GELU_FALLBACK_MAX_SHARE, msg
            fallback.append(l)
        else:
            assert msg is None, msg
            assert gpu['h'][l][1] is not None, f'layer {l} emitted no int8 indices'
    assert len(fallback) <= len(declined)
    assert chained_exact == first_declined, f'[{case}] chained: layer {chained_exact} differs although every layer does teacher-forced'
    return dict(accepted=accepted, declined=declined, chained_exact_layers=chained_exact)


_TWIN_MEMO = {}


def _run_case(case, recipe, layers, B, monkeypatch, model=None, graph=False, model_key=None):
    """common procedure: calibrate on the GPU, twin = deep copy on the host, GPU forward and twin forward under the product
    default, same launches on both sides, chained + teacher-forced comparison"""
    from quantization import _hip, options
    from quantization.autoquant_utils import INT8_STATS
    from tests._exact_backend import ExactBackend
    assert options.INT8_LINEAR == 'auto'
    T = 128
    if model is None:
        model = _calibrate(_model(recipe, layers, 'cuda'), recipe, [_ids(10, B, T).cuda(), _ids(11, B, T).cuda()])
    ids = _ids(3, B, T)
    am = _padded_mask(B, T) if case in ('a', 'f') else None
    args = (ids.cuda(),) + (() if am is None else (am.cuda(),))
    twin = _twin_of(model)
    log = _hip_census(monkeypatch)
    with torch.no_grad(), _Capture(model) as cap:
        k0 = INT8_STATS['kernel_calls']
        fb0 = INT8_STATS['unsigned_weight_fallbacks']
        model(*args)
        torch.cuda.synchronize()
        kernel_calls = INT8_STATS['kernel_calls'] - k0
        assert INT8_STATS['unsigned_weight_fallbacks'] == fb0
        census = list(log)
        gpu = _host(cap.runs[-1])
        replay = None
        if graph:
            from quantization.graphs import GraphedForward
            g = GraphedForward(model, *args)
            static = cap.runs[-1]                               # the capture pass: the graph's own tensors
            g(*args)
            torch.cuda.synchronize()
            replay = _host(static)
    memo = _TWIN_MEMO.get((recipe, layers, B)) if model_key is not None else None
    if memo is not None and memo[0] == model_key:
        twin, be, chained, twin_calls, twin_census, seconds = memo[1:]       # same calibrated model, same input: same twin
    else:
        be = ExactBackend(rules=_hip.backend())
        chained, twin_calls, twin_census, seconds = _twin_chained(twin, be, ids, am)
        if model_key is not None:
            _TWIN_MEMO[(recipe, layers, B)] = (model_key, twin, be, chained, twin_calls, twin_census, seconds)
    print(f'[{case}] {recipe}, {layers} layers, [{B},{T}]: {len(census)} launches ({kernel_calls} integer Linears), '
          f'twin forward {seconds:.1f} s on the CPU')
    assert kernel_calls == twin_calls, (kernel_calls, twin_calls)
    assert census == twin_census, [(i, a, b) for i, (a, b) in enumerate(zip(census, twin_census)) if a != b][:4]
    stair = [e[-1] for e in census if e[0] in ('linear_i8', 'linear_i8_cls', 'linear_i16x8') and e[2] == 3072]
    assert len(stair) == layers
    assert census == _expected_census(recipe, layers, B, T, stair=stair[0]) and len(set(stair)) == 1
    if replay is not None:
        for where in ('emb', 'attn', 'h'):
            for l, (r, e) in enumerate(zip(replay[where], gpu[where])):
                assert torch.equal(r[0], e[0]) and (r[1] is None) == (e[1] is None) and (r[1] is None or torch.equal(r[1], e[1])), \
                    f'[{case}] hipGraph replay differs from the eager forward: {where} {l}'
        gpu = replay
    out = _compare(case, model, twin, be, gpu, chained, am, layers)
    assert all(torch.isfinite(h).all() for h, _ in gpu['h'])
    out.update(launches=len(census), twin_seconds=seconds)
    print(f'[{case}]', out)
    return out


_BERT_BASE = []


def _bert_base():
    """the calibrated 12-layer model of tests/test_bert_e2e.py, built once for cases a and f"""
    from tests.test_bert_e2e import _build, _calibrate_and_run, _fixture
    if not _BERT_BASE:
        z = _fixture()
        model, _ = _build('cuda')
        _calibrate_and_run(model, torch.from_numpy(z['input_ids']))
        _BERT_BASE.append(model)
    return _BERT_BASE[0]


@pytest.mark.gpu
@pytest.mark.default_route
def test_bert_base_w8a8_equals_the_twin(monkeypatch):
    """case a: BERT-base W8A8 per-tensor, 12 layers (fixture bert_base_w8a8), [8,128] with one padded sample"""
    _run_case('a', 'w8a8', 12, 8, monkeypatch, model=_bert_base(), model_key='bert_base_w8a8')


@pytest.mark.gpu
@pytest.mark.default_route
def test_bert_w8a8_large_batch_equals_the_twin(monkeypatch):
    """case b: the same recipe, 2 layers at [64,128]: M = 8192 puts every Linear of the layer on the 128 x 128 tiles
    (tile_plan: >= 384 tiles, K >= 512; the narrowest, N = 768, has 64 x 6 = 384) and FFN1 (64 x 24 = 1536 >= 1024 tiles,
    `stair_bins_for`) on the 1536-bin staircase table"""
    _run_case('b', 'w8a8', 2, 64, monkeypatch)
    from quantization import _hip
    assert _hip.backend().stair_bins_for(64 * 128, 3072) == _hip.backend().STAIR_BINS_BIG


@pytest.mark.gpu
@pytest.mark.default_route
def test_bert_peg_recipe_equals_the_twin(monkeypatch):
    """case c: {'x', 'h', 'y'}: 'ng6', 3 layers: class-ordered FFN1 and both per-column tails"""
    _run_case('c', 'peg', 3, 8, monkeypatch)


@pytest.mark.gpu
@pytest.mark.default_route
def test_bert_permuted_peg_recipe_equals_the_twin(monkeypatch):
    """case d: 'ngp6', 3 layers: the groups scattered over the columns"""
    _run_case('d', 'peg_permuted', 3, 8, monkeypatch)


@pytest.mark.gpu
@pytest.mark.default_route
def test_bert_mixed_precision_recipe_equals_the_twin(monkeypatch):
    """case e: {'x': 16, 'h': 16, 'y': 16}, 3 layers: byte planes + the 16-bit integer Linear, 16-bit sites in the tails"""
    _run_case('e', 'mp16', 3, 8, monkeypatch)


@pytest.mark.gpu
@pytest.mark.default_route
def test_bert_base_w8a8_graph_replay_equals_eager_equals_the_twin(monkeypatch):
    """case f: case a through quantization.graphs.GraphedForward: the replay's hidden states equal the eager forward's, which
    equal the twin's"""
    _run_case('f', 'w8a8', 12, 8, monkeypatch, model=_bert_base(), graph=True, model_key='bert_base_w8a8')


# ---- CPU: the twin itself ---------------------------------------------------------------------------------------------------
def _cpu_route(recipe, layers, B, T, want_backend=False):
    from quantization import _hip, options
    from quantization.autoquant_utils import INT8_STATS
    from tests._exact_backend import ExactBackend
    be = ExactBackend()
    prev = _hip.set_backend(be)
    try:
        assert options.INT8_LINEAR == 'auto'
        model = _calibrate(_model(recipe, layers, 'cpu'), recipe, [_ids(10, B, T)])
    finally:
        _hip.set_backend(prev)
    del be.tail_bindings[:]
    rec, calls, census, seconds = _twin_chained(model, be, _ids(3, B, T), None)
    return (model, rec, calls, census, seconds) + ((be,) if want_backend else ())


@pytest.mark.default_route
@pytest.mark.parametrize('recipe', list(RECIPES))
def test_twin_takes_the_default_routes_launches_cpu(recipe):
    """2 layers per recipe: the twin's default-route forward is the census the GPU tests expect, and every hidden state lies
    on the grid of the quantizer that produced it"""
    model, rec, calls, census, _, be = _cpu_route(recipe, 2, 2, 64, want_backend=True)
    assert census == _expected_census(recipe, 2, 2, 64), census
    assert calls == 2 * 6                                     # Q, K, V, attention output, FFN1, FFN2 per layer
    # every tail launch got ITS three quantizers, in the order (dense output, residual sum, LayerNorm output): the twin shares
    # the host code with the GPU side, so an exchange there is invisible to the GPU comparison and is pinned here
    ptr = lambda m: getattr(m, 'activation_quantizer', m).quantizer._delta.data_ptr()
    assert be.tail_bindings == [(ptr(b.dense.activation_quantizer), ptr(b.res_act_quantizer.activation_quantizer),
                                 ptr(b.LayerNorm.activation_quantizer)) for L in model.layers for b in (L.attention_output, L.output)]
    for l, (h, idx) in enumerate(rec['h']):
        q = model.layers[l].output.LayerNorm.activation_quantizer.quantizer
        i, y = O.fake_quant(h, q._delta, q._zero_float, 8, False)
        assert torch.equal(y, h) and idx is not None and torch.equal(idx.float() + 128, i)


@pytest.mark.default_route
def test_twelve_layer_twin_forward_fits_the_suite_cpu():
    """BERT-base, 12 layers, [8,128], W8A8: one twin forward.  Measured on the CPU box this suite runs on: 42 s (3.5 s per
    layer; the C oracle's integer contractions run on one thread); it fits the CPU suite, so case a keeps all 12 layers."""
    model, rec, calls, census, seconds = _cpu_route('w8a8', 12, 8, 128)
    print('12-layer twin forward: %.1f s' % seconds)
    assert len(census) == 1 + 12 * 7 and calls == 12 * 6
    assert all(torch.isfinite(h).all() and i is not None for h, i in rec['h'])


def _q7(lo, hi, n_bits=8, per_column=None, g=None):
    if per_column is None:
        d, z = O.asym_params_from_range(lo, hi, n_bits)
        return (d.reshape(1), z.reshape(1), None, n_bits, False, False, 1e-8)
    los = lo * (0.5 + torch.rand(6, generator=g))[(torch.arange(per_column) * 6) // per_column]
    his = hi * (0.5 + torch.rand(6, generator=g))[(torch.arange(per_column) * 6) // per_column]
    d, z = O.asym_params_from_range(los, his, n_bits)
    return (d.contiguous(), z.contiguous(), None, n_bits, False, False, 1e-8)


def _spec(q):
    return None if q is None else (q[0] if q[0].numel() > 1 else q[0].reshape(()), q[1] if q[1].numel() > 1 else q[1].reshape(()),
                                   q[3], False, False, q[6])


def test_twin_tails_are_the_shared_chains_cpu():
    """ExactBackend's tails and embedding block == the chains the kernel tests import (a later edit cannot fork them)"""
    from tests._exact_backend import ExactBackend, embeddings_chain, ln_tail_chain
    be = ExactBackend()
    g = torch.Generator().manual_seed(5)
    d = 768
    a, r = torch.randn(4, 33, d, generator=g) * 2, torch.randn(4, 33, d, generator=g) * 1.5
    w, b = 1 + 0.1 * torch.randn(d, generator=g), 0.05 * torch.randn(d, generator=g)
    for dtype in (torch.float32, torch.bfloat16):
        for per_col in ((None, None, None), (d, d, None), (None, None, d), (d, None, d)):
            for use in ((1, 1, 1), (0, 1, 1), (1, 0, 0)):
                qs = [(_q7(lo, hi, per_column=pc, g=g) if u else None)
                      for (lo, hi), pc, u in zip(((-7.0, 7.5), (-20.0, 22.0), (-6.0, 11.0)), per_col, use)]
                axis = any(pc for pc, u in zip(per_col, use) if u)
                fn = be.residual_layernorm_quant_axis if axis else be.residual_layernorm_quant
                want_idx = qs[2] is not None
                out = fn(a.to(dtype), r.to(dtype), qs[0], qs[1], w, b, 1e-12, qs[2], want_idx=want_idx)
                y, idx, _ = ln_tail_chain(a.to(dtype).reshape(-1, d), r.to(dtype).reshape(-1, d), _spec(qs[0]), _spec(qs[1]), w, b,
                                          1e-12, _spec(qs[2]))
                got = out[0] if want_idx else out
                assert got.dtype == dtype and torch.equal(got.reshape(-1, d), y.to(dtype))
                if want_idx:
                    assert torch.equal(out[1].reshape(-1, d).float() + 128, idx)
    word, typ, pos = torch.randn(50, d, generator=g), torch.randn(2, d, generator=g) * 0.3, torch.randn(40, d, generator=g) * 0.5
    ids, tok = torch.randint(0, 50, (3, 17), generator=g), torch.randint(0, 2, (3, 17), generator=g)
    pid = torch.arange(17).unsqueeze(0).expand(3, 17).contiguous()
    qs = [_q7(-8.0, 9.0), _q7(-9.0, 10.0), _q7(-5.0, 7.0)]
    y, idx = be.embeddings_layernorm_quant(word, ids, typ, tok, pos, pid, qs[0], qs[1], w, b, 1e-12, qs[2], want_idx=True)
    ry, ridx, _ = embeddings_chain(word, ids.reshape(-1), typ, tok.reshape(-1), pos, pid.reshape(-1), _spec(qs[0]), _spec(qs[1]),
                                   w, b, 1e-12, _spec(qs[2]))
    assert torch.equal(y, ry) and torch.equal(idx.float() + 128, ridx)
    # kernel order is not torch's order: the twin must not be F.layer_norm in disguise (tests/test_fused_ln.py's two statements)
    t = ln_tail_chain(a.reshape(-1, d), r.reshape(-1, d), None, None, w, b, 1e-12, None, kernel_order=False)[0]
    k = be.residual_layernorm_quant(a, r, None, None, w, b, 1e-12, None).reshape(-1, d)
    assert not torch.equal(t, k) and torch.allclose(t, k, rtol=2e-5, atol=1e-5)


@pytest.mark.parametrize('activation,stair_ok', [(0, None), (2, None), (2, True), (2, False)])
def test_twin_linears_are_the_shared_formulas_cpu(activation, stair_ok):
    """ExactBackend.linear_i8_cls / quantize_hilo / linear_i16x8 == the formulas the kernel tests import followed by the C
    oracle's epilogue (code 4 behind an accepted table, else the code itself); with one class / an 8-bit grid they equal the
    inherited `linear_i8` (oracle/tq_int_oracle.c) bit for bit, as include/tq_hip.h states for the kernels"""
    import numpy as np
    from tests._exact_backend import ExactBackend, cls_pre, i16x8_pre, i16x8_tot, oracle_epilogue
    be = ExactBackend()
    rng = np.random.default_rng(7)
    M, N, K = 64, 128, 768
    w = torch.from_numpy(rng.integers(-127, 128, (N, K)).astype(np.int8))
    wd = torch.from_numpy(rng.uniform(0.001, 0.004, N).astype(np.float32))
    bias = torch.from_numpy((rng.standard_normal(N) * 0.1).astype(np.float32))
    q_out = _q7(-0.2, 3.2) if activation else None
    stair = None if stair_ok is None else ('exact-stair', 768, stair_ok)
    code = 4 if (activation == 2 and stair_ok) else activation
    junk = torch.zeros(6, N, dtype=torch.int32)                # row sums are never taken from the caller
    # class-ordered: 6 classes of 128 columns
    dc, zc = rng.uniform(0.01, 0.03, 6).astype(np.float32), rng.uniform(0, 255, 6).astype(np.float32)
    xd, xz = torch.from_numpy(np.repeat(dc, 128)), torch.from_numpy(np.repeat(zc, 128))
    x = torch.from_numpy((rng.integers(0, 256, (M, K)) - 128).astype(np.int8))
    ends, reps = [128 * (c + 1) for c in range(6)], [128 * c + 5 for c in range(6)]
    out = be.linear_i8_cls(x.reshape(2, 32, K), w, junk, bias, (xd, xz, 8, 1e-8), be.cls_table(ends, reps), wd, 1e-8, activation,
                           q_out, torch.float32, want_idx=q_out is not None, stair=stair)
    pre = cls_pre(x.numpy(), w.numpy(), ends, reps, xd.numpy(), xz.numpy(), 8, 1e-8, wd.numpy(), 1e-8, bias.numpy())
    ry, ri = oracle_epilogue(pre, code, q_out)
    got = out[0] if q_out is not None else out
    assert torch.equal(got.reshape(M, N).view(torch.int32), ry.view(torch.int32))
    if q_out is not None:
        assert torch.equal(out[1].reshape(M, N), ri)
    with pytest.raises(AssertionError):                          # a boundary that does not match the buffers is refused
        be.linear_i8_cls(x, w, junk, bias, (xd, xz, 8, 1e-8), be.cls_table([256, 256 + 128] + ends[3:], reps[:1] + reps[2:]), wd,
                         1e-8, activation, q_out, torch.float32)
    one = (xd[:1].clone(), xz[:1].clone(), 8, 1e-8)
    a = be.linear_i8_cls(x, w, junk[:1], bias, (xd[:1].expand(K).contiguous(), xz[:1].expand(K).contiguous(), 8, 1e-8),
                         be.cls_table([K], [3]), wd, 1e-8, activation, q_out, torch.float32, stair=stair)
    b = be.linear_i8(x, w, junk[0], bias, one, wd, 1e-8, activation, q_out, torch.float32, stair=stair)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # 16-bit input
    d16, z16 = torch.tensor([3.1e-4]), torch.tensor([0.37 * 65535])
    xf = torch.from_numpy(((rng.uniform(-0.1, 1.1, (M, K)) * 65535 - float(z16)) * float(d16)).astype(np.float32))
    hi, lo = be.quantize_hilo(xf, (d16, z16, 16, 1e-8))
    idx = O.fake_quant(xf, d16.reshape(()), z16.reshape(()), 16, False)[0]
    assert torch.equal(256 * (hi.int() + 128) + (lo.int() + 128), idx.int()) and int(idx.min()) == 0 and int(idx.max()) == 65535
    out = be.linear_i16x8(hi, lo, w, junk[0], bias, (d16, z16, 16, 1e-8), wd, 1e-8, activation, q_out, torch.float32,
                          want_idx=q_out is not None, stair=stair)
    z = int(np.clip(np.rint(float(z16)), 0, 65535))
    pre = i16x8_pre(i16x8_tot(idx.numpy().astype(np.int32), w.numpy(), z), float(d16), 1e-8, wd.numpy(), 1e-8, bias.numpy())
    ry, ri = oracle_epilogue(pre, code, q_out)
    got = out[0] if q_out is not None else out
    assert torch.equal(got.view(torch.int32), ry.view(torch.int32))
    if q_out is not None:
        assert torch.equal(out[1], ri)
    lo8 = x
    a = be.linear_i16x8(torch.full_like(lo8, -128), lo8, w, junk[0], bias, one, wd, 1e-8, activation, q_out, torch.float32, stair=stair)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
