"""Host logic of options.INT8_PEG_ATTENTION, replayed on the CPU with the exact twin (tests/_peg_attention_twin.py): under
`apply_activation_granularity(model, per_groups=N)` the attention half of every BERT layer is ONE index-only grouped
class-ordered Linear (Q | K | V) and ONE attention core with a grid per head; every decline happens before the first launch
(the census is then exactly the census with the switch off); quantization/peg.py's block helper on hand-made buffers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.default_route

D = 768
GROUPED, CORE, CLS, AXIS, LIN = ('linear_i8_cls_grouped', 'attention_i8', 'linear_i8_cls', 'residual_layernorm_quant_axis',
                                 'linear_i8')
LAYER_ON = [GROUPED, CORE, CLS, AXIS, CLS, LIN, AXIS]       # attention half, attention-output Linear + tail, FFN1, FFN2, tail
LAYER_OFF = LAYER_ON[2:]                                    # today's: the attention half is layered (no census entry)
_MODELS = {}


def _ids(seed, B=2, T=64):
    return torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(seed))


def _twin():
    from tests._peg_attention_twin import PegAttentionTwin
    return PegAttentionTwin()


def _under(be):
    from quantization import _hip

    class Ctx:
        def __enter__(self):
            self.prev = _hip.set_backend(be)
            return be

        def __exit__(self, *exc):
            _hip.set_backend(self.prev)
            return False
    return Ctx()


def _model(layers, per_groups=6, permute=False, per_embd=False):
    """calibrated once per configuration at [2, 64] on the twin (calibrating forwards are layered: no launch of the route)"""
    key = (layers, per_groups, permute, per_embd)
    if key not in _MODELS:
        from harness.bert import apply_activation_granularity, estimate_permutation_ranges
        from quantization.quantizers import QMethods
        from quantization.range_estimators import RangeEstimators
        from tests.harness_bert import build_bert_base
        from utils.utils import pass_data_for_range_estimation
        qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
                  weight_range_method=RangeEstimators.current_minmax,
                  act_range_method=RangeEstimators.current_minmax if permute else RangeEstimators.running_minmax)
        model, _ = build_bert_base(seed=1000, num_layers=layers, **qp)
        apply_activation_granularity(model, per_embd=per_embd, per_groups=None if per_embd else per_groups, permute=permute)
        model.eval()
        be = _twin()
        with _under(be), torch.no_grad():
            batches = [(_ids(10),), (_ids(11),)]
            if permute:
                estimate_permutation_ranges(model, batches)
            pass_data_for_range_estimation(batches, model, act_quant=True, weight_quant=True, max_num_batches=2)
            model.fix_ranges()
        assert not [e for e in be.census if e[0] in (GROUPED, CORE)]
        _MODELS[key] = model
    return _MODELS[key]


def _run(model, ids, monkeypatch, on=True, call=None, grad=False, **switches):
    """-> (output, census) of one forward on a fresh twin"""
    from quantization import options
    assert options.INT8_LINEAR == 'auto' and options.INT8_PEG_ATTENTION is False
    for k, v in dict(INT8_PEG_ATTENTION=on, **switches).items():
        monkeypatch.setattr(options, k, v)
    be = _twin()
    with _under(be), (torch.enable_grad() if grad else torch.no_grad()):
        out = (call or (lambda m: m(ids)))(model)
    monkeypatch.setattr(options, 'INT8_PEG_ATTENTION', False)
    out = out[0] if isinstance(out, (tuple, list)) else out
    return out.detach().clone(), list(be.census)


def _names(census):
    return [e[0] for e in census]


@pytest.mark.parametrize('layers', [1, 3])
def test_census_of_the_route_cpu(layers, monkeypatch):
    model, ids = _model(layers), _ids(3)
    on, census = _run(model, ids, monkeypatch)
    off, census_off = _run(model, ids, monkeypatch, on=False)
    assert _names(census_off) == LAYER_OFF * layers, census_off
    assert _names(census) == LAYER_ON * layers, census
    s = (2, 64, D)
    per_layer = [e for e in census if e[0] in (GROUPED, CORE)]
    assert per_layer == [(GROUPED, s, 3 * D, (D, D, D), 128, False), (CORE, s, 'per-head')] * layers
    # everything behind the attention half is today's launch for launch
    assert [e for e in census if e[0] not in (GROUPED, CORE)] == census_off
    # "equal to the switch-off forward where both are exact": the switch-off forward runs Q / K / V and the core layered (fp32
    # GEMMs in torch's order), and everything behind the attention half consumes its output -- so no tensor of the two
    # forwards is computed exactly from equal inputs, and the exact statement that remains is the census above.  For the
    # values the bar is the one of the route against the layered modules (tests/test_bert_peg_route.py).
    d = float((on - off).abs().max())
    assert d <= 0.05 * float(off.abs().max()), (d, float(off.abs().max()))
    again, _ = _run(model, ids, monkeypatch)
    assert torch.equal(again, on)


def test_hidden_states_against_the_layered_modules_cpu(monkeypatch):
    """every layer's hidden state with the switch on against the layered route (INT8_LINEAR off): the existing bar"""
    from tests.test_bert_exact_route import _Capture, _host
    model, ids = _model(3), _ids(4)
    with _Capture(model) as cap:
        _run(model, ids, monkeypatch)
        on = _host(cap.runs[-1])
        _run(model, ids, monkeypatch, on=False, INT8_LINEAR=False)
        layered = _host(cap.runs[-1])
    for l, ((h, hi), (r, _)) in enumerate(zip(on['h'], layered['h'])):
        assert hi is not None and hi.shape == h.shape, f'layer {l}: the hidden state carries no int8 indices'
        d, top = float((h - r).abs().max()), float(r.abs().max())
        print(f'layer {l}: max |on - layered| = {d:.4f}, max |layered| = {top:.4f}')
        assert d <= 0.05 * top, (l, d, top)


@pytest.mark.parametrize('per_groups,block,k_ops', [(12, 64, 1536), (4, 64, 1024), (6, 128, D), (3, 128, D)])
def test_other_group_widths_take_the_route_cpu(per_groups, block, k_ops, monkeypatch):
    """runs of 64 (12 groups), 192 (4), 128 (6) and 256 (3) columns: whole heads and whole 64-column blocks; the launch's block
    width is the widest of (128, 64) over which every output grid is constant.

    The layer INPUT of 12 / 4 groups is itself on a 64- / 192-column grid, and the class-ordered kernel flushes a class between
    its 128-column K slabs: the route pads every class to whole slabs (quantization/peg.py PaddedClassLayout: 12 classes of 128 =
    1536, 4 of 256 = 1024 operand columns, zero weights in the pad columns), so the attention half takes it.  The other
    class-ordered Linears of these two recipes (attention output, FFN1) have no class layout today and stay layered, switch or
    no switch: everything behind the attention half is the census with the switch off."""
    model, ids = _model(1, per_groups=per_groups), _ids(5)
    _, census = _run(model, ids, monkeypatch)
    _, census_off = _run(model, ids, monkeypatch, on=False)
    assert _names(census)[:2] == [GROUPED, CORE] and census[2:] == census_off, census
    assert census[0] == (GROUPED, (2, 64, k_ops), 3 * D, (D, D, D), block, False) and census[1] == (CORE, (2, 64, D), 'per-head')
    if k_ops == D:
        assert _names(census) == LAYER_ON
    else:
        assert _names(census_off) == [AXIS, LIN, AXIS]


@pytest.mark.parametrize('per_groups', [12, 4])
def test_padded_classes_give_the_unpadded_arithmetic_cpu(per_groups, monkeypatch):
    """the context of the route at 64- / 192-column input groups (classes padded to whole K slabs) against the same launches
    composed by hand WITHOUT padding: `cls_pre` on the natural-order operands with the true class boundaries (the numpy formula
    takes any class size), the C oracle's epilogue block by block, the twin's per-head core -- bit for bit"""
    import numpy as np
    from quantization import _hip, options, peg, provenance
    from tests._exact_backend import cls_pre, oracle_epilogue
    model, ids = _model(1, per_groups=per_groups), _ids(5)
    A = model.layers[0].attention_self
    be = _twin()
    with _under(be), torch.no_grad():
        x = model.embeddings(ids)
        src = provenance.quantizer_of(x)
        assert src is not None and peg.class_layout(src, D) is None
        lay = peg.padded_class_layout(src, D)
        assert isinstance(lay, peg.PaddedClassLayout) and lay.ends[-1] % 128 == 0 and int(lay.pad.sum()) == lay.ends[-1] - D
        assert sorted(lay.order[~lay.pad].tolist()) == list(range(D))
        mask = torch.zeros(2, 1, 1, 64)
        mask[1, ..., 50:] = -10000.0
        monkeypatch.setattr(options, 'INT8_PEG_ATTENTION', True)
        ctx = A(x, mask)
        monkeypatch.setattr(options, 'INT8_PEG_ATTENTION', False)
        assert [e[0] for e in be.census if e[0] in (GROUPED, CORE)] == [GROUPED, CORE]
        # by hand, unpadded
        order, ends, reps = peg.classes_from_params(src._delta.reshape(-1).numpy(), src._zero_float.reshape(-1).numpy(), multiple=1)
        x_idx = be.quantize_to_int8(x, src._delta, src._zero_float, None, src.n_bits, False, False, src.eps, D, 1, True)
        cols = []
        for l in (A.query, A.key, A.value):
            w_idx, _, signed = l._int8_weights()
            assert signed
            wq, oq = l.weight_quantizer.quantizer, l.activation_quantizer.quantizer
            pre = cls_pre(x_idx.reshape(-1, D).numpy()[:, order], w_idx.numpy()[:, order], ends, reps, src._delta.reshape(-1).numpy(),
                          src._zero_float.reshape(-1).numpy(), src.n_bits, src.eps, wq._delta.reshape(-1).numpy(), wq.eps,
                          l.bias.detach().numpy())
            d, z = oq._delta.reshape(-1).numpy(), oq._zero_float.reshape(-1).numpy()
            yi = np.empty(pre.shape, np.int8)
            for c0 in range(0, D, 64):
                yi[:, c0:c0 + 64] = oracle_epilogue(np.ascontiguousarray(pre[:, c0:c0 + 64]), 0,
                                                    (float(d[c0]), float(z[c0]), None, 8, False, False, oq.eps))[1].numpy()
            cols.append((torch.from_numpy(yi).reshape(2, 64, D), (oq._delta.reshape(-1), oq._zero_float.reshape(-1), None, 8, False,
                                                                   False, oq.eps)))
        q7 = lambda m: (lambda q: (q._delta.reshape(-1), q._zero_float.reshape(-1), None, q.n_bits, False, False, q.eps))(
            m.activation_quantizer.quantizer)
        want, want_idx = be.attention_i8(cols[0][0], cols[1][0], cols[2][0], A.heads, mask.reshape(2, 64), 8.0, cols[0][1], cols[1][1],
                                         cols[2][1], q7(A.attn_scores_act_quantizer), q7(A.attn_probs_act_quantizer),
                                         q7(A.context_act_quantizer), want_idx=True)
    assert torch.equal(provenance.indices_of(ctx), want_idx) and torch.equal(ctx, want)


def _declines(model, ids, monkeypatch, what, **kw):
    _, off = _run(model, ids, monkeypatch, on=False, **{k: v for k, v in kw.items() if k not in ('call', 'grad')}, **{
        k: v for k, v in kw.items() if k in ('call', 'grad')})
    _, on = _run(model, ids, monkeypatch, **kw)
    assert not [e for e in on if e[0] in (GROUPED,)] and on == off, f'{what}: {on[:3]}'


def test_permuted_groups_and_per_embedding_grids_decline_cpu(monkeypatch):
    _declines(_model(1, permute=True), _ids(6), monkeypatch, 'permuted groups')
    _declines(_model(1, per_embd=True), _ids(6), monkeypatch, 'per-embedding grids')


def test_declines_happen_before_the_first_launch_cpu(monkeypatch):
    import copy
    from quantization import options
    ids = _ids(7)
    base = _model(1)
    _, census = _run(base, ids, monkeypatch)
    assert _names(census) == LAYER_ON                         # premise: this model takes the route

    def mutated(change):
        m = copy.deepcopy(base)
        change(m.layers[0].attention_self)
        return m
    hook = lambda A: A.key.activation_quantizer.register_forward_hook(lambda m, a, o: None)
    _declines(mutated(hook), ids, monkeypatch, 'a hook on an output quantizer')
    _declines(mutated(lambda A: A.context_act_quantizer.register_forward_hook(lambda m, a, o: None)), ids, monkeypatch,
              'a hook on the context site')

    def save_target(A):
        A.value.activation_save_target = {}
        A.value.activation_save_name = 'v'
    _declines(mutated(save_target), ids, monkeypatch, 'a save target')
    _declines(mutated(lambda A: setattr(A.query.activation_quantizer.quantizer, 'n_bits', 16)), ids, monkeypatch, 'a 16-bit grid')
    _declines(mutated(lambda A: setattr(A.context_act_quantizer.activation_quantizer.quantizer, 'n_bits', 16)), ids, monkeypatch,
              'a 16-bit context grid')
    _declines(mutated(lambda A: A.value.activation_quantizer.estimate_ranges()), ids, monkeypatch, 'an estimating quantizer')

    def misaligned(A):                                       # the first group one column longer: no longer whole heads
        q = A.key.activation_quantizer.quantizer
        q._delta.reshape(-1)[128] = q._delta.reshape(-1)[127]
        q._zero_float.reshape(-1)[128] = q._zero_float.reshape(-1)[127]
    _declines(mutated(misaligned), ids, monkeypatch, 'groups that are not head-aligned')
    # grad mode; a ragged B * T without INT8_RAGGED + INT8_RAGGED_RECIPES; packed batches
    _declines(base, ids, monkeypatch, 'grad mode', grad=True)
    _declines(base, _ids(8, 3, 50), monkeypatch, 'a ragged token count without the ragged switches')
    _declines(base, _ids(8, 3, 50), monkeypatch, 'a ragged token count with INT8_RAGGED alone', INT8_RAGGED=True)
    from harness.bert import pack_batch
    p_ids, p_pos, seq_start, max_len = pack_batch(_ids(9, 3, 50), torch.ones(3, 50, dtype=torch.long))
    _declines(base, None, monkeypatch, 'a packed batch', INT8_RAGGED=True, INT8_RAGGED_RECIPES=True,
              call=lambda m: m.forward_packed(p_ids, p_pos, seq_start, max_len))
    assert options.INT8_PEG_ATTENTION is False


def test_per_tensor_recipe_keeps_its_own_launches_cpu(monkeypatch):
    """no per-column grid anywhere (plain W8A8: per_groups None leaves every site per-tensor): the switch changes nothing, the
    attention half stays on the launches of the per-tensor route"""
    model, ids = _model(1, per_groups=None), _ids(7)
    q = model.layers[0].attention_self.query.activation_quantizer.quantizer
    assert q._delta.numel() == 1
    off, census_off = _run(model, ids, monkeypatch, on=False)
    on, census = _run(model, ids, monkeypatch)
    assert census == census_off and GROUPED not in _names(census) and 'attention_i8' in _names(census), census
    assert torch.equal(on, off)


def _make_symmetric(mgr):
    """replace the manager's fixed asymmetric quantizer by a fixed SYMMETRIC per-tensor one over the same overall range (a
    symmetric quantizer has no per-column form: quantizers.py `_adjust_params_per_axis`)"""
    from quantization.quantizers import SymmetricUniformQuantizer
    old = mgr.quantizer
    assert not old.symmetric and old.is_initialized
    new = SymmetricUniformQuantizer(n_bits=old.n_bits, eps=old.eps)
    with _under(_twin()), torch.no_grad():
        new.set_quant_range(float(old.x_min.min()), float(old.x_max.max()))
    assert new.symmetric and new.is_initialized and new.n_bits == 8
    mgr.quantizer = new


@pytest.mark.parametrize('site', ['query', 'key', 'value', 'context', 'input'])
def test_symmetric_grids_decline_before_the_first_launch_cpu(site, monkeypatch):
    """a symmetric grid at any of the five sites of the attention half -- the Q, K or V output quantizer, the context
    quantizer, the grid x arrives on -- leaves the census exactly the one with the switch off"""
    import copy
    from quantization import provenance
    ids = _ids(7)
    base = _model(1)
    _, census = _run(base, ids, monkeypatch)
    assert _names(census) == LAYER_ON                         # premise: this model takes the route
    m = copy.deepcopy(base)
    A = m.layers[0].attention_self
    if site == 'input':
        with _under(_twin()), torch.no_grad():
            src = provenance.quantizer_of(m.embeddings(ids))
        from quantization.quantization_manager import QuantizationManager
        owners = [mod for mod in m.modules() if isinstance(mod, QuantizationManager) and mod.quantizer is src]
        assert src is not None and len(owners) == 1           # the embedding block's output quantizer
        _make_symmetric(owners[0])
        with _under(_twin()), torch.no_grad():
            assert provenance.quantizer_of(m.embeddings(ids)).symmetric
    elif site == 'context':
        _make_symmetric(A.context_act_quantizer.activation_quantizer)
    else:
        _make_symmetric(getattr(A, site).activation_quantizer)
    _declines(m, ids, monkeypatch, f'a symmetric {site} grid')


def test_ragged_shapes_take_the_route_with_both_ragged_switches_cpu(monkeypatch):
    model = _model(1)
    _, census = _run(model, _ids(8, 3, 50), monkeypatch, INT8_RAGGED=True, INT8_RAGGED_RECIPES=True)
    assert _names(census) == [GROUPED, 'attention_i8_ragged'] + LAYER_ON[2:], census
    assert census[1] == ('attention_i8_ragged', (3, 50, D), 'per-head')
    _, census = _run(model, _ids(8, 3, 64), monkeypatch, INT8_RAGGED=True, INT8_RAGGED_RECIPES=True)   # T % 64 == 0, B * T = 192
    assert _names(census) == LAYER_ON


def test_block_helper_on_hand_made_buffers_cpu():
    from quantization import peg
    d = np.repeat(np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], np.float32), 128)
    z = np.repeat(np.array([1, 2, 3, 4, 5, 6], np.float32), 128)
    assert peg.widest_constant_block(d, z) == 128 and peg.constant_over(d, z, 64) and peg.constant_over(d, z, 32)
    assert not peg.constant_over(d, z, 256) and not peg.constant_over(d, z, 96) and not peg.constant_over(d, z, 100)
    # misaligned by one column: neither 128 nor 64
    d1 = d.copy()
    d1[128] = d1[127]
    assert peg.widest_constant_block(d1, z) is None and not peg.constant_over(d1, z, 64)
    z1 = z.copy()
    z1[63] = z1[64] + 1                                     # the zero point alone decides too
    assert peg.widest_constant_block(d, z1) is None
    # runs of 64 and of 192 columns: 64
    d64 = np.repeat(np.arange(12, dtype=np.float32) + 1, 64)
    assert peg.widest_constant_block(d64, d64) == 64
    d192 = np.repeat(np.arange(4, dtype=np.float32) + 1, 192)
    assert peg.widest_constant_block(d192, d192) == 64 and not peg.constant_over(d192, d192, 128)
    # merged equal groups (two neighbours with the same pair) change nothing; a single group is constant over everything
    dm = np.repeat(np.array([0.1, 0.1, 0.3, 0.4, 0.4, 0.4], np.float32), 128)
    assert peg.widest_constant_block(dm, dm) == 128 and peg.constant_over(dm, dm, 64)
    one = np.full(768, 0.25, np.float32)
    assert peg.widest_constant_block(one, one) == 128 and peg.constant_over(one, one, 768)
    # -0.0 and 0.0 are different bit patterns: not constant (the kernels would read either)
    zz = np.zeros(128, np.float32)
    zz[5] = -0.0
    assert peg.widest_constant_block(one[:128], zz) is None
    assert peg.widest_constant_block(np.zeros(0, np.float32), np.zeros(0, np.float32)) is None
    assert peg.widest_constant_block(one[:96], one[:96]) is None                  # no width divides 96


def test_block_layout_is_cached_per_range_state_cpu(monkeypatch):
    from quantization import peg
    model = _model(1)
    q = model.layers[0].attention_self.query.activation_quantizer.quantizer
    reads = []
    orig = peg.BlockLayout.__init__
    monkeypatch.setattr(peg.BlockLayout, '__init__', lambda self, *a: (reads.append(1), orig(self, *a))[1])
    q.__dict__.pop('_peg_blocks', None)
    a = peg.block_layout(q, D)
    assert a is peg.block_layout(q, D) and len(reads) == 1 and a.block == 128 and a.constant_over(64)
    with torch.no_grad():
        q._zero_float.add_(0.0)                              # an in-place change of the zero point alone: a new state
    assert peg.block_layout(q, D) is not a and len(reads) == 2
    assert peg.block_layout(q, 512) is None
