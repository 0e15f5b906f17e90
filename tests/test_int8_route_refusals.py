"""Every reason a helper of the integer route DECLINES (quantization/fused.py, QuantLinear._int8_*): the half of the host
logic the launch censuses of tests/test_bert_exact_route.py, tests/test_bert_ragged_route.py and
tests/test_mobilebert_e2e.py do not state.  CPU only, on the backend doubles.

Models: ONE encoder layer of BERT-base W8A8 (hidden 768, the recipe of tests/test_bert_ragged_route.py::_cpu_model, on
tests/_ragged_twin.RaggedTwin, whose census names every launch) and ONE layer of MobileBERT W8A8 (the shape of
test_mobilebert_grouped_and_chained_launches_host_logic_cpu, on tests/_oracle_backend.OracleBackend behind a counting
wrapper), both at [2,64].  Unperturbed, every helper is on its fused / integer launch (`BERT_BASE`, `MOBILE_BASE`).

Each case applies ONE perturbation to a fresh copy and asserts
  * the launches, in call order: the helper concerned makes none of its fused launches and what runs in its place is the
    layered modules or the next-narrower helper -- the sequences are written down from the helpers' code, not from a run;
  * the output is `torch.equal` to the output of a reference forward in which the helper concerned (only the call that
    gets the perturbed modules) is replaced by the fallback its docstring names.  A perturbation that leaves the model's
    function alone (`same=True`: a save target on a LayerNorm, a mask view, eps below every scale) is held to the
    UNPERTURBED model's reference forward; one that changes the function itself (another grid, an estimating quantizer, a
    Linear that turns from the exact integer contraction to its fp32 simulation: a save target on it, training mode, an
    unsigned grid) to the reference forward of an equally perturbed copy -- the unperturbed model computes something else.

Perturbations of the list this file was written to and where they are: save targets on intermediate / dense / layer_norm
(BERT feed-forward helper; MobileBERT feed-forward helper and chain, one run shows both), a tail quantizer estimating, log
domain (the probabilities' quantizer), intermediate symmetric / 9 bits, probabilities symmetric / off, a leaf in
training mode, grad mode with one trainable weight behind a frozen input, float64, an unsigned weight grid (with
INT8_STATS['unsigned_weight_fallbacks']), eps mismatch between stacked Linears, a mask that is not [B,1,1,T], value_out with
another quantizer's record.

Omitted (1 of 14): a TAIL quantizer in the log scale domain.  For a per-tensor quantizer that is no refusal -- the tail kernels
take log-domain descriptors, the helpers pass them on -- and where a log-domain grid does make a helper decline (the
intermediate quantizer, a chain block's output) the next-narrower helper hands it to an integer launch, which both doubles
answer with `assert not log_domain` (oracle/int_oracle.py, tests/_exact_backend.py): no double can represent the fallback.  The
log-domain refusal the doubles can follow to its end, the probabilities' quantizer, is here."""
import contextlib
import copy

import pytest
import torch

pytestmark = pytest.mark.default_route

B, T = 2, 64


# ---- models, built once -----------------------------------------------------------------------------------------------------
_MEMO = {}


def _bert():
    from quantization import _hip
    from tests._ragged_twin import RaggedTwin
    from tests.test_bert_exact_route import _calibrate, _ids, _model
    if 'bert' not in _MEMO:
        prev = _hip.set_backend(RaggedTwin())
        try:
            _MEMO['bert'] = _calibrate(_model('w8a8', 1, 'cpu'), 'w8a8', [_ids(10, B, T)])
        finally:
            _hip.set_backend(prev)
    return copy.deepcopy(_MEMO['bert'])


def _mobile():
    from harness.mobilebert import build_mobilebert
    from quantization import _hip
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from tests._oracle_backend import OracleBackend
    from utils.utils import pass_data_for_range_estimation
    if 'mobile' not in _MEMO:
        qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
                  weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
        model, _ = build_mobilebert(seed=1000, num_layers=1, **qp)
        model = model.eval()
        prev = _hip.set_backend(OracleBackend())
        try:
            with torch.no_grad():
                pass_data_for_range_estimation([(_inputs()[0],)], model, act_quant=True, weight_quant=True, max_num_batches=1)
                model.fix_ranges()
        finally:
            _hip.set_backend(prev)
        _MEMO['mobile'] = model
    return copy.deepcopy(_MEMO['mobile'])


def _inputs():
    ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(3))
    am = torch.ones(B, T, dtype=torch.long)
    am[1, T - T // 4:] = 0                                    # one padded sample
    return ids, am


# ---- launches, as one letter each ---------------------------------------------------------------------------------------------
# E embedding block | G grouped index-only Linears | A attention core | L integer Linear | I integer Linear, index-only output |
# R residual + LayerNorm / NoNorm tail kernel | N integer Linear + NoNorm tail | P the grouped form of N | F feed-forward block |
# C chain of feed-forward blocks | S scores -> softmax -> probabilities kernel
_LETTER = {'embeddings_layernorm_quant': 'E', 'linear_i8_grouped': 'G', 'attention_i8': 'A', 'linear_i8': 'L',
           'residual_layernorm_quant': 'R', 'linear_i8_nonorm': 'N', 'linear_i8_nonorm_grouped': 'P', 'ffn_i8_nonorm': 'F',
           'ffn_chain_i8_nonorm': 'C', 'scores_softmax_quant': 'S'}
BERT_BASE = 'EGALRILR'             # tests/test_bert_exact_route.py::_expected_census('w8a8', 1, ...), S never: the core has it
MOBILE_BASE = 'PGANCN'             # bottleneck pair + value | query + key | core | attention output | four blocks | output bottleneck


class _Counting:
    """counts the launches of a backend double in call order (the doubles' grouped / chained entry points call their parts
    through `self`: only the outermost call counts)"""

    def __init__(self, be):
        self.log, self.depth = [], 0
        for name, letter in _LETTER.items():
            if hasattr(be, name):
                setattr(be, name, self._wrap(getattr(be, name), name, letter))

    def _wrap(self, orig, name, letter):
        def counted(*a, **k):
            if self.depth == 0:
                self.log.append('I' if name == 'linear_i8' and not k.get('want_y', True) else letter)
            self.depth += 1
            try:
                return orig(*a, **k)
            finally:
                self.depth -= 1
        return counted


def _mentions(args, target):
    return any(a is target or (isinstance(a, (tuple, list)) and _mentions(a, target)) for a in args)


# the fallback each helper's docstring names
_FALLBACK = {
    'quantized_bert_ffn': lambda f, i, d, r, ln, x, res: f.residual_layernorm_quant(d, r, ln, i(x), res),
    'quantized_ffn': lambda f, i, d, r, ln, x: f.residual_layernorm_quant(d, r, ln, i(x), x),
    'residual_layernorm_quant': lambda f, d, r, ln, x, res: ln(r(d(x) + res)),
    'linear_nonorm_quant': lambda f, d, ln, x: ln(d(x)),
    'quantized_ffn_chain': lambda f, *a, **k: None,
    'linear_nonorm_quant_pair': lambda f, *a, **k: None,
    'quantized_self_attention': lambda f, *a, **k: None,
    'quantized_attention': lambda f, *a, **k: None,
    'first_token_linear': lambda f, *a, **k: None,
}


def _scores_fallback(f, sq, pq, scores, mask, denom):
    s = sq(scores) / denom
    return pq(torch.softmax(s if mask is None else s + mask, dim=-1))


_FALLBACK['scores_softmax_quant'] = _scores_fallback


@contextlib.contextmanager
def _declined(helpers, target):
    """the named helpers of quantization.fused take their fallback for calls that are handed `target`"""
    from quantization import fused
    keep = {h: getattr(fused, h) for h in helpers}
    try:
        for h, orig in keep.items():
            def patched(*a, _h=h, _o=orig, **k):
                if _mentions(a, target) or _mentions(tuple(k.values()), target):
                    return _FALLBACK[_h](fused, *a, **k)
                return _o(*a, **k)
            setattr(fused, h, patched)
        yield
    finally:
        for h, orig in keep.items():
            setattr(fused, h, orig)


def _forward(model, family, grad=False, extra=None):
    """-> (launch letters, output, unsigned-weight fallbacks counted)"""
    from quantization import _hip
    from quantization.autoquant_utils import INT8_STATS
    from tests._oracle_backend import OracleBackend
    from tests._ragged_twin import RaggedTwin
    be = RaggedTwin() if family == 'bert' else OracleBackend()
    counter = _Counting(be)
    prev = _hip.set_backend(be)
    fb0 = INT8_STATS['unsigned_weight_fallbacks']
    try:
        with (torch.enable_grad() if grad else torch.no_grad()), (extra or contextlib.nullcontext()):
            y = model(*_inputs())
    finally:
        _hip.set_backend(prev)
    return ''.join(counter.log), y.detach(), INT8_STATS['unsigned_weight_fallbacks'] - fb0


# ---- perturbation tools ----------------------------------------------------------------------------------------------------------
def _save_target(m):
    m.activation_save_target, m.activation_save_name = {}, 'probe'


def _regrid(site, cls=None, n_bits=None, scale_domain='linear'):
    """the site's fixed quantizer replaced by one of another class / width / scale domain over the same range"""
    from quantization import _hip, quantizers
    from tests._oracle_backend import OracleBackend
    mgr = site.activation_quantizer
    old = mgr.quantizer
    prev = _hip.set_backend(OracleBackend())
    try:
        lo, hi = float(old.x_min), float(old.x_max)
        new = (cls or quantizers.AsymmetricUniformQuantizer)(n_bits or old.n_bits, scale_domain=scale_domain, eps=old.eps)
        new.set_quant_range(lo, hi)
    finally:
        _hip.set_backend(prev)
    mgr.quantizer = new


def _symmetric(site):
    from quantization.quantizers import SymmetricUniformQuantizer
    _regrid(site, cls=SymmetricUniformQuantizer)


def _unsigned(linear):
    wq = linear.weight_quantizer.quantizer
    wq._signed = torch.zeros_like(wq._signed)
    linear.cached_params = None                              # the eval-mode cache of the fake-quantized weight


def _freeze_all_but(model, *params):
    for p in model.parameters():
        p.requires_grad_(False)
    for p in params:
        p.requires_grad_(True)


def _wide_mask(attention, pos):
    """the attention block sees the same additive mask as a [B,1,T,T] view, not [B,1,1,T] (pos: its positional index)"""
    fwd = type(attention).forward

    def wide(*a, _m=attention, **k):
        mask = a[pos]
        return fwd(_m, *a[:pos], mask.expand(-1, -1, mask.shape[-1], -1), *a[pos + 1:], **k)
    attention.forward = wide


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# name -> (perturbation(model), helpers that decline, module whose calls decline (model -> module), launches, same function?)
_out = lambda m: m.layers[0].output
_att = lambda m: m.layers[0].attention_self
_FFN = ('quantized_bert_ffn',)
_FFN_TAIL = ('quantized_bert_ffn', 'residual_layernorm_quant')
_CORE = ('quantized_self_attention', 'quantized_attention', 'scores_softmax_quant')

BERT_CASES = {
    # save targets: the feed-forward helper declines all three; the tail helper behind it takes dense and layer_norm to heart;
    # a Linear that records its activations is layered itself (_int8_weight_side_ok)
    'save_intermediate': (lambda m: _save_target(m.layers[0].intermediate[0]), _FFN, _out, 'EGALRLR', False),
    'save_dense': (lambda m: _save_target(_out(m).dense), _FFN_TAIL, _out, 'EGALRL', False),
    'save_layer_norm': (lambda m: _save_target(_out(m).LayerNorm), _FFN_TAIL, _out, 'EGALRLL', True),
    # dense's quantizer estimating (not the probe of the harness' switch): no tail; dense itself takes the calibrating integer
    # forward (options.INT8_CALIBRATION), which is a Linear launch
    'tail_estimating': (lambda m: _out(m).dense.activation_quantizer.estimate_ranges(), _FFN_TAIL, _out, 'EGALRLL', False),
    # intermediate quantizer: symmetric / 9 bits -> no index-only Linear; the Linear itself stays integer, and
    # `dense` finds no <= 8-bit asymmetric linear-domain grid under its input: fp32 GEMM inside the tail helper
    'intermediate_symmetric': (lambda m: _symmetric(m.layers[0].intermediate[0]), _FFN, _out, 'EGALRLR', False),
    'intermediate_9_bits': (lambda m: _regrid(m.layers[0].intermediate[0], n_bits=9), _FFN, _out, 'EGALRLR', False),
    # probabilities: symmetric / log domain / switched off -> neither integer core; Q, K, V on their own; the softmax kernel
    # takes any fixed per-tensor pair
    'probs_symmetric': (lambda m: _symmetric(_att(m).attn_probs_act_quantizer), _CORE[:2], _att, 'ELLLSLRILR', False),
    'probs_log': (lambda m: _regrid(_att(m).attn_probs_act_quantizer, scale_domain='log'), _CORE[:2], _att, 'ELLLSLRILR', False),
    'probs_off': (lambda m: setattr(_att(m).attn_probs_act_quantizer, '_quant_a', False), _CORE[:2], _att, 'ELLLSLRILR', False),
    # a leaf in training mode (its container in eval mode): no grouped launch, the Linear itself layered under 'auto'; its
    # output quantizer still emits indices, so the core runs
    'query_training': (lambda m: _att(m).query.train(), _CORE[:1], _att, 'ELLALRILR', False),
    'key_eps': (lambda m: setattr(_att(m).key.weight_quantizer.quantizer, 'eps', 1e-7), _CORE[:1], _att, 'ELLLALRILR', True),
    'mask_shape': (lambda m: _wide_mask(_att(m), 1), _CORE, _att, 'ELLLLRILR', True),
    # unsigned weight grids: found by the stacking / by `dense._int8_weights()` without a count, then counted by the Linear
    # itself when its own integer forward gives up
    'unsigned_dense': (lambda m: _unsigned(_out(m).dense), _FFN, _out, 'EGALRLR', False),
    'unsigned_query': (lambda m: _unsigned(_att(m).query), _CORE[:1], _att, 'ELLALRILR', False),
}


def _reference(family, case, perturb, helpers, where, same):
    key = (family, helpers, where) if same else (family, case)
    if key not in _MEMO:
        model = _bert() if family == 'bert' else _mobile()
        if not same:
            perturb(model)
        with _declined(helpers, where(model)):
            _MEMO[key] = _forward(model, family)[1]
    return _MEMO[key]


def test_unperturbed_models_take_every_fused_launch():
    assert _forward(_bert(), 'bert')[0] == BERT_BASE
    assert _forward(_mobile(), 'mobile')[0] == MOBILE_BASE


@pytest.mark.parametrize('case', sorted(BERT_CASES))
def test_bert_helper_declines(case):
    perturb, helpers, where, launches, same = BERT_CASES[case]
    model = _bert()
    perturb(model)
    got, y, fallbacks = _forward(model, 'bert')
    assert got == launches, (got, launches)
    assert torch.equal(y, _reference('bert', case, perturb, helpers, where, same))
    assert (fallbacks >= 1) == case.startswith('unsigned'), fallbacks


def test_bert_float64_is_layered_throughout():
    """x in float64: every helper declines (fp32 only), nothing is launched but the layered modules"""
    model = _bert().double()
    got, y, _ = _forward(model, 'bert')
    assert got == '' and y.dtype == torch.float64
    ref = _bert().double()
    with _declined(tuple(_FALLBACK), None), _all_declined():
        want = _forward(ref, 'bert')[1]
    assert torch.equal(y, want)


@contextlib.contextmanager
def _all_declined():
    from quantization import fused, options
    keep = {h: getattr(fused, h) for h in _FALLBACK}, options.INT8_LINEAR
    try:
        for h in _FALLBACK:
            setattr(fused, h, lambda *a, _h=h, **k: _FALLBACK[_h](fused, *a, **k))
        options.INT8_LINEAR = False
        yield
    finally:
        for h, orig in keep[0].items():
            setattr(fused, h, orig)
        options.INT8_LINEAR = keep[1]


@pytest.mark.parametrize('which', ['dense', 'query'])
def test_bert_trainable_weight_behind_a_frozen_input(which, monkeypatch):
    """grad mode on (options.INT8_LINEAR = True: 'auto' would switch the whole route off), every parameter frozen: the base
    launches.  ONE weight trainable: the helper that would bypass its layer declines.  `dense`: fp32 GEMM inside the tail
    helper.  `query`: the Linear on its own under _Int8LinearSTE; its output requires grad, so behind it every helper declines
    its input and the four Linears that see it (query, attention output, intermediate, output) run under the STE wrapper, key
    and value plainly: six Linear launches, no core, no tail."""
    from quantization import options
    from quantization.autoquant_utils import INT8_STATS
    monkeypatch.setattr(options, 'INT8_LINEAR', True)
    model = _bert()
    _freeze_all_but(model)
    assert _forward(model, 'bert', grad=True)[0] == BERT_BASE
    pick = (lambda m: _out(m).dense.weight) if which == 'dense' else (lambda m: _att(m).query.weight)
    helpers, where, launches = (_FFN, _out, 'EGALRLR') if which == 'dense' else (_CORE[:1], _att, 'ELLLLLL')
    _freeze_all_but(model, pick(model))
    a0 = INT8_STATS['autograd_calls']
    got, y, _ = _forward(model, 'bert', grad=True)
    assert got == launches, (got, launches)
    assert INT8_STATS['autograd_calls'] - a0 == (4 if which == 'query' else 0)
    ref = _bert()
    _freeze_all_but(ref, pick(ref))
    with _declined(helpers, where(ref)):
        assert torch.equal(y, _forward(ref, 'bert', grad=True)[1])


# ---- MobileBERT ------------------------------------------------------------------------------------------------------------------
_blk = lambda m: m.layers[0].ffn[1]
_matt = lambda m: m.layers[0].attention_self
_MFFN = ('quantized_ffn_chain', 'quantized_ffn')
_MFFN_TAIL = _MFFN + ('residual_layernorm_quant',)


def _foreign_value_record(model):
    """the value the bottleneck pair's launch computed along, handed on with ANOTHER quantizer's record (the key Linear's)"""
    from quantization import fused, provenance
    orig = fused.linear_nonorm_quant_pair
    other = _matt(model).key.activation_quantizer.quantizer

    def pair(*a, **k):
        out = orig(*a, **k)
        if out is not None and len(out) == 3:
            provenance.tag(out[2], other, provenance.indices_of(out[2]))
        return out

    @contextlib.contextmanager
    def installed():
        fused.linear_nonorm_quant_pair = pair
        try:
            yield
        finally:
            fused.linear_nonorm_quant_pair = orig
    return installed()


MOBILE_CASES = {
    # one block of the chain (the second of four): no chain, that block not fused, the three others one launch each
    'save_intermediate': (lambda m: _save_target(_blk(m).intermediate[0]), _MFFN, _blk, 'PGANFNFFN', False),
    'save_dense': (lambda m: _save_target(_blk(m).output.dense), _MFFN_TAIL, _blk, 'PGANFLFFN', False),
    'save_layer_norm': (lambda m: _save_target(_blk(m).output.LayerNorm), _MFFN_TAIL, _blk, 'PGANFLLFFN', True),
    'tail_estimating': (lambda m: _blk(m).output.dense.activation_quantizer.estimate_ranges(), _MFFN_TAIL, _blk, 'PGANFLLFFN', False),
    'intermediate_symmetric': (lambda m: _symmetric(_blk(m).intermediate[0]), _MFFN, _blk, 'PGANFLRFFN', False),
    'intermediate_9_bits': (lambda m: _regrid(_blk(m).intermediate[0], n_bits=9), _MFFN, _blk, 'PGANFLRFFN', False),
    'unsigned_dense': (lambda m: _unsigned(_blk(m).output.dense), _MFFN, _blk, 'PGANFLRFFN', False),
    # stacked Linears share one eps argument: no pair (each bottleneck its own launch, the value Linear its own grouped launch)
    'bottleneck_eps': (lambda m: setattr(m.layers[0].bottleneck_attention.dense.weight_quantizer.quantizer, 'eps', 1e-7),
                       ('linear_nonorm_quant_pair',), lambda m: m.layers[0].bottleneck_attention.dense, 'NNGGANCN', True),
    # neither core: the layered attention returns a view, which carries no record, so the attention output's Linear is an
    # fp32 GEMM in front of the tail kernel (R instead of N)
    'probs_symmetric': (lambda m: _symmetric(_matt(m).attn_probs_act_quantizer), _CORE[:2], _matt, 'PLLRCN', False),
    'mask_shape': (lambda m: _wide_mask(_matt(m), 3), _CORE[:2], _matt, 'PLLRCN', True),
}


@pytest.mark.parametrize('case', sorted(MOBILE_CASES))
def test_mobilebert_helper_declines(case):
    perturb, helpers, where, launches, same = MOBILE_CASES[case]
    model = _mobile()
    perturb(model)
    got, y, fallbacks = _forward(model, 'mobile')
    assert got == launches, (got, launches)
    assert torch.equal(y, _reference('mobile', case, perturb, helpers, where, same))
    assert (fallbacks >= 1) == case.startswith('unsigned'), fallbacks


def test_mobilebert_value_out_with_another_quantizers_record():
    """the grouped attention declines a value_out whose record is not the value Linear's own quantizer: query and key run on
    their own and the core takes the three tensors by their records"""
    model = _mobile()
    got, y, _ = _forward(model, 'mobile', extra=_foreign_value_record(model))
    assert got == 'PLLANCN', got
    ref = _mobile()
    with _declined(_CORE[:1], _matt(ref)):
        want = _forward(ref, 'mobile', extra=_foreign_value_record(ref))[1]
    assert torch.equal(y, want)
