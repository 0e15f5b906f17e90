"""options.FUSED_SOFTMAX_TRAINING: `fused.scores_softmax_quant` under autograd = the forward launch + the one-launch backward,
against the layered modules' autograd and against the float64 reference of tests/test_softmax_quant_bwd.py (K).  The fused side
meets the kernel-level bounds; the layered side carries fp32 round-off of its own, so the two agree within TWICE those bounds
(L_block = 18: fq_bwd_tensor adds 8 elements per thread of the [2, H, 64, 64] tensors, + 6 wave steps + 4 LDS adds)."""
import copy

import pytest
import torch

from tests import test_softmax_quant_bwd as K

pytestmark = pytest.mark.gpu
SITES = (('q1', 0, '_delta', 'd'), ('q1', 0, '_zero_float', 'z'), ('q2', 1, '_delta', 'd'), ('q2', 1, '_zero_float', 'z'))


@pytest.fixture
def switch():
    from quantization import options
    options.FUSED_SOFTMAX_TRAINING = False
    yield lambda on: setattr(options, 'FUSED_SOFTMAX_TRAINING', on)
    options.FUSED_SOFTMAX_TRAINING = False


def _sites(learn, T=64, dev='cuda'):
    """two QuantizedActivations with K's ranges ([-70, 80] over 24 randn scores, [0, 0.5] over the probabilities: every clamp
    cuts), scores, grad_probs and a [2, 1, 1, T] mask"""
    from quantization.base_quantized_classes import QuantizedActivation
    from quantization.quantizers import QMethods
    s, gy, _ = K._inputs(T, (2, 4, 64), 3, False)
    mask = torch.zeros(2, 1, 1, T)
    mask[1, ..., T - 10:] = -10000.0
    qs = [QuantizedActivation(act_method=QMethods.asymmetric_uniform, n_bits_act=8).to(dev) for _ in range(2)]
    for m, (lo, hi) in zip(qs, ((-70.0, 80.0), (0.0, 0.5))):
        m.quantized_acts()
        m.activation_quantizer.set_quant_range(torch.tensor(lo, device=dev), torch.tensor(hi, device=dev))
        m.learn_ranges() if learn else m.fix_ranges()
    return qs, s.to(dev), gy.to(dev), mask.to(dev)


def _qdict(m):
    q = m.activation_quantizer.quantizer
    return dict(delta=q._delta.detach().cpu().reshape(()), zf=q._zero_float.detach().cpu().reshape(()), signed=False,
                symmetric=False, domain='linear')


def _grads(qs, s, gy, mask):
    """-> [probs, scores.grad, the range gradients in SITES order (learnable ranges only)]"""
    from quantization.fused import scores_softmax_quant
    x = s.clone().requires_grad_(True)
    for m in qs:
        m.zero_grad()
    y = scores_softmax_quant(qs[0], qs[1], x, mask, K.DENOM)
    y.backward(gy)
    prm = [getattr(qs[i].activation_quantizer.quantizer, attr) for _, i, attr, _ in SITES]
    return [y.detach(), x.grad] + [p.grad.clone() for p in prm if p.requires_grad]


def _assert_range_gradients(on, off, ref):
    """each of the four against the float64 terms within the kernel-level bound, and against layered autograd within twice it"""
    for (name, _, _, key), a, b in zip(SITES, on, off):
        lim = K._param_bounds(ref[name], name, 18)['dz'.index(key)]
        assert abs(float(a) - ref[name][key]) <= lim and abs(float(a) - float(b)) <= 2 * lim, (name, key, float(a), float(b), lim)


@pytest.mark.parametrize('learn', [False, True])
def test_gradients_match_layered_autograd(learn, switch):
    from quantization.fused import scores_softmax_quant
    qs, s, gy, mask = _sites(learn)
    off = _grads(qs, s, gy, mask)
    switch(True)
    on = _grads(qs, s, gy, mask)
    with torch.no_grad():
        assert torch.equal(on[0], scores_softmax_quant(qs[0], qs[1], s, mask, K.DENOM))      # the value is the fused forward's
    ref = K._reference(s.cpu(), gy.cpu(), mask.reshape(2, -1).cpu(), _qdict(qs[0]), _qdict(qs[1]), on[0].cpu())
    assert bool(((on[1] - off[1]).cpu().double().abs() <= 2 * (2e-5 + (8 + 8) * K.U) * ref['mag']).all())
    assert len(on) == (6 if learn else 2) and all(a.shape == b.shape for a, b in zip(on, off))
    _assert_range_gradients(on[2:], off[2:], ref)


@pytest.mark.parametrize('decline', ['off', 'hook', 'Tk48'])
def test_declines_are_bit_equal_to_today(decline, switch):
    qs, s, gy, mask = _sites(True, T=48 if decline == 'Tk48' else 64)
    if decline == 'hook':
        qs[0].activation_quantizer.register_forward_hook(lambda *a: None)
    ref = _grads(qs, s, gy, mask)                       # today's: the option is off
    switch(decline != 'off')
    assert all(torch.equal(a, b) for a, b in zip(ref, _grads(qs, s, gy, mask)))


def _step_arms(base, inputs, targets, loss_fn, switch):
    """one training step with the option off, on (eager) and on (GraphedTrainStep): eager == graphed bit for bit, loss == off's"""
    from quantization.data_parallel import GradientBuckets, train_step
    from quantization.graphs import GraphedTrainStep
    out = {}
    for arm in ('off', 'eager', 'graphed'):
        switch(arm != 'off')
        model = copy.deepcopy(base)
        opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3)
        if arm == 'graphed':
            loss = GraphedTrainStep(model, loss_fn, opt, inputs, targets)(inputs, targets).clone()
        else:
            loss = train_step(model, loss_fn, opt, GradientBuckets(model.parameters()), inputs, targets)
        out[arm] = [loss] + [p.detach().clone() for p in model.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(out['eager'], out['graphed']))
    assert torch.allclose(out['eager'][0], out['off'][0], rtol=1e-5, atol=0)


def test_whole_model_step_eager_and_graphed(switch):
    from transformers import BertConfig, BertForSequenceClassification
    from quantization.quantizers import QMethods
    from tests.harness_bert import QBertForSequenceClassification
    torch.manual_seed(0)
    cfg = BertConfig(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, num_labels=2,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    base = QBertForSequenceClassification(BertForSequenceClassification(cfg).eval(), method=QMethods.symmetric_uniform,
                                          act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8).cuda()
    g = torch.Generator().manual_seed(0)
    ids, labels = torch.randint(1000, 30000, (2, 64), generator=g).cuda(), torch.randint(0, 2, (2,), generator=g).cuda()
    with torch.no_grad():
        base.set_quant_state(True, True)
        base.estimate_ranges()
        base(ids)
    base.learn_ranges()
    _step_arms(base.train(), (ids,), (labels,), torch.nn.functional.cross_entropy, switch)


def test_mobilebert_attention_module(switch):
    """the MobileBERT harness attention alone (2 heads of 64: denom 8): the step as above, and the range gradients of its two
    chain quantizers against the float64 terms built from the scores and grad_probs the layered run saw (a loss linear in the
    output, so grad_probs does not depend on which forward ran)"""
    from transformers import MobileBertConfig
    from transformers.models.mobilebert.modeling_mobilebert import MobileBertSelfAttention
    from harness.mobilebert import QMobileSelfAttention
    from quantization.quantizers import QMethods
    torch.manual_seed(0)
    cfg = MobileBertConfig(hidden_size=128, num_attention_heads=2, true_hidden_size=128, intra_bottleneck_size=128)
    att = QMobileSelfAttention(MobileBertSelfAttention(cfg).eval(), act_method=QMethods.asymmetric_uniform, n_bits=8,
                               n_bits_act=8).cuda()
    att.quantized()
    g = torch.Generator().manual_seed(1)
    h, w = torch.randn(2, 64, 128, generator=g).cuda(), torch.randn(2, 64, 128, generator=g).cuda()
    mask = torch.zeros(2, 1, 1, 64).cuda()
    mask[1, ..., 50:] = -10000.0
    with torch.no_grad():
        att(h, h, h, mask)
    att.learn_ranges()
    att.train()
    _step_arms(att, (h, h, h, mask), (), lambda y: (y * w).sum(), switch)
    qs, cap, grads = (att.attn_scores_act_quantizer, att.attn_probs_act_quantizer), {}, []
    hooks = [qs[0].register_forward_pre_hook(lambda m, a: cap.update(s=a[0].detach())),
             qs[1].register_forward_hook(lambda m, a, o: (cap.update(y=o.detach()), o.register_hook(lambda g_: cap.update(gy=g_)))[0])]
    for on in (False, True):                            # off with the hooks (layered anyway), then on without them
        switch(on)
        att.zero_grad()
        (att(h, h, h, mask) * w).sum().backward()
        grads.append([getattr(qs[i].activation_quantizer.quantizer, attr).grad.clone() for _, i, attr, _ in SITES])
        for hk in hooks:
            hk.remove()
    ref = K._reference(cap['s'].cpu(), cap['gy'].cpu(), mask.reshape(2, -1).cpu(), _qdict(qs[0]), _qdict(qs[1]), cap['y'].cpu())
    _assert_range_gradients(grads[1], grads[0], ref)
