"""Timings for options.FUSED_ACT_AXIS_TRAINING (bias + per-column output quantizer of a QuantLinear in a PEG QAT step as
tq_bias_act_quant_axis_fwd + the one-launch backward tq_bias_act_quant_axis_bwd), always against the same build with the
switch off.

1. A query-like Linear forward + backward under autograd (a quantized Linear 768 -> 768 without activation function whose output
   quantizer runs per_groups=6, `layer(x).backward(gy)`; the GEMM, its backward and the weight quantizer run in both arms) at
   [1024, 768] and [16384, 768] (as [rows / 128, 128, 768]), with fixed and with learnable ranges: eager calls between two
   events, the two arms alternating in one process, medians with quartiles over 60 rounds after 10 warm-up rounds.
2. One BERT-base (12 layers) W8A8 QAT step under apply_activation_granularity(per_groups=6) with learnable ranges at [8,128]
   (quantization.data_parallel.train_step), eager and as a GraphedTrainStep, on against off, with options.FUSED_SOFTMAX_TRAINING,
   FUSED_LN_TRAINING, FUSED_LN_AXIS_TRAINING and FUSED_ACT_TRAINING on in BOTH arms: one model per arm from the same seed.
Usage: python tools/tuning/act_axis_training_time.py [query] [qat] [> profiles/r28/act_axis_training.txt]   (no name: both)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import options  # noqa: E402
from ires_time import alternating, report  # noqa: E402

OTHERS = ('FUSED_SOFTMAX_TRAINING', 'FUSED_LN_TRAINING', 'FUSED_LN_AXIS_TRAINING', 'FUSED_ACT_TRAINING')


def query():
    from quantization.autoquant_utils import quantize_model
    from quantization.quantizers import QMethods
    from utils.per_embd_quant_utils import set_act_quant_axis_and_groups
    print('Query-like Linear (768 -> 768 + per_groups=6 quantizer) forward + backward under autograd: us per call, eager, arms alternating')
    for rows in (1024, 16384):
        g = torch.Generator().manual_seed(28)
        x = torch.randn(rows // 128, 128, 768, generator=g).cuda().requires_grad_(True)
        gy = torch.randn(rows // 128, 128, 768, generator=g).cuda()
        for learn in (False, True):
            torch.manual_seed(0)
            layer = quantize_model(torch.nn.Linear(768, 768), method=QMethods.symmetric_uniform,
                                   act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8).cuda()
            with torch.no_grad():
                layer.quantized()
                set_act_quant_axis_and_groups(layer, axis=2, n_groups=6)
                layer.estimate_ranges()
                layer(x)
            layer.learn_ranges() if learn else layer.fix_ranges()
            layer.train()

            def call():
                x.grad = None
                layer.zero_grad()
                layer(x).backward(gy)
            off, on = alternating([(False, call), (True, call)], 'FUSED_ACT_AXIS_TRAINING')
            report(f'[{rows}, 768 -> 768] {"learnable" if learn else "fixed"} ranges', off, on)


def qat_step():
    from harness.bert import apply_activation_granularity, build_bert_base
    from quantization.data_parallel import GradientBuckets, train_step
    from quantization.graphs import GraphedTrainStep
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    for name in OTHERS:
        setattr(options, name, True)
    print('BERT-base W8A8 PEG (per_groups=6) QAT step, learnable ranges, [8,128], ' + ', '.join(OTHERS) + ' on in both arms: us per step')
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    g = torch.Generator(device='cuda').manual_seed(6000)
    ids = torch.randint(1000, 30000, (8, 128), device='cuda', generator=g)
    labels = torch.randint(0, 2, (8,), device='cuda', generator=g)
    loss_fn = torch.nn.functional.cross_entropy
    eager, graphed = [], []
    for on in (False, True):
        options.FUSED_ACT_AXIS_TRAINING = on
        model = build_bert_base(seed=1000, **qp)[0]
        apply_activation_granularity(model, per_groups=6)
        model = model.cuda()
        with torch.no_grad():
            model.eval()
            model.set_quant_state(True, True)
            model.estimate_ranges()
            model(ids)
        model.learn_ranges()
        model.set_quant_state(True, True)
        model.train()
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.SGD(params, lr=1e-4)
        gb = GradientBuckets(params)
        eager.append((on, lambda model=model, opt=opt, gb=gb: train_step(model, loss_fn, opt, gb, (ids,), (labels,))))
        step = GraphedTrainStep(model, loss_fn, opt, (ids,), (labels,), grad_sync=gb)
        graphed.append((on, lambda step=step: step((ids,), (labels,))))
    report('eager train_step', *alternating(eager, 'FUSED_ACT_AXIS_TRAINING'))
    report('GraphedTrainStep', *alternating(graphed, 'FUSED_ACT_AXIS_TRAINING'))
    for name in OTHERS:
        setattr(options, name, False)


if __name__ == '__main__':
    print(f'device: {torch.cuda.get_device_name(0)}')
    sections = {'query': query, 'qat': qat_step}
    for name in sys.argv[1:] or sections:
        sections[name]()
