"""Timings for options.FUSED_ACT_TRAINING (bias + activation function + output quantizer of a QuantLinear in a QAT step as
tq_bias_act_quant_fwd + the one-launch backward tq_bias_act_quant_bwd).

1. FFN1 forward + backward under autograd (a quantized Linear 768 -> 3072 + GELU, `layer(x).backward(gy)`; the GEMM, its
   backward and the weight quantizer run in both arms) with the switch off (the layered modules) against on, at [1024, 768] and
   [16384, 768], with fixed and with learnable ranges: eager calls between two events, the two arms alternating in one process,
   medians with quartiles over 60 rounds after 10 warm-up rounds.
2. One BERT-base (12 layers) W8A8 QAT step with learnable ranges at [8,128] (quantization.data_parallel.train_step, built as
   bench.py's qat_dp block builds its model), eager and as a GraphedTrainStep, on against off, with
   options.FUSED_SOFTMAX_TRAINING and options.FUSED_LN_TRAINING on in BOTH arms: one model per arm from the same seed.
Usage: python tools/tuning/act_training_time.py [ffn1] [qat] [> profiles/r24/act_training.txt]   (no name: both)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import options  # noqa: E402
from ires_time import alternating, report  # noqa: E402



def ffn1():
    from quantization.autoquant_utils import quantize_model
    from quantization.quantizers import QMethods
    print('FFN1 (Linear 768 -> 3072 + GELU + quantizer) forward + backward under autograd: us per call, eager, arms alternating')
    for rows in (1024, 16384):
        g = torch.Generator().manual_seed(24)
        x = torch.randn(rows, 768, generator=g).cuda().requires_grad_(True)
        gy = torch.randn(rows, 3072, generator=g).cuda()
        for learn in (False, True):
            torch.manual_seed(0)
            layer = quantize_model(torch.nn.Sequential(torch.nn.Linear(768, 3072), torch.nn.GELU()), method=QMethods.symmetric_uniform,
                                   act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8)[0].cuda()
            with torch.no_grad():
                layer.quantized()
                layer.estimate_ranges()
                layer(x)
            layer.learn_ranges() if learn else layer.fix_ranges()
            layer.train()

            def call():
                x.grad = None
                layer.zero_grad()
                layer(x).backward(gy)
            off, on = alternating([(False, call), (True, call)], 'FUSED_ACT_TRAINING')
            report(f'[{rows}, 768 -> 3072] {"learnable" if learn else "fixed"} ranges', off, on)


def qat_step():
    from harness.bert import build_bert_base
    from quantization.data_parallel import GradientBuckets, train_step
    from quantization.graphs import GraphedTrainStep
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    options.FUSED_SOFTMAX_TRAINING = options.FUSED_LN_TRAINING = True
    print('BERT-base W8A8 QAT step, learnable ranges, [8,128], FUSED_SOFTMAX_TRAINING and FUSED_LN_TRAINING on in both arms: us per step')
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    g = torch.Generator(device='cuda').manual_seed(6000)
    ids = torch.randint(1000, 30000, (8, 128), device='cuda', generator=g)
    labels = torch.randint(0, 2, (8,), device='cuda', generator=g)
    loss_fn = torch.nn.functional.cross_entropy
    eager, graphed = [], []
    for on in (False, True):
        options.FUSED_ACT_TRAINING = on
        model = build_bert_base(seed=1000, **qp)[0].cuda()
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
    report('eager train_step', *alternating(eager, 'FUSED_ACT_TRAINING'))
    report('GraphedTrainStep', *alternating(graphed, 'FUSED_ACT_TRAINING'))
    options.FUSED_SOFTMAX_TRAINING = options.FUSED_LN_TRAINING = False


if __name__ == '__main__':
    print(f'device: {torch.cuda.get_device_name(0)}')
    sections = {'ffn1': ffn1, 'qat': qat_step}
    for name in sys.argv[1:] or sections:
        sections[name]()
