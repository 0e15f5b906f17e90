"""Timings for options.FUSED_SOFTMAX_TRAINING (the attention-probability chain of a QAT step as tq_scores_softmax_quant_fwd +
the one-launch backward tq_scores_softmax_quant_bwd).

1. Forward + backward of the chain under autograd (`fused.scores_softmax_quant` on two QuantizedActivations, `y.backward(gy)`)
   with the switch off (the layered modules) against on, at [8,12,128,128], [32,12,128,128] and MobileBERT's [32,4,128,128],
   with fixed and with learnable ranges: eager calls between two events, the two arms alternating in one process, medians
   with quartiles over 60 rounds after 10 warm-up rounds.
2. One BERT-base (12 layers) W8A8 QAT step with learnable ranges at [8,128] (quantization.data_parallel.train_step, built as
   bench.py's qat_dp block builds its model), eager and as a GraphedTrainStep, on against off: one model per arm from the same
   seed, the arms alternating.
Usage: python tools/tuning/softmax_training_time.py [> profiles/r22/softmax_training.txt]"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import options  # noqa: E402
from ires_time import alternating, report  # noqa: E402



def chain():
    from quantization.base_quantized_classes import QuantizedActivation
    from quantization.fused import scores_softmax_quant
    from quantization.quantizers import QMethods
    print('chain forward + backward under autograd: us per call, eager, arms alternating')
    for shape in ((8, 12, 128, 128), (32, 12, 128, 128), (32, 4, 128, 128)):
        g = torch.Generator().manual_seed(22)
        s = (torch.randn(*shape, generator=g) * 20).cuda().requires_grad_(True)
        gy = torch.randn(*shape, generator=g).cuda()
        mask = torch.zeros(shape[0], 1, 1, shape[3]).cuda()
        mask[-1, ..., 100:] = -10000.0
        for learn in (False, True):
            qa, qb = (QuantizedActivation(act_method=QMethods.asymmetric_uniform, n_bits_act=8).cuda() for _ in range(2))
            with torch.no_grad():
                for m in (qa, qb):
                    m.quantized_acts()
                qb(torch.softmax(qa(s) / 8.0 + mask, dim=-1))
            for m in (qa, qb):
                m.learn_ranges() if learn else m.fix_ranges()

            def call():
                s.grad = None
                scores_softmax_quant(qa, qb, s, mask, 8.0).backward(gy)
            off, on = alternating([(False, call), (True, call)], 'FUSED_SOFTMAX_TRAINING')
            report(f'{list(shape)} {"learnable" if learn else "fixed"} ranges', off, on)


def qat_step():
    from harness.bert import build_bert_base
    from quantization.data_parallel import GradientBuckets, train_step
    from quantization.graphs import GraphedTrainStep
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    print('BERT-base W8A8 QAT step, learnable ranges, [8,128]: us per step, arms alternating')
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    g = torch.Generator(device='cuda').manual_seed(6000)
    ids = torch.randint(1000, 30000, (8, 128), device='cuda', generator=g)
    labels = torch.randint(0, 2, (8,), device='cuda', generator=g)
    loss_fn = torch.nn.functional.cross_entropy
    eager, graphed = [], []
    for on in (False, True):
        options.FUSED_SOFTMAX_TRAINING = on
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
    report('eager train_step', *alternating(eager, 'FUSED_SOFTMAX_TRAINING'))
    report('GraphedTrainStep', *alternating(graphed, 'FUSED_SOFTMAX_TRAINING'))


if __name__ == '__main__':
    print(f'device: {torch.cuda.get_device_name(0)}; denominators: sqrt(64) = {math.sqrt(64.0)}')
    chain()
    qat_step()
