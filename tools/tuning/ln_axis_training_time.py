"""Timings for options.FUSED_LN_AXIS_TRAINING (the residual + LayerNorm tail of a PEG QAT step as
tq_residual_layernorm_quant_axis_fwd + the one-launch backward tq_residual_layernorm_quant_axis_bwd), always against the same
build with the switch off.

1. Forward + backward of the tail under autograd (`fused.residual_layernorm_quant` on a harness tail block 768 -> 768 whose three
   activation quantizers run per_groups=6, `y.backward(gy)`; the GEMM and its backward run in both arms) at [1024,768] and
   [16384,768] (as [rows / 128, 128, 768]), with fixed and with learnable ranges: eager calls between two events, the two arms
   alternating in one process, medians with quartiles over 60 rounds after 10 warm-up rounds.
2. One BERT-base (12 layers) W8A8 QAT step under apply_activation_granularity(per_groups=6) with learnable ranges at [8,128]
   (quantization.data_parallel.train_step), eager and as a GraphedTrainStep: one model per arm from the same seed, arms
   alternating.
Usage: python tools/tuning/ln_axis_training_time.py [tail] [qat] [> profiles/r25/ln_axis_training.txt]   (no name: both)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import options  # noqa: E402
from ires_time import alternating, report  # noqa: E402

QP = dict(n_bits=8, n_bits_act=8)


def tail():
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertSelfOutput
    from harness.bert import QResidualBlock
    from quantization.fused import residual_layernorm_quant
    from quantization.quantizers import QMethods
    from utils.per_embd_quant_utils import set_act_quant_axis_and_groups
    print('PEG tail (per_groups=6) forward + backward under autograd (GEMM 768 -> 768 included in both arms): us per call, eager, '
          'arms alternating')
    for rows in (1024, 16384):
        g = torch.Generator().manual_seed(25)
        x, r, gy = (torch.randn(rows // 128, 128, 768, generator=g).cuda() for _ in range(3))
        x.requires_grad_(True), r.requires_grad_(True)
        for learn in (False, True):
            torch.manual_seed(0)
            blk = QResidualBlock(BertSelfOutput(BertConfig(hidden_dropout_prob=0.0)).eval(), method=QMethods.symmetric_uniform,
                                 act_method=QMethods.asymmetric_uniform, **QP)
            for m in (blk.dense, blk.res_act_quantizer, blk.LayerNorm):
                set_act_quant_axis_and_groups(m, axis=2, n_groups=6)
            blk.cuda()
            with torch.no_grad():
                blk.set_quant_state(True, True)
                blk.estimate_ranges()
                blk(x, r)
            blk.learn_ranges() if learn else blk.fix_ranges()
            blk.train()

            def call():
                x.grad = r.grad = None
                blk.zero_grad()
                residual_layernorm_quant(blk.dense, blk.res_act_quantizer, blk.LayerNorm, x, r).backward(gy)
            off, on = alternating([(False, call), (True, call)], 'FUSED_LN_AXIS_TRAINING')
            report(f'[{rows}, 768] {"learnable" if learn else "fixed"} ranges', off, on)


def qat_step():
    from harness.bert import apply_activation_granularity, build_bert_base
    from quantization.data_parallel import GradientBuckets, train_step
    from quantization.graphs import GraphedTrainStep
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    print('BERT-base W8A8 PEG (per_groups=6) QAT step, learnable ranges, [8,128]: us per step')
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, **QP,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    g = torch.Generator(device='cuda').manual_seed(6000)
    ids = torch.randint(1000, 30000, (8, 128), device='cuda', generator=g)
    labels = torch.randint(0, 2, (8,), device='cuda', generator=g)
    loss_fn = torch.nn.functional.cross_entropy
    eager, graphed = [], []
    for on in (False, True):
        options.FUSED_LN_AXIS_TRAINING = on
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
    report('eager train_step', *alternating(eager, 'FUSED_LN_AXIS_TRAINING'))
    report('GraphedTrainStep', *alternating(graphed, 'FUSED_LN_AXIS_TRAINING'))


if __name__ == '__main__':
    print(f'device: {torch.cuda.get_device_name(0)}')
    sections = {'tail': tail, 'qat': qat_step}
    for name in sys.argv[1:] or sections:
        sections[name]()
