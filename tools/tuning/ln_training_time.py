"""Timings for options.FUSED_LN_TRAINING (the residual + LayerNorm tail of a QAT step as tq_residual_layernorm_quant_fwd + the
one-launch backward tq_residual_layernorm_quant_bwd).

1. Forward + backward of the tail under autograd (`fused.residual_layernorm_quant` on a harness tail block 768 -> 768,
   `y.backward(gy)`; the GEMM and its backward run in both arms) with the switch off (the layered modules) against on, at
   [1024,768] and [16384,768], with fixed and with learnable ranges: eager calls between two events, the two arms alternating
   in one process, medians with quartiles over 60 rounds after 10 warm-up rounds.
2. One BERT-base (12 layers) W8A8 QAT step with learnable ranges at [8,128] (quantization.data_parallel.train_step, built as
   bench.py's qat_dp block builds its model), eager and as a GraphedTrainStep, on against off -- once with
   options.FUSED_SOFTMAX_TRAINING off and once with it on in BOTH arms: one model per arm from the same seed, arms alternating.
3. The backward call alone at both shapes, for three sets of requested outputs (`backward_alone`).
Usage: python tools/tuning/ln_training_time.py [tail] [qat] [backward] [> profiles/r23/ln_training.txt]   (no name: all three)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import options  # noqa: E402
from ires_time import alternating, fmt, report  # noqa: E402



def tail():
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertSelfOutput
    from harness.bert import QResidualBlock
    from quantization.fused import residual_layernorm_quant
    from quantization.quantizers import QMethods
    print('tail forward + backward under autograd (GEMM 768 -> 768 included in both arms): us per call, eager, arms alternating')
    for rows in (1024, 16384):
        g = torch.Generator().manual_seed(23)
        x = torch.randn(rows, 768, generator=g).cuda().requires_grad_(True)
        r = torch.randn(rows, 768, generator=g).cuda().requires_grad_(True)
        gy = torch.randn(rows, 768, generator=g).cuda()
        for learn in (False, True):
            torch.manual_seed(0)
            blk = QResidualBlock(BertSelfOutput(BertConfig(hidden_dropout_prob=0.0)).eval(), method=QMethods.symmetric_uniform,
                                 act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8).cuda()
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
            off, on = alternating([(False, call), (True, call)], 'FUSED_LN_TRAINING')
            report(f'[{rows}, 768] {"learnable" if learn else "fixed"} ranges', off, on)


def qat_step(softmax_too):
    from harness.bert import build_bert_base
    from quantization.data_parallel import GradientBuckets, train_step
    from quantization.graphs import GraphedTrainStep
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    options.FUSED_SOFTMAX_TRAINING = softmax_too
    print(f'BERT-base W8A8 QAT step, learnable ranges, [8,128], FUSED_SOFTMAX_TRAINING = {softmax_too} in both arms: us per step')
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    g = torch.Generator(device='cuda').manual_seed(6000)
    ids = torch.randint(1000, 30000, (8, 128), device='cuda', generator=g)
    labels = torch.randint(0, 2, (8,), device='cuda', generator=g)
    loss_fn = torch.nn.functional.cross_entropy
    eager, graphed = [], []
    for on in (False, True):
        options.FUSED_LN_TRAINING = on
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
    report('eager train_step', *alternating(eager, 'FUSED_LN_TRAINING'))
    report('GraphedTrainStep', *alternating(graphed, 'FUSED_LN_TRAINING'))
    options.FUSED_SOFTMAX_TRAINING = False


def backward_alone():
    """the backward call by itself (main + final launch): 20 calls back to back between two events, so a figure is the larger
    of the host's enqueue time and the device time per call; a kernel trace of this section gives the kernels' own times"""
    from quantization import _hip
    be = _hip.backend()
    print('residual_layernorm_quant_bwd alone: us per call (20 back to back), GB/s at 20 B per element')
    mk = lambda d, z: (torch.tensor([d], device='cuda'), torch.tensor([z], device='cuda'), None, 8, False, False, 1e-8)
    q1, q2, q3 = mk(0.02, 128.0), mk(0.025, 120.0), mk(0.017, 119.0)
    for rows in (1024, 16384):
        g = torch.Generator().manual_seed(23)
        a, r, gy = (torch.randn(rows, 768, generator=g).cuda() for _ in range(3))
        w, b = torch.ones(768, device='cuda'), torch.zeros(768, device='cuda')
        for name, want in (('data gradients only', ('dense', 'residual')),
                           ('+ affine', ('dense', 'residual', 'ln_weight', 'ln_bias')),
                           ('+ affine + ranges', ('dense', 'residual', 'ln_weight', 'ln_bias', 'q_dense', 'q_sum', 'q_out'))):
            def call():
                for _ in range(20):
                    be.residual_layernorm_quant_bwd(a, r, gy, q1, q2, w, b, 1e-12, q3, want=want)
            s, = alternating([(False, call)], 'FUSED_LN_TRAINING')
            print(f'[{rows}, 768] {name}\n    {fmt({k: v / 20 for k, v in s.items()})}    {rows * 768 * 20 / (s["med"] / 20) / 1e3:.0f} GB/s',
                  flush=True)


if __name__ == '__main__':
    print(f'device: {torch.cuda.get_device_name(0)}')
    sections = {'tail': tail, 'qat': lambda: (qat_step(False), qat_step(True)), 'backward': backward_alone}
    for name in sys.argv[1:] or sections:
        sections[name]()
