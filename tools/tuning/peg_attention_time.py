"""Timings for options.INT8_PEG_ATTENTION (the attention half of a BERT layer on the integer route under `--per-groups N`:
tq_linear_i8_cls_grouped_fwd + the attention core with a grid per head).

1. BERT-base forward under apply_activation_granularity(per_groups=6), default route, as a hipGraph replay with the switch on
   against the same build with it off, at [8,128] and [128,128]: one calibrated model, one graph per arm, replayed alternately;
   medians with quartiles.  (The arms differ numerically: the off arm runs the attention half layered.)
2. The two new launches alone at those shapes: the index-only grouped class-ordered Linear [B * 128, 768] -> Q | K | V (six
   classes, per-column output grids of six groups, q_block 128) and the core with per-head grids (H = 12, d = 64), the latter
   beside the same launch with per-tensor grids.
3. `--core`: the per-tensor core alone at B = 8 and B = 64, T = 128, with whatever library TQ_LIB_PATH points at: run once per
   library, alternating, to compare two builds (the non-regression check of a change to the shared kernel body).
Usage: python tools/tuning/peg_attention_time.py [--core] [> profiles/r20/peg_attention.txt]"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import capture  # noqa: E402
from ires_time import fmt, interleaved, stats, verdict  # noqa: E402

EPS = 1e-8
H, HD, D = 12, 64, 768


def _grid(lo, hi, groups, seed, d=D):
    g = torch.Generator().manual_seed(seed)
    l = lo * (1 + 0.5 * torch.rand(groups, generator=g))
    h = hi * (1 + 0.5 * torch.rand(groups, generator=g))
    delta = (h - l) / 255
    zf = -l / delta
    if groups > 1:
        col = (torch.arange(d) * groups) // d
        delta, zf = delta[col], zf[col]
    return (delta.contiguous().cuda(), zf.contiguous().cuda(), None, 8, False, False, EPS)


def _core_operands(B, T=128):
    g = torch.Generator().manual_seed(B)
    q, k, v = (torch.randint(-128, 128, (B, T, D), generator=g).to(torch.int8).cuda() for _ in range(3))
    mask = torch.zeros(B, T)
    mask[1, 100:] = -10000.0
    return q, k, v, mask.cuda()


def core_only():
    be = _hip.backend()
    print(f'library: {_hip.LIB_PATH}')
    per_tensor = [_grid(-3, 3, 1, s) for s in (1, 2, 3)] + [_grid(-60, 60, 1, 4), _grid(0, 1, 1, 5), _grid(-1.2, 1.2, 1, 6)]
    for B, inner in ((8, 50), (64, 20)):
        q, k, v, mask = _core_operands(B)
        g = capture(lambda: be.attention_i8(q, k, v, H, mask, 8.0, *per_tensor, want_idx=True), inner)
        s = stats(interleaved([g], inner, 60)[0])
        print(f'  per-tensor core [{B},128,768]  us per launch {fmt(s)}')


def launches():
    be = _hip.backend()
    print('the two launches alone: us per launch, hipGraph replays, arms interleaved')
    per_tensor = [_grid(-3, 3, 1, s) for s in (1, 2, 3)] + [_grid(-60, 60, 1, 4), _grid(0, 1, 1, 5), _grid(-1.2, 1.2, 1, 6)]
    wide = [_grid(-3, 3, 6, s) for s in (1, 2, 3)] + per_tensor[3:5] + [_grid(-1.2, 1.2, 6, 6)]
    for B, inner in ((8, 50), (128, 10)):
        q, k, v, mask = _core_operands(B)
        arms = [capture(lambda: be.attention_i8(q, k, v, H, mask, 8.0, *per_tensor, want_idx=True), inner),
                capture(lambda: be.attention_i8(q, k, v, H, mask, 8.0, *wide, want_idx=True), inner)]
        a, b = (stats(t) for t in interleaved(arms, inner, 40))
        print(f'  core [{B},128,768]  per-tensor grids {fmt(a)}')
        print(f'  {"":16s}  per-head grids   {fmt(b)}   {b["med"] / a["med"]:.3f} x: {verdict(b, a, "per-tensor")}')
        # grouped class-ordered Linear: six classes of 128 input columns, Q | K | V with per-column output grids
        M = B * 128
        gen = torch.Generator().manual_seed(M)
        x = torch.randint(-128, 128, (M, D), generator=gen).to(torch.int8).cuda()
        w = torch.randint(-127, 128, (3 * D, D), generator=gen).to(torch.int8).cuda()
        ends = [128 * (c + 1) for c in range(6)]
        rs = torch.stack([be.rowsum_i8(w[:, e - 128:e].contiguous()) for e in ends]).contiguous()
        xq = _grid(-4, 4, 6, 9)
        table = be.cls_table(ends, [e - 128 for e in ends])
        wd = (0.002 + 0.001 * torch.rand(3 * D, generator=gen)).cuda()
        bias = torch.zeros(3 * D).cuda()
        outs = [_grid(-8, 8, 6, s) for s in (11, 12, 13)]
        one = [_grid(-8, 8, 1, s) for s in (11, 12, 13)]
        xq1 = (xq[0][:1].contiguous(), xq[1][:1].contiguous(), 8, EPS)
        arms = [capture(lambda: be.linear_i8_grouped(x, w, rs.sum(0, dtype=torch.int32), bias, xq1, wd, EPS, 0, one), inner),
                capture(lambda: be.linear_i8_cls_grouped(x, w, rs, bias, (xq[0], xq[1], 8, EPS), table, wd, EPS, 0, outs, 128), inner)]
        a, b = (stats(t) for t in interleaved(arms, inner, 40))
        print(f'  Q | K | V Linear [{M},768] -> 2304, index-only:  per-tensor route (tq_linear_i8_grouped_fwd) {fmt(a)}')
        print(f'  {"":16s}  tq_linear_i8_cls_grouped_fwd (6 classes, per-column outputs) {fmt(b)}   {b["med"] / a["med"]:.3f} x')
        del arms
        torch.cuda.empty_cache()


def calibrated_model(B, T):
    from harness.bert import apply_activation_granularity, build_bert_base
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, **qp)
    apply_activation_granularity(model, per_groups=6)
    model = model.cuda().eval()
    ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(B)).cuda()
    with torch.no_grad():
        pass_data_for_range_estimation([(ids,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
        model.fix_ranges()
    return model, ids


def models():
    print('BERT-base forward, apply_activation_granularity(per_groups=6), default route, hipGraph replay: us per forward, '
          'INT8_PEG_ATTENTION on / off interleaved')
    counted = {}
    names = ('linear_i8_cls_grouped', 'attention_i8', 'linear_i8_cls')
    orig = {n: getattr(_hip.HipBackend, n) for n in names}
    for n, f in orig.items():
        def wrapped(self, *a, _n=n, _f=f, **k):
            counted[_n] = counted.get(_n, 0) + 1
            return _f(self, *a, **k)
        setattr(_hip.HipBackend, n, wrapped)
    try:
        for B in (8, 128):
            model, ids = calibrated_model(B, 128)
            graphs, logits, calls = [], [], []
            for on in (True, False):
                options.INT8_LINEAR, options.INT8_PEG_ATTENTION = 'auto', on
                counted.clear()
                with torch.no_grad():
                    out = [None]

                    def run():
                        out[0] = model(ids)
                    graphs.append(capture(run, 1))
                calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
                logits.append(out[0].clone())
            options.INT8_PEG_ATTENTION = False
            on, off = (stats(t) for t in interleaved(graphs, 1, 60))
            print(f'  [{B},128]  on  {fmt(on)}   launches per forward {calls[0]}')
            print(f'  {"":9s}  off {fmt(off)}   launches per forward {calls[1]}')
            print(f'  {"":9s}  on / off {on["med"] / off["med"]:.4f}: {verdict(on, off)};   max |logit difference| '
                  f'{float((logits[0] - logits[1]).abs().max()):.4f} of max |off| {float(logits[1].abs().max()):.4f}')
            del graphs, model
            torch.cuda.empty_cache()
    finally:
        options.INT8_PEG_ATTENTION = False
        for n, f in orig.items():
            setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    if '--core' in sys.argv:
        core_only()
    else:
        launches()
        models()
