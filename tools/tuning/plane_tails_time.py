"""Timings for options.INT8_PLANE_TAILS (LayerNorm tails that write the byte planes of their 16-bit output;
tq_residual_layernorm_quant_planes_fwd).

1. The tail alone, fp32, d = 768, all three quantizers on, 16-bit output grid, at [1024, 768] and [131072, 768]: the two
   launches of the default route -- the existing tail (y: 12 B per element) followed by quantize_hilo over y (6 B) -- against
   the one launch that writes y and both planes (14 B).  hipGraph replays of `inner` repetitions, the arms interleaved round by
   round in one process; median, min and the quartiles of the time per repetition over the rounds.  The existing tail alone
   is a third arm: what the planes add to it.
2. BERT-base forward under the mixed-precision recipe {'x': 16, 'h': 16, 'y': 16}, default route, as a hipGraph replay with the
   option on against off, at [8,128] and [128,128]: one calibrated model, one graph per arm, replayed alternately.  The logits
   of the two arms must be equal (asserted).
The verdict lines compare each "on" arm's median with the spread (quartiles) of the "off" arm's repeats.
Usage: python tools/tuning/plane_tails_time.py [> profiles/r15/plane_tails.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import capture  # noqa: E402
from ires_time import fmt, interleaved, stats, verdict  # noqa: E402

EPS = 1e-8
RECIPE = {'x': 16, 'h': 16, 'y': 16}


def tails():
    be = _hip.backend()
    mk = lambda d, z, bits=8: (torch.tensor([d], device='cuda'), torch.tensor([z], device='cuda'), None, bits, False, False, EPS)
    q1, q2, q3 = mk(0.05, 120.0), mk(0.07, 131.0), mk(2.0e-4, 30000.0, 16)
    x_q = (q3[0], q3[1], 16, EPS)
    d = 768
    print('residual + LayerNorm tail alone, fp32, d = 768, three quantizers on, 16-bit output grid: us per repetition, hipGraph '
          'replays, arms interleaved')
    for rows, inner, reps in ((1024, 50, 40), (131072, 4, 40)):
        g = torch.Generator(device='cuda').manual_seed(rows)
        a = torch.randn(rows, d, device='cuda', generator=g) * 2.0
        r = torch.randn(rows, d, device='cuda', generator=g) * 1.5
        w, b = 1.0 + 0.1 * torch.randn(d, device='cuda', generator=g), 0.1 * torch.randn(d, device='cuda', generator=g)
        y_old = be.residual_layernorm_quant(a, r, q1, q2, w, b, 1e-12, q3)
        hi_old, lo_old = be.quantize_hilo(y_old, x_q)
        y_new, (hi, lo) = be.residual_layernorm_quant_planes(a, r, q1, q2, w, b, 1e-12, q3)
        assert torch.equal(y_old, y_new) and torch.equal(hi_old, hi) and torch.equal(lo_old, lo)

        def two_launches():
            be.quantize_hilo(be.residual_layernorm_quant(a, r, q1, q2, w, b, 1e-12, q3), x_q)
        arms = [capture(two_launches, inner),
                capture(lambda: be.residual_layernorm_quant_planes(a, r, q1, q2, w, b, 1e-12, q3), inner),
                capture(lambda: be.residual_layernorm_quant(a, r, q1, q2, w, b, 1e-12, q3), inner)]
        res = [stats(t) for t in interleaved(arms, inner, reps)]
        print(f'  [{rows}, {d}]   {inner} repetitions per replay, {reps} rounds')
        for name, bpe, s in (('existing tail + quantize_hilo (2 launches)', 18, res[0]), ('plane tail (1 launch)', 14, res[1]),
                             ('existing tail alone, no planes', 12, res[2])):
            print(f'    {name:44s} {bpe:2d} B/elem  {fmt(s)}   {rows * d * bpe / s["med"] * 1e-6:6.2f} TB/s at the median')
        print(f'    {"plane tail":44s} {res[1]["med"] / res[0]["med"]:.3f} x the two launches: '
              f'{verdict(res[1], res[0], "the two launches")};  {res[1]["med"] / res[2]["med"]:.3f} x the existing tail alone')
        del arms
        torch.cuda.empty_cache()


def calibrated_model(B, T):
    from harness.bert import apply_quant_dict, build_bert_base
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, **qp)
    apply_quant_dict(model, RECIPE)
    model = model.cuda().eval()
    ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(B)).cuda()
    with torch.no_grad():
        pass_data_for_range_estimation([(ids,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
        model.fix_ranges()
    return model, ids


def models():
    print(f'BERT-base forward, {RECIPE}, default route, hipGraph replay: us per forward, INT8_PLANE_TAILS on / off interleaved')
    counted = {}
    names = ('residual_layernorm_quant', 'residual_layernorm_quant_planes', 'quantize_hilo', 'linear_i16x8')
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
                options.INT8_LINEAR, options.INT8_PLANE_TAILS = 'auto', on
                counted.clear()
                with torch.no_grad():
                    out = [None]

                    def run():
                        out[0] = model(ids)
                    graphs.append(capture(run, 1))
                calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
                logits.append(out[0].clone())
            options.INT8_PLANE_TAILS = False
            on, off = (stats(t) for t in interleaved(graphs, 1, 60))
            equal = torch.equal(logits[0], logits[1])
            print(f'  [{B},128]  on  {fmt(on)}   launches per forward {calls[0]}')
            print(f'  {"":9s}  off {fmt(off)}   launches per forward {calls[1]}')
            print(f'  {"":9s}  on / off {on["med"] / off["med"]:.4f}: {verdict(on, off)};   logits equal: {equal}')
            assert equal, 'the logits of the two arms differ'
            del graphs, model
            torch.cuda.empty_cache()
    finally:
        options.INT8_PLANE_TAILS = False
        for n, f in orig.items():
            setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    tails()
    models()
