"""Timings for options.INT8_PLANE_RESIDUALS (site x of a W8A16 layer as byte planes and row flags alone;
tq_residual_layernorm_quant_pres_fwd).

1. The two forms alone, fp32, d = 768, all three quantizers on, at [1024, 768] and [131072, 768], each beside the launch it
   replaces under INT8_PLANE_TAILS: hipGraph replays of `inner` repetitions, the arms interleaved round by round in one
   process; median, min and the quartiles of the time per repetition over the rounds.
     F1 (attention-output tail)  plane tail (fp32 residual; y + planes: 14 B per element) against planes-out with the residual
                                 as fp32 (4 + 4 + 2 = 10 B) and as int8 indices + flags (4 + 1 + 2 = 7 B)
     F2 (feed-forward tail)      existing tail with y_idx (fp32 residual: 4 + 4 + 4 + 1 = 13 B) against planes-in (4 + 2 + 4 + 1
                                 = 11 B)
2. BERT-base forward under the mixed-precision recipe {'x': 16, 'h': 16, 'y': 16}, default route, as a hipGraph replay at [8,128]
   and [128,128]: INT8_PLANE_RESIDUALS on against the same build with it off and INT8_PLANE_TAILS on; one calibrated model, one
   graph per arm, replayed alternately.  The logits of the two arms must be equal (asserted).
The verdict lines compare each new arm's median with the spread (quartiles) of the arm it replaces.
Usage: python tools/tuning/plane_residuals_time.py [> profiles/r17/plane_residuals.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import capture  # noqa: E402
from ires_time import fmt, interleaved, stats, verdict  # noqa: E402
from plane_tails_time import RECIPE, calibrated_model  # noqa: E402

EPS = 1e-8


def tails():
    be = _hip.backend()
    mk = lambda d, z, bits=8: (torch.tensor([d], device='cuda'), torch.tensor([z], device='cuda'), None, bits, False, False, EPS)
    q1, q2, q8, q16, qh = mk(0.05, 120.0), mk(0.07, 131.0), mk(0.03, 128.0), mk(2.0e-4, 30000.0, 16), mk(0.04, 127.0)
    d = 768
    print('the two forms alone, fp32, d = 768, three quantizers on: us per repetition, hipGraph replays, arms interleaved')
    for rows, inner, reps in ((1024, 50, 40), (131072, 4, 40)):
        g = torch.Generator(device='cuda').manual_seed(rows)
        a = torch.randn(rows, d, device='cuda', generator=g) * 2.0
        h, h_idx = be.fake_quant_int8(torch.randn(rows, d, device='cuda', generator=g) * 1.5, qh[0], qh[1], 8, EPS)
        w, b = 1.0 + 0.1 * torch.randn(d, device='cuda', generator=g), 0.1 * torch.randn(d, device='cuda', generator=g)
        flags = torch.zeros(rows, dtype=torch.uint8, device='cuda')
        x, planes = be.residual_layernorm_quant_planes(a, h, q1, q2, w, b, 1e-12, q16)
        for res in ((h, None, None, None, None), (None, h_idx, None, qh, flags)):
            _, _, p, n = be.residual_layernorm_quant_pres(a, *res, q1, q2, w, b, 1e-12, q16, want_y=False, want_planes=True)
            assert torch.equal(p[0], planes[0]) and torch.equal(p[1], planes[1]) and not bool(n.any())
        y_old, i_old = be.residual_layernorm_quant(a, x, q1, q2, w, b, 1e-12, q8, want_idx=True)
        y_new, i_new, _, n = be.residual_layernorm_quant_pres(a, None, None, planes, q16, flags, q1, q2, w, b, 1e-12, q8,
                                                              want_y=True, want_idx=True)
        assert torch.equal(y_old, y_new) and torch.equal(i_old, i_new) and not bool(n.any())
        f1 = [capture(lambda: be.residual_layernorm_quant_planes(a, h, q1, q2, w, b, 1e-12, q16), inner),
              capture(lambda: be.residual_layernorm_quant_pres(a, h, None, None, None, None, q1, q2, w, b, 1e-12, q16, want_y=False,
                                                               want_planes=True), inner),
              capture(lambda: be.residual_layernorm_quant_pres(a, None, h_idx, None, qh, flags, q1, q2, w, b, 1e-12, q16, want_y=False,
                                                               want_planes=True), inner)]
        f2 = [capture(lambda: be.residual_layernorm_quant(a, x, q1, q2, w, b, 1e-12, q8, want_idx=True), inner),
              capture(lambda: be.residual_layernorm_quant_pres(a, None, None, planes, q16, flags, q1, q2, w, b, 1e-12, q8, want_y=True,
                                                               want_idx=True), inner)]
        res = [stats(t) for t in interleaved(f1 + f2, inner, reps)]
        print(f'  [{rows}, {d}]   {inner} repetitions per replay, {reps} rounds')
        rows_out = (('F1  plane tail (fp32 residual, y + planes)', 14, res[0]), ('F1  planes out, fp32 residual', 10, res[1]),
                    ('F1  planes out, int8 index residual + flags', 7, res[2]), ('F2  existing tail, fp32 residual, y + y_idx', 13, res[3]),
                    ('F2  planes in + flags, y + y_idx', 11, res[4]))
        for name, bpe, s in rows_out:
            print(f'    {name:46s} {bpe:2d} B/elem  {fmt(s)}   {rows * d * bpe / s["med"] * 1e-6:6.2f} TB/s at the median')
        for new, old, what in ((1, 0, 'F1 fp32 residual'), (2, 0, 'F1 index residual'), (4, 3, 'F2')):
            print(f'    {what:46s} {res[new]["med"] / res[old]["med"]:.3f} x the launch it replaces: '
                  f'{verdict(res[new], res[old], "the launch it replaces")}')
        del f1, f2
        torch.cuda.empty_cache()


def models():
    print(f'BERT-base forward, {RECIPE}, default route, hipGraph replay: us per forward, INT8_PLANE_RESIDUALS on against off with '
          'INT8_PLANE_TAILS on, interleaved')
    counted = {}
    names = ('residual_layernorm_quant', 'residual_layernorm_quant_planes', 'residual_layernorm_quant_pres', 'quantize_hilo',
             'linear_i16x8')
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
                options.INT8_LINEAR, options.INT8_PLANE_TAILS, options.INT8_PLANE_RESIDUALS = 'auto', True, on
                counted.clear()
                with torch.no_grad():
                    out = [None]

                    def run():
                        out[0] = model(ids)
                    graphs.append(capture(run, 1))
                calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
                logits.append(out[0].clone())
            options.INT8_PLANE_TAILS = options.INT8_PLANE_RESIDUALS = False
            on, off = (stats(t) for t in interleaved(graphs, 1, 60))
            equal = torch.equal(logits[0], logits[1])
            print(f'  [{B},128]  on  {fmt(on)}   launches per forward {calls[0]}')
            print(f'  {"":9s}  off {fmt(off)}   launches per forward {calls[1]}')
            print(f'  {"":9s}  on / off {on["med"] / off["med"]:.4f}: {verdict(on, off)};   logits equal: {equal}')
            assert equal, 'the logits of the two arms differ'
            del graphs, model
            torch.cuda.empty_cache()
    finally:
        options.INT8_PLANE_TAILS = options.INT8_PLANE_RESIDUALS = False
        for n, f in orig.items():
            setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    tails()
    models()
