"""Timings for options.INT8_INDEX_RESIDUALS (residuals as int8 indices in the residual + LayerNorm tails;
tq_residual_layernorm_quant_ires_fwd).

1. The tail alone, fp32, d = 768, all three quantizers on, at [1024, 768] and [131072, 768], in three forms: the existing
   entry (fp32 residual, y + y_idx: 13 B per element), the new entry with the residual as indices + row flags and y + y_idx
   (10 B), and the same index-only (6 B) -- hipGraph replays of `inner` launches, the three arms interleaved round by round in
   one process; median, min and the quartiles of the per-launch time over the rounds, and bytes / median.
2. BERT-base W8A8 default-route forward as a hipGraph replay with the option on against off, at [8,128] and [128,128]: one
   calibrated model, one graph per arm, replayed alternately.  The logits of the two arms must be equal (asserted).
The verdict lines compare each "on" arm's median with the spread (quartiles) of the "off" arm's repeats.
Usage: python tools/tuning/ires_time.py [> profiles/r12/index_residuals.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import calibrated_model, capture  # noqa: E402

EPS = 1e-8


def interleaved(graphs, inner, reps):
    """per graph the sorted per-launch times in us over `reps` rounds; one replay of each graph per round"""
    ts = [[] for _ in graphs]
    for _ in range(reps):
        for k, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / inner)
    return [sorted(t) for t in ts]


def stats(t):
    n = len(t)
    return dict(med=t[n // 2], min=t[0], q1=t[n // 4], q3=t[(3 * n) // 4])


def fmt(s):
    return f"{s['med']:9.2f} (min {s['min']:9.2f}, quartiles {s['q1']:9.2f} .. {s['q3']:9.2f})"


def verdict(on, off, base='off'):
    """an "on" median against the spread of the repeats of the arm it is compared with"""
    if on['med'] < off['q1']:
        return f'ahead of {base} (below its lower quartile)'
    if on['med'] > off['q3']:
        return f'behind {base} (above its upper quartile)'
    return f'level with {base} (inside its quartiles)'


def tails():
    be = _hip.backend()
    mk = lambda d, z: (torch.tensor([d], device='cuda'), torch.tensor([z], device='cuda'), None, 8, False, False, EPS)
    q1, q2, q3, qr = mk(0.05, 120.0), mk(0.07, 131.0), mk(0.03, 128.0), mk(0.04, 127.0)
    d = 768
    print('residual + LayerNorm tail alone, fp32, d = 768, three quantizers on: us per launch, hipGraph replays, arms interleaved')
    for rows, inner, reps in ((1024, 50, 40), (131072, 4, 40)):
        g = torch.Generator(device='cuda').manual_seed(rows)
        a = torch.randn(rows, d, device='cuda', generator=g) * 2.0
        r, r_idx = be.fake_quant_int8(torch.randn(rows, d, device='cuda', generator=g) * 1.5, qr[0], qr[1], 8, EPS)
        flags = torch.zeros(rows, dtype=torch.uint8, device='cuda')
        w, b = 1.0 + 0.1 * torch.randn(d, device='cuda', generator=g), 0.1 * torch.randn(d, device='cuda', generator=g)
        y_old, i_old = be.residual_layernorm_quant(a, r, q1, q2, w, b, 1e-12, q3, want_idx=True)
        y_new, i_new, _ = be.residual_layernorm_quant_ires(a, None, r_idx, qr, flags, q1, q2, w, b, 1e-12, q3)
        assert torch.equal(y_old, y_new) and torch.equal(i_old, i_new)
        arms = [capture(lambda: be.residual_layernorm_quant(a, r, q1, q2, w, b, 1e-12, q3, want_idx=True), inner),
                capture(lambda: be.residual_layernorm_quant_ires(a, None, r_idx, qr, flags, q1, q2, w, b, 1e-12, q3), inner),
                capture(lambda: be.residual_layernorm_quant_ires(a, None, r_idx, qr, flags, q1, q2, w, b, 1e-12, q3, want_y=False),
                        inner)]
        res = [stats(t) for t in interleaved(arms, inner, reps)]
        print(f'  [{rows}, {d}]   {inner} launches per replay, {reps} rounds')
        for name, bpe, s in (('existing entry (fp32 residual, y + idx)', 13, res[0]),
                             ('index residual, y + idx', 10, res[1]), ('index residual, index-only', 6, res[2])):
            print(f'    {name:42s} {bpe:2d} B/elem  {fmt(s)}   {rows * d * bpe / s["med"] * 1e-6:6.2f} TB/s at the median')
        for name, s in (('index residual, y + idx', res[1]), ('index residual, index-only', res[2])):
            print(f'    {name:42s} {s["med"] / res[0]["med"]:.3f} x the existing entry: {verdict(s, res[0], "the existing entry")}')
        del arms
        torch.cuda.empty_cache()


def models():
    print('BERT-base W8A8 forward, default route, hipGraph replay: us per forward, INT8_INDEX_RESIDUALS on / off interleaved')
    counted = {}
    names = ('residual_layernorm_quant', 'residual_layernorm_quant_ires')
    orig = {n: getattr(_hip.HipBackend, n) for n in names}
    for n, f in orig.items():
        def wrapped(self, *a, _n=n, _f=f, **k):
            counted[_n] = counted.get(_n, 0) + 1
            return _f(self, *a, **k)
        setattr(_hip.HipBackend, n, wrapped)
    for B in (8, 128):
        model, ids = calibrated_model(B, 128)
        graphs, logits, calls = [], [], []
        for on in (True, False):
            options.INT8_LINEAR, options.INT8_INDEX_RESIDUALS = 'auto', on
            counted.clear()
            with torch.no_grad():
                out = [None]

                def run():
                    out[0] = model(ids)
                graphs.append(capture(run, 1))
            calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
            logits.append(out[0].clone())
        options.INT8_INDEX_RESIDUALS = False
        on, off = (stats(t) for t in interleaved(graphs, 1, 60))
        equal = torch.equal(logits[0], logits[1])
        print(f'  [{B},128]  on  {fmt(on)}   tail launches per forward {calls[0]}')
        print(f'  {"":9s}  off {fmt(off)}   tail launches per forward {calls[1]}')
        print(f'  {"":9s}  on / off {on["med"] / off["med"]:.4f}: {verdict(on, off)};   logits equal: {equal}')
        assert equal, 'the logits of the two arms differ'
        del graphs, model
        torch.cuda.empty_cache()
    for n, f in orig.items():
        setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    tails()
    models()
