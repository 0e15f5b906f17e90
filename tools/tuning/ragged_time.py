"""Timings for the integer route at sequence lengths that are no multiple of 64 (options.INT8_RAGGED:
tq_attention_i8_ragged_fwd + row tails of the tiled integer Linears).

1. The ragged attention core at T = 100 beside the whole-tile core at T = 128 (the launch a caller who pads to the tile pays),
   B = 8 and B = 64, 12 heads of 64, as hipGraph replays of 40 launches, the arms interleaved round by round in one process.
2. BERT-base W8A8 default-route forward as a hipGraph replay at [8, 100] and [128, 100]: INT8_RAGGED on, off (off is the route of
   the commit before the option existed: encoder Linears and attention layered) and the default route on the same batch padded
   by the caller to T = 128 with attention_mask = 0 on the pads.  One calibrated model, one graph per arm, replayed alternately.
Usage: python tools/tuning/ragged_time.py [> profiles/r10/ragged_route.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import calibrated_model, capture, interleaved_us  # noqa: E402

EPS = 1e-8


def core():
    be = _hip.backend()
    H, D = 12, 64
    mk = lambda d, z: (torch.tensor([d], device='cuda'), torch.tensor([z], device='cuda'), None, 8, False, False, EPS)
    P = (mk(0.011, 120.0), mk(0.013, 131.0), mk(0.009, 128.0), mk(0.35, 128.0), mk(1.0 / 255, 0.0), mk(0.012, 125.0))
    print('attention core, 12 heads of 64: median (min) us per launch, 40 launches per replay, interleaved')
    for B in (8, 64):
        arms = []
        for T, fn in ((100, be.attention_i8_ragged), (128, be.attention_i8)):
            g = torch.Generator().manual_seed(T)
            qi, ki, vi = (torch.randint(-128, 128, (B, T, H * D), generator=g).to(torch.int8).cuda() for _ in range(3))
            mask = torch.zeros(B, T, device='cuda')
            mask[1, T - 20:] = -10000.0
            arms.append(capture(lambda fn=fn, a=(qi, ki, vi, mask): fn(a[0], a[1], a[2], H, a[3], 8.0, *P, want_idx=True), 40))
        (mr, nr), (mw, nw) = interleaved_us(arms, 40)
        print(f'  B = {B:3d}   ragged T = 100 {mr:7.2f} ({nr:7.2f})   whole-tile T = 128 {mw:7.2f} ({nw:7.2f})   ratio {mr / mw:.3f}')


def models():
    print('BERT-base W8A8 forward, hipGraph replay: median (min) us; INT8_RAGGED on | off at [B, 100] | default route at [B, 128] '
          '(the batch padded by the caller), interleaved')
    counted = {}
    orig = {n: getattr(_hip.HipBackend, n) for n in ('attention_i8_ragged', 'attention_i8', 'linear_i8', 'linear_i8_grouped')}
    for n, f in orig.items():
        def wrapped(self, *a, _n=n, _f=f, **k):
            counted[_n] = counted.get(_n, 0) + 1
            return _f(self, *a, **k)
        setattr(_hip.HipBackend, n, wrapped)
    for B in (8, 128):
        model, _ = calibrated_model(B, 128)
        T = 100
        ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(B + 1)).cuda()
        am = torch.ones(B, T, dtype=torch.long, device='cuda')
        am[1, 80:] = 0
        ids_p = torch.cat([ids, torch.full((B, 28), 1000, device='cuda')], 1)
        am_p = torch.cat([am, torch.zeros(B, 28, dtype=torch.long, device='cuda')], 1)
        graphs, logits, calls = [], [], []
        for on, args in ((True, (ids, am)), (False, (ids, am)), (False, (ids_p, am_p))):
            options.INT8_LINEAR, options.INT8_RAGGED = 'auto', on
            counted.clear()
            with torch.no_grad():
                out = [None]

                def run():
                    out[0] = model(*args)
                graphs.append(capture(run, 1))
            calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
            logits.append(out[0].clone())
        options.INT8_RAGGED = False
        (mon, non), (moff, noff), (mpad, npad) = interleaved_us(graphs, 1, reps=60)
        print(f'  [{B:3d}, 100]  on {mon:9.1f} ({non:9.1f})   off {moff:9.1f} ({noff:9.1f})   padded to 128 {mpad:9.1f} ({npad:9.1f})   '
              f'on / off {mon / moff:.3f}   on / padded {mon / mpad:.3f}')
        print(f'              integer launches per forward: on {calls[0]}   off {calls[1]}   padded {calls[2]}')
        print(f'              max |logits on - off| {(logits[0] - logits[1]).abs().max().item():.3e}   '
              f'max |logits on - padded| {(logits[0] - logits[2]).abs().max().item():.3e}')
        del graphs, model
        torch.cuda.empty_cache()
    for n, f in orig.items():
        setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    core()
    models()
