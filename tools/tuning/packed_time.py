"""Timings for PACKED variable-length batches on the integer route (tq_attention_i8_varlen_fwd, harness.bert.forward_packed)
beside the same batch padded to its longest sequence (options.INT8_RAGGED: the best route before packing existed).

Lengths: seeded, uniform in 16..128, one sequence forced to 128; B = 8 and B = 128.
1. The attention core alone, 12 heads of 64: the variable-length core over the M packed rows beside the ragged core over
   [B, 128] with -inf on the pad keys, as hipGraph replays of 40 launches, the arms interleaved round by round in one process.
   (The variable-length core still loops over all T_pad keys of a short sequence; it saves the workgroups beyond len_b.)
2. BERT-base W8A8 forward as a hipGraph replay: packed [1, M] beside padded [B, 128] with its attention mask, one calibrated
   model, one graph per arm, replayed alternately; M, B * max_len and whether the logits are equal.
Usage: python tools/tuning/packed_time.py [> profiles/r11/packed_route.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import calibrated_model, capture, interleaved_us  # noqa: E402

EPS = 1e-8
T_MAX = 128


def lengths_of(B):
    n = torch.randint(16, T_MAX + 1, (B,), generator=torch.Generator().manual_seed(1000 + B))
    n[0] = T_MAX
    return [int(v) for v in n]


def core():
    be = _hip.backend()
    H, D = 12, 64
    mk = lambda d, z: (torch.tensor([d], device='cuda'), torch.tensor([z], device='cuda'), None, 8, False, False, EPS)
    P = (mk(0.011, 120.0), mk(0.013, 131.0), mk(0.009, 128.0), mk(0.35, 128.0), mk(1.0 / 255, 0.0), mk(0.012, 125.0))
    print('attention core, 12 heads of 64: median (min) us per launch, 40 launches per replay, interleaved')
    for B in (8, 128):
        lens = lengths_of(B)
        M = sum(lens)
        g = torch.Generator().manual_seed(B)
        start = torch.tensor([0] + lens, dtype=torch.int32).cumsum(0).to(torch.int32).cuda()
        pq, pk, pv = (torch.randint(-128, 128, (1, M, H * D), generator=g).to(torch.int8).cuda() for _ in range(3))
        rq, rk, rv = (torch.randint(-128, 128, (B, T_MAX, H * D), generator=g).to(torch.int8).cuda() for _ in range(3))
        mask = torch.zeros(B, T_MAX, device='cuda')
        for b, n in enumerate(lens):
            mask[b, n:] = float('-inf')
        arms = [capture(lambda: be.attention_i8_varlen(pq, pk, pv, H, start, T_MAX, None, 8.0, *P, want_idx=True), 40),
                capture(lambda: be.attention_i8_ragged(rq, rk, rv, H, mask, 8.0, *P, want_idx=True), 40)]
        (mv, nv), (mr, nr) = interleaved_us(arms, 40)
        print(f'  B = {B:3d}  M = {M:5d}  B * max_len = {B * T_MAX:5d}   varlen {mv:7.2f} ({nv:7.2f})   ragged [B, 128] {mr:7.2f} ({nr:7.2f})   '
              f'ratio {mv / mr:.3f}')


def models():
    from harness.bert import pack_batch
    print('BERT-base W8A8 forward, hipGraph replay, INT8_RAGGED on: median (min) us; packed [1, M] | padded [B, 128] with its '
          'attention mask, interleaved')
    counted = {}
    names = ('attention_i8_varlen', 'attention_i8_ragged', 'attention_i8', 'linear_i8', 'linear_i8_grouped')
    orig = {n: getattr(_hip.HipBackend, n) for n in names}
    for n, f in orig.items():
        def wrapped(self, *a, _n=n, _f=f, **k):
            counted[_n] = counted.get(_n, 0) + 1
            return _f(self, *a, **k)
        setattr(_hip.HipBackend, n, wrapped)
    options.INT8_LINEAR, options.INT8_RAGGED = 'auto', True
    for B in (8, 128):
        model, _ = calibrated_model(B, T_MAX)
        lens = lengths_of(B)
        ids = torch.randint(1000, 30000, (B, T_MAX), generator=torch.Generator().manual_seed(B + 1))
        am = torch.zeros(B, T_MAX, dtype=torch.long)
        for b, n in enumerate(lens):
            am[b, :n] = 1
        p_ids, p_pos, start, max_len = pack_batch(ids, am)
        M = p_ids.shape[1]
        packed_args = (p_ids.cuda(), p_pos.cuda(), start.cuda(), max_len)
        padded_args = (ids.cuda(), am.cuda())
        graphs, logits, calls = [], [], []
        for fn in (lambda: model.forward_packed(*packed_args), lambda: model(*padded_args)):
            counted.clear()
            with torch.no_grad():
                out = [None]

                def run():
                    out[0] = fn()
                graphs.append(capture(run, 1))
            calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
            logits.append(out[0].clone())
        (mp, np_), (md, nd) = interleaved_us(graphs, 1, reps=60)
        print(f'  B = {B:3d}  M = {M:5d}  B * max_len = {B * max_len:5d} (rows {M / (B * max_len):.3f})   packed {mp:9.1f} ({np_:9.1f})   '
              f'padded {md:9.1f} ({nd:9.1f})   packed / padded {mp / md:.3f}')
        print(f'              integer launches per forward: packed {calls[0]}   padded {calls[1]}')
        print(f'              logits equal: {torch.equal(logits[0], logits[1])}   max |packed - padded| '
              f'{(logits[0] - logits[1]).abs().max().item():.3e}')
        del graphs, model
        torch.cuda.empty_cache()
    options.INT8_RAGGED = False
    for n, f in orig.items():
        setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    core()
    models()
