"""Timings for options.INT8_PEG_EMBEDDINGS (BERT's embedding block behind per-column quantizers as one launch:
tq_embeddings_layernorm_quant_axis_fwd).

1. The new launch alone at [1024,768] and [16384,768] (BERT-base tables, six column groups per site, y + y_idx), beside the
   per-tensor tq_embeddings_layernorm_quant_fwd on the same tables and ids and beside tq_residual_layernorm_quant_axis_fwd on
   dense rows of the same shape with the same quantizers: hipGraph replays, arms interleaved in one process, medians with
   quartiles.
2. BERT-base forward under apply_activation_granularity(per_groups=6), default route, as a hipGraph replay with the switch on
   against the same build with it off (the layered block: the route from before there was a switch), at [8,128] and
   [128,128], each once with INT8_PEG_ATTENTION on and once with it off: one calibrated model per shape, one graph per arm,
   replayed alternately.  (The arms differ numerically: the off arm runs torch's LayerNorm.)
Usage: python tools/tuning/peg_embeddings_time.py [> profiles/r21/peg_embeddings.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import capture  # noqa: E402
from ires_time import fmt, interleaved, stats, verdict  # noqa: E402
from peg_attention_time import _grid, calibrated_model  # noqa: E402

D, VOCAB, TYPES, POSITIONS = 768, 30522, 2, 512


def launches():
    be = _hip.backend()
    print('the launch alone: us per launch, hipGraph replays, arms interleaved')
    g = torch.Generator().manual_seed(21)
    word = (torch.randn(VOCAB, D, generator=g) * 1.6).cuda()
    typ = (torch.randn(TYPES, D, generator=g) * 1.2).cuda()
    pos = (torch.randn(POSITIONS, D, generator=g) * 1.5).cuda()
    w, b = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.05 * torch.randn(D, generator=g)).cuda()
    wide = [_grid(-7, 7, 6, 1), _grid(-9, 9, 6, 2), _grid(-5, 5, 6, 3)]
    one = [_grid(-7, 7, 1, 1), _grid(-9, 9, 1, 2), _grid(-5, 5, 1, 3)]
    for B, inner in ((8, 50), (128, 10)):
        rows = B * 128
        ids = torch.randint(0, VOCAB, (rows,), generator=g).cuda()
        tok = torch.randint(0, TYPES, (rows,), generator=g).cuda()
        pid = (torch.arange(rows) % 128).cuda()
        a = (word[ids] + typ[tok]).contiguous()
        r = pos[pid].contiguous()
        arms = [capture(lambda: be.embeddings_layernorm_quant_axis(word, ids, typ, tok, pos, pid, wide[0], wide[1], w, b, 1e-12,
                                                                   wide[2], want_idx=True), inner),
                capture(lambda: be.embeddings_layernorm_quant(word, ids, typ, tok, pos, pid, one[0], one[1], w, b, 1e-12, one[2],
                                                              want_idx=True), inner),
                capture(lambda: be.residual_layernorm_quant_axis(a, r, wide[0], wide[1], w, b, 1e-12, wide[2], want_idx=True),
                        inner)]
        new, tensor, tail = (stats(t) for t in interleaved(arms, inner, 40))
        print(f'  [{rows},768]  tq_embeddings_layernorm_quant_axis_fwd (six groups per site) {fmt(new)}')
        print(f'  {"":12s}  tq_embeddings_layernorm_quant_fwd (per-tensor)                {fmt(tensor)}   new / this '
              f'{new["med"] / tensor["med"]:.3f}')
        print(f'  {"":12s}  tq_residual_layernorm_quant_axis_fwd (dense rows)             {fmt(tail)}   new / this '
              f'{new["med"] / tail["med"]:.3f}')
        be.raise_deferred(sync=True)
        del arms, a, r
        torch.cuda.empty_cache()


def models():
    print('BERT-base forward, apply_activation_granularity(per_groups=6), default route, hipGraph replay: us per forward, '
          'INT8_PEG_EMBEDDINGS on / off interleaved')
    counted = {}
    names = ('embeddings_layernorm_quant_axis', 'linear_i8_cls_grouped')
    orig = {n: getattr(_hip.HipBackend, n) for n in names}
    for n, f in orig.items():
        def wrapped(self, *a, _n=n, _f=f, **k):
            counted[_n] = counted.get(_n, 0) + 1
            return _f(self, *a, **k)
        setattr(_hip.HipBackend, n, wrapped)
    try:
        for B in (8, 128):
            model, ids = calibrated_model(B, 128)
            for attention in (True, False):
                graphs, logits, calls = [], [], []
                for on in (True, False):
                    options.INT8_LINEAR, options.INT8_PEG_ATTENTION, options.INT8_PEG_EMBEDDINGS = 'auto', attention, on
                    counted.clear()
                    with torch.no_grad():
                        out = [None]

                        def run():
                            out[0] = model(ids)
                        graphs.append(capture(run, 1))
                    calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
                    logits.append(out[0].clone())
                options.INT8_PEG_EMBEDDINGS = options.INT8_PEG_ATTENTION = False
                on, off = (stats(t) for t in interleaved(graphs, 1, 60))
                print(f'  [{B},128]  INT8_PEG_ATTENTION {"on " if attention else "off"}  on  {fmt(on)}   launches per forward {calls[0]}')
                print(f'  {"":32s}  off {fmt(off)}   launches per forward {calls[1]}')
                print(f'  {"":32s}  on / off {on["med"] / off["med"]:.4f}: {verdict(on, off)};   max |logit difference| '
                      f'{float((logits[0] - logits[1]).abs().max()):.4f} of max |off| {float(logits[1].abs().max()):.4f}')
                del graphs
                torch.cuda.empty_cache()
            del model
            torch.cuda.empty_cache()
    finally:
        options.INT8_PEG_EMBEDDINGS = options.INT8_PEG_ATTENTION = False
        for n, f in orig.items():
            setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    launches()
    models()
