"""Timings for options.INT8_PEG_INDEX_RESIDUALS (residuals as int8 indices in the per-column LayerNorm tails;
tq_residual_layernorm_quant_axis_ires_fwd).

1. The two tail launches of a PEG layer alone, fp32, d = 768, all three quantizers on, 6 contiguous groups, at [1024, 768] and
   [131072, 768], each against tq_residual_layernorm_quant_axis_fwd with the same quantizers (fp32 residual, y + y_idx: 13 B per
   element): the attention-output tail (q_dense, q_sum per-tensor, q_out per-column) index-only with its residual as indices on
   a per-tensor grid (6 B) and with an fp32 residual (9 B: layer 0); the feed-forward tail (q_dense, q_sum per-column, q_out
   per-tensor) with its residual as indices on a per-column grid and y + y_idx (10 B) -- hipGraph replays of `inner` launches,
   the arms interleaved round by round in one process; median, min and the quartiles of the per-launch time over the rounds,
   and bytes / median.
2. BERT-base forward under {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'}, default route, as a hipGraph replay with the switch on against
   the same build with it off, at [8,128] and [128,128]: one calibrated model, one graph per arm, replayed alternately.  The
   logits of the two arms must be equal (asserted).
The verdict lines compare each "on" arm's median with the spread (quartiles) of the repeats of the arm it is compared with.
Usage: python tools/tuning/peg_ires_time.py [> profiles/r18/peg_index_residuals.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import capture  # noqa: E402
from ires_time import fmt, interleaved, stats, verdict  # noqa: E402

EPS = 1e-8
RECIPE = {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'}


def _grid(d, lo, hi, groups, seed):
    """7-tuple of an 8-bit asymmetric quantizer: one range (groups = 1, per-tensor) or `groups` contiguous runs of columns"""
    g = torch.Generator().manual_seed(seed)
    l = lo * (1 + 0.5 * torch.rand(groups, generator=g))
    h = hi * (1 + 0.5 * torch.rand(groups, generator=g))
    delta = (h - l) / 255
    zf = -l / delta
    if groups > 1:
        col = (torch.arange(d) * groups) // d
        delta, zf = delta[col], zf[col]
    return (delta.contiguous().cuda(), zf.contiguous().cuda(), None, 8, False, False, EPS)


def tails():
    be = _hip.backend()
    d = 768
    t = lambda lo, hi, s: _grid(d, lo, hi, 1, s)
    c = lambda lo, hi, s: _grid(d, lo, hi, 6, s)
    # (q_dense, q_sum, q_out, q_res) of the two tails of a PEG layer
    attn = (t(-6, 6, 1), t(-9, 9, 2), c(-4, 4, 3), t(-5, 5, 4))
    ffn = (c(-6, 6, 5), c(-9, 9, 6), t(-4, 4, 7), c(-5, 5, 8))
    print('per-column residual + LayerNorm tails alone, fp32, d = 768, three quantizers on, 6 groups: us per launch, hipGraph '
          'replays, arms interleaved')
    for rows, inner, reps in ((1024, 50, 40), (131072, 4, 40)):
        g = torch.Generator(device='cuda').manual_seed(rows)
        a = torch.randn(rows, d, device='cuda', generator=g) * 2.0
        r0 = torch.randn(rows, d, device='cuda', generator=g) * 1.5
        flags = torch.zeros(rows, dtype=torch.uint8, device='cuda')
        w, b = 1.0 + 0.1 * torch.randn(d, device='cuda', generator=g), 0.1 * torch.randn(d, device='cuda', generator=g)
        print(f'  [{rows}, {d}]   {inner} launches per replay, {reps} rounds')
        for name, (q1, q2, q3, qr), want_y in (('attention-output tail', attn, False), ('feed-forward tail', ffn, True)):
            n = qr[0].numel()
            r, _ = be.fake_quant(r0, qr[0], qr[1], None, 8, False, False, EPS, n, 1)
            r_idx = be.quantize_to_int8(r0, qr[0], qr[1], None, 8, False, False, EPS, n, 1, minus_128=True)
            y_old, i_old = be.residual_layernorm_quant_axis(a, r, q1, q2, w, b, 1e-12, q3, want_idx=True)
            y_new, i_new, _ = be.residual_layernorm_quant_axis_ires(a, None, r_idx, qr, flags, q1, q2, w, b, 1e-12, q3)
            assert torch.equal(y_old, y_new) and torch.equal(i_old, i_new)
            arms = [capture(lambda: be.residual_layernorm_quant_axis(a, r, q1, q2, w, b, 1e-12, q3, want_idx=True), inner),
                    capture(lambda: be.residual_layernorm_quant_axis_ires(a, None, r_idx, qr, flags, q1, q2, w, b, 1e-12, q3,
                                                                          want_y=want_y), inner)]
            rows_out = [('axis tail (fp32 residual, y + idx)', 13), (f'index residual, {"y + idx" if want_y else "index-only"}',
                                                                      10 if want_y else 6)]
            if not want_y:
                arms.append(capture(lambda: be.residual_layernorm_quant_axis_ires(a, r, None, None, None, q1, q2, w, b, 1e-12, q3,
                                                                                  want_y=False), inner))
                rows_out.append(('fp32 residual, index-only (layer 0)', 9))
            res = [stats(ts) for ts in interleaved(arms, inner, reps)]
            print(f'    {name}')
            for (what, bpe), s in zip(rows_out, res):
                print(f'      {what:40s} {bpe:2d} B/elem  {fmt(s)}   {rows * d * bpe / s["med"] * 1e-6:6.2f} TB/s at the median')
            for (what, _), s in list(zip(rows_out, res))[1:]:
                print(f'      {what:40s} {s["med"] / res[0]["med"]:.3f} x the axis tail: {verdict(s, res[0], "the axis tail")}')
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
    print(f'BERT-base forward, {RECIPE}, default route, hipGraph replay: us per forward, INT8_PEG_INDEX_RESIDUALS on / off '
          'interleaved')
    counted = {}
    names = ('residual_layernorm_quant_axis', 'residual_layernorm_quant_axis_ires', 'linear_i8_cls')
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
                options.INT8_LINEAR, options.INT8_PEG_INDEX_RESIDUALS = 'auto', on
                counted.clear()
                with torch.no_grad():
                    out = [None]

                    def run():
                        out[0] = model(ids)
                    graphs.append(capture(run, 1))
                calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
                logits.append(out[0].clone())
            options.INT8_PEG_INDEX_RESIDUALS = False
            on, off = (stats(t) for t in interleaved(graphs, 1, 60))
            equal = torch.equal(logits[0], logits[1])
            print(f'  [{B},128]  on  {fmt(on)}   launches per forward {calls[0]}')
            print(f'  {"":9s}  off {fmt(off)}   launches per forward {calls[1]}')
            print(f'  {"":9s}  on / off {on["med"] / off["med"]:.4f}: {verdict(on, off)};   logits equal: {equal}')
            assert equal, 'the logits of the two arms differ'
            del graphs, model
            torch.cuda.empty_cache()
    finally:
        options.INT8_PEG_INDEX_RESIDUALS = False
        for n, f in orig.items():
            setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    tails()
    models()
