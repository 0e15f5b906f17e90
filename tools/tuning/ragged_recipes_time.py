"""Timings for options.INT8_RAGGED_RECIPES (the W8A16 and PEG recipes on the integer route at any token count: FFN1 as
tq_linear_i16x8_fwd / tq_linear_i8_cls_fwd over 64 * ceil(M / 64) rows instead of a requantize, an fp32 hipBLASLt GEMM, a
[M, 3072] fp32 activation, GELU and a fake-quant).

BERT-base forward as a hipGraph replay, INT8_RAGGED on in both arms: INT8_RAGGED_RECIPES on against the same build with it off
(the parent's route at these shapes); one calibrated model, one graph per arm, replayed alternately, 60 rounds; median, min and
quartiles.  Recipes {'x': 16, 'h': 16, 'y': 16} and {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'}.
1. padded batches [8,100] (M = 800 rows: 12.5 tiles) and [128,100] (M = 12800 = 200 whole tiles: FFN1 is on the integer route
   in both arms there, the switch changes no launch -- that pair is the control of the measurement)
2. packed batches (harness.bert.forward_packed), B = 8 and B = 128, lengths seeded, uniform in 16..128 (tools/tuning/packed_time.py)
3. the logits of the two arms.  They differ in FFN1 alone -- exact integer contraction against an fp32 GEMM -- so the logits
   differ by that GEMM's round-off, amplified by every quantized layer behind it.  The default-against-layered bar of
   tests/test_bert_mp16_route.py, max |on - off| <= 5 % of max |off|, is a statement about a 3-layer model: it is checked (and
   asserted) on 3-layer models of both recipes at [8,100]; the 12-layer figures of the timed models are printed beside it.
Usage: python tools/tuning/ragged_recipes_time.py [> profiles/r19/ragged_recipes.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import capture  # noqa: E402
from ires_time import fmt, interleaved, stats, verdict  # noqa: E402
from packed_time import T_MAX, lengths_of  # noqa: E402

RECIPES = (('W8A16', {'x': 16, 'h': 16, 'y': 16}), ('PEG', {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'}))
COUNTED = ('linear_i8', 'linear_i8_cls', 'linear_i16x8', 'quantize_hilo', 'attention_i8_ragged', 'attention_i8_varlen')
BAR = 0.05


def calibrated_model(recipe, B, T, layers=None):
    """BERT-base (or its first `layers` layers) under `recipe`, calibrated on one [B, T] batch on the default route"""
    from harness.bert import apply_quant_dict, build_bert_base
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_layers=layers, **qp)
    apply_quant_dict(model, recipe)
    model = model.cuda().eval()
    ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(B)).cuda()
    saved, options.INT8_RAGGED = options.INT8_RAGGED, False
    try:
        with torch.no_grad():
            pass_data_for_range_estimation([(ids,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
            model.fix_ranges()
    finally:
        options.INT8_RAGGED = saved
    return model


def logit_distance(logits):
    d = float((logits[0].float() - logits[1].float()).abs().max())
    return d, d / float(logits[1].float().abs().max())


def two_arms(fn, counted):
    """one graph per arm of `fn` (switch on, then off) -> (stats on, stats off, launches per forward of each, logits of each)"""
    graphs, logits, calls = [], [], []
    for on in (True, False):
        options.INT8_RAGGED_RECIPES = on
        counted.clear()
        with torch.no_grad():
            out = [None]

            def run():
                out[0] = fn()
            graphs.append(capture(run, 1))
        calls.append({k: v // 4 for k, v in counted.items()})       # 3 warm-up forwards + the captured one
        logits.append(out[0].clone())
    options.INT8_RAGGED_RECIPES = False
    s_on, s_off = (stats(t) for t in interleaved(graphs, 1, 60))
    return s_on, s_off, calls, logits


def report(label, s_on, s_off, calls, logits):
    d, share = logit_distance(logits)
    print(f'  {label}  on  {fmt(s_on)}   launches per forward {calls[0]}')
    print(f'  {"":{len(label)}s}  off {fmt(s_off)}   launches per forward {calls[1]}')
    print(f'  {"":{len(label)}s}  on / off {s_on["med"] / s_off["med"]:.4f}: {verdict(s_on, s_off)};   max |on - off| of the logits '
          f'{d:.3e} = {share:.4f} of max |off|')


def models():
    from harness.bert import pack_batch
    counted = {}
    orig = {n: getattr(_hip.HipBackend, n) for n in COUNTED}
    for n, f in orig.items():
        def wrapped(self, *a, _n=n, _f=f, **k):
            counted[_n] = counted.get(_n, 0) + 1
            return _f(self, *a, **k)
        setattr(_hip.HipBackend, n, wrapped)
    options.INT8_LINEAR, options.INT8_RAGGED = 'auto', True
    try:
        for name, recipe in RECIPES:
            print(f'BERT-base forward, {name} {recipe}, hipGraph replay, INT8_RAGGED on: us per forward, INT8_RAGGED_RECIPES on '
                  'against off, interleaved')
            for B in (8, 128):
                model = calibrated_model(recipe, B, T_MAX)          # (calibrated on the default route, whole tiles)
                ids = torch.randint(1000, 30000, (B, 100), generator=torch.Generator().manual_seed(B + 2)).cuda()
                report(f'padded [{B},100]', *two_arms(lambda: model(ids), counted))
                lens = lengths_of(B)
                p = torch.randint(1000, 30000, (B, T_MAX), generator=torch.Generator().manual_seed(B + 1))
                am = torch.zeros(B, T_MAX, dtype=torch.long)
                for b, n in enumerate(lens):
                    am[b, :n] = 1
                p_ids, p_pos, start, max_len = pack_batch(p, am)
                args = (p_ids.cuda(), p_pos.cuda(), start.cuda(), max_len)
                report(f'packed B = {B}, M = {p_ids.shape[1]}', *two_arms(lambda: model.forward_packed(*args), counted))
                del model
                torch.cuda.empty_cache()
    finally:
        options.INT8_RAGGED = options.INT8_RAGGED_RECIPES = False
        for n, f in orig.items():
            setattr(_hip.HipBackend, n, f)


def bar():
    """the logits of the two arms on 3-layer models at [8,100], against the bar of tests/test_bert_mp16_route.py"""
    print(f'3-layer models at [8,100], eager: max |on - off| of the logits against the bar of tests/test_bert_mp16_route.py ({BAR} of '
          'max |off|)')
    options.INT8_LINEAR, options.INT8_RAGGED = 'auto', True
    try:
        for name, recipe in RECIPES:
            model = calibrated_model(recipe, 8, T_MAX, layers=3)
            ids = torch.randint(1000, 30000, (8, 100), generator=torch.Generator().manual_seed(10)).cuda()
            logits = []
            for on in (True, False):
                options.INT8_RAGGED_RECIPES = on
                with torch.no_grad():
                    logits.append(model(ids).clone())
            d, share = logit_distance(logits)
            print(f'  {name:6s} max |on - off| {d:.3e} = {share:.4f} of max |off|: {"within" if share <= BAR else "OUTSIDE"} the bar')
            assert share <= BAR, 'the logits of the two arms differ by more than the default-against-layered bar'
            del model
    finally:
        options.INT8_RAGGED = options.INT8_RAGGED_RECIPES = False


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    models()
    bar()
