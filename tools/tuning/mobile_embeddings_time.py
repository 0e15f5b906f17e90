"""Timings for options.INT8_MOBILE_EMBEDDINGS (MobileBERT's embedding block as one exact integer launch:
tq_mobile_embeddings_nonorm_quant_fwd).

1. The block alone at [8,128] and [128,128] on the calibrated W4A4 model's own tables: the one launch beside the launches it
   replaces (the layered lines of QMobileEmbeddings.forward: look-up, pads and concat, fp32 GEMM, two look-ups, two adds,
   three fake-quant launches, the NoNorm launch), each as hipGraph replays, arms interleaved in one process, medians with
   quartiles.
2. The 24-layer MobileBERT W4A4 forward on the default route as a hipGraph replay with the switch on against the same build
   with it off, at the same shapes: one calibrated model per shape, one graph per arm, replayed alternately.  (The arms differ
   numerically: the off arm's transformation is an fp32 GEMM.)
Usage: python tools/tuning/mobile_embeddings_time.py [> profiles/r29/mobile_embeddings.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402
from head_time import capture  # noqa: E402
from ires_time import fmt, interleaved, stats, verdict  # noqa: E402

NAMES = ('mobile_embeddings_nonorm_quant', 'linear_i8_nonorm_grouped')


def calibrated_model(B, T):
    from harness.mobilebert import build_mobilebert
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=4, n_bits_act=4,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax,
              quant_dict={'attn_probs_n_bits_act': 8})
    model, _ = build_mobilebert(seed=1000, **qp)
    model = model.cuda().eval()
    ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(B)).cuda()
    with torch.no_grad():
        pass_data_for_range_estimation([(ids,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
        model.fix_ranges()
    return model, ids


def arms_of(fn, inner, counted):
    """one graph of `fn` per switch position (on, off) -> (graphs, outputs, launches per call)"""
    graphs, outs, calls = [], [], []
    for on in (True, False):
        options.INT8_MOBILE_EMBEDDINGS = on
        counted.clear()
        with torch.no_grad():
            out = [None]

            def run():
                out[0] = fn()
            graphs.append(capture(run, inner))
        calls.append(dict(counted))
        outs.append(out[0].clone())
    options.INT8_MOBILE_EMBEDDINGS = False
    return graphs, outs, calls


def main():
    counted = {}
    orig = {n: getattr(_hip.HipBackend, n) for n in NAMES}
    for n, f in orig.items():
        def wrapped(self, *a, _n=n, _f=f, **k):
            counted[_n] = counted.get(_n, 0) + 1
            return _f(self, *a, **k)
        setattr(_hip.HipBackend, n, wrapped)
    try:
        for B, inner in ((8, 20), (128, 5)):
            model, ids = calibrated_model(B, 128)
            graphs, outs, calls = arms_of(lambda: model.embeddings(ids), inner, counted)
            on, off = (stats(t) for t in interleaved(graphs, inner, 40))
            print(f'[{B},128]  the embedding block alone, us per call, hipGraph replays, arms interleaved')
            print(f'  one launch (switch on)          {fmt(on)}   calls while warming up and capturing {calls[0]}')
            print(f'  the launches it replaces (off)  {fmt(off)}')
            print(f'  on / off {on["med"] / off["med"]:.4f}: {verdict(on, off)};   outputs differ in '
                  f'{float((outs[0] != outs[1]).float().mean()):.5f} of the elements')
            del graphs
            graphs, outs, calls = arms_of(lambda: model(ids), 1, counted)
            on, off = (stats(t) for t in interleaved(graphs, 1, 60))
            print(f'[{B},128]  MobileBERT W4A4 forward (24 layers), default route, us per forward, hipGraph replays, arms interleaved')
            print(f'  switch on   {fmt(on)}   calls while warming up and capturing {calls[0]}')
            print(f'  switch off  {fmt(off)}   calls while warming up and capturing {calls[1]}')
            print(f'  on / off {on["med"] / off["med"]:.4f}: {verdict(on, off)}')
            del graphs, model
            torch.cuda.empty_cache()
    finally:
        options.INT8_MOBILE_EMBEDDINGS = False
        for n, f in orig.items():
            setattr(_hip.HipBackend, n, f)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    main()
