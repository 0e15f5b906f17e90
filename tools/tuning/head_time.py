"""Timings for BERT's head on the integer route (options.INT8_HEAD: tq_linear_i8_skinny_fwd for pooler and classifier).

1. The two skinny launches alone beside torch's F.linear on fp32 operands at the same shapes -- pooler (8, 768, 768) with Tanh
   and an 8-bit output quantizer (indices emitted), classifier (8, 2, 768) with an 8-bit output quantizer -- as hipGraph
   replays, the arms interleaved round by round in one process.  F.linear is the GEMM ALONE of the layered route, which
   runs a Tanh and a fake-quant launch behind it.
2. BERT-base W8A8 default-route forward as a hipGraph replay at [8, 128] and [128, 128] with INT8_HEAD on and off; off is the
   route of the commit before the option existed.  The same calibrated model is captured once per arm and the two graphs are
   replayed alternately.  The head's launches per arm are counted from the backend methods during capture.
Usage: python tools/tuning/head_time.py [> profiles/r09/int8_head.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from quantization import _hip, options  # noqa: E402

EPS = 1e-8


def capture(fn, inner):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def interleaved_us(graphs, inner, reps=40):
    """[(median, min)] per graph; one replay of each per round"""
    ts = [[] for _ in graphs]
    for _ in range(reps):
        for k, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / inner)
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0]))
    return out


def kernels():
    be = _hip.backend()
    gen = torch.Generator().manual_seed(0)
    print('skinny integer Linear beside F.linear (fp32 GEMM alone): median (min) us per launch, interleaved, 50 launches per replay')
    for name, (M, N, K), act in (('pooler', (8, 768, 768), _hip.ACT_TANH), ('classifier', (8, 2, 768), _hip.ACT_NONE)):
        # the pooler reads the first token of each sequence of a [8, 128, 768] index tensor in place
        idx = torch.randint(-128, 128, (M, 128, K) if name == 'pooler' else (M, 1, K), generator=gen).to(torch.int8).cuda()
        x = idx[:, 0]
        w = torch.randint(-127, 128, (N, K), generator=gen).to(torch.int8).cuda()
        rs = be.rowsum_i8(w)
        b = (0.1 * torch.randn(N, generator=gen)).cuda()
        wd = torch.full((1,), 1.0 / (0.02 * 74 * 73.6 * K ** 0.5)).cuda()
        xq = (torch.tensor([0.02], device='cuda'), torch.tensor([127.3], device='cuda'), 8, EPS)
        q = (torch.tensor([2.0 / 255], device='cuda'), torch.tensor([127.5], device='cuda'), None, 8, False, False, EPS)
        xf, wf = torch.randn(M, K, generator=gen).cuda(), torch.randn(N, K, generator=gen).cuda()
        fs = lambda: be.linear_i8_skinny(x, w, rs, b, xq, wd, EPS, act, q, torch.float32, want_idx=True)
        ff = lambda: F.linear(xf, wf, b)
        inner = 50
        (ms, ns), (mf, nf) = interleaved_us([capture(fs, inner), capture(ff, inner)], inner)
        print(f'  {name:10s} ({M}, {N}, {K})  linear_i8_skinny {ms:7.2f} ({ns:7.2f})   F.linear {mf:7.2f} ({nf:7.2f})   ratio {ms / mf:.2f}')


def calibrated_model(B, T):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from harness.bert import build_bert_base
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, **qp)
    model = model.cuda().eval()
    ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(B)).cuda()
    with torch.no_grad():
        pass_data_for_range_estimation([(ids,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
        model.fix_ranges()
    return model, ids


def models():
    print('BERT-base W8A8 forward, default route, hipGraph replay: median (min) us, INT8_HEAD on / off interleaved')
    counted = {}
    orig = _hip.HipBackend.linear_i8_skinny

    def skinny(self, *a, **k):
        counted['skinny'] = counted.get('skinny', 0) + 1
        return orig(self, *a, **k)
    _hip.HipBackend.linear_i8_skinny = skinny
    for B in (8, 128):
        model, ids = calibrated_model(B, 128)
        graphs, logits, calls = [], [], []
        for on in (True, False):
            options.INT8_LINEAR, options.INT8_HEAD = 'auto', on
            counted.clear()
            with torch.no_grad():
                out = [None]

                def run():
                    out[0] = model(ids)
                graphs.append(capture(run, 1))
            calls.append(counted.get('skinny', 0) // 4)             # 3 warm-up forwards + the captured one
            logits.append(out[0].clone())
        options.INT8_HEAD = False
        (mon, non), (moff, noff) = interleaved_us(graphs, 1, reps=60)
        d = (logits[0] - logits[1]).abs().max().item()
        print(f'  [{B:3d}, 128]  INT8_HEAD on {mon:9.1f} ({non:9.1f}), {calls[0]} skinny launches per forward   off {moff:9.1f} ({noff:9.1f}), '
              f'{calls[1]}   on - off {mon - moff:+7.1f} us   ratio {mon / moff:.4f}   max |logits on - off| {d:.3e}')
        del graphs, model
        torch.cuda.empty_cache()
    _hip.HipBackend.linear_i8_skinny = orig


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    kernels()
    models()
