"""Timings for the 16-bit integer Linear (tq_linear_i16x8_fwd) and its byte-plane producer (tq_quantize_hilo_fwd).

1. BERT's first feed-forward Linear (768 -> 3072, GELU, 8-bit output quantizer through the staircase, index-only) on a
   16-bit input beside tq_linear_i8_stair_fwd at the same shape on an 8-bit input, M = 1024 and 16384: hipGraph replays,
   the two kernels interleaved round by round in one process.
2. quantize_hilo on [1024, 768] and [16384, 768] fp32.
3. BERT-base forward, README mixed-precision recipe ({'x': 16, 'h': 16, 'y': 16}), default route, hipGraph replay, at
   [8, 128] and [128, 128]: with the two backend methods, and with them hidden -- which is exactly the route of the commit
   before them (autoquant_utils.py asks `hasattr`): FFN1 as torch's fp32 GEMM + GELU + fake-quant launches.  The two
   graphs are replayed alternately in one process.
Usage: python tools/tuning/mp16_ffn_time.py [> profiles/r08/mp16_ffn.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT]
import torch  # noqa: E402

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


def interleaved_us(graphs, inner, reps=30):
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
    N, K = 3072, 768
    gen = torch.Generator().manual_seed(0)
    print('FFN1 768 -> 3072, GELU + 8-bit quantizer (staircase), index-only: median (min) us per launch, interleaved')
    for M in (1024, 16384):
        idx16 = torch.randint(0, 65536, (M, K), generator=gen)
        hi = ((idx16 >> 8) - 128).to(torch.int8).cuda()
        lo = ((idx16 & 255) - 128).to(torch.int8).cuda()
        x8 = torch.randint(-128, 128, (M, K), generator=gen).to(torch.int8).cuda()
        w = torch.randint(-127, 128, (N, K), generator=gen).to(torch.int8).cuda()
        rs = be.rowsum_i8(w)
        b = (0.1 * torch.randn(N, generator=gen)).cuda()
        wd = (0.001 + 0.002 * torch.rand(N, generator=gen)).cuda()
        xq16 = (torch.tensor([4e-4], device='cuda'), torch.tensor([30000.0], device='cuda'), 16, EPS)
        xq8 = (torch.tensor([0.1], device='cuda'), torch.tensor([117.0], device='cuda'), 8, EPS)
        q = (torch.tensor([0.0125], device='cuda'), torch.tensor([13.6], device='cuda'), None, 8, False, False, EPS)
        t16 = be.act_stair(_hip.ACT_GELU, q, be.i16x8_stair_bins_for(M, N, K))
        t8 = be.act_stair(_hip.ACT_GELU, q, be.stair_bins_for(M, N))
        f16 = lambda: be.linear_i16x8(hi, lo, w, rs, b, xq16, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, want_y=False, stair=t16)
        f8 = lambda: be.linear_i8(x8, w, rs, b, xq8, wd, EPS, _hip.ACT_GELU, q, torch.float32, want_idx=True, want_y=False, stair=t8)
        inner = 20 if M <= 4096 else 4
        (m16, n16), (m8, n8) = interleaved_us([capture(f16, inner), capture(f8, inner)], inner)
        print(f'  M = {M:5d}  linear_i16x8 {m16:8.2f} ({n16:8.2f})   linear_i8 {m8:8.2f} ({n8:8.2f})   ratio {m16 / m8:.2f}')
    print('quantize_hilo, fp32 input: median (min) us per launch; GB/s = (4 B read + 2 B written) per element / median')
    for M in (1024, 16384):
        x = torch.randn(M, K, generator=gen).cuda()
        xq = (torch.tensor([2e-4], device='cuda'), torch.tensor([30000.0], device='cuda'), 16, EPS)
        inner = 20
        (med, mn), = interleaved_us([capture(lambda: be.quantize_hilo(x, xq), inner)], inner)
        print(f'  [{M:5d}, {K}]  {med:8.2f} ({mn:8.2f}) us   {6 * x.numel() / med / 1e3:7.1f} GB/s')


def model_graph(B, T, with_route):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from harness.bert import apply_quant_dict, build_bert_base
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, **qp)
    apply_quant_dict(model, {'x': 16, 'h': 16, 'y': 16})
    model = model.cuda().eval()
    gen = torch.Generator().manual_seed(B)
    ids = torch.randint(1000, 30000, (B, T), generator=gen).cuda()
    hidden = {}
    if not with_route:
        for name in ('quantize_hilo', 'linear_i16x8'):
            hidden[name] = getattr(_hip.HipBackend, name)
            delattr(_hip.HipBackend, name)
    try:
        with torch.no_grad():
            pass_data_for_range_estimation([(ids,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
            model.fix_ranges()
            options.INT8_LINEAR = 'auto'
            g = capture(lambda: model(ids), 1)
    finally:
        for name, fn in hidden.items():
            setattr(_hip.HipBackend, name, fn)
    return g, model, ids


def models():
    print("BERT-base forward, {'x': 16, 'h': 16, 'y': 16}, default route, hipGraph replay: median (min) us, interleaved")
    for B in (8, 128):
        a = model_graph(B, 128, True)
        b = model_graph(B, 128, False)
        (ma, na), (mb, nb) = interleaved_us([a[0], b[0]], 1, reps=40)
        print(f'  [{B:3d}, 128]  with linear_i16x8 {ma:9.1f} ({na:9.1f})   methods hidden {mb:9.1f} ({nb:9.1f})   ratio {ma / mb:.3f}')
        del a, b
        torch.cuda.empty_cache()


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    kernels()
    models()
