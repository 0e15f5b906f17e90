"""Timings for the per-column residual + LayerNorm tail (tq_residual_layernorm_quant_axis_fwd).

1. The kernel alone beside the per-tensor kernel (res_ln_quant_k) on the same shapes, hipGraph replays of 20 launches.
2. BERT-base forward, README PEG recipe ({'x', 'h', 'y'}: 'ng6') and the per-tensor recipe, default route, hipGraph replay, at
   [8, 128] and [128, 128]: with the per-column tail, and with the backend method hidden -- which is exactly the route of the
   commit before it (fused.py asks `hasattr`): layered tails, fp32 FFN2, FFN1 writing its fp32 output.
Usage: python tools/tuning/peg_tail_time.py [> profiles/r07/peg_tail.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT]
import torch  # noqa: E402

from oracle import tq_oracle as O  # noqa: E402
from quantization import _hip, options  # noqa: E402


def graph_us(fn, inner=20, reps=30):
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
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def kernels():
    be = _hip.backend()
    d = 768
    gen = torch.Generator().manual_seed(0)
    print('kernel alone: median (min) us per launch; GB/s = (2 reads + 1 write) / median')
    for rows in (1024, 131072):
        for dtype in (torch.float32, torch.bfloat16):
            a = (torch.randn(rows, d, generator=gen) * 2).to(dtype).cuda()
            r = (torch.randn(rows, d, generator=gen) * 1.5).to(dtype).cuda()
            w, b = (1 + 0.1 * torch.randn(d, generator=gen)).cuda(), (0.05 * torch.randn(d, generator=gen)).cuda()
            group = (torch.arange(d) * 6) // d
            qt, qc = [], []
            for lo, hi in ((-7.0, 7.5), (-20.0, 22.0), (-6.0, 11.0)):
                dl, zf = O.asym_params_from_range(lo, hi, 8)
                qt.append((dl.cuda(), zf.cuda(), None, 8, False, False, 1e-8))
                dl, zf = O.asym_params_from_range(lo + 0.3 * group, hi - 0.2 * group, 8)
                qc.append((dl.contiguous().cuda(), zf.contiguous().cuda(), None, 8, False, False, 1e-8))
            nbytes = 3 * a.numel() * a.element_size()
            for name, fn in (('per-tensor res_ln_quant_k     ', lambda: be.residual_layernorm_quant(a, r, qt[0], qt[1], w, b, 1e-12, qt[2])),
                             ('per-column res_ln_quant_axis_k', lambda: be.residual_layernorm_quant_axis(a, r, qc[0], qc[1], w, b, 1e-12, qc[2])),
                             ('per-column kernel, y_idx      ', lambda: be.residual_layernorm_quant_axis(a, r, qc[0], qc[1], w, b, 1e-12, qc[2], want_idx=True))):
                med, mn = graph_us(fn, inner=20 if rows <= 4096 else 4)
                print(f'  [{rows:6d}, {d}] {str(dtype)[6:]:8s} {name}  {med:8.2f} ({mn:8.2f}) us   {nbytes / med / 1e3:7.1f} GB/s')


def model_forward(recipe, B, T, with_axis):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from harness.bert import apply_quant_dict, build_bert_base
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, **qp)
    apply_quant_dict(model, recipe)
    model = model.cuda().eval()
    gen = torch.Generator().manual_seed(B)
    ids = torch.randint(1000, 30000, (B, T), generator=gen).cuda()
    hidden = None
    if not with_axis:
        hidden = _hip.HipBackend.residual_layernorm_quant_axis
        del _hip.HipBackend.residual_layernorm_quant_axis
    try:
        with torch.no_grad():
            pass_data_for_range_estimation([(ids,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
            model.fix_ranges()
            options.INT8_LINEAR = 'auto'
            med, mn = graph_us(lambda: model(ids), inner=1, reps=40)
    finally:
        if hidden is not None:
            _hip.HipBackend.residual_layernorm_quant_axis = hidden
    return med, mn


def models():
    print("BERT-base forward, default route, hipGraph replay: median (min) us")
    for B in (8, 128):
        for name, recipe in (("PEG {'x','h','y'}: 'ng6'", {'x': 'ng6', 'h': 'ng6', 'y': 'ng6'}), ('per-tensor', {})):
            for with_axis in (False, True):
                med, mn = model_forward(recipe, B, 128, with_axis)
                print(f'  [{B:3d}, 128] {name:26s} {"with the per-column tail" if with_axis else "per-column tail hidden  "}  {med:9.1f} ({mn:9.1f}) us')


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    kernels()
    models()
