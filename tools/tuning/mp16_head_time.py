"""Timings for BERT's head on tq_linear_i16x8_skinny_fwd (options.INT8_HEAD under the mixed-precision recipes and on packed
batches).  Everything is a hipGraph replay, the arms of a comparison interleaved round by round in one process; per arm the
median and the quartiles [q1, q3] in us.

1. The kernel alone beside tq_linear_i8_skinny_fwd at the same shapes: classifier (8, 2, 768) with planes in (16-bit input grid),
   pooler (8, 768, 768) on the first-token view with Tanh and planes out (16-bit output grid), and (200, 768, 768), the encoder
   Linear that takes the skinny plan with INT8_RAGGED and INT8_HEAD both on (25 row groups per column); the 16-bit entry's
   8-bit form (x_hi == NULL, int8 indices out) at every shape too, which is the 8-bit entry's launch and gives its bits.
2. BERT-base forward under the STS-B recipe {'x': 16, 'h': 16, 'y': 16, 'P': 16, 'C': 16} (one label) at [8, 128] and [128, 128],
   INT8_HEAD on, against the same build with `linear_i16x8_skinny` hidden from the backend -- the parent's route: pooler on the
   old skinny entry, classifier a layered fp32 GEMM.
3. `forward_packed` of BERT-base W8A8 with lengths uniform in 16..128 at B = 8 and B = 128, INT8_RAGGED and INT8_HEAD on,
   against the same hidden-method arm (the parent's packed head: index_select and two layered fp32 GEMMs).
The arms of 2 and 3 differ in the head's GEMM (exact integer against fp32), so their logits are compared as a maximum
difference, not for equality.
Usage: python tools/tuning/mp16_head_time.py [> profiles/r13/mp16_head.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT]
import torch  # noqa: E402

from quantization import _hip, options  # noqa: E402

EPS = 1e-8
STS_B = {'x': 16, 'h': 16, 'y': 16, 'P': 16, 'C': 16}


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
    """[(median, q1, q3)] per graph; one replay of each per round"""
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
        out.append((t[len(t) // 2], t[len(t) // 4], t[(3 * len(t)) // 4]))
    return out


def fmt(t, w=8, p=2):
    return f'{t[0]:{w}.{p}f} [{t[1]:{w}.{p}f}, {t[2]:{w}.{p}f}]'


def kernels():
    be = _hip.backend()
    gen = torch.Generator().manual_seed(0)
    print('skinny integer Linears alone: median [q1, q3] us per launch, interleaved, 50 launches per replay')
    inner = 50
    for name, (M, N, K), act in (('classifier', (8, 2, 768), _hip.ACT_NONE), ('pooler', (8, 768, 768), _hip.ACT_TANH),
                                 ('attn-out', (200, 768, 768), _hip.ACT_NONE)):
        pooler = name == 'pooler'
        idx = torch.randint(-128, 128, (M, 128, K) if pooler else (M, 1, K), generator=gen).to(torch.int8).cuda()
        x = idx[:, 0]                                         # the pooler reads the first token of a [8, 128, 768] index tensor in place
        w = torch.randint(-127, 128, (N, K), generator=gen).to(torch.int8).cuda()
        rs = be.rowsum_i8(w)
        b = (0.1 * torch.randn(N, generator=gen)).cuda()
        wd = torch.full((1,), 1.0 / (0.02 * 74 * 73.6 * K ** 0.5)).cuda()
        xq8 = (torch.tensor([0.02], device='cuda'), torch.tensor([127.3], device='cuda'), 8, EPS)
        q8 = (torch.tensor([2.0 / 255], device='cuda'), torch.tensor([127.5], device='cuda'), None, 8, False, False, EPS)
        q16 = (torch.tensor([2.0 / 65535], device='cuda'), torch.tensor([32767.5], device='cuda'), None, 16, False, False, EPS)
        old = lambda: be.linear_i8_skinny(x, w, rs, b, xq8, wd, EPS, act, q8, torch.float32, want_idx=True)
        new8 = lambda: be.linear_i16x8_skinny(x, w, rs, b, xq8, wd, EPS, act, q8, torch.float32, want_idx=True)
        a, c = old(), new8()
        same = torch.equal(a[0].view(torch.int32), c[0].view(torch.int32)) and torch.equal(a[1], c[1])
        if pooler:                                            # 8-bit input in place, y and both planes out
            what, wide = 'planes out', lambda: be.linear_i16x8_skinny(x, w, rs, b, xq8, wd, EPS, act, q16, torch.float32, want_planes=True)
        else:                                                 # planes in (a 16-bit pooled tensor), 16-bit logits
            hi = torch.randint(-128, 128, (M, K), generator=gen).to(torch.int8).cuda()
            lo = torch.randint(-128, 128, (M, K), generator=gen).to(torch.int8).cuda()
            xq16 = (torch.tensor([2.0 / 65535], device='cuda'), torch.tensor([32767.5], device='cuda'), 16, EPS)
            wd16 = wd / 256
            what, wide = 'planes in', lambda: be.linear_i16x8_skinny((hi, lo), w, rs, b, xq16, wd16, EPS, act, q16, torch.float32)
        t_old, t_new8, t_wide = interleaved_us([capture(f, inner) for f in (old, new8, wide)], inner)
        print(f'  {name:10s} ({M}, {N}, {K})  linear_i8_skinny {fmt(t_old)}   linear_i16x8_skinny 8-bit form {fmt(t_new8)} '
              f'(bits equal: {same})   {what} {fmt(t_wide)}')


def calibrated_model(B, T, quant_dict, num_labels):
    from quantization.quantizers import QMethods
    from quantization.range_estimators import RangeEstimators
    from harness.bert import apply_quant_dict, build_bert_base
    from utils.utils import pass_data_for_range_estimation
    qp = dict(method=QMethods.symmetric_uniform, act_method=QMethods.asymmetric_uniform, n_bits=8, n_bits_act=8,
              weight_range_method=RangeEstimators.current_minmax, act_range_method=RangeEstimators.running_minmax)
    model, _ = build_bert_base(seed=1000, num_labels=num_labels, **qp)
    apply_quant_dict(model, quant_dict)
    model = model.cuda().eval()
    ids = torch.randint(1000, 30000, (B, T), generator=torch.Generator().manual_seed(B)).cuda()
    with torch.no_grad():
        pass_data_for_range_estimation([(ids,)], model, act_quant=True, weight_quant=True, max_num_batches=1)
        model.fix_ranges()
    return model, ids


class _Counter:
    """launch counts of the two skinny backend methods; `hide()` takes linear_i16x8_skinny away from the backend"""

    def __init__(self):
        self.n = {}
        self.orig = {m: getattr(_hip.HipBackend, m) for m in ('linear_i8_skinny', 'linear_i16x8_skinny')}
        for m in self.orig:
            self.show(m)

    def show(self, m='linear_i16x8_skinny'):
        orig, n = self.orig[m], self.n

        def counted(be, *a, **k):
            n[m] = n.get(m, 0) + 1
            return orig(be, *a, **k)
        setattr(_hip.HipBackend, m, counted)

    def hide(self):
        delattr(_hip.HipBackend, 'linear_i16x8_skinny')

    def restore(self):
        for m, f in self.orig.items():
            setattr(_hip.HipBackend, m, f)


def two_arms(run_of, counter):
    """capture `run_of()` with the new method shown, then hidden -> (graphs, logits, launches per forward)"""
    graphs, logits, calls = [], [], []
    for shown in (True, False):
        counter.show() if shown else counter.hide()
        counter.n.clear()
        out = [None]
        with torch.no_grad():
            run = run_of(out)
            graphs.append(capture(run, 1))
        calls.append({m.replace('linear_', ''): c // 4 for m, c in sorted(counter.n.items())})   # 3 warm-up forwards + the captured one
        logits.append(out[0].clone())
    counter.show()
    return graphs, logits, calls


def report(label, graphs, logits, calls):
    on, off = interleaved_us(graphs, 1, reps=60)
    d = (logits[0] - logits[1]).abs().max().item()
    print(f'  {label}  new entry {fmt(on, 9, 1)} {calls[0]}   hidden {fmt(off, 9, 1)} {calls[1]}   '
          f'new - hidden {on[0] - off[0]:+7.1f} us   ratio {on[0] / off[0]:.4f}   max |logits new - hidden| {d:.3e}')


def models(counter):
    print('BERT-base, STS-B recipe (one label), INT8_HEAD on, hipGraph replay: median [q1, q3] us; launches of the skinny methods '
          'per forward; hidden = linear_i16x8_skinny taken from the backend (the parent\'s route)')
    options.INT8_LINEAR, options.INT8_HEAD = 'auto', True
    for B in (8, 128):
        model, ids = calibrated_model(B, 128, STS_B, 1)

        def run_of(out):
            def run():
                out[0] = model(ids)
            return run
        report(f'[{B:3d}, 128]', *two_arms(run_of, counter))
        del model
        torch.cuda.empty_cache()
    options.INT8_HEAD = False


def packed(counter):
    from harness.bert import pack_batch
    print('BERT-base W8A8 forward_packed, lengths uniform in 16..128, INT8_RAGGED and INT8_HEAD on, hipGraph replay: as above')
    for B in (8, 128):
        options.INT8_LINEAR, options.INT8_RAGGED, options.INT8_HEAD = 'auto', False, False
        model, _ = calibrated_model(B, 128, {}, 2)
        g = torch.Generator().manual_seed(100 + B)
        lens = torch.randint(16, 129, (B,), generator=g)
        T = int(lens.max())
        ids = torch.randint(1000, 30000, (B, T), generator=g)
        am = (torch.arange(T)[None, :] < lens[:, None]).long()
        p_ids, p_pos, seq_start, max_len = pack_batch(ids, am)
        args = tuple(t.cuda() for t in (p_ids, p_pos, seq_start))
        options.INT8_RAGGED, options.INT8_HEAD = True, True

        def run_of(out):
            def run():
                out[0] = model.forward_packed(*args, max_len)
            return run
        report(f'B = {B:3d}, M = {p_ids.shape[1]:5d}', *two_arms(run_of, counter))
        del model
        torch.cuda.empty_cache()
    options.INT8_RAGGED, options.INT8_HEAD = False, False


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0))
    kernels()
    c = _Counter()
    try:
        models(c)
        packed(c)
    finally:
        c.restore()
