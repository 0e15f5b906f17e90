"""Every residual + LayerNorm tail form alone, for an A/B of two builds of csrc/tq_fused_ln.hip: time and bits.

One process measures the library it was started with (TQ_LIB_PATH; build the other one with tools/tuning/build_ab_lib.py).
Seeded inputs without NaN, the three quantizers on, d = 768 at [1024, 768] and [131072, 768]:
  the eleven index / plane forms (RK, WY, IDX, PL) through their three entries (res_ln_quant_ires_k, res_ln_quant_pres_k and
  the plane tail, res_ln_quant_planes_k),
  res_ln_quant_k in fp32 and bf16 with and without y_idx, NoNorm at [1024, 512], the per-column tail in fp32 and bf16.
Per arm: median, min and quartiles of the time per launch over hipGraph replays, all arms of a size interleaved round by
round, and a digest of every output buffer (y, y_idx, both planes, row flags).

    python tools/tuning/tail_forms_ab.py --out run.json      one run: prints the table, keeps the raw times and digests
    python tools/tuning/tail_forms_ab.py --compare DIR       DIR/parent_*.json against DIR/new_*.json: per arm the digests
                                                             must be equal and the new median is placed against the
                                                             quartiles of the parent's replays (ires_time.verdict)
Run the two libraries as alternating child processes (parent, new, parent, new, ...: at least three of each), every run
under a time limit of its own and the next one only after the last one ended well:
    AB=$PWD/tools/tuning/_ab/libtq_hip.so; O=out; mkdir -p $O
    for i in 1 2 3; do
      TQ_LIB_PATH=$AB timeout -k 10 280 python tools/tuning/tail_forms_ab.py --out $O/parent_$i.json > $O/parent_$i.txt || exit 1
      timeout -k 10 280 python tools/tuning/tail_forms_ab.py --out $O/new_$i.json > $O/new_$i.txt || exit 1
    done
    python tools/tuning/tail_forms_ab.py --compare $O > profiles/r18/tail_forms_ab.txt"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, 'transformer-quantization_amd'), ROOT, os.path.dirname(os.path.abspath(__file__))]

EPS = 1e-8
LN_EPS = 1e-12


def digest(*tensors):
    """two position-dependent integer sums over the bytes of each buffer (exact, computed on the device)"""
    import torch
    out = []
    for t in tensors:
        if t is None:
            out.append('-')
            continue
        b = t.contiguous().view(torch.uint8).reshape(-1).to(torch.int64)
        pos = torch.arange(b.numel(), device=b.device, dtype=torch.int64)
        out.append(f'{int((b * (pos % 65521 + 1)).sum()) & (2 ** 64 - 1):016x}.{int((b * (pos % 251 + 3)).sum()) & (2 ** 32 - 1):08x}')
    return ' '.join(out)


def arms_for(be, rows, d, nonorm_d):
    """[(label, fn -> tuple of output buffers)] on seeded inputs of [rows, d]"""
    import torch
    mk = lambda dl, z, bits=8: (torch.tensor([dl], device='cuda'), torch.tensor([z], device='cuda'), None, bits, False, False, EPS)
    q1, q2, q8, q16, qh = mk(0.05, 120.0), mk(0.07, 131.0), mk(0.03, 128.0), mk(2.0e-4, 30000.0, 16), mk(0.04, 127.0)
    g = torch.Generator(device='cuda').manual_seed(rows)
    a = torch.randn(rows, d, device='cuda', generator=g) * 2.0
    h, h_idx = be.fake_quant_int8(torch.randn(rows, d, device='cuda', generator=g) * 1.5, qh[0], qh[1], 8, EPS)
    w, b = 1.0 + 0.1 * torch.randn(d, device='cuda', generator=g), 0.1 * torch.randn(d, device='cuda', generator=g)
    flags = torch.zeros(rows, dtype=torch.uint8, device='cuda')
    x, planes = be.residual_layernorm_quant_planes(a, h, q1, q2, w, b, LN_EPS, q16)
    ab, hb = a.bfloat16(), h.bfloat16()
    col = lambda q, s: (q[0].expand(d) * (1.0 + 0.25 * torch.rand(d, device='cuda', generator=g)) * s, q[1].expand(d).clone()) + q[2:]
    c1, c2, c3 = col(q1, 1.0), col(q2, 1.0), col(q8, 1.0)
    arms = []
    for rk, res in ((0, (h, None, None, None)), (1, (None, h_idx, qh, flags))):
        for wy, wi in ((False, True), (True, True), (True, False)):
            arms.append((f'ires   ({rk},{int(wy)},{int(wi)},0)',
                         lambda res=res, wy=wy, wi=wi: be.residual_layernorm_quant_ires(a, *res, q1, q2, w, b, LN_EPS, q8, want_y=wy,
                                                                                      want_idx=wi)))
    flat = lambda r: (r[0], r[1]) + (r[2] if r[2] is not None else (None, None)) + (r[3],)
    for wi in (True, False):
        arms.append((f'pres   (2,1,{int(wi)},0)',
                     lambda wi=wi: flat(be.residual_layernorm_quant_pres(a, None, None, planes, q16, flags, q1, q2, w, b, LN_EPS, q8,
                                                                         want_y=True, want_idx=wi))))
    arms.append(('pres   (1,0,0,1)', lambda: flat(be.residual_layernorm_quant_pres(a, None, h_idx, None, qh, flags, q1, q2, w, b, LN_EPS,
                                                                                   q16, want_y=False, want_planes=True))))
    arms.append(('pres   (0,0,0,1)', lambda: flat(be.residual_layernorm_quant_pres(a, h, None, None, None, None, q1, q2, w, b, LN_EPS, q16,
                                                                                   want_y=False, want_planes=True))))

    def plane_tail():
        y, (hi, lo) = be.residual_layernorm_quant_planes(a, h, q1, q2, w, b, LN_EPS, q16)
        return y, hi, lo
    arms.append(('planes (0,1,0,1)', plane_tail))
    for name, aa, rr in (('fp32', a, h), ('bf16', ab, hb)):
        arms.append((f'res_ln_quant_k {name}', lambda aa=aa, rr=rr: (be.residual_layernorm_quant(aa, rr, q1, q2, w, b, LN_EPS, q8),)))
        arms.append((f'res_ln_quant_k {name} + y_idx',
                     lambda aa=aa, rr=rr: be.residual_layernorm_quant(aa, rr, q1, q2, w, b, LN_EPS, q8, want_idx=True)))
        arms.append((f'axis tail {name} + y_idx',
                     lambda aa=aa, rr=rr: be.residual_layernorm_quant_axis(aa, rr, c1, c2, w, b, LN_EPS, c3, want_idx=True)))
    if nonorm_d:
        an, hn = a[:, :nonorm_d].contiguous(), h[:, :nonorm_d].contiguous()
        wn, bn = w[:nonorm_d].contiguous(), b[:nonorm_d].contiguous()
        arms.append((f'NoNorm fp32 [{rows}, {nonorm_d}]', lambda: (be.residual_layernorm_quant(an, hn, q1, q2, wn, bn, None, q8),)))
    return arms


def run(out_path):
    import torch
    from quantization import _hip
    from head_time import capture
    from ires_time import fmt, interleaved, stats
    be = _hip.backend()
    print(torch.cuda.get_device_name(0), ' library:', _hip.LIB_PATH)
    record = {}
    for rows, inner, reps, nonorm_d in ((1024, 50, 40, 512), (131072, 4, 40, 0)):
        arms = arms_for(be, rows, 768, nonorm_d)
        digests = []
        for _, fn in arms:
            r = fn()
            digests.append(digest(*(r if isinstance(r, tuple) else (r,))))
        graphs = [capture(fn, inner) for _, fn in arms]
        times = interleaved(graphs, inner, reps)
        print(f'[{rows}, 768]   {inner} launches per replay, {reps} rounds, {len(arms)} arms interleaved: us per launch')
        for (label, _), t, dg in zip(arms, times, digests):
            print(f'  {label:32s} {fmt(stats(t))}   {dg}')
            record[f'[{rows}] {label}'] = dict(times=t, digest=dg)
        del graphs
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, 'w') as f:
            json.dump(record, f)


def compare(folder):
    from ires_time import fmt, stats, verdict
    load = lambda pat: [json.load(open(p)) for p in sorted(glob.glob(os.path.join(folder, pat)))]
    par, new = load('parent_*.json'), load('new_*.json')
    assert len(par) >= 3 and len(new) >= 3, 'at least three runs of each library'
    print(f'{len(par)} runs of the parent library, {len(new)} of the new one, alternating; per arm: all replays of a library pooled')
    print('rule: the median of the new library\'s pooled replays against the quartiles of the parent\'s pooled replays '
          '(ires_time.verdict); the medians of the single runs are printed beside them')
    bad = []
    for arm in par[0]:
        dig = {r[arm]['digest'] for r in par + new}
        p = stats(sorted(t for r in par for t in r[arm]['times']))
        n = stats(sorted(t for r in new for t in r[arm]['times']))
        meds = lambda rs: ' '.join(f'{stats(r[arm]["times"])["med"]:.2f}' for r in rs)
        v = verdict(n, p, 'the parent')
        print(f'{arm}\n    parent {fmt(p)}   medians by run {meds(par)}\n    new    {fmt(n)}   medians by run {meds(new)}\n'
              f'    new / parent {n["med"] / p["med"]:.4f}: {v};   digests equal: {len(dig) == 1}')
        if len(dig) != 1 or v.startswith('behind'):
            bad.append(arm)
    print('arms behind the parent or with unequal digests:', bad if bad else 'none')
    return 1 if bad else 0


if __name__ == '__main__':
    if '--compare' in sys.argv:
        sys.exit(compare(sys.argv[sys.argv.index('--compare') + 1]))
    run(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None)
