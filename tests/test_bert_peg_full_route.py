"""BERT with the README's PEG recipe ({'x', 'h', 'y'}: 'ng6') on the GPU, default route: both residual + LayerNorm tails of
every layer run as the per-column kernel (tq_residual_layernorm_quant_axis_fwd), FFN1 index-only through the class-ordered
integer Linear and FFN2 through the integer Linear on its indices; a hipGraph replay and a second eager run equal the first
bit for bit; one block fed the same input on both routes meets the fused tail's contract against F.layer_norm
(tests/test_fused_ln.py: >= 99.9 % identical, the rest one grid step of the column away).

Whole model, default vs layered route, 3 layers at [8, 128]: bound max |diff| <= 0.05 * max |layered| (the bar of
tests/test_bert_peg_route.py).  Measured on one MI355X: max |diff| = 0.00958 with max |layered| = 0.453 (bar: 0.0227).
One block, same input on both routes: attention-output tail 99.9999 % identical, the rest one step; feed-forward tail
identical."""
import pytest
import torch

from tests.test_bert_peg_route import _calibrated, _ids, _out

pytestmark = [pytest.mark.gpu, pytest.mark.default_route]


def _counters(monkeypatch):
    from quantization import _hip
    n = {'axis': [], 'cls': [], 'lin': []}

    def wrap(name, key, rec):
        orig = getattr(_hip.HipBackend, name)

        def counted(self, *a, **k):
            n[key].append(rec(a, k))
            return orig(self, *a, **k)
        monkeypatch.setattr(_hip.HipBackend, name, counted)
    wrap('residual_layernorm_quant_axis', 'axis', lambda a, k: tuple(None if q is None else q[0].numel() for q in (a[2], a[3], a[7])))
    wrap('linear_i8_cls', 'cls', lambda a, k: k.get('want_y', True))
    wrap('linear_i8', 'lin', lambda a, k: a[0].shape[-1])
    return n


def test_peg_recipe_whole_feed_forward_block_on_the_integer_route(monkeypatch):
    from quantization import options
    from quantization.graphs import GraphedForward
    n = _counters(monkeypatch)
    model = _calibrated(3)
    assert n['axis'] == [] and n['cls'] == []                  # calibrating forwards: layered tails
    ids = _ids(3)
    with torch.no_grad():
        options.INT8_LINEAR = False
        layered = _out(model(ids)).clone()
        assert n['axis'] == [] and n['cls'] == []
        options.INT8_LINEAR = 'auto'
        n['lin'].clear()
        fast = _out(model(ids)).clone()
        assert n['axis'] == [(1, 1, 768), (768, 768, 1)] * 3
        assert n['cls'] == [False] * 3                          # FFN1 index-only: no [tokens, 3072] fp32 tensor
        assert sum(1 for k in n['lin'] if k == 3072) == 3       # FFN2 on FFN1's indices
        again = _out(model(ids)).clone()
    assert torch.equal(fast, again)
    g = GraphedForward(model, ids)
    assert torch.equal(_out(g(ids)).clone(), fast)
    d = float((fast.float() - layered.float()).abs().max())
    print('PEG recipe, 3 layers [8,128]: max |default - layered| = %.6g, max |layered| = %.6g' % (d, float(layered.abs().max())))
    assert d <= 0.05 * float(layered.abs().max())
    # a hook on a module the fused launch would not call, and autograd, keep the layered tails
    k = len(n['axis'])
    h = model.layers[1].output.res_act_quantizer.register_forward_hook(lambda m, a, o: None)
    try:
        with torch.no_grad():
            model(ids)
    finally:
        h.remove()
    assert len(n['axis']) == k + 5
    options.INT8_LINEAR = True
    model(ids)
    assert len(n['axis']) == k + 5


@pytest.mark.parametrize('block', ['attention_output', 'output'])
def test_one_block_same_input_on_both_routes(block):
    """QResidualBlock of the calibrated model, the same (h, residual) on both routes.  The layered route's GEMM is fp32 and
    its LayerNorm torch's; the fused tail's contract against that chain is the one tests/test_fused_ln.py states.  To
    separate the GEMM from the tail, the tail is also fed the LAYERED GEMM output through the backend call; and the oracle
    chain (kernel order) vs F.layer_norm is checked on the CPU for these inputs first, so a failure points at the kernel."""
    from oracle import tq_oracle as O
    from oracle.ln_sum import layer_norm_kernel_order
    from quantization import _hip, options
    model = _calibrated(3)
    L = model.layers[1]
    blk = getattr(L, block)
    with torch.no_grad():
        options.INT8_LINEAR = False
        hidden = model.embeddings(_ids(3))
        mask = torch.zeros(8, 1, 1, 128, device='cuda')
        hidden = model.layers[0](hidden, mask)
        if block == 'attention_output':
            x, res = L.attention_self(hidden, mask), hidden
        else:
            res = L.attention_output(L.attention_self(hidden, mask), hidden)
            x = L.intermediate(res)
        gemm = blk.dense.run_forward(x, *blk.dense.get_params())
        layered = blk.LayerNorm(blk.res_act_quantizer(blk.dense.activation_quantizer(gemm) + res))
        qs = [m.activation_quantizer.quantizer for m in (blk.dense, blk.res_act_quantizer, blk.LayerNorm)]
        w, b = blk.LayerNorm.get_params()
        args = [(q._delta.reshape(-1), q._zero_float.reshape(-1), None, 8, False, False, q.eps) for q in qs]
        fused = _hip.backend().residual_layernorm_quant_axis(gemm, res, args[0], args[1], w, b, blk.LayerNorm.eps, args[2])
    step = torch.clamp_min(qs[2]._delta.reshape(-1), qs[2].eps).cpu()

    def contract(y, ref, what):
        diff = (y.cpu().float() - ref.cpu().float()).abs().reshape(-1, 768)
        same = float((diff == 0).float().mean())
        print(block, what, 'identical %.6f, max diff / step %.4f' % (same, float((diff / step).max())))
        assert same >= 0.999, (what, same)
        assert bool((diff <= step * 1.01).all()), what
    # the oracle alone (CPU): kernel-order statistics vs torch's
    fq = lambda v, q: O.fake_quant(v, q._delta.cpu().reshape(-1), q._zero_float.cpu().reshape(-1), 8, False, False, q.eps)[1]
    u = fq(fq(gemm.cpu().reshape(-1, 768), qs[0]) + res.cpu().reshape(-1, 768), qs[1])
    ref_k = fq(layer_norm_kernel_order(u, w.cpu().float(), b.cpu().float(), blk.LayerNorm.eps, torch.float32), qs[2])
    ref_t = fq(torch.nn.functional.layer_norm(u, (768,), w.cpu().float(), b.cpu().float(), blk.LayerNorm.eps), qs[2])
    contract(ref_k, ref_t, 'oracle: kernel order vs F.layer_norm')
    assert torch.equal(fused.cpu().reshape(-1, 768), ref_k)              # the kernel IS the oracle chain
    contract(fused, layered, 'kernel vs layered modules (same GEMM output)')
