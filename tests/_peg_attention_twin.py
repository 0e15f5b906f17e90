"""TEST INFRASTRUCTURE: the exact CPU twin of a backend that runs the attention half of a BERT layer on the integer route
under per-embedding-group grids (options.INT8_PEG_ATTENTION).

Two methods, both restating the contracts the kernel tests hold the kernels to:

    linear_i8_cls_grouped     tests/test_linear_i8_cls_grouped.py: `cls_pre` of the stacked operands, then the C oracle's epilogue
                              block by block with the parameters at each block's first column
    attention_i8 / _ragged    tests/test_attention_i8_head_grids.py: a wide Q / K / V / context quantizer = the PARENT's core
                              called head by head with H = 1 on the head's column slice and the head's parameters as
                              per-tensor quantizers

Every call leaves a census entry.  `NoPegAttentionTwin` is the same backend without the grouped method: options.int8_peg_attention
is False for it whatever the switch says, i.e. today's route.  Nothing outside tests/ imports this."""
import numpy as np
import torch

from tests._exact_backend import cls_pre, oracle_epilogue
from tests._ragged_recipes_twin import RaggedRecipesTwin

NoPegAttentionTwin = RaggedRecipesTwin


def _wide(q):
    return q is not None and q[0].numel() != 1


def _head_q(q, h, head_dim):
    """head h's parameters of a wide 7-tuple as a per-tensor one (the element at the head's first column)"""
    if not _wide(q):
        return q
    at = lambda t: None if t is None else t.detach().reshape(-1)[h * head_dim].reshape(())
    return (at(q[0]), at(q[1])) + tuple(q[2:])


class PegAttentionTwin(RaggedRecipesTwin):
    name = 'exact-twin-peg-attention'

    def linear_i8_cls_grouped(self, x_idx, w_idx, cls_rowsum, bias, x_q, cls, w_delta, w_eps, activation, q_outs, q_block,
                              want_y=False, want_idx=True, out_dtype=torch.float32):
        G, N, K = len(q_outs), w_idx.shape[0], x_idx.shape[-1]
        gc = N // G
        self._count('linear_i8_cls_grouped', tuple(x_idx.shape), N, tuple(int(q[0].numel()) for q in q_outs), int(q_block), want_y)
        assert 1 <= G <= 3 and N % G == 0 and q_block % 64 == 0 and gc % q_block == 0 and activation in (0, 1)
        n = int(cls.n_classes)
        ends, reps = [int(cls.end[c]) for c in range(n)], [int(cls.rep[c]) for c in range(n)]
        delta, zf, n_bits, eps = x_q
        dl, zl = delta.detach().reshape(-1).numpy(), zf.detach().reshape(-1).numpy()
        assert ends[-1] == K and dl.size >= 1 and max(reps) < dl.size        # (K: the operands' columns, padded classes included)
        # the per-class row sums against the operand they were derived from
        for c, (s, e) in enumerate(zip([0] + ends[:-1], ends)):
            assert torch.equal(cls_rowsum[c].long(), w_idx[:, s:e].long().sum(1)), f'class {c}: row sums of another operand'
        pre = cls_pre(x_idx.reshape(-1, K).numpy(), w_idx.numpy(), ends, reps, dl, zl, n_bits, eps,
                      w_delta.detach().reshape(-1).numpy(), w_eps, None if bias is None else bias.detach().numpy())
        y, yi = np.empty_like(pre), np.empty(pre.shape, np.int8)
        for g, q in enumerate(q_outs):
            d, z = q[0].detach().reshape(-1).numpy(), q[1].detach().reshape(-1).numpy()
            assert d.size in (1, gc) and z.size == d.size and not q[4] and not q[5]
            for c0 in range(0, gc, q_block):
                at = 0 if d.size == 1 else c0
                # the caller's promise: constant over the block
                assert d.size == 1 or ((d[c0:c0 + q_block].view(np.uint32) == d[c0:c0 + 1].view(np.uint32)).all()
                                       and (z[c0:c0 + q_block].view(np.uint32) == z[c0:c0 + 1].view(np.uint32)).all())
                cols = slice(g * gc + c0, g * gc + c0 + q_block)
                by, bi = oracle_epilogue(np.ascontiguousarray(pre[:, cols]), activation,
                                         (float(d[at]), float(z[at]), None, q[3], False, False, q[6]))
                y[:, cols], yi[:, cols] = by.numpy(), bi.numpy()
        shape = tuple(x_idx.shape[:-1]) + (N,)
        return (torch.from_numpy(y).reshape(shape).to(out_dtype) if want_y else None,
                torch.from_numpy(yi).reshape(shape) if want_idx else None)

    def _per_head(self, core, q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx, want_idx):
        B, T, D = q_idx.shape
        hd = D // num_heads
        for q in (q_q, q_k, q_v, q_ctx):
            if _wide(q):
                for what, t in (('delta', q[0]), ('zero_float', q[1])):           # bit patterns, as the kernel reads them
                    w = t.detach().reshape(-1).contiguous().view(torch.int32)
                    assert w.numel() == D and torch.equal(w.view(num_heads, hd), w.view(num_heads, hd)[:, :1].expand(num_heads, hd)), \
                        f'a wide quantizer must be constant over every head ({what} is not)'
        ctx, ci = torch.empty(B, T, D), torch.empty(B, T, D, dtype=torch.int8)
        for h in range(num_heads):
            sl = slice(h * hd, (h + 1) * hd)
            out = core(q_idx[..., sl].contiguous(), k_idx[..., sl].contiguous(), v_idx[..., sl].contiguous(), 1, mask, denom,
                       _head_q(q_q, h, hd), _head_q(q_k, h, hd), _head_q(q_v, h, hd), q_scores, q_probs, _head_q(q_ctx, h, hd),
                       want_idx=want_idx)
            if want_idx:
                ctx[..., sl], ci[..., sl] = out
            else:
                ctx[..., sl] = out
        return (ctx, ci) if want_idx else ctx

    def attention_i8(self, q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx, want_idx=False):
        if not any(_wide(q) for q in (q_q, q_k, q_v, q_ctx)):
            return super().attention_i8(q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx,
                                        want_idx=want_idx)
        self._count('attention_i8', tuple(q_idx.shape), 'per-head')
        from tests._oracle_backend import OracleBackend
        core = lambda *a, **k: OracleBackend.attention_i8(self, *a, **k)                     # the uncounted oracle core
        return self._per_head(core, q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx, want_idx)

    def attention_i8_ragged(self, q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx,
                            want_idx=False):
        if not any(_wide(q) for q in (q_q, q_k, q_v, q_ctx)):
            return super().attention_i8_ragged(q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx,
                                               want_idx=want_idx)
        self._count('attention_i8_ragged', tuple(q_idx.shape), 'per-head')
        from tests._ragged_twin import ragged_attention_reference

        def core(q, k, v, heads, m, dn, *qs, want_idx=False):
            ctx, ci = ragged_attention_reference(q, k, v, heads, m, dn, *[self._q7(x) for x in qs])
            return (ctx, ci) if want_idx else ctx
        return self._per_head(core, q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx, want_idx)
