"""TEST INFRASTRUCTURE: the exact CPU twin of a backend that runs BERT's embedding block behind per-column quantizers as one
launch (options.INT8_PEG_EMBEDDINGS).

One method, restating the contract tests/test_embeddings_ln_axis.py holds the kernel to:

    embeddings_layernorm_quant_axis     `embeddings_chain` of tests/_exact_backend.py with [d] parameters where a quantizer
                                        is per-column (the chain takes them as it takes scalars)

Every call leaves a census entry (name, shape of the ids, parameters per site, want_idx) and is counted in `embedding_calls`.
With that switch a packed batch takes the attention route of INT8_PEG_ATTENTION too, so the twin also has

    attention_i8_varlen with wide grids  the packed core called head by head with H = 1 on the head's column slice and the
                                         head's parameters as per-tensor quantizers (the rule of tests/_peg_attention_twin.py,
                                         which tests/test_attention_i8_head_grids.py holds the variable-length kernel to)

`NoPegEmbeddingsTwin` is the same backend without the method: options.int8_peg_embeddings is False for it whatever the switch
says, i.e. the layered block.  Nothing outside tests/ imports this."""
import torch

from tests._exact_backend import _p, embeddings_chain
from tests._peg_attention_twin import PegAttentionTwin, _wide

NoPegEmbeddingsTwin = PegAttentionTwin
NAME = 'embeddings_layernorm_quant_axis'


class PegEmbeddingsTwin(PegAttentionTwin):
    name = 'exact-twin-peg-embeddings'

    def __init__(self, rules=None):
        super().__init__(rules)
        self.embedding_calls = 0

    def embeddings_layernorm_quant_axis(self, word, word_ids, typ, type_ids, pos, pos_ids, q_sum1, q_sum2, ln_weight, ln_bias,
                                        ln_eps, q_out, want_idx=False):
        d = word.shape[-1]
        for q in (q_sum1, q_sum2, q_out):
            assert q is None or (q[0].numel() in (1, d) and (q[1] is None or q[1].numel() == q[0].numel()))
        assert word_ids.dtype == type_ids.dtype == pos_ids.dtype == torch.int64
        assert word_ids.numel() == type_ids.numel() == pos_ids.numel()
        self.embedding_calls += 1
        self._count(NAME, tuple(word_ids.shape), tuple(None if q is None else int(q[0].numel()) for q in (q_sum1, q_sum2, q_out)),
                    want_idx)
        y, idx, _ = embeddings_chain(word.detach().float(), word_ids.reshape(-1), typ.detach().float(), type_ids.reshape(-1),
                                     pos.detach().float(), pos_ids.reshape(-1), _p(q_sum1), _p(q_sum2),
                                     ln_weight.detach().float(), ln_bias.detach().float(), ln_eps, _p(q_out))
        return (y, (idx - 128).to(torch.int8)) if want_idx else y

    def attention_i8_varlen(self, q_idx, k_idx, v_idx, num_heads, seq_start, max_len, mask, denom, q_q, q_k, q_v, q_scores,
                            q_probs, q_ctx, want_idx=False):
        if not any(_wide(q) for q in (q_q, q_k, q_v, q_ctx)):
            return super().attention_i8_varlen(q_idx, k_idx, v_idx, num_heads, seq_start, max_len, mask, denom, q_q, q_k, q_v,
                                               q_scores, q_probs, q_ctx, want_idx=want_idx)
        self._count('attention_i8_varlen', tuple(q_idx.shape), 'per-head')
        from tests._packed_twin import packed_attention_reference

        def core(q, k, v, heads, m, dn, *qs, want_idx=False):
            ctx, ci = packed_attention_reference(q, k, v, heads, seq_start, max_len, m, dn, *[self._q7(x) for x in qs])
            return (ctx, ci) if want_idx else ctx
        return self._per_head(core, q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx, want_idx)
