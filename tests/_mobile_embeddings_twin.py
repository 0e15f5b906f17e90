"""TEST INFRASTRUCTURE: the exact reference of MobileBERT's one-launch embedding block (tq_mobile_embeddings_nonorm_quant_fwd,
options.INT8_MOBILE_EMBEDDINGS) and the CPU twin of a backend that has it.

`mobile_embeddings_chain` is what tests/test_mobile_embeddings.py holds the kernel to: a numpy gather of the int8 word rows
into the trigram, an int64 contraction, then the element functions the other exact tests use (tests/_exact_backend.py: the
pre-activation of an integer Linear as single fp32 operations, the oracle's fake-quant).  `MobileEmbeddingsTwin` binds it to
the backend method, so the twin computes what the kernel was tested against.  Nothing outside tests/ imports this."""
import numpy as np
import torch

from tests._exact_backend import _exact_matmul, _p, fq, i16x8_pre
from tests._oracle_backend import OracleBackend

NAME = 'mobile_embeddings_nonorm_quant'


def trigram(e_idx, ids):
    """int8 [vocab, E], int64 [B, T] -> int8 [B * T, 3E]: rows t+1 | t | t-1 of each sequence, zeros past its ends"""
    B, T = ids.shape
    e = e_idx[ids]                                                        # [B, T, E]
    z = np.zeros_like(e[:, :1])
    return np.concatenate([np.concatenate([e[:, 1:], z], 1), e, np.concatenate([z, e[:, :-1]], 1)], 2).reshape(B * T, -1)


def mobile_embeddings_chain(e_idx, ids, e_delta, e_eps, w_idx, w_delta, w_eps, bias, pos, pos_ids, typ, type_ids, nn_w, nn_b,
                            q_t, q_1, q_2, q_3):
    """numpy / torch CPU operands, quantizers in the chains' form (`_p`) -> (y fp32 [B * T, N], indices of y or None, tri)"""
    tri = trigram(e_idx, ids)
    lin = torch.from_numpy(i16x8_pre(_exact_matmul(tri, w_idx), float(e_delta), e_eps, np.asarray(w_delta, np.float32).reshape(-1),
                                     w_eps, None if bias is None else np.asarray(bias, np.float32)))
    u = fq(fq(lin, q_t)[1] + pos[pos_ids], q_1)[1]
    v = fq(u + typ[type_ids], q_2)[1]
    idx, y = fq(v * nn_w + nn_b, q_3)
    return y, idx, tri


class MobileEmbeddingsMethod:
    """The one-launch embedding block for any CPU backend double (mix in first); every call leaves (NAME, ids shape,
    want_idx) in `census`."""
    MOBILE_EMBEDDING_SIZE, MOBILE_HIDDEN_MULTIPLE = 128, 128

    def mobile_embeddings_nonorm_quant(self, e_idx, e_delta, e_eps, word_ids, w_idx, w_delta, w_eps, bias, pos_tab, pos_ids,
                                       type_tab, type_ids, nn_weight, nn_bias, q_t, q_sum1, q_sum2, q_out, want_idx=False):
        assert e_idx.dtype == w_idx.dtype == torch.int8 and word_ids.dtype == pos_ids.dtype == type_ids.dtype == torch.int64
        assert word_ids.dim() == 2 and pos_ids.numel() == type_ids.numel() == word_ids.numel()
        self.__dict__.setdefault('census', []).append((NAME, tuple(word_ids.shape), want_idx))
        f = lambda t: None if t is None else t.detach().float()
        y, idx, _ = mobile_embeddings_chain(
            e_idx.numpy(), word_ids.numpy(), float(e_delta), e_eps, w_idx.numpy(), w_delta.detach().numpy(), w_eps,
            None if bias is None else bias.detach().numpy(), f(pos_tab), pos_ids.reshape(-1), f(type_tab), type_ids.reshape(-1),
            f(nn_weight), f(nn_bias), _p(q_t), _p(q_sum1), _p(q_sum2), _p(q_out))
        return (y, (idx - 128).to(torch.int8)) if want_idx else y


class MobileEmbeddingsTwin(MobileEmbeddingsMethod, OracleBackend):
    name = 'oracle-twin-mobile-embeddings'

    def __init__(self):
        self.census = []
