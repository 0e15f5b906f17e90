"""TEST INFRASTRUCTURE: the reference of tq_attention_i8_ragged_fwd and the exact CPU twin that answers
`attention_i8_ragged` with it (options.INT8_RAGGED: the integer route for any sequence length).

The contract of include/tq_hip.h, restated with the existing oracle and nothing else:

    ragged(q, k, v, mask)[b, :T] == oracle.int_oracle.attention_i8(pad(q), pad(k), pad(v), pad_mask)[b, :T]

with every sequence padded to T_pad = 64 * ceil(T / 64) rows of ARBITRARY content and the mask extended by -inf at the pad
keys (zeros elsewhere when there was no mask).  A pad key's exponential is exactly 0.0f (tq_exp_neg below -86), its
probability index the zero point, its term of the second contraction 0 -- `pad` below chooses what the pad rows hold and
tests/test_attention_i8_ragged.py::test_reference_does_not_depend_on_pad_rows_cpu shows that it does not matter.

tests/test_attention_i8_ragged.py holds the kernel to `ragged_attention_reference`; `RaggedTwin` binds the same function to
the backend method, so the twin computes what the kernel was tested against.  Nothing outside tests/ imports this."""
import torch

from oracle import int_oracle
from tests._exact_backend import ExactBackend


def t_pad_of(T):
    return -(-T // 64) * 64


def _pad_rows(t, T_pad, pad, g):
    """t [B, T, D] int8 -> [B, T_pad, D]; pad rows: 'zeros' | 'random' bytes | copies of the 'last' valid row"""
    B, T, D = t.shape
    out = torch.zeros(B, T_pad, D, dtype=t.dtype)
    out[:, :T] = t
    if pad == 'random':
        out[:, T:] = torch.randint(-128, 128, (B, T_pad - T, D), generator=g).to(t.dtype)
    elif pad == 'last':
        out[:, T:] = t[:, T - 1:T]
    else:
        assert pad == 'zeros'
    return out


def ragged_attention_reference(q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx,
                               pad='zeros', seed=0):
    """q / k / v int8(index - 128) [B, T, H * D] (any strides), mask fp32 [B, T] or None, q_*: 7-tuples of python scalars or
    None (what OracleBackend._q7 returns).  -> (ctx fp32 [B, T, H * D], ctx_idx int8)"""
    B, T, _ = q_idx.shape
    T_pad = t_pad_of(T)
    g = torch.Generator().manual_seed(seed)
    qp, kp, vp = (_pad_rows(t.detach().cpu().contiguous(), T_pad, pad, g) for t in (q_idx, k_idx, v_idx))
    m = torch.zeros(B, T_pad, dtype=torch.float32)
    if mask is not None:
        m[:, :T] = mask.detach().cpu().float().reshape(B, T)
    m[:, T:] = float('-inf')
    ctx, ci = int_oracle.attention_i8(qp, kp, vp, num_heads, m.contiguous(), denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx)
    return ctx[:, :T].contiguous(), ci[:, :T].contiguous()


class RaggedTwin(ExactBackend):
    """ExactBackend that pads row tails (every oracle Linear takes any row count already) and has `attention_i8_ragged`;
    every call leaves a census entry ('attention_i8_ragged', shape of q_idx)"""
    name = 'exact-twin-ragged'
    PADS_ROWS = True

    def attention_i8_ragged(self, q_idx, k_idx, v_idx, num_heads, mask, denom, q_q, q_k, q_v, q_scores, q_probs, q_ctx,
                            want_idx=False):
        self._count('attention_i8_ragged', tuple(q_idx.shape))
        ctx, ci = ragged_attention_reference(q_idx, k_idx, v_idx, num_heads, mask, denom,
                                             *[self._q7(q) for q in (q_q, q_k, q_v, q_scores, q_probs, q_ctx)])
        return (ctx, ci) if want_idx else ctx
