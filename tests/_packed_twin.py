"""TEST INFRASTRUCTURE: the reference of tq_attention_i8_varlen_fwd and the exact CPU twin that answers
`attention_i8_varlen` with it (packed variable-length batches on the integer route: no pad tokens).

The contract of include/tq_hip.h, restated with the ragged reference and nothing else: sequence b owns rows
seq_start[b] .. seq_start[b + 1] - 1 of the packed [1, M, D] operands, and on those rows

    varlen(q, k, v, seq_start, max_len, mask) == ragged(pad(q), pad(k), pad(v), pad_mask)[b, :len_b]

on the [B, max_len] batch that holds sequence b at [b, :len_b], ARBITRARY content in its pad rows, mask[seq_start[b] + t] at
the key (b, t < len_b) (zero without a mask) and -inf at every key t >= len_b.  `packed_attention_reference` builds that batch and
calls tests._ragged_twin.ragged_attention_reference (which pads max_len on to a multiple of 64 in the same way);
tests/test_attention_i8_varlen.py shows that the choice of the pad rows does not matter and holds the kernel to the ragged
KERNEL on the same batch.  `PackedTwin` binds the function to the backend method.  Nothing outside tests/ imports this."""
import torch

from tests._ragged_twin import RaggedTwin, ragged_attention_reference


def pad_packed(t, seq_start, max_len, pad='zeros', g=None):
    """t [1, M, D] (any strides) -> [B, max_len, D]; pad rows: 'zeros' | 'random' bytes | copies of the 'last' valid row"""
    s = [int(v) for v in seq_start]
    B, D = len(s) - 1, t.shape[-1]
    out = torch.zeros(B, max_len, D, dtype=t.dtype)
    for b in range(B):
        n = s[b + 1] - s[b]
        assert 0 <= n <= max_len and s[b + 1] <= t.shape[1]
        out[b, :n] = t[0, s[b]:s[b + 1]]
        if pad == 'random':
            out[b, n:] = torch.randint(-128, 128, (max_len - n, D), generator=g).to(t.dtype)
        elif pad == 'last' and n:
            out[b, n:] = t[0, s[b + 1] - 1]
        else:
            assert pad in ('zeros', 'last')
    return out


def padded_mask(mask, seq_start, max_len):
    """packed additive mask fp32 [M] or None -> [B, max_len] with -inf at the pad keys"""
    s = [int(v) for v in seq_start]
    m = torch.full((len(s) - 1, max_len), float('-inf'))
    for b in range(len(s) - 1):
        n = s[b + 1] - s[b]
        m[b, :n] = 0.0 if mask is None else mask.detach().cpu().float().reshape(-1)[s[b]:s[b + 1]]
    return m


def unpad_packed(y, seq_start, M, fill=0):
    """y [B, max_len, D] -> [1, M, D]: the valid rows in their packed places, `fill` in rows nobody owns"""
    s = [int(v) for v in seq_start]
    out = torch.full((1, M, y.shape[-1]), fill, dtype=y.dtype)
    for b in range(len(s) - 1):
        out[0, s[b]:s[b + 1]] = y[b, :s[b + 1] - s[b]]
    return out


def packed_attention_reference(q_idx, k_idx, v_idx, num_heads, seq_start, max_len, mask, denom, q_q, q_k, q_v, q_scores, q_probs,
                               q_ctx, pad='zeros', seed=0):
    """q / k / v int8(index - 128) [1, M, H * D], seq_start [B + 1], mask fp32 [M] or None, q_*: 7-tuples of python scalars or
    None.  -> (ctx fp32 [1, M, H * D], ctx_idx int8), zeros in rows nobody owns"""
    g = torch.Generator().manual_seed(seed)
    s = seq_start.detach().cpu()
    qp, kp, vp = (pad_packed(t.detach().cpu(), s, max_len, pad, g) for t in (q_idx, k_idx, v_idx))
    ctx, ci = ragged_attention_reference(qp, kp, vp, num_heads, padded_mask(mask, s, max_len), denom, q_q, q_k, q_v, q_scores,
                                         q_probs, q_ctx, pad=pad, seed=seed)
    M = q_idx.shape[1]
    return unpad_packed(ctx, s, M), unpad_packed(ci, s, M)


class PackedTwin(RaggedTwin):
    """RaggedTwin that has `attention_i8_varlen`; every call leaves a census entry ('attention_i8_varlen', shape of q_idx)"""
    name = 'exact-twin-packed'

    def attention_i8_varlen(self, q_idx, k_idx, v_idx, num_heads, seq_start, max_len, mask, denom, q_q, q_k, q_v, q_scores,
                            q_probs, q_ctx, want_idx=False):
        self._count('attention_i8_varlen', tuple(q_idx.shape))
        ctx, ci = packed_attention_reference(q_idx, k_idx, v_idx, num_heads, seq_start, max_len, mask, denom,
                                             *[self._q7(q) for q in (q_q, q_k, q_v, q_scores, q_probs, q_ctx)])
        return (ctx, ci) if want_idx else ctx
