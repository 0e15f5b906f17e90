"""TEST INFRASTRUCTURE: the exact CPU twin of the HIP backend for the fixed-range entry points of BERT's default route, and
the reference chains the kernel-level GPU tests hold those entry points to.

Every function below IS the reference of a kernel test (they import it from here), so "the twin computes what the kernel
was tested against" holds by construction:

    ln_tail_chain       tests/test_fused_ln.py, tests/test_fused_ln_axis.py   (tq_residual_layernorm_quant[_axis]_fwd)
    embeddings_chain    tests/test_fused_ln.py                                (tq_embeddings_layernorm_quant_fwd)
    cls_pre             tests/test_linear_i8_peg.py                           (tq_linear_i8_cls_fwd)
    i16x8_tot / _pre    tests/test_linear_i16x8.py                            (tq_linear_i16x8_fwd)
    oracle_epilogue     tests/test_linear_i16x8.py                            (the epilogue of oracle/tq_int_oracle.c)

`ExactBackend` binds them to the method surface of quantization._hip.HipBackend; what it inherits from OracleBackend
(linear_i8, linear_i8_grouped, attention_i8, rowsum_i8, fake_quant*) already is oracle/tq_int_oracle.c / oracle/tq_oracle.py.
Row sums are never taken from the caller: the twin contracts the index operands it is given and derives everything else,
so a row-sum tensor bound to the wrong operand shows as a difference to the GPU.  Nothing outside tests/ imports this."""
import numpy as np
import torch

from oracle import tq_oracle as O
from tests._oracle_backend import OracleBackend


# ---- quantizer chains -------------------------------------------------------------------------------------------------------
def fq(v, p):
    """p: None or (delta, zero_float, n_bits, symmetric, signed[, eps]); delta / zero_float scalars or [d] along the last
    axis.  -> (indices or None, y)"""
    if p is None:
        return None, v
    return O.fake_quant(v, *p)


def ln_tail_chain(a, r, q1, q2, w, b, eps, q3, kernel_order=True):
    """Q3(LayerNorm(Q2(Q1(a) + r))) on [rows, d]; kernel_order: the fp32 statistics in the summation order of the fused tail
    kernels (oracle/ln_sum.py, storage dtype = a.dtype), else torch's.  -> (y fp32, indices of y or None, LayerNorm output)"""
    u = fq(fq(a.float(), q1)[1] + r.float(), q2)[1]
    if kernel_order:
        from oracle.ln_sum import layer_norm_kernel_order
        v = layer_norm_kernel_order(u, w, b, eps, a.dtype)
    else:
        v = torch.nn.functional.layer_norm(u, (u.shape[-1],), w, b, eps)
    idx, y = fq(v, q3)
    return y, idx, v


def embeddings_chain(word, word_ids, typ, type_ids, pos, pos_ids, q1, q2, w, b, eps, q3):
    """Q3(LayerNorm(Q2(Q1(word[ids] + type[ids]) + pos[ids]))), statistics in the kernel's order (fp32 rows).
    -> (y [rows, d], indices or None, LayerNorm output)"""
    from oracle.ln_sum import layer_norm_kernel_order
    d = word.shape[-1]
    u = fq(fq(word[word_ids] + typ[type_ids], q1)[1] + pos[pos_ids], q2)[1].reshape(-1, d)
    v = layer_norm_kernel_order(u, w, b, eps, torch.float32)
    idx, y = fq(v, q3)
    return y, idx, v


# ---- integer Linears: the pre-activation formulas of include/tq_hip.h ------------------------------------------------------
def _exact_matmul(a, w):
    """sum_k a[m,k] w[n,k] as int64: float64 products and partial sums of these integers stay below 2^53"""
    return (torch.from_numpy(np.ascontiguousarray(a)).double() @ torch.from_numpy(np.ascontiguousarray(w)).double().T
            ).numpy().astype(np.int64)


def cls_pre(x_c, w_c, ends, reps, x_delta, x_zf, n_bits, x_eps, w_delta, w_eps, bias):
    """tq_linear_i8_cls_fwd: x_c int8 [M, K] and w_c int8 [N, K] with their columns in class order, x_delta / x_zf the raw
    per-column buffers (natural order), w_delta [1] or [N]; numpy in, fp32 [M, N] out.  Int class sums, then fp32 operations
    one by one in class order."""
    N = w_c.shape[0]
    sw = np.broadcast_to(np.maximum(np.asarray(w_delta, np.float32), np.float32(w_eps)).astype(np.float32), (N,))
    acc, s = None, 0
    for e, r in zip(ends, reps):
        A = _exact_matmul(x_c[:, s:e], w_c[:, s:e])
        rs = w_c[:, s:e].astype(np.int64).sum(1)
        z = int(np.clip(np.rint(x_zf[r]), 0, 2 ** n_bits - 1))
        T = A + (128 - z) * rs[None, :]
        sx = np.float32(max(x_delta[r], np.float32(x_eps)))
        pc = T.astype(np.float32) * (sx * sw)[None, :].astype(np.float32)
        acc = pc if acc is None else (acc + pc).astype(np.float32)
        s = e
    if bias is not None:
        acc = (acc + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
    return acc.astype(np.float32)


def i16x8_tot(idx, w, z):
    """tot of tq_linear_i16x8_fwd as int64 from the grid indices themselves: sum_k index w - z rowsum
    (= 256 A_hi + A_lo + (32896 - z) rowsum: tests/test_linear_i16x8.py::test_plane_identity_of_the_restatement)"""
    return _exact_matmul(idx, w) - int(z) * w.astype(np.int64).sum(1)[None, :]


def i16x8_pre(tot, x_delta, x_eps, w_delta, w_eps, bias):
    """pre = RN32(tot) * (max(x_delta, eps) * s_w[n]) + b[n], every fp32 operation rounded on its own"""
    sw = np.maximum(np.asarray(w_delta, np.float32), np.float32(w_eps)).astype(np.float32)
    sx = np.float32(max(np.float32(x_delta), np.float32(x_eps)))
    pre = tot.astype(np.float32) * (sx * np.broadcast_to(sw, (tot.shape[1],))).astype(np.float32)[None, :]
    if bias is not None:
        pre = (pre + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
    return pre.astype(np.float32)


def oracle_epilogue(pre, activation, q):
    """The C oracle's epilogue (bias already in `pre`): activation code 0 / 1 / 2 / 4, then the output quantizer q (a
    7-tuple or None).  -> (y fp32, int8(index - 128)) of pre's shape"""
    from oracle import int_oracle
    q7 = None if q is None else (float(q[0]), None if q[1] is None else float(q[1]), None if q[2] is None else bool(q[2]),
                                 q[3], q[4], q[5], q[6])
    t = pre if torch.is_tensor(pre) else torch.from_numpy(np.ascontiguousarray(pre))
    return int_oracle.epilogue(t, activation, q7)


# ---- the twin -----------------------------------------------------------------------------------------------------------
def _p(q):
    """backend 7-tuple (delta, zero_float, signed, n_bits, symmetric, log_domain, eps) -> the chains' quantizer spec"""
    if q is None:
        return None
    delta, zf, sg, n_bits, sym, log, eps = q
    assert not log, 'exact twin: linear scale domain only'
    flat = lambda t: None if t is None else (t.detach().float().reshape(()) if t.numel() == 1 else t.detach().float().reshape(-1))
    return (flat(delta), flat(zf), n_bits, sym, bool(sg.item()) if sg is not None else False, eps)


def stair_header_ok(table):
    """the builder's verdict in a staircase table's 16-byte header {1 / bin width, offset, n_bins - 1, ok}"""
    return bool(table[:16].cpu().view(torch.float32)[3].item() == 1.0)


class ExactBackend(OracleBackend):
    """OracleBackend whose fused tails, embedding block, class-ordered and 16-bit Linears are the kernel tests' references.

    rules: where the staircase decisions come from -- an object with `stair_bins_for`, `cls_stair_bins_for`,
    `i16x8_stair_bins_for` (host-only rules of the HIP backend) and `act_stair` (the device builder, whose header carries
    its verdict).  The GPU tests pass the real backend, so the twin's host code takes the branches the GPU's took and GELU is
    evaluated as code 4 (correctly rounded, the accepted table's specification) or code 2 (the arithmetic fit) exactly where
    the kernel does.  Without rules (CPU-only tests) every table counts as accepted and has the bin counts below."""
    name = 'exact-twin'
    STAIR_BINS, STAIR_BINS_BIG = 768, 1536

    def __init__(self, rules=None):
        self.rules = rules
        self.census = []              # (method, shape of the main operand, output form) per launch
        self.stairs = []              # (n_bins, accepted) per table built
        self.tail_bindings = []       # per LayerNorm tail: the buffers of (q_dense, q_sum, q_out) it was handed

    def _count(self, name, *what):
        self.census.append((name,) + tuple(what))

    # -- staircase decisions
    def stair_bins_for(self, M, N):
        if self.rules is not None:
            return self.rules.stair_bins_for(M, N)
        big = M % 128 == 0 and N % 128 == 0 and (M // 128) * (N // 128) >= 1024
        return self.STAIR_BINS_BIG if big else self.STAIR_BINS

    def cls_stair_bins_for(self, M, N, K, n_classes):
        return self.rules.cls_stair_bins_for(M, N, K, n_classes) if self.rules is not None else self.STAIR_BINS

    def i16x8_stair_bins_for(self, M, N, K):
        return self.rules.i16x8_stair_bins_for(M, N, K) if self.rules is not None else self.STAIR_BINS

    def act_stair(self, activation, q_out, n_bins=None):
        n_bins = int(n_bins or self.STAIR_BINS)
        ok = True
        if self.rules is not None:
            dev = lambda t: None if t is None else t.detach().to('cuda')
            table, _ = self.rules.act_stair(activation, (dev(q_out[0]), dev(q_out[1]), dev(q_out[2])) + tuple(q_out[3:]), n_bins)
            ok = stair_header_ok(table)
        self.stairs.append((n_bins, ok))
        return ('exact-stair', n_bins, ok)

    @staticmethod
    def _act(activation, stair):
        """activation code the epilogue evaluates: 4 where an accepted table is passed for a GELU, else the code itself"""
        return 4 if (activation == 2 and stair is not None and stair[2]) else activation

    # -- fused tails
    def _tail(self, dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out, want_idx):
        d = dense_out.shape[-1]
        for q in (q_dense, q_sum, q_out):
            assert q is None or q[0].numel() in (1, d)
        self.tail_bindings.append(tuple(None if q is None else q[0].data_ptr() for q in (q_dense, q_sum, q_out)))
        y, idx, _ = ln_tail_chain(dense_out.detach().reshape(-1, d), residual.detach().to(dense_out.dtype).reshape(-1, d),
                                  _p(q_dense), _p(q_sum), ln_weight.detach().float(), ln_bias.detach().float(), ln_eps, _p(q_out))
        y = y.to(dense_out.dtype).reshape(dense_out.shape)
        return (y, (idx - 128).to(torch.int8).reshape(dense_out.shape)) if want_idx else y

    def residual_layernorm_quant(self, dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out, want_idx=False):
        if ln_eps is None:            # NoNorm: no statistics, the parent's element chain is exact
            return super().residual_layernorm_quant(dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out,
                                                    want_idx=want_idx)
        for q in (q_dense, q_sum, q_out):
            assert q is None or q[0].numel() == 1, 'per-tensor entry point'
        self._count('residual_layernorm_quant', tuple(dense_out.shape), want_idx)
        return self._tail(dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out, want_idx)

    def residual_layernorm_quant_axis(self, dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out,
                                      want_idx=False):
        self._count('residual_layernorm_quant_axis', tuple(dense_out.shape),
                    tuple(None if q is None else q[0].numel() for q in (q_dense, q_sum, q_out)), want_idx)
        return self._tail(dense_out, residual, q_dense, q_sum, ln_weight, ln_bias, ln_eps, q_out, want_idx)

    def embeddings_layernorm_quant(self, word, word_ids, typ, type_ids, pos, pos_ids, q_sum1, q_sum2, ln_weight, ln_bias, ln_eps,
                                   q_out, want_idx=False):
        self._count('embeddings_layernorm_quant', tuple(word_ids.shape), want_idx)
        y, idx, _ = embeddings_chain(word.detach().float(), word_ids.reshape(-1), typ.detach().float(), type_ids.reshape(-1),
                                     pos.detach().float(), pos_ids.reshape(-1), _p(q_sum1), _p(q_sum2),
                                     ln_weight.detach().float(), ln_bias.detach().float(), ln_eps, _p(q_out))
        return (y, (idx - 128).to(torch.int8)) if want_idx else y

    # -- integer Linears
    def linear_i8(self, x_idx, w_idx, w_rowsum, bias, x_q, w_delta, w_eps, activation, q_out, out_dtype, want_idx=False,
                  want_y=True, stair=None):
        self._count('linear_i8', tuple(x_idx.shape), w_idx.shape[0], want_y, stair is not None)
        from oracle import int_oracle
        y, yi = int_oracle.linear_i8(x_idx, w_idx, bias, tuple(float(v) for v in x_q), w_delta, w_eps,
                                     self._act(activation, stair), self._q7(q_out))
        y = y.to(out_dtype) if want_y else None
        return (y, yi) if want_idx else y

    def linear_i8_grouped(self, x_idx, *a, **k):
        self._count('linear_i8_grouped', tuple(x_idx.shape), a[0].shape[0])
        return super().linear_i8_grouped(x_idx, *a, **k)

    def attention_i8(self, q_idx, *a, **k):
        self._count('attention_i8', tuple(q_idx.shape))
        return super().attention_i8(q_idx, *a, **k)

    def _finish(self, pre, shape, activation, q_out, out_dtype, want_idx, want_y, stair):
        y, yi = oracle_epilogue(pre, self._act(activation, stair), q_out)
        y = y.reshape(shape).to(out_dtype) if want_y else None
        return (y, yi.reshape(shape)) if want_idx else y

    def cls_table(self, ends, reps):
        from quantization import _hip
        t = _hip.tq_cls_table()                                     # the ctypes struct itself: no device involved
        t.n_classes = len(ends)
        for c, (e, r) in enumerate(zip(ends, reps)):
            t.end[c], t.rep[c] = int(e), int(r)
        return t

    def linear_i8_cls(self, x_idx, w_idx, cls_rowsum, bias, x_q, cls, w_delta, w_eps, activation, q_out, out_dtype,
                      want_idx=False, want_y=True, stair=None):
        self._count('linear_i8_cls', tuple(x_idx.shape), w_idx.shape[0], want_y, stair is not None)
        n = int(cls.n_classes)
        ends, reps = [int(cls.end[c]) for c in range(n)], [int(cls.rep[c]) for c in range(n)]
        delta, zf, n_bits, eps = x_q
        dl, zl = delta.detach().reshape(-1).numpy(), zf.detach().reshape(-1).numpy()
        K = x_idx.shape[-1]
        # the table against the raw buffers: class c has exactly the columns that share its representative's pair
        assert ends[-1] == K and dl.size == K
        for c, (s, e) in enumerate(zip([0] + ends[:-1], ends)):
            members = int(((dl.view(np.uint32) == dl.view(np.uint32)[reps[c]])
                           & (zl.view(np.uint32) == zl.view(np.uint32)[reps[c]])).sum())
            assert members == e - s, f'class {c}: boundaries [{s}, {e}) but {members} columns carry its (delta, zero_float)'
        pre = cls_pre(x_idx.reshape(-1, K).numpy(), w_idx.numpy(), ends, reps, dl, zl, n_bits, eps,
                      w_delta.detach().reshape(-1).numpy(), w_eps, None if bias is None else bias.detach().numpy())
        return self._finish(pre, tuple(x_idx.shape[:-1]) + (w_idx.shape[0],), activation, q_out, out_dtype, want_idx, want_y,
                            stair)

    def quantize_hilo(self, x, q4):
        self._count('quantize_hilo', tuple(x.shape))
        delta, zf, n_bits, eps = q4
        idx = O.fake_quant(x.detach().float(), delta.reshape(()), zf.reshape(()), n_bits, False, False, eps, 'linear')[0].long()
        return ((idx >> 8) - 128).to(torch.int8), ((idx & 255) - 128).to(torch.int8)

    def linear_i16x8(self, x_hi, x_lo, w_idx, w_rowsum, bias, x_q, w_delta, w_eps, activation, q_out, out_dtype,
                     want_idx=False, want_y=True, stair=None):
        self._count('linear_i16x8', tuple(x_hi.shape), w_idx.shape[0], want_y, stair is not None)
        delta, zf, n_bits, eps = x_q
        K = x_hi.shape[-1]
        idx = 256 * (x_hi.reshape(-1, K).numpy().astype(np.int32) + 128) + (x_lo.reshape(-1, K).numpy().astype(np.int32) + 128)
        z = int(np.clip(np.rint(float(zf)), 0, 2 ** n_bits - 1))
        pre = i16x8_pre(i16x8_tot(idx, w_idx.numpy(), z), float(delta), eps, w_delta.detach().reshape(-1).numpy(), w_eps,
                        None if bias is None else bias.detach().numpy())
        return self._finish(pre, tuple(x_hi.shape[:-1]) + (w_idx.shape[0],), activation, q_out, out_dtype, want_idx, want_y,
                            stair)
