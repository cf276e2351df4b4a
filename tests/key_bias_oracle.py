"""float64 oracle of the fused attention WITH an additive key bias (``ir_shared_attn_bias_args``), built from the oracle's own
head split / extended K/V / head merge (``oracle.shared_attn_oracle``):

    P = softmax_j(scale * <q_i, k_j> + bias[b, h, j])         over the packed extended key axis [self] ++ ref 0 ++ ... ++ ref N-1

A key whose bias is ``-inf`` or ``<= MASKED`` (-1e4, diffusers' convention) is masked: probability exactly 0.  A ``(b, h)`` with every
key masked gives zeros, ``lse = -inf`` and zero masses.  AdaIN statistics are not masked (``extended_kv_np`` computes them over every
reference token, as the reference's ``adain`` does)."""
import numpy as np

from oracle.shared_attn_oracle import batch_to_head_dim_np, extended_kv_np, head_to_batch_dim_np

MASKED = -1.0e4


def bias_rows_np(key_bias, batch, heads, lkv):
    """(B, Lkv) or (B, H, Lkv) -> float64 (B * H, 1, Lkv) in head_to_batch_dim order"""
    kb = np.asarray(key_bias, dtype=np.float64)
    if kb.ndim == 2:
        kb = np.broadcast_to(kb[:, None, :], (batch, heads, lkv))
    assert kb.shape == (batch, heads, lkv), (kb.shape, (batch, heads, lkv))
    return kb.reshape(batch * heads, 1, lkv)


def biased_attention_np(q, k_self, v_self, ref_k, ref_v, heads, scale, key_bias, use_adain=False, train_input=True,
                        seg_lens=None):
    """q, k_self, v_self: (B, L, C); ref_k, ref_v: (B, N, Lr, C) or None; key_bias: (B, Lkv) / (B, H, Lkv) or None.
    Returns ``out`` (B, Lq, C), ``lse`` (B, H, Lq) and, with ``seg_lens`` (the segment lengths in key order), ``mass``
    (B, H, Lq, S)."""
    c = lambda t: None if t is None else np.asarray(t, dtype=np.float64)
    q, k_self, v_self, ref_k, ref_v = map(c, (q, k_self, v_self, ref_k, ref_v))
    B = q.shape[0]
    qh = head_to_batch_dim_np(q, heads)
    ek, ev = extended_kv_np(k_self, v_self, ref_k, ref_v, heads, use_adain, train_input)
    lkv = ek.shape[1]
    s = np.matmul(qh, ek.transpose(0, 2, 1)) * np.float64(scale)
    masked = np.zeros((B * heads, 1, lkv), dtype=bool)
    if key_bias is not None:
        kb = bias_rows_np(key_bias, B, heads, lkv)
        masked = ~(kb > MASKED)                       # -inf and <= MASKED
        s = s + np.where(masked, 0.0, kb)
    s = np.where(masked, -np.inf, s)
    m = s.max(axis=-1, keepdims=True)
    dead = ~np.isfinite(m)                            # every key masked
    e = np.exp(s - np.where(dead, 0.0, m))            # masked: exp(-inf) = 0 exactly
    l = e.sum(axis=-1, keepdims=True)
    p = e / np.where(dead, 1.0, l)
    with np.errstate(divide="ignore"):
        lse = np.where(dead, -np.inf, m + np.log(np.where(dead, 1.0, l)))
    out = batch_to_head_dim_np(np.matmul(p, ev), heads)
    lse = lse.reshape(B, heads, qh.shape[1])
    if seg_lens is None:
        return out, lse
    assert sum(seg_lens) == lkv, (seg_lens, lkv)
    edges = np.concatenate([[0], np.cumsum(seg_lens)])
    mass = np.stack([p[..., edges[i]:edges[i + 1]].sum(axis=-1) for i in range(len(seg_lens))], axis=-1)
    return out, lse, mass.reshape(B, heads, qh.shape[1], len(seg_lens))
