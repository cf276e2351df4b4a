"""float64 oracle of the fused attention WITH per-query region masks (``ir_shared_attn_region_args``), built from the oracle's own
head split / extended K/V / head merge (``oracle.shared_attn_oracle``) in the style of ``tests/key_bias_oracle.py``:

    allowed(b, i, j) = key_region[b, j] in [0, 31]  and  (q_allow[b, i] >> key_region[b, j]) & 1
    P = softmax over the allowed j of scale * <q_i, k_j>       over the packed extended key axis [self] ++ ref 0 ++ ... ++ ref N-1

One rule for all heads.  A pair that is not allowed is masked as a masked key of the bias is: probability exactly 0, whatever its
score.  A row with no allowed key is dead: zeros, ``lse = -inf`` and zero masses.  AdaIN statistics are not masked
(``extended_kv_np`` computes them over every reference token)."""
import numpy as np

from oracle.shared_attn_oracle import batch_to_head_dim_np, extended_kv_np, head_to_batch_dim_np

REGION_MAX = 32


def allowed_np(q_allow, key_region):
    """q_allow (B, Lq) - int32 or uint32 storage of the 32-bit words - and key_region (B, Lkv) int -> bool (B, 1, Lq, Lkv)"""
    qa = np.asarray(q_allow).astype(np.int64) & 0xFFFFFFFF          # the 32 bits, whatever the storage's sign
    kr = np.asarray(key_region).astype(np.int64)
    assert qa.ndim == 2 and kr.ndim == 2 and qa.shape[0] == kr.shape[0], (qa.shape, kr.shape)
    somebody = (kr >= 0) & (kr < REGION_MAX)
    bit = (qa[:, :, None] >> np.where(somebody, kr, 0)[:, None, :]) & 1
    return ((bit == 1) & somebody[:, None, :])[:, None]


def masked_attention_np(q, k_self, v_self, ref_k, ref_v, heads, scale, allowed, use_adain=False, train_input=True, seg_lens=None):
    """q, k_self, v_self: (B, L, C); ref_k, ref_v: (B, N, Lr, C) or None; allowed: bool (B, 1, Lq, Lkv) or None (everything).
    Returns ``out`` (B, Lq, C), ``lse`` (B, H, Lq) and, with ``seg_lens`` (the segment lengths in key order), ``mass``
    (B, H, Lq, S)."""
    c = lambda t: None if t is None else np.asarray(t, dtype=np.float64)
    q, k_self, v_self, ref_k, ref_v = map(c, (q, k_self, v_self, ref_k, ref_v))
    B = q.shape[0]
    qh = head_to_batch_dim_np(q, heads)
    ek, ev = extended_kv_np(k_self, v_self, ref_k, ref_v, heads, use_adain, train_input)
    lq, lkv = qh.shape[1], ek.shape[1]
    s = np.matmul(qh, ek.transpose(0, 2, 1)) * np.float64(scale)
    masked = np.zeros((B * heads, lq, lkv), dtype=bool)
    if allowed is not None:
        al = np.asarray(allowed, dtype=bool)
        assert al.shape == (B, 1, lq, lkv), (al.shape, (B, 1, lq, lkv))
        masked = ~np.broadcast_to(al, (B, heads, lq, lkv)).reshape(B * heads, lq, lkv)      # head_to_batch_dim order
    s = np.where(masked, -np.inf, s)
    m = s.max(axis=-1, keepdims=True)
    dead = ~np.isfinite(m)                            # no allowed key
    e = np.exp(s - np.where(dead, 0.0, m))            # masked: exp(-inf) = 0 exactly
    l = e.sum(axis=-1, keepdims=True)
    p = e / np.where(dead, 1.0, l)
    with np.errstate(divide="ignore"):
        lse = np.where(dead, -np.inf, m + np.log(np.where(dead, 1.0, l)))
    out = batch_to_head_dim_np(np.matmul(p, ev), heads)
    lse = lse.reshape(B, heads, lq)
    if seg_lens is None:
        return out, lse
    assert sum(seg_lens) == lkv, (seg_lens, lkv)
    edges = np.concatenate([[0], np.cumsum(seg_lens)])
    mass = np.stack([p[..., edges[i]:edges[i + 1]].sum(axis=-1) for i in range(len(seg_lens))], axis=-1)
    return out, lse, mass.reshape(B, heads, lq, len(seg_lens))


def region_attention_np(q, k_self, v_self, ref_k, ref_v, heads, scale, q_allow, key_region, **kw):
    """the same from the compact form the kernel takes"""
    return masked_attention_np(q, k_self, v_self, ref_k, ref_v, heads, scale, allowed_np(q_allow, key_region), **kw)
