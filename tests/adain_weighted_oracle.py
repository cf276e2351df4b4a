"""float64 oracle of the mask-aware AdaIN statistics (``ir_token_stats_weighted`` / ``ir_adain_affine_from_stats``), built on the
oracle's own statistics lines (``oracle.shared_attn_oracle.token_stats_np`` / ``adain_affine_np``) in the style of
``tests/region_oracle.py``.  Per (b, m, channel), with the effective weight ``w_t = w[b, m, t] if t < c[b, m] else 0``:

    W = sum w_t,  W2 = sum w_t^2,  mean = sum w_t x_t / W,  M2 = sum w_t (x_t - mean)^2,  std = sqrt(M2 / (W - W2 / W))

the unbiased estimator under reliability weights.  For 0/1 weights ``W - W2 / W = count - 1``: ``token_stats_np`` of the kept
tokens alone (``subset_token_stats_np`` computes exactly that, and tests/test_adain_weighted_cpu.py ties the two).  The rules of
the interface: ``W == 0`` gives (0, 0); ``W - W2 / W <= 0`` (one effective token) gives (that token's value, 0); a token of
weight 0 is selected away, never multiplied."""
import numpy as np

from oracle.shared_attn_oracle import ADAIN_EPS, shared_attention_np, token_stats_np


def effective_weights_np(shape, weights=None, lens=None):
    """(B, M, L) float64 effective weights from ``weights`` (B or 1, M, L) / ``lens`` (B, M), either may be None"""
    B, M, L = shape
    w = np.ones((B, M, L)) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), (B, M, L)).copy()
    if lens is not None:
        c = np.clip(np.asarray(lens).astype(np.int64), 0, L)
        w = np.where(np.arange(L)[None, None, :] < c[:, :, None], w, 0.0)
    return w


def weighted_token_stats_np(x, weights=None, lens=None):
    """x (B, M, L, C) -> mean, std (B, M, C) float64, and W (B, M)"""
    x = np.asarray(x, dtype=np.float64)
    B, M, L, C = x.shape
    w = effective_weights_np((B, M, L), weights, lens)
    mean, std, wsum = np.zeros((B, M, C)), np.zeros((B, M, C)), np.zeros((B, M))
    for b in range(B):
        for m in range(M):
            sel = w[b, m] > 0                         # selected away: whatever the bytes of the others
            ws, xs = w[b, m][sel][:, None], x[b, m][sel]
            W, W2 = ws.sum(), (ws ** 2).sum()
            wsum[b, m] = W
            if W == 0:
                continue
            mean[b, m] = (ws * xs).sum(axis=0) / W
            den = W - W2 / W
            if den > 1e-12 * W:
                std[b, m] = np.sqrt((ws * (xs - mean[b, m]) ** 2).sum(axis=0) / den)
    return mean, std, wsum


def subset_token_stats_np(x, keep):
    """``token_stats_np`` of ``x[:, kept]`` per (b, m): the reference's own statistics lines on the kept tokens.  x (B, M, L, C),
    keep bool (B, M, L) -> mean, std (B, M, C); no kept token gives (0, 0), one gives (x, 0) (where token_stats_np says NaN)"""
    x = np.asarray(x, dtype=np.float64)
    B, M, L, C = x.shape
    mean, std = np.zeros((B, M, C)), np.zeros((B, M, C))
    for b in range(B):
        for m in range(M):
            xs = x[b, m][np.asarray(keep[b, m], dtype=bool)]
            if xs.shape[0] == 0:
                continue
            mu, sd = token_stats_np(xs[None])
            mean[b, m] = mu[0, 0]
            if xs.shape[0] > 1:
                std[b, m] = sd[0, 0]
    return mean, std


def affine_from_stats_np(style, content, eps=ADAIN_EPS):
    """``adain_affine_np``'s expression on finished statistics: style (mean, std) (B, C), content (mean, std) (B, N, C) ->
    a, b (B, N, C); a = 0 where the content std is exactly 0, as the oracle reports it"""
    (mu_v, sd_v), (mu_x, sd_x) = style, content
    a = (sd_v[:, None] + eps) / (sd_x + eps)
    a = np.where(sd_x == 0, 0.0, a)
    return a, mu_v[:, None] - mu_x * a


def weighted_adain_affine_np(v_self, ref_v, self_w=None, ref_w=None, self_lens=None, ref_lens=None):
    """v_self (B, L, C), ref_v (B, N, Lr, C); self_w (B, L), ref_w (B, N, Lr) or None -> a, b (B, N, C)"""
    sm, ss, _ = weighted_token_stats_np(np.asarray(v_self, dtype=np.float64)[:, None], None if self_w is None else np.asarray(self_w)[:, None],
                                        None if self_lens is None else np.asarray(self_lens)[:, None])
    cm, cs, _ = weighted_token_stats_np(ref_v, ref_w, ref_lens)
    return affine_from_stats_np((sm[:, 0], ss[:, 0]), (cm, cs))


def weighted_adain_attention_np(q, k_self, v_self, ref_k, ref_v, heads, scale, self_w=None, ref_w=None, train_input=True):
    """float64 attention whose reference V is renormalised with the weighted (kept-token) statistics"""
    a, b = weighted_adain_affine_np(v_self, ref_v, self_w, ref_w)
    rv = np.asarray(ref_v, dtype=np.float64) * a[:, :, None, :] + b[:, :, None, :]
    return shared_attention_np(q, k_self, v_self, ref_k, rv, heads, scale, False, train_input)
