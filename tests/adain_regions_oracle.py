"""float64 oracle of per-region AdaIN (``ir_token_stats_labelled`` / ``ir_adain_apply_labelled`` / ``ops.adain_affine_regions``),
in the style of ``tests/adain_weighted_oracle.py``.  Per (b, m, region r) the statistics are the reference's own lines
(attn_processors.py:9-10) on the tokens of the region alone,

    mean = x[:, labels == r].mean(dim=1),     std = x[:, labels == r].std(dim=1)        (unbiased)

with the rules of the interface: a label outside [0, R) is no region, an empty region gives (0, 0) and count 0, a region of one
token (x, 0) and count 1.  The affine table has R + 1 slots per (b, n): slot r < R takes the regional pair of statistics when
both sides hold at least ``min_tokens`` tokens of the region and the whole-face pair otherwise; slot R is the whole-face affine."""
import numpy as np

from oracle.shared_attn_oracle import ADAIN_EPS, shared_attention_np, token_stats_np


def region_token_stats_np(x, labels, R):
    """x (B, M, L, C), labels int (B or 1, M, L) -> mean, std (B, R, M, C) float64, count (B, R, M)"""
    x = np.asarray(x, dtype=np.float64)
    B, M, L, C = x.shape
    lab = np.broadcast_to(np.asarray(labels), (B, M, L))
    mean, std, count = np.zeros((B, R, M, C)), np.zeros((B, R, M, C)), np.zeros((B, R, M))
    for b in range(B):
        for m in range(M):
            for r in range(R):
                xs = x[b, m][lab[b, m] == r]                # selected: whatever the bytes of the others
                count[b, r, m] = xs.shape[0]
                if xs.shape[0] == 0:
                    continue
                mu, sd = token_stats_np(xs[None])           # mean(dim=1) / std(dim=1) of the reference
                mean[b, r, m] = mu[0, 0]
                if xs.shape[0] > 1:
                    std[b, r, m] = sd[0, 0]
    return mean, std, count


def _affine(mu_v, sd_v, mu_x, sd_x, eps):
    a = np.where(sd_x == 0, 0.0, (sd_v + eps) / (sd_x + eps))       # a = 0 on a constant content channel, as adain_affine_np reports it
    return a, mu_v - mu_x * a


def region_affine_table_np(v_self, ref_v, q_labels, r_labels, R, min_tokens=8, eps=ADAIN_EPS):
    """v_self (B, L, C), ref_v (B, N, Lr, C), q_labels (B, L), r_labels (B, N, Lr) -> a, b (B, N, R + 1, C) and the bool
    (B, N, R) of the slots that carry regional statistics"""
    v_self, ref_v = np.asarray(v_self, dtype=np.float64), np.asarray(ref_v, dtype=np.float64)
    B, N, Lr, C = ref_v.shape
    sm, ss, sc = region_token_stats_np(v_self[:, None], np.asarray(q_labels)[:, None], R)      # (B, R, 1, C), (B, R, 1)
    cm, cs, cc = region_token_stats_np(ref_v, r_labels, R)                                       # (B, R, N, C), (B, R, N)
    gm, gs = token_stats_np(v_self)                                                              # (B, 1, C)
    hm = np.stack([token_stats_np(ref_v[:, n])[0][:, 0] for n in range(N)], axis=1)              # (B, N, C)
    hs = np.stack([token_stats_np(ref_v[:, n])[1][:, 0] for n in range(N)], axis=1)
    a, b = np.zeros((B, N, R + 1, C)), np.zeros((B, N, R + 1, C))
    regional = np.zeros((B, N, R), dtype=bool)
    for bb in range(B):
        for n in range(N):
            for r in range(R):
                regional[bb, n, r] = sc[bb, r, 0] >= min_tokens and cc[bb, r, n] >= min_tokens
                if regional[bb, n, r]:
                    a[bb, n, r], b[bb, n, r] = _affine(sm[bb, r, 0], ss[bb, r, 0], cm[bb, r, n], cs[bb, r, n], eps)
                else:                                        # BOTH sides fall back to the whole-face statistics
                    a[bb, n, r], b[bb, n, r] = _affine(gm[bb, 0], gs[bb, 0], hm[bb, n], hs[bb, n], eps)
            a[bb, n, R], b[bb, n, R] = _affine(gm[bb, 0], gs[bb, 0], hm[bb, n], hs[bb, n], eps)
    return a, b, regional


def region_apply_np(ref_v, r_labels, a, b):
    """ref_v (B, N, Lr, C) renormalised per token: slot = label if 0 <= label < R else R"""
    ref_v = np.asarray(ref_v, dtype=np.float64)
    R = a.shape[2] - 1
    lab = np.broadcast_to(np.asarray(r_labels), ref_v.shape[:3]).astype(np.int64)
    slot = np.where((lab >= 0) & (lab < R), lab, R)
    bi, ni = np.arange(ref_v.shape[0])[:, None, None], np.arange(ref_v.shape[1])[None, :, None]
    return ref_v * a[bi, ni, slot] + b[bi, ni, slot]


def region_adain_attention_np(q, k_self, v_self, ref_k, ref_v, q_labels, r_labels, R, heads, scale, train_input=True, min_tokens=8):
    """float64 attention whose reference V is renormalised per token with the per-region affine table"""
    a, b, _ = region_affine_table_np(v_self, ref_v, q_labels, r_labels, R, min_tokens)
    return shared_attention_np(q, k_self, v_self, ref_k, region_apply_np(ref_v, r_labels, a, b), heads, scale, False, train_input)
