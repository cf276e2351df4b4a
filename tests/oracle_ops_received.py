"""TEST-ONLY: the float64 per-key sums of the attention over the query rows for both forms of ``ir_attn_received``; and
``tests/oracle_ops_transfer`` plus an ``attn_received`` built on them, for the host logic of
``SharedAttnProcessor.attention_received_weights`` on the GPU-less box."""
import numpy as np
import torch

from oracle_ops_transfer import *  # noqa: F401,F403
from oracle_ops_transfer import CALLS, LAST_LSE, O, _np, segment_edges  # noqa: F401


def weights_np(weights, batch, len_q):
    """``None`` (one channel of ones), ``(L,)``, ``(B, L)``, ``(L, C)``, ``(1, L, C)`` or ``(B, L, C)`` -> float64 ``(B, L, C)``"""
    if weights is None:
        return np.ones((batch, len_q, 1))
    w = weights.detach().double().cpu().numpy() if hasattr(weights, "detach") else np.asarray(weights, dtype=np.float64)
    if w.ndim == 1 or (w.ndim == 2 and w.shape[0] != len_q):
        w = w[..., None]
    if w.ndim == 2:
        w = w[None]
    return np.broadcast_to(w, (batch,) + w.shape[1:])


def received_np(p, weights=None):
    """``p`` float64 ``(B, H, L, Lkv)``, ``weights`` as for :func:`weights_np` -> ``(recv, recv_hm)``: per head ``(B, H, Lkv, C)`` and
    its mean over the heads ``(B, Lkv, C)``"""
    w = weights_np(weights, p.shape[0], p.shape[2])
    recv = np.einsum("bhij,bic->bhjc", p, w)
    return recv, recv.mean(axis=1)


def attn_received(q, k_self, ref_k, lse, weights=None, *, heads, scale, include_self=True, reduce="none", q_prescaled=False):
    CALLS.append(("attn_received", dict(reduce=reduce, lse=lse, weights=weights)))
    qn, kn, rkn = map(_np, (q, k_self, ref_k))
    _, p = O.shared_attention_np(qn, kn, kn, rkn, rkn, heads, scale, False, include_self, return_probs=True)
    r0, r1 = received_np(p, weights)
    return torch.from_numpy(np.ascontiguousarray(r1 if reduce == "head_mean" else r0)).float()
