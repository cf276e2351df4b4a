"""TEST-ONLY: the float64 per-segment k best values of the oracle's probability matrix and their keys, for both forms of
``ir_attn_topk``; and ``tests/oracle_ops_match`` plus an ``attn_topk`` built on them, for the host logic of
``SharedAttnProcessor.attention_topk_index`` on the GPU-less box."""
import numpy as np
import torch

from oracle_ops_match import *  # noqa: F401,F403
from oracle_ops_match import CALLS, LAST_LSE, O, _np, gather_rows, key_bias, segment_edges, shared_attention  # noqa: F401


def topk_np(p_rows, edges, k, head_mean):
    """``p_rows`` float64 (B, H, R, Lkv) -> ``(values, indices)``, both (..., S, k): per segment the ``k`` first elements under
    (value descending, key ascending) - a stable descending sort - as float64 values and int64 keys counted inside the segment;
    a segment with fewer than ``k`` keys is padded with value 0, index -1.  ``head_mean``: of ``p_rows.mean(axis=1)`` (leading
    shape (B, R)); else per head (leading shape (B, H, R))."""
    x = p_rows.mean(axis=1) if head_mean else p_rows
    vals, idxs = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        seg = x[..., a:b]
        order = np.argsort(-seg, axis=-1, kind="stable")[..., :k]
        v = np.take_along_axis(seg, order, axis=-1)
        pad = k - order.shape[-1]
        if pad > 0:
            v = np.concatenate([v, np.zeros(v.shape[:-1] + (pad,))], axis=-1)
            order = np.concatenate([order, -np.ones(order.shape[:-1] + (pad,), dtype=order.dtype)], axis=-1)
        vals.append(v)
        idxs.append(order.astype(np.int64))
    return np.stack(vals, axis=-2), np.stack(idxs, axis=-2)


def attn_topk(q, k_self, ref_k, lse, rows=None, *, k, heads, scale, include_self=True, reduce="none", q_prescaled=False):
    CALLS.append(("attn_topk", dict(reduce=reduce, rows=rows, lse=lse, k=k)))
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 8:
        raise ValueError(f"k must be an integer in 1 ... 8, got {k!r}")
    if reduce not in ("none", "head_mean"):
        raise ValueError(f"reduce must be one of ['head_mean', 'none'], got {reduce!r}")
    qn, kn, rkn = map(_np, (q, k_self, ref_k))
    _, p = O.shared_attention_np(qn, kn, kn, rkn, rkn, heads, scale, False, include_self, return_probs=True)
    B, _, L, _ = p.shape
    idx = np.arange(L) if rows is None else torch.as_tensor(rows).long().cpu().numpy()
    if idx.ndim == 1:
        idx = np.broadcast_to(idx, (B, idx.shape[0]))
    edges = segment_edges(kn.shape[1], 0 if rkn is None else rkn.shape[1], 0 if rkn is None else rkn.shape[2], include_self)
    vals, keys = topk_np(gather_rows(p, idx), edges, k, reduce == "head_mean")
    return torch.from_numpy(keys.astype(np.int32)), torch.from_numpy(vals).float()
