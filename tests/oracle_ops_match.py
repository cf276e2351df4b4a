"""TEST-ONLY: the float64 per-segment maxima of the oracle's probability matrix and their sets of maximisers, for both forms of
``ir_attn_match``; and ``tests/oracle_ops_rows`` plus an ``attn_match`` built on them, for the host logic of
``SharedAttnProcessor.attention_match_index`` on the GPU-less box.  ``shared_attention`` keeps the LSE it returned in
``LAST_LSE`` so a test can tell that the read-out was handed that very tensor."""
import numpy as np
import torch

import oracle_ops_rows as _base
from oracle_ops_rows import *  # noqa: F401,F403
from oracle_ops_rows import CALLS, O, _np  # noqa: F401
from instantrestore_amd.ops import key_bias  # noqa: F401  (plain torch on either device: the processor builds its bias row with it)

LAST_LSE = [None]


def segment_edges(len_self, n_refs, len_ref, include_self):
    """column edges of ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1``: S + 1 numbers"""
    edges = [0] + ([len_self] if include_self else [])
    for _ in range(n_refs):
        edges.append(edges[-1] + len_ref)
    return edges


def gather_rows(p, idx):
    """(B, H, L, Lkv) -> (B, H, R, Lkv); ``idx``: (B, R) integers"""
    idx = np.asarray(idx)
    return np.stack([p[b][:, idx[b]] for b in range(p.shape[0])])


def match_np(p_rows, edges, head_mean):
    """``p_rows`` float64 (B, H, R, Lkv) -> ``(best, first, sets)``: the maximum of every segment (..., S), the lowest key inside
    the segment that attains it (..., S), and per segment the boolean array (..., len_s) of ALL its maximisers.  ``head_mean``:
    of ``p_rows.mean(axis=1)`` (leading shape (B, R)); else per head (leading shape (B, H, R))."""
    x = p_rows.mean(axis=1) if head_mean else p_rows
    best, first, sets = [], [], []
    for a, b in zip(edges[:-1], edges[1:]):
        seg = x[..., a:b]
        m = seg.max(axis=-1)
        eq = seg == m[..., None]
        best.append(m)
        first.append(eq.argmax(axis=-1))          # NumPy: the first True
        sets.append(eq)
    return np.stack(best, axis=-1), np.stack(first, axis=-1), sets


def shared_attention(*args, **kw):
    res = _base.shared_attention(*args, **kw)
    LAST_LSE[0] = res[1] if kw.get("return_lse", False) else None
    return res


def attn_match(q, k_self, ref_k, lse, rows=None, *, heads, scale, include_self=True, reduce="none", q_prescaled=False):
    CALLS.append(("attn_match", dict(reduce=reduce, rows=rows, lse=lse)))
    qn, kn, rkn = map(_np, (q, k_self, ref_k))
    _, p = O.shared_attention_np(qn, kn, kn, rkn, rkn, heads, scale, False, include_self, return_probs=True)
    B, _, L, _ = p.shape
    idx = np.arange(L) if rows is None else torch.as_tensor(rows).long().cpu().numpy()
    if idx.ndim == 1:
        idx = np.broadcast_to(idx, (B, idx.shape[0]))
    edges = segment_edges(kn.shape[1], 0 if rkn is None else rkn.shape[1], 0 if rkn is None else rkn.shape[2], include_self)
    best, first, _ = match_np(gather_rows(p, idx), edges, reduce == "head_mean")
    return torch.from_numpy(first.astype(np.int32)), torch.from_numpy(best).float()
