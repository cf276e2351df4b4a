"""TEST-ONLY: the column maxima of a probability matrix and the lowest row that attains each, for both forms of
``ir_attn_key_match``; the mutual (cycle) check restated in NumPy; and ``tests/oracle_ops_received`` plus an ``attn_key_match``
built on them, for the host logic of ``SharedAttnProcessor.attention_key_match_reduce`` on the GPU-less box."""
import numpy as np
import torch

from oracle_ops_received import *  # noqa: F401,F403
from oracle_ops_received import CALLS, LAST_LSE, O, _np, segment_edges  # noqa: F401


def first_argmax_np(x, axis):
    """(the maximum along ``axis``, the LOWEST position that holds it) - the comparison is exact, in ``x``'s own type"""
    m = x.max(axis=axis)
    eq = x == np.expand_dims(m, axis)
    return m, eq.argmax(axis=axis)                # NumPy: the first True


def key_match_np(p, head_mean):
    """``p`` float64 or fp32 ``(B, H, L, Lkv)`` -> ``(best, first)``: the maximum of every column over the L rows and the lowest row
    that attains it.  ``head_mean``: of ``p.mean(axis=1)`` (shape (B, Lkv)); else per head (shape (B, H, Lkv))."""
    return first_argmax_np(p.mean(axis=1) if head_mean else p, -2)


def key_match_of_matrix_np(x):
    """the same of a matrix that is already in its form: ``(..., L, Lkv)`` -> two arrays ``(..., Lkv)``"""
    return first_argmax_np(x, -2)


def match_of_matrix_np(x, edges):
    """the lowest best key of every row inside every segment: ``(..., L, Lkv)`` -> ``(..., L, S)``, counted inside the segment"""
    return np.stack([first_argmax_np(x[..., a:b], -1)[1] for a, b in zip(edges[:-1], edges[1:])], axis=-1)


def mutual_np(match_index, key_index, edges, rows=None):
    """``match_index`` ``(..., R, S)`` (keys inside their segments, -1: none), ``key_index`` ``(..., Lkv)`` (rows), ``rows`` ``(R,)`` or
    ``(B, R)`` (default ``arange(R)``) -> bool ``(..., R, S)``: pair (row r, its key of segment s) survives iff the key's best row
    is row r.  A plain loop: the statement, not an implementation"""
    match_index, key_index = np.asarray(match_index), np.asarray(key_index)
    R, S = match_index.shape[-2:]
    rows = np.arange(R) if rows is None else np.asarray(rows)
    out = np.zeros(match_index.shape, dtype=bool)
    for lead in np.ndindex(*match_index.shape[:-2]):
        rr = rows if rows.ndim == 1 else rows[lead[0]]
        for r in range(R):
            for s in range(S):
                j = int(match_index[lead + (r, s)])
                if j < 0 or rr[r] < 0:
                    continue
                out[lead + (r, s)] = int(key_index[lead + (edges[s] + j,)]) == int(rr[r])
    return out


def attn_key_match(q, k_self, ref_k, lse, *, heads, scale, include_self=True, reduce="none", q_prescaled=False):
    CALLS.append(("attn_key_match", dict(reduce=reduce, lse=lse)))
    qn, kn, rkn = map(_np, (q, k_self, ref_k))
    _, p = O.shared_attention_np(qn, kn, kn, rkn, rkn, heads, scale, False, include_self, return_probs=True)
    best, first = key_match_np(p, reduce == "head_mean")
    return torch.from_numpy(first.astype(np.int32)), torch.from_numpy(np.ascontiguousarray(best)).float()
