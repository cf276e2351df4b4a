"""TEST-ONLY: the float64 attention-weighted sums of a per-key payload, per K/V segment, for both forms of ``ir_attn_transfer``; and
``tests/oracle_ops_match`` plus an ``attn_transfer`` built on them, for the host logic of
``SharedAttnProcessor.attention_transfer_payload`` on the GPU-less box."""
import numpy as np
import torch

from oracle_ops_match import *  # noqa: F401,F403
from oracle_ops_match import CALLS, LAST_LSE, O, _np, gather_rows, segment_edges  # noqa: F401


def payload_np(payload, batch):
    """``(Lkv, C)``, ``(1, Lkv, C)`` or ``(B, Lkv, C)`` -> float64 ``(B, Lkv, C)``"""
    y = payload.detach().double().cpu().numpy() if hasattr(payload, "detach") else np.asarray(payload, dtype=np.float64)
    if y.ndim == 2:
        y = y[None]
    return np.broadcast_to(y, (batch,) + y.shape[1:])


def transfer_np(p_rows, payload, edges):
    """``p_rows`` float64 ``(B, H, R, Lkv)`` (the probability rows of the chosen tokens), ``payload`` as for :func:`payload_np`,
    ``edges`` of :func:`segment_edges` -> ``(sums, mass, sums_hm, mass_hm)``: per head ``(B, H, R, S, C)`` / ``(B, H, R, S)``, and their
    means over the heads ``(B, R, S, C)`` / ``(B, R, S)``"""
    y = payload_np(payload, p_rows.shape[0])
    sums, mass = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        sums.append(np.einsum("bhrj,bjc->bhrc", p_rows[..., a:b], y[:, a:b]))
        mass.append(p_rows[..., a:b].sum(axis=-1))
    sums, mass = np.stack(sums, axis=-2), np.stack(mass, axis=-1)
    return sums, mass, sums.mean(axis=1), mass.mean(axis=1)


def attn_transfer(q, k_self, ref_k, lse, payload, rows=None, *, heads, scale, include_self=True, reduce="none", normalize=False,
                  q_prescaled=False):
    CALLS.append(("attn_transfer", dict(reduce=reduce, rows=rows, lse=lse, payload=payload)))
    qn, kn, rkn = map(_np, (q, k_self, ref_k))
    _, p = O.shared_attention_np(qn, kn, kn, rkn, rkn, heads, scale, False, include_self, return_probs=True)
    B, _, L, _ = p.shape
    idx = np.arange(L) if rows is None else torch.as_tensor(rows).long().cpu().numpy()
    if idx.ndim == 1:
        idx = np.broadcast_to(idx, (B, idx.shape[0]))
    edges = segment_edges(kn.shape[1], 0 if rkn is None else rkn.shape[1], 0 if rkn is None else rkn.shape[2], include_self)
    s0, m0, s1, m1 = transfer_np(gather_rows(p, idx), payload, edges)
    sums, mass = (s1, m1) if reduce == "head_mean" else (s0, m0)
    return torch.from_numpy(np.ascontiguousarray(sums)).float(), torch.from_numpy(np.ascontiguousarray(mass)).float()
