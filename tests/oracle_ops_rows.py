"""TEST-ONLY: ``tests/oracle_ops`` plus ``attn_rows`` (the oracle's probability matrix, gathered and reduced in float64), for
the host logic of ``SharedAttnProcessor.attention_rows_index`` on the GPU-less box.  ``shared_attention`` additionally logs
whether the LSE was asked for (``("return_lse", bool)`` in ``CALLS``, before the call's own entry)."""
import numpy as np
import torch

import oracle_ops as _base
from oracle_ops import *  # noqa: F401,F403
from oracle_ops import CALLS, O, _np  # noqa: F401


def shared_attention(*args, **kw):
    CALLS.append(("return_lse", bool(kw.get("return_lse", False))))
    return _base.shared_attention(*args, **kw)


def attn_rows(q, k_self, ref_k, lse, rows, *, heads, scale, include_self=True, reduce="none", q_prescaled=False):
    CALLS.append(("attn_rows", dict(reduce=reduce)))
    qn, kn, rkn = map(_np, (q, k_self, ref_k))
    _, p = O.shared_attention_np(qn, kn, kn, rkn, rkn, heads, scale, False, include_self, return_probs=True)
    B = p.shape[0]
    idx = torch.as_tensor(rows).long().cpu().numpy()
    if idx.ndim == 1:
        idx = np.broadcast_to(idx, (B, idx.shape[0]))
    g = np.stack([p[b][:, idx[b]] for b in range(B)])          # (B, H, R, Lkv)
    if reduce == "none":
        return torch.from_numpy(g).to(q.dtype)
    hm = g.mean(axis=1)
    return torch.from_numpy(hm if reduce == "head_mean" else hm.sum(axis=1)).float()
