"""Inputs and float64 references of the item-grid tests (tests/test_gpu_item_grid.py, tests/test_item_grid_oracle_cpu.py).

Three input sets, one per work-item height of the fused attention forward; their plans are pinned by the "grid" rows of
tests/test_attn_plan_cpu.py.  Both K/V forms hold 16 tiles of 64 keys, so the remainder round is cut in 16 / 8 = 2 pieces:

    self+fold     self segment of 384 keys + 2 references of 320, AdaIN: the cut (tile 8) lies inside reference 0
    noself+plain  4 references of 256 keys, no self segment, no AdaIN: the cut lies on the boundary of references 1 and 2

(``form_shape(form, long=True)``: every segment ``LONG`` = 4 times as long, 64 tiles and up to 8 pieces whose cuts fall inside segments
and on their boundaries alike - what the bf16 runs on the GPU use, tests/test_gpu_item_grid.py says why.)

``reference`` gives, for EVERY (b, h, row): the attention output (oracle/shared_attn_oracle.py::shared_attention_np, float64,
evaluated entry by entry - the whole batch's score matrix would be gigabytes), the log-sum-exp m + log sum exp(s - m) and the
mass of each K/V segment (block sums of the probabilities).  Results are cached per (set, form, dtype, pre-scaled Q or not,
valid counts): kernels that share inputs share one evaluation, and nobody changes a cached array."""
import numpy as np
import torch

from oracle import shared_attn_oracle as O

LOG2E = 1.4426950408889634
SCALE = 0.125
QC = SCALE * LOG2E

# B, H, Lq, query rows per work item
SETS = {"A": (47, 3, 600, 512), "B": (59, 3, 700, 256), "C": (37, 3, 650, 128)}
# include_self, Ls, N, Lr, AdaIN
FORMS = {"self+fold": (True, 384, 2, 320, True), "noself+plain": (False, 64, 4, 256, False)}
LONG = 4   # the bf16 runs on the GPU: every segment four times as long (64 tiles), see tests/test_gpu_item_grid.py


def form_shape(form, long=False):
    inc, Ls, N, Lr, adain = FORMS[form]
    return (inc, Ls * LONG if inc else Ls, N, Lr * LONG, adain) if long else FORMS[form]


def make_inputs(B, H, Lq, Ls, N, Lr, dtype, seed, device):
    """tests/test_gpu_w128.py::_inputs: q, the pre-scaled q (Q * scale * log2 e, rounded once), k, v, ref_k, ref_v"""
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, device=device)
    C = H * 64
    q = rnd(B, Lq, C).to(dtype)
    k, v = rnd(B, Ls, C).to(dtype), (rnd(B, Ls, C) * 0.9 + 0.3).to(dtype)
    rk = rnd(B, N, Lr, C).to(dtype)
    rv = (rnd(B, N, Lr, C) * 1.4 - 0.2).to(dtype)
    qs = (q.float() * QC).to(dtype)
    return q, qs, k, v, rk, rv


def set_inputs(name, form, dtype, device, batch=None, long=False):
    B, H, Lq, _ = SETS[name]
    _, Ls, N, Lr, _ = form_shape(form, long)
    seed = 7000 + 100 * sorted(SETS).index(name) + 10 * sorted(FORMS).index(form) + (dtype == torch.float16)
    return make_inputs(batch or B, H, Lq, Ls, N, Lr, dtype, seed, device)


def np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def lse_and_mass(q, k_self, ref_k, heads, scale, include_self):
    """float64, entry by entry: lse (B, H, Lq) = m + log sum exp(s - m) over all keys, mass (B, H, Lq, include_self + N) = the sums
    of exp(s - lse) over each segment's keys.  q (B, Lq, C), k_self (B, Ls, C), ref_k (B, N, Lr, C) or None"""
    B, Lq, C = q.shape
    d = C // heads
    lse = np.empty((B, heads, Lq))
    nseg = (1 if include_self else 0) + (0 if ref_k is None else ref_k.shape[1])
    mass = np.empty((B, heads, Lq, nseg))
    for b in range(B):
        segs = ([k_self[b]] if include_self else []) + ([] if ref_k is None else list(ref_k[b]))
        kk = np.concatenate(segs, axis=0).reshape(-1, heads, d).transpose(1, 2, 0)          # (H, d, Lkv)
        s = np.matmul(q[b].reshape(Lq, heads, d).transpose(1, 0, 2), kk) * scale             # (H, Lq, Lkv)
        m = s.max(-1, keepdims=True)
        e = np.exp(s - m)
        tot = e.sum(-1)
        lse[b] = m[..., 0] + np.log(tot)
        edge = 0
        for i, sg in enumerate(segs):
            mass[b, :, :, i] = e[..., edge:edge + sg.shape[0]].sum(-1) / tot
            edge += sg.shape[0]
    return lse, mass


def reference(q, k_self, v_self, ref_k, ref_v, heads, scale, use_adain, include_self):
    """(out (B, Lq, C), lse, mass) in float64 of float64 arrays"""
    out = np.concatenate([O.shared_attention_np(q[b:b + 1], k_self[b:b + 1], v_self[b:b + 1], None if ref_k is None else ref_k[b:b + 1],
                                                None if ref_v is None else ref_v[b:b + 1], heads, scale, use_adain, include_self)
                          for b in range(q.shape[0])])
    lse, mass = lse_and_mass(q, k_self, ref_k, heads, scale, include_self)
    return out, lse, mass


_CACHE = {}


def cached_reference(key, q_eff, k, v, rk, rv, heads, use_adain, include_self):
    """``reference`` of 16-bit tensors (``q_eff``: fp32, the Q the kernel works with divided by what it was pre-scaled by), once
    per ``key``; the arrays come back read-only"""
    if key not in _CACHE:
        res = reference(np64(q_eff), np64(k), np64(v), np64(rk), np64(rv), heads, SCALE, use_adain, include_self)
        for a in res:
            a.setflags(write=False)
        _CACHE[key] = res
    return _CACHE[key]
