"""Shapes and seeded input families of the LSE tests (tests/test_gpu_lse.py on the GPU, tests/test_lse_bounds_cpu.py for the
fp32 emulation and the lost-key / lost-tile shifts): the smallest shapes at which each forward path exists.

Families: N(0, 1); N(0, 1.5^2); peaky (2.5-scaled Q and K); and the recipes of
tests/test_gpu_round2.py::test_reference_checked_after_the_exponentials shrunk to these lengths - "ramp" (|k| grows along the key
axis: the lazy reference moves on most tiles), "spike" (one key of the last reference times 6, late in the walk) and "low" (the
walk's first tile far below zero).  IR_SWEEP_SEED offsets every seed."""
import os
from types import SimpleNamespace

import numpy as np
import torch

SCALE = 0.125
LOG2E = 1.4426950408889634
QC = SCALE * LOG2E
NEG = float("-inf")
FAMILIES = ["n1", "n15", "peaky", "ramp", "spike", "low"]
GAUSSIAN = ["n1", "n15"]                         # the families of the lost-key / lost-tile check

# B, H, Lq, Ls, N, Lr, include_self
PIPE32 = [(2, 2, 72, 72, 3, 40, True), (2, 2, 72, 72, 3, 40, False)]            # ragged tiles, partial row block
ODD = [(2, 2, 33, 33, 2, 37, True), (1, 1, 77, 77, 1, 1, True)]                 # nothing aligned; one-token reference
TAILS = [(1, 2, 300, 304, 2, 136, True)]                                        # key tails of 8 / 48 keys
W64 = [(2, 2, 64, 64, 2, 64, True), (1, 1, 576, 576, 3, 192, False)]
W128 = [(1, 1, 128, 128, 0, 0, True), (2, 2, 64, 64, 2, 64, True), (1, 2, 192, 128, 17, 64, True), (3, 2, 512, 512, 4, 256, False)]
W128_VALID = {(3, 2, 512, 512, 4, 256, False): [1, 3, 0]}
PIECES = [(4, 2, 128, 128, 4, 256, True), (4, 2, 128, 128, 4, 256, False)]
BIASED = (2, 2, 200, 72, 3, 200, True)
COUNTS = [[200, 0, 65], [1, 64, 137]]
FAMILY_SHAPES = PIPE32 + W64 + W128 + PIECES


def sid(s):
    return "B%dH%dLq%dLs%dN%dLr%d%s" % (s[0], s[1], s[2], s[3], s[4], s[5], "s" if s[6] else "n")


def seed_offset():
    return int(os.environ.get("IR_SWEEP_SEED", "0"))


def lkv(shape):
    B, H, Lq, Ls, N, Lr, inc = shape
    return (Ls if inc or N == 0 else 0) + N * Lr


def np64(t):
    return None if t is None else t.detach().float().cpu().numpy().astype(np.float64)


_CACHE = {}


def inputs(shape, family, dtype, valid=None):
    """CPU tensors rounded to ``dtype``, once per key and left unchanged: q, the pre-scaled qs = Q * scale * log2(e) rounded once,
    k, v, rk, rv (references n >= valid[b] zero-filled when ``valid`` is given)"""
    key = (shape, family, dtype, None if valid is None else tuple(valid), seed_offset())
    if key in _CACHE:
        return _CACHE[key]
    B, H, Lq, Ls, N, Lr, inc = shape
    C = H * 64
    seed = 9000 + 131 * FAMILIES.index(family) + 17 * Lq + 3 * N + Lr + int(inc) + (dtype == torch.float16) + 1000003 * seed_offset()
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    sc = {"n15": 1.5, "peaky": 2.5}.get(family, 1.0)
    q, k, v = rnd(B, Lq, C) * sc, rnd(B, Ls, C) * sc, rnd(B, Ls, C) * 0.9 + 0.3
    rk = rnd(B, N, Lr, C) * sc if N else None
    rv = rnd(B, N, Lr, C) * 1.4 - 0.2 if N else None
    walk_self = inc or N == 0
    if family == "ramp":
        if walk_self:
            k = k * torch.linspace(0.2, 6.0, Ls).view(1, Ls, 1)
        if N:
            rk = rk * torch.linspace(6.0 if walk_self else 0.2, 14.0, N * Lr).view(1, N, Lr, 1)
    elif family == "spike":
        if N:
            rk[:, N - 1, Lr // 2] *= 6.0
        else:
            k[:, (3 * Ls) // 4] *= 6.0
    elif family == "low":
        q = q + 1.5
        if walk_self:
            k[:, :min(64, Ls // 2)] -= 20.0
        else:
            rk[:, 0, :min(64, Lr // 2)] -= 20.0
    if valid is not None:
        for b in range(B):
            rk[b, valid[b]:] = 0
            rv[b, valid[b]:] = 0
    r = lambda t: None if t is None else t.to(dtype)
    q, k, v, rk, rv = r(q), r(k), r(v), r(rk), r(rv)
    qs = (q.float() * QC).to(dtype)
    res = SimpleNamespace(shape=shape, family=family, dtype=dtype, valid=valid, q=q, qs=qs, k=k, v=v, rk=rk, rv=rv)
    _CACHE[key] = res
    return res


def q_true(x, presc):
    """float64 (B, Lq, C): the Q whose scores the call computes - the 16-bit q, or what the pre-scaled bits stand for"""
    return np64(x.qs) / QC if presc else np64(x.q)


def bias_patterns(shape, seed=0):
    """name -> (B, Lkv) fp32 bias of the BIAS forms' case: a -inf mask over scattered keys, a finite bias of both signs, each with
    one fully masked entry (the last)"""
    B = shape[0]
    n = lkv(shape)
    g = torch.Generator().manual_seed(77 + seed + 1000003 * seed_offset())
    scatter = torch.zeros(B, n)
    m = torch.rand(B, n, generator=g) < 0.3
    m[:, 0] = False
    scatter[m] = NEG
    finite = torch.rand(B, n, generator=g) * 12 - 6
    dead = finite.clone()
    dead[B - 1] = NEG
    return {"scatter": scatter, "finite": finite, "finite_one_entry_masked": dead}


def tail_bias(shape, counts):
    """(B, Lkv) float64: -inf on every key t >= counts[b][n] of every reference - the oracle's form of ref_lens"""
    B, H, Lq, Ls, N, Lr, inc = shape
    off = Ls if inc else 0
    bias = np.zeros((B, off + N * Lr))
    for b in range(B):
        for n in range(N):
            bias[b, off + n * Lr + min(max(counts[b][n], 0), Lr): off + (n + 1) * Lr] = NEG
    return bias


def cpu_sets(dtypes=(torch.bfloat16, torch.float16)):
    """every input set of tests/test_gpu_lse.py as (id, q_true (B, Lq, C), packed keys (B, Lkv, C), heads, bias or None, family):
    what the CPU tests run their emulation and their lost-key experiments on"""
    from lse_bounds import pack_keys
    for dtype in dtypes:
        dt = "bf16" if dtype == torch.bfloat16 else "f16"
        for shape in FAMILY_SHAPES + ODD + TAILS:
            fams = FAMILIES if shape in FAMILY_SHAPES else ["n15"]
            for fam in fams:
                x = inputs(shape, fam, dtype, W128_VALID.get(shape))
                keys = pack_keys(x.k, x.rk, shape[6])
                for presc in ((False, True) if fam in GAUSSIAN else (True,)):
                    yield f"{sid(shape)}-{fam}-{dt}-{'prescq' if presc else 'plainq'}", q_true(x, presc), keys, shape[1], None, fam
        x = inputs(BIASED, "n1", dtype)
        keys = pack_keys(x.k, x.rk, True)
        for name, bias in bias_patterns(BIASED).items():
            yield f"{sid(BIASED)}-bias-{name}-{dt}", q_true(x, False), keys, BIASED[1], bias.double().numpy(), "bias"
        yield f"{sid(BIASED)}-counts-{dt}", q_true(x, True), keys, BIASED[1], tail_bias(BIASED, COUNTS), "counts"
