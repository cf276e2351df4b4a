"""Shapes and seeded input families of the LSE tests (tests/test_gpu_lse.py on the GPU, tests/test_lse_bounds_cpu.py for the
fp32 emulation and the lost-key / lost-tile shifts): the smallest shapes at which each forward path exists.

Families: N(0, 1); N(0, 1.5^2); peaky (2.5-scaled Q and K); and the recipes of
tests/test_gpu_round2.py::test_reference_checked_after_the_exponentials shrunk to these lengths - "ramp" (|k| grows along the key
axis: the lazy reference moves on most tiles), "spike" (one key of the last reference times 6, late in the walk) and "low" (the
walk's first tile far below zero).  IR_SWEEP_SEED offsets every seed.

The output walks (tests/test_gpu_out_walks.py, tests/test_out_bounds_cpu.py) add, without changing any of the above: the boundary
spikes "at:<where>" - one dominant key (times SPIKE_X) at a named place of the walk (``boundary_keys``), ``styled_values`` (AdaIN
scales that differ by 20x and 80x between neighbouring segments, a near-constant style channel), the masks of the BIAS, RAGGED and
REGION forms' cases (``case_mask``) and the list of cases (``out_walk_cases``, ``relied_on``)."""
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
# ---- the output walks (tests/test_gpu_out_walks.py, tests/test_out_bounds_cpu.py) ----
WALK_FAMILIES = ["peaky", "ramp", "spike", "low"]                   # the existing families that move the lazy reference
BOUNDARY = ["tile_last", "tile_first", "seg_last", "seg_first", "tail_last", "piece_first"]
MASKED_SPIKES = ["behind_masked"]                                   # an allowed key directly behind a fully masked tile
AT = BOUNDARY + MASKED_SPIKES
SPIKE_X = 16.0       # the "spike" recipe (one key times 6) raised: a score of N(0, (16 * 1.44)^2) exponent units outgrows a reference
#                      by the 11 units of the partial-sum rule on more than 10 % of the rows, not only by the 6 of the row-max rule
KVB = 64             # keys per K/V tile of every kernel's walk
REGION = (2, 2, 200, 72, 3, 200, True)                              # the REGION forms' case: the size of BIASED


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


def inputs(shape, family, dtype, valid=None, style=False, counts=None):
    """CPU tensors rounded to ``dtype``, once per key and left unchanged: q, the pre-scaled qs = Q * scale * log2(e) rounded once,
    k, v, rk, rv (references n >= valid[b] zero-filled when ``valid`` is given).  ``family`` is one of FAMILIES or "at:<where>", a
    boundary spike (``boundary_keys``; ``counts`` are the token counts its "tail_last" needs).  ``style``: the values of
    ``styled_values`` instead of the plain ones - q and k are the same either way"""
    key = (shape, family, dtype, None if valid is None else tuple(valid), seed_offset(), style, None if counts is None else str(counts))
    if key in _CACHE:
        return _CACHE[key]
    B, H, Lq, Ls, N, Lr, inc = shape
    C = H * 64
    fam_index = FAMILIES.index(family) if family in FAMILIES else len(FAMILIES) + AT.index(family[3:])
    seed = 9000 + 131 * fam_index + 17 * Lq + 3 * N + Lr + int(inc) + (dtype == torch.float16) + 1000003 * seed_offset()
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
    if family.startswith("at:"):
        where = boundary_keys(shape, family[3:], counts)
        assert where is not None, (shape, family)
        for b in range(B):
            j = where[b]
            if walk_self and j < Ls:
                k[b, j] *= SPIKE_X
            else:
                rk[b].view(N * Lr, C)[j - (Ls if walk_self else 0)] *= SPIKE_X
    if style:
        styled_values(v, rv, seed)
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


def seg_lens(shape):
    B, H, Lq, Ls, N, Lr, inc = shape
    return ([Ls] if inc or N == 0 else []) + [Lr] * N


def tiles(shape, counts_b=None):
    """(first key, one past the last EXISTING key, segment) of every 64-key tile of the walk over the packed key axis; with
    ``counts_b`` (the token counts of one entry's references) a tile ends at its segment's count and tiles without keys are left out"""
    out, off = [], 0
    lens = seg_lens(shape)
    first_ref = len(lens) - shape[4]
    for s, n in enumerate(lens):
        have = n if counts_b is None or s < first_ref else min(max(int(counts_b[s - first_ref]), 0), n)
        out += [(off + t, min(off + t + KVB, off + have), s) for t in range(0, have, KVB)]
        off += n
    return out


def masked_tile(shape):
    """(first, one past the last) key of the tile the masked forms' cases mask for everybody: the second tile of the middle segment"""
    lens = seg_lens(shape)
    s = len(lens) // 2
    assert lens[s] > 2 * KVB, shape
    lo = sum(lens[:s]) + KVB
    return lo, lo + KVB


def boundary_keys(shape, where, counts=None):
    """per entry b, the packed key index of the dominant key of the boundary spike ``where`` - or None where the shape has no such
    place.  tile_last / tile_first: the two sides of the walk's last tile boundary inside a segment; seg_last / seg_first: the two
    sides of its last segment boundary; tail_last: the last existing key of the walk's last tile when that tile is ragged; piece_first: the first key of the second of two K/V-range pieces
    (tile ntiles // 2, the kernels' cut); behind_masked: the first key behind ``masked_tile``.  With ``counts`` (the references' token
    counts) every place is taken among the keys that exist, entry by entry"""
    B = shape[0]
    keys = [_boundary_key(shape, where, tiles(shape, None if counts is None else counts[b])) for b in range(B)]
    return None if any(k is None for k in keys) else keys


def _boundary_key(shape, where, tl):
    """one entry's key from its existing tiles ``tl``; None where it has no such place or the place is in the walk's first tile (a
    dominant key there moves no reference after the first tile)"""
    if where in ("tile_last", "tile_first"):
        inner = [t for i, t in enumerate(tl) if i and tl[i - 1][2] == t[2]]
        key = inner[-1][0] - (where == "tile_last") if inner else None
    elif where in ("seg_last", "seg_first"):
        edge = [i for i in range(1, len(tl)) if tl[i - 1][2] != tl[i][2]]
        key = (tl[edge[-1] - 1][1] - 1 if where == "seg_last" else tl[edge[-1]][0]) if edge else None
    elif where == "tail_last":
        key = tl[-1][1] - 1 if tl and tl[-1][1] - tl[-1][0] < KVB else None
    elif where == "piece_first":
        key = tl[len(tl) // 2][0] if len(tl) >= 2 else None
    elif where == "behind_masked":
        key = masked_tile(shape)[1]
    else:
        raise KeyError(where)
    return None if key is None or key < tl[0][1] else key


def styled_values(v, rv, seed):
    """in place, fp32, ahead of the rounding: reference values whose AdaIN scales differ by 20x and 80x between neighbouring
    segments (a fold applied in the neighbour's frame moves the output by far more than any bound), an outlier content channel,
    and one near-constant style channel per head (a -> sigma_style / sigma_ref ~ 1e-3: there A << S, the fp32 term of
    tests/out_bounds.py shows) - the recipe of tests/test_gpu_parity.py::test_massive_activation_channels"""
    g = torch.Generator().manual_seed(seed + 500009)
    v[..., 3::64] = 0.7 + 1e-3 * torch.randn(v.shape[0], v.shape[1], v.shape[2] // 64, generator=g)
    if rv is not None:
        for n in range(rv.shape[1]):
            rv[:, n] *= (1.0, 0.05, 4.0)[n % 3]
        rv[..., 9] *= 30.0


def region_rule(shape, seed=0):
    """(q_allow (B, Lq) int32, key_region (B, Lkv) int32) of the REGION forms' case: segment s is region s, ``masked_tile`` is
    nobody's (-1); the rows may attend everything / self and reference 1 / references 0 and 2 / self and reference 2 in turn
    (shifted by one per entry), so the fold meets segments that are masked for some rows only, and two rows nothing at all"""
    B, Lq = shape[0], shape[2]
    lens = seg_lens(shape)
    kr = torch.cat([torch.full((n,), s, dtype=torch.int32) for s, n in enumerate(lens)]).repeat(B, 1)
    lo, hi = masked_tile(shape)
    kr[:, lo:hi] = -1
    sets = torch.tensor([0b1111, 0b0101, 0b1010, 0b1001], dtype=torch.int32)
    qa = torch.stack([sets[(torch.arange(Lq) + b + seed) % 4] for b in range(B)])
    qa[:, 7] = 0
    qa[B - 1, Lq - 50] = 0
    return qa, kr


def masked_tile_bias(shape):
    """(B, Lkv) fp32: -inf on ``masked_tile``, 0 elsewhere"""
    bias = torch.zeros(shape[0], lkv(shape))
    lo, hi = masked_tile(shape)
    bias[:, lo:hi] = NEG
    return bias


def dominant_key(shape, family, counts=None):
    """per entry, the packed index of the one key a family makes dominant ("spike", the boundary spikes), or None"""
    B, H, Lq, Ls, N, Lr, inc = shape
    if family == "spike":
        return [((Ls if inc else 0) + (N - 1) * Lr + Lr // 2) if N else (3 * Ls) // 4] * B
    return boundary_keys(shape, family[3:], counts) if family.startswith("at:") else None


def relied_on(shape, family, kind="plain", which=None, rule11=False):
    """whether the output walks rely on a case to move the reference after the first tile: everything but "low" where its block of
    keys far below zero, min(64, L // 2) keys, does not fill the walk's first tile (the ordinary keys behind it then set the first
    reference and nothing moves it), and "spike" - one key times 6 - under COUNTS (the key lies behind entry 0's count) and under the region rule (a quarter of the rows may not attend
    it), and behind more than 1024 keys, whose maximum leaves fewer than a tenth of the rows 6 exponent units of room (the boundary
    spikes are one key times 16).  Those cases run all the same"""
    B, H, Lq, Ls, N, Lr, inc = shape
    if rule11 and family in ("spike", "peaky"):      # the 2^11 partial-sum rule of the forms that check after the exponentials
        return False
    if family == "spike" and (lkv(shape) > 1024 + Lr or kind in ("counts", "region")):
        return False
    return family != "low" or (Ls if inc or N == 0 else Lr) >= 2 * KVB


def walk_families(shape, counts=None, masked=False, pieces=True):
    """the families of the output walks at a shape: the reference-moving ones and every boundary spike the shape has a place for
    (``pieces=False``: a call that runs a single piece has no "piece_first")"""
    at = [w for w in BOUNDARY if (pieces or w != "piece_first") and boundary_keys(shape, w, counts) is not None] + (MASKED_SPIKES if masked else [])
    return WALK_FAMILIES + ["at:" + w for w in at]


def out_walk_cases():
    """(shape, family, kind, which) of every input set of the output walks: kind "plain", "bias" (which: a ``bias_patterns`` name or
    "masked_tile"), "counts" (COUNTS) or "region" (``region_rule``).  The masked kinds run a single piece; where a tile is masked for
    everybody, a boundary spike whose key lies in it is left out (a masked key is inert: a test of its own)"""
    def unmasked(fams, shape):
        lo, hi = masked_tile(shape)
        return [f for f in fams if not (f.startswith("at:") and lo <= boundary_keys(shape, f[3:])[0] < hi)]
    cases = []
    for shape in dict.fromkeys(PIPE32 + W64 + W128 + PIECES):
        cases += [(shape, fam, "plain", None) for fam in walk_families(shape)]
    for pattern in ("scatter", "finite"):
        cases += [(BIASED, fam, "bias", pattern) for fam in walk_families(BIASED, pieces=False)]
    cases += [(BIASED, fam, "bias", "masked_tile") for fam in unmasked(walk_families(BIASED, masked=True, pieces=False), BIASED)]
    cases += [(BIASED, fam, "counts", None) for fam in walk_families(BIASED, counts=COUNTS, pieces=False)]
    cases += [(REGION, fam, "region", None) for fam in unmasked(walk_families(REGION, masked=True, pieces=False), REGION)]
    return cases


def case_mask(shape, kind, which, family=None):
    """(bias (B, Lkv) fp32 or None, counts or None, (q_allow, key_region) or None) of a case of ``out_walk_cases``; the scattered
    mask leaves the family's dominant key, where it has one, unmasked and the finite bias gives it the top of its range, +6"""
    if kind == "bias":
        bias = masked_tile_bias(shape) if which == "masked_tile" else bias_patterns(shape)[which].clone()
        dom = dominant_key(shape, family) if family and which in ("scatter", "finite") else None
        for b in range(shape[0] if dom else 0):
            bias[b, dom[b]] = 0.0 if which == "scatter" else 6.0
        return bias, None, None
    if kind == "counts":
        return None, COUNTS, None
    if kind == "region":
        return None, None, region_rule(shape)
    return None, None, None


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
