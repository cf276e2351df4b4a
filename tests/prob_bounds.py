"""The bound every oracle comparison of an attention READ-OUT probability is held to - the sibling of tests/lse_bounds.py (the
LSE and the by-product masses) and tests/out_bounds.py (the forward's outputs).

Every read-out (``ir_attn_probs[_ex]``, ``ir_attn_rows``, ``ir_attn_match``, ``ir_attn_topk``, ``ir_attn_key_match``,
``ir_attn_transfer``, ``ir_attn_received``) recomputes the same fp32 probability from the LSE of the fused forward
(csrc/ir_readout.h) and rounds or reduces it:

    p = exp2(fma(<q, k>, scale*log2(e), -lse*log2(e)))

It is held ELEMENT BY ELEMENT, RELATIVE to its own size, against float64 on the same 16-bit-rounded inputs.

References.  Both float64; under IR_FLAG_Q_PRESCALED ``scale * <q, k>`` is ``ln2 * <qs, k>`` (callers hand ``q_true = qs / (scale
log2 e)``, ``lse_cases.q_true``, which is the same number).
  A (device LSE)   p_A[b,h,i,j] = exp(scale <q_i, k_j> - lse_dev[b,h,i])  with the LSE the forward returned, read back: the read-out's
                   own arithmetic and nothing else;
  B (oracle)       p_B = exp(scale <q_i, k_j> - lse_ref).  A device probability is p_A * exp(+-delta_i), delta_i =
                   ``lse_bounds.bound(row_scale_i, klass)`` (klass "frame" when the LSE came from a pre-scaled-Q forward, else
                   "fp32"), and |exp(delta) - 1| <= 2 delta: against B the bound grows by 2 * delta_i * p_B.  Derived, not measured:
                   tests/test_gpu_lse.py holds the LSE.

The bound of an fp32 probability (``prob`` of match, topk and key_match, a one-hot channel of received or transfer, the per-head
terms of the fp32 row forms):

    |p - p_A| <= K_P * 2^-23 * E_ij * p_A  +  2^-126
    E_ij = max(1, |lse_dev[b,h,i]|, scale * sum_d |q_id k_jd|)

E is PER ELEMENT: the size of what is rounded in fp32 on the way to that element's exponent - the partial sums of the 64-term MFMA
dot product, lse * log2(e) (rounded once in ``load_q``), the fused multiply-add - and v_exp_f32 adds one ulp of the result.  An
exponent that is off by x moves the probability by |exp(x) - 1|, so a RELATIVE bound in 2^-23 * E is what fp32 arithmetic owes.
2^-126: ``fast_exp2`` is the raw builtin and flushes results below the smallest normal fp32.

Starting value of K_P, derived as tests/out_bounds.py derives its own: in units of 2^-23 * E of the natural-log exponent, at worst
one rounding of 2^-24 * (sum of magnitudes) per term of the 64-term dot product = 32 units (log2(e) on the way into the exp2 domain
and ln 2 on the way out cancel), one rounding each for scale * log2(e) (2^-24 of the score: 0.5), lse * log2(e) (0.5) and the
fused multiply-add (0.5), and one ulp of the result for v_exp_f32 (1 / E <= 1): about 35 -> 64 before the measurement, which
replaces it (below).  The measured constants are far smaller for the reason tests/out_bounds.py gives: the matrix pipe does not
round once per term, and E - the sum of the terms' magnitudes - overstates what a score of a few units loses.

16-bit outputs (the dump, form "none" of rows): the one rounding on top, u * p_A * (1 + rel) with u = 2^-8 (bf16) / 2^-11 (fp16)
and rel the relative part of the fp32 bound, plus the type's subnormal step - 2^-25 for fp16 (half the spacing of its subnormals),
2^-126 for bf16 (a flush is allowed).

Reduced forms.  Head mean: the mean over the heads of the per-head bounds plus (H + 1) * 2^-24 times the reference mean (H - 1
additions, 1 / H and the product).  Map: the sum over the rows of the head-mean bounds plus R * 2^-24 times the reference sum.

Indices (match, topk, key_match): p_A[index_t] >= (t-th largest p_A) * (1 - 2 * rel_t) - 2^-126 with rel_t the relative part of the
bound at the returned element - an order statistic moves by at most the sup of the relative error, on both sides.

Every check returns r = max(0, |err| - derived terms) / (2^-23 * E * p_ref), the largest over the elements: what is left for the
calibrated term, in its own unit; the comparison holds iff r <= K_P.  The derived terms are the floors, the 16-bit rounding, 2 delta
p_B and the summation terms of the reduced forms.  For a 16-bit output the rounding explains nearly everything and r is mostly 0 -
the fp32 outputs calibrate.  Rows without a key (lse = -inf) and rows of an out-of-range index (``dead``) must be exact zeros; NaN,
Inf and a shape mismatch fail.

Cases (``cases``): the smallest shapes at which each store shape and gather path of the read-outs exists, with the families of
tests/lse_cases.py.  Where the exponent range of a family leaves more than 10 % of a comparison's elements below 2^-100, where the
floor excuses them, the family leaves the list (tests/test_prob_bounds_cpu.py asserts the cap on what is listed): see DROPPED.

How K_P was fixed: against float64 only - reference A, never one kernel against another (IR_PROB_SOFT=1 and IR_PARITY_LOG=<file>
on the MI355X, tests/test_gpu_prob_bounds.py at IR_SWEEP_SEED 0, 1, 2); the largest r per class; constant = 4 * r rounded up to a
power of two (a factor 2 for the maximum of a rounding random walk moving between seeds, a factor 2 for a runtime whose exp2
differs in the last bit - the rule of tests/lse_bounds.py); no ratio above half the constant at any of the three seeds.
tests/test_prob_bounds_cpu.py shows that a sequential fp32 emulation of the expression stays inside the bound and that an LSE
rounded to fp16, scale * log2(e) rounded to bf16, an exponent clamped at -14 and a score rounded to 16 bit each leave it by more
than 4x on more than a tenth of the rows, where the old absolute gate (1e-3 fp16 / 8e-3 bf16) accepted the first and the third.

MEASURED on an MI355X (IR_PARITY_LOG records of tests/test_gpu_prob_bounds.py at IR_SWEEP_SEED 0, 1, 2; reference A; unit: 2^-23 * E * p_A):
    class    comparisons   median   largest   where                                                                      constant
    plain    13020         0.56     1.60      seed 2, attn_received one-hot rows, B1 H1 Lq77 Ls77 N1 Lr1 self,           8
                                              N(0, 1.5^2), fp16, row 76 key 16 (seeds 0, 1: 1.49, 1.59 - the head mean
                                              of attn_rows over all rows, B1 H1 Lq1024 Ls1024 N4 Lr1024 self)
    presc    1980          0.45     1.47      seed 0, attn_rows head mean over all rows, B1 H1 Lq576 N3 Lr192 no self,   8
                                              "ramp", fp16, row 500 key 317 (seeds 1, 2: 1.35, 1.42)
    By output, the largest of the three seeds (plain / presc): the fp32 window of received and transfer 1.60 / 1.30; rows head mean
    1.59 / 1.47, map 1.09 / 1.02; match per head 1.26 / 1.15, head mean 1.18 / 1.11; topk 1.34, 1.26; key_match 1.26, 1.18; the 16-bit
    outputs (dump, rows "none"; 1710 comparisons) 0 throughout - their one rounding explains every error.  The pre-scaled flag does
    not measure differently: one value, kept per class for the records.  Reference B (15000 comparisons): 0 throughout - 2 delta p_B,
    with KAPPA 16 / 8 of tests/lse_bounds.py, covers what the device's LSE moves.  No ratio above half the constant at any seed
    (largest 1.49 / 1.59 / 1.60).  The fp32 emulation of tests/test_prob_bounds_cpu.py reaches 2.91 / 2.74 over 114 input sets:
    sequential accumulation loses more than the matrix pipe does.  Families dropped for the 10 % cap: "low" at every shape but the
    eight-reference one (DROPPED); "ramp" stays everywhere.

IR_PARITY_LOG=<file> appends one JSON record per comparison (test id, kind, class, r, r / K_P, max error, where); IR_PROB_SOFT=1
records violations of the bound without failing (calibration runs only - no committed file sets it; NaN / Inf / shape / dead rows
still fail).
"""
import json
import os

import numpy as np
import torch

import lse_bounds as LB
import lse_cases as LC
from lse_bounds import _to64, bound, pack_keys, row_scale          # noqa: F401  (re-exported: the siblings' helpers)

EPS = 2.0 ** -23
FLOOR32 = 2.0 ** -126                                           # fast_exp2 flushes below the smallest normal fp32
K_P_DERIVED = 64.0                                              # the starting value (module docstring)
K_P = {"plain": 8.0, "presc": 8.0}                              # measured, see the table above: 4 x 1.60 / 4 x 1.47, rounded up
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUB16 = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25}
OLD_TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}           # the absolute gate of tests/test_gpu_probs.py, for the record
LN2 = 0.6931471805599453
TINY_P = 2.0 ** -100                                            # below this the floor excuses an element: at most CAP of a comparison
CAP = 0.10

# ---- the cases of tests/test_gpu_prob_bounds.py and tests/test_prob_bounds_cpu.py -------------------------------------------------
FAMILIES = ["n1", "n15", "peaky", "spike", "low", "ramp"]
BIG = (1, 1, 1024, 1024, 4, 1024, True)                         # family "n15" only; key chunks cut the segments
SHAPES = LC.PIPE32 + LC.ODD + [LC.TAILS[0], LC.W64[1], (2, 1, 64, 64, 8, 64, True), (1, 2, 96, 96, 0, 0, True)]   # see the GPU file's table
PRESC_SHAPES = [LC.PIPE32[0], LC.TAILS[0], LC.W64[1]]
EIGHT_REFS = SHAPES[6]
# shape -> the families the 10 % cap removes.  "low" puts min(64, L // 2) keys of the walk's first segment about 240 below the others
# (p ~ e^-240): 11 % of the keys at the two longest shapes, 15 % to 50 % at the short ones, 5.6 % with eight references - the one
# shape that keeps it.  "ramp" stays everywhere: its steep rows leave at most 0.4 % of the elements below 2^-100.
DROPPED = {s: ("low",) for s in SHAPES if s != EIGHT_REFS}
DTYPES = [torch.float16, torch.bfloat16]


def cases():
    """(shape, family) of every input set"""
    out = [(s, f) for s in SHAPES for f in FAMILIES if f not in DROPPED.get(s, ())]
    return out + [(BIG, "n15")]


def presc_cases():
    return [(s, f) for s in PRESC_SHAPES for f in FAMILIES if f not in DROPPED.get(s, ())]


def klass_of(presc):
    return "presc" if presc else "plain"


# ---- references ---------------------------------------------------------------------------------------------------------------------
def scores_and_sizes(q_true, keys, heads, scale):
    """float64 (B, H, Lq, Lkv): s = scale * <q_i, k_j> and T = |scale| * sum_d |q_id k_jd| per head, for q_true (B, Lq, C) and packed
    keys (B, Lkv, C) (``pack_keys``)"""
    q, kk = _to64(q_true), _to64(keys)
    B, Lq, C = q.shape
    d, lkv = C // heads, kk.shape[1]
    qh = q.reshape(B, Lq, heads, d).transpose(0, 2, 1, 3)
    kh = kk.reshape(B, lkv, heads, d).transpose(0, 2, 3, 1)
    return np.matmul(qh, kh) * scale, np.matmul(np.abs(qh), np.abs(kh)) * abs(scale)


def lse_of(s):
    """float64 log-sum-exp over the last axis, (B, H, Lq); -inf for a row without keys"""
    if s.shape[-1] == 0:
        return np.full(s.shape[:-1], -np.inf)
    m = s.max(-1, keepdims=True)
    return (m + np.log(np.exp(s - m).sum(-1, keepdims=True)))[..., 0]


def probs_given_lse(s, lse):
    """reference A with the device's LSE, reference B with the oracle's: exp(s - lse), exact zeros on the rows whose LSE is -inf"""
    lse = _to64(lse)[..., None]
    live = np.isfinite(lse)
    with np.errstate(over="ignore"):
        return np.where(live, np.exp(s - np.where(live, lse, 0.0)), 0.0)


def dead_rows(lse):
    """bool, the shape of ``lse`` with a last axis of 1: the rows without a key (lse = -inf), whose probabilities must be exact zeros -
    the ``dead`` of ``check_probs``"""
    return np.isneginf(_to64(lse))[..., None]


def elem_scale(T, lse):
    """E_ij = max(1, |lse_i|, T_ij), (B, H, Lq, Lkv)"""
    lse = _to64(lse)[..., None]
    return np.maximum(np.maximum(1.0, np.where(np.isfinite(lse), np.abs(lse), 0.0)), T)


def lse_delta(q_true, keys, scale, lse_ref, presc):
    """delta_i (B, H, Lq): what the device's LSE may be off by - ``lse_bounds.bound`` at the row's scale, class "frame" for the LSE
    of a pre-scaled-Q forward"""
    return LB.bound(LB.row_scale(q_true, keys, scale, lse_ref, frame=presc), "frame" if presc else "fp32")


# ---- the bound, in two parts --------------------------------------------------------------------------------------------------------
def terms(ref, E, dtype=None, delta=None, klass="plain"):
    """(cal, derived) of |got - ref| <= K_P[klass] * cal + derived, element-wise: cal = 2^-23 * E * ref is the unit of the calibrated
    term; derived holds the fp32 floor, 2 * delta * ref (reference B; ``delta`` broadcastable to ``ref``) and, for a 16-bit output
    ``dtype``, its rounding u * ref * (1 + rel) and subnormal step"""
    ref, E = np.asarray(ref, dtype=np.float64), np.asarray(E, dtype=np.float64)
    cal = EPS * E * ref
    d2 = 0.0 if delta is None else 2.0 * np.asarray(delta, dtype=np.float64)
    derived = FLOOR32 + d2 * ref
    if dtype is not None:
        rel = K_P[klass] * EPS * E + d2
        derived = derived + U16[dtype] * ref * (1.0 + rel) + SUB16[dtype]
    return cal, derived


def head_mean_terms(cal, derived, ref, axis=1):
    """the head-mean form from the per-head terms (B, H, ...): the mean of the bounds plus (H + 1) * 2^-24 * the reference mean"""
    H = ref.shape[axis]
    return cal.mean(axis), derived.mean(axis) + (H + 1) * 2.0 ** -24 * ref.mean(axis), ref.mean(axis)


def map_terms(cal_hm, derived_hm, ref_hm, axis=1):
    """the map from the head-mean terms (B, R, Lkv): the sum over the rows plus R * 2^-24 * the reference sum"""
    R = ref_hm.shape[axis]
    return cal_hm.sum(axis), derived_hm.sum(axis) + R * 2.0 ** -24 * ref_hm.sum(axis), ref_hm.sum(axis)


def _soft():
    return os.environ.get("IR_PROB_SOFT") == "1"


def _record(kind, what, klass, r, err, at):
    log = os.environ.get("IR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"kind": kind, "what": str(what)[:200], "test": os.environ.get("PYTEST_CURRENT_TEST", "")[:200], "class": klass,
                                "r": r, "r_over_k": r / K_P[klass], "err": err, "at": [int(i) for i in at], "k_p": K_P[klass]}) + "\n")


def check_terms(got, ref, cal, derived, what, klass="plain", kind="prob", enforce=True, dead=None):
    """|got - ref| <= K_P[klass] * cal + derived element-wise; exact zeros where ``dead`` (bool, broadcastable); nothing non-finite.
    Returns r = max(0, |err| - derived) / cal, the largest over the elements (``enforce=False``: also where it is above K_P - for the
    tests that plant a defect and want the figure)"""
    got, ref = _to64(got), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape}, the reference has {ref.shape}"
    cal, derived = np.broadcast_to(cal, ref.shape), np.broadcast_to(derived, ref.shape)
    assert np.isfinite(got).all(), f"{what}: NaN or Inf in the result"
    assert np.isfinite(ref).all() and (ref >= 0).all(), f"{what}: the reference is not a probability"
    if dead is not None:
        dead = np.broadcast_to(dead, ref.shape)
        assert (got[dead] == 0.0).all(), f"{what}: a row without a key or of an invalid index is not exactly 0"
    err = np.abs(got - ref)
    left = np.maximum(0.0, err - derived)
    ratio = np.where(left > 0.0, left / np.maximum(cal, np.finfo(np.float64).tiny), 0.0)
    if dead is not None:
        ratio = np.where(dead, 0.0, ratio)
    r = float(ratio.max()) if ratio.size else 0.0
    at = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.size else ()
    _record(kind, what, klass, r, float(err.max()) if err.size else 0.0, at)
    print(f"{kind} {what}: largest ratio {r:.3f} x 2^-23 E p (K_P {K_P[klass]:g}), largest |err| {float(err.max()) if err.size else 0.0:.3e}")
    if enforce and not _soft() and r > K_P[klass]:
        raise AssertionError(f"{what}: {kind} off by {err[at]:.3e} at {tuple(int(i) for i in at)} = {r:.1f} x 2^-23 x E x p beyond the derived terms "
                             f"{derived[at]:.3e} (K_P {K_P[klass]:g}; unit {cal[at]:.3e}, reference {ref[at]:.6e})")
    return r


def check_probs(got, ref, E, dtype, what, delta=None, enforce=True, klass="plain", dead=None, kind=None):
    """``got`` against ``ref`` (p_A, or p_B with ``delta``) of the same shape under the element-wise bound: fp32 (``dtype`` None) or
    the 16-bit type's.  ``E`` and ``delta`` broadcastable to ``ref``.  Returns the largest ratio (``check_terms``)."""
    cal, derived = terms(ref, E, dtype, delta, klass)
    kind = kind or ("prob" + ("32" if dtype is None else "16") + ("A" if delta is None else "B"))
    return check_terms(got, ref, cal, derived, what, klass, kind, enforce, dead)


def check_index(ref_at_index, ref_order_stat, rel_at_index, what):
    """the index rule: p_ref[index_t] >= (t-th largest p_ref) * (1 - 2 * rel_t) - 2^-126, element-wise.  Returns the largest
    shortfall (t-th largest - p_ref[index_t]) / (t-th largest), 0 where the returned key is a maximiser"""
    a, best, rel = (np.asarray(x, dtype=np.float64) for x in (ref_at_index, ref_order_stat, rel_at_index))
    assert a.shape == best.shape, (what, a.shape, best.shape)
    rel = np.broadcast_to(np.where(np.isfinite(rel), rel, 1.0), a.shape)
    ok = a >= best * (1.0 - 2.0 * rel) - FLOOR32
    gap = np.where(best > 0, (best - a) / np.maximum(best, np.finfo(np.float64).tiny), 0.0)
    worst = float(gap.max()) if gap.size else 0.0
    print(f"index {what}: largest (t-th largest p - p[index_t]) / t-th largest {worst:.3e}")
    if not _soft():
        assert ok.all(), f"{what}: the returned key is not a maximiser within 2 rel: {a[~ok][:4]} against {best[~ok][:4]} (rel {rel[~ok][:4]})"
    return worst


def rel_part(cal, derived, ref, klass="plain"):
    """the relative part of the bound at every element: bound / reference (inf where the reference is 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref > 0, (K_P[klass] * cal + derived) / ref, np.inf)


def check_ranked(index, prob, ref, cal, der, edges, bad_rows, what, klass="plain", kind="ranked", tops=None, kmax=8):
    """``index`` / ``prob`` (..., R, S, k) against ``ref`` / ``cal`` / ``der`` (..., R, n) over the segments ``edges`` of the last axis:
    ``prob`` under the bound at the returned element, the index rule against the t-th largest reference of the segment, and -1 / 0
    on the ranks a segment does not have and on the rows ``bad_rows`` (..., R).  ``tops``: a dict that keeps the sorted head of every
    segment of ``ref`` between calls with the same ``ref``"""
    tops = {} if tops is None else tops
    index = (index.cpu().numpy() if isinstance(index, torch.Tensor) else np.asarray(index)).astype(np.int64)
    prob = _to64(prob)
    assert index.shape == prob.shape and index.shape[:-2] == ref.shape[:-1], (what, index.shape, prob.shape, ref.shape)
    k = index.shape[-1]
    ref_at, cal_at, best = np.zeros(index.shape), np.zeros(index.shape), np.zeros(index.shape)
    der_at = np.full(index.shape, FLOOR32)
    dead = np.ones(index.shape, dtype=bool)
    for si, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        n = min(k, b - a)
        ix = index[..., si, :n]
        ok = np.broadcast_to(~bad_rows[..., None], ix.shape)
        assert (ix[ok] >= 0).all() and (ix[ok] < b - a).all(), f"{what}: an index outside segment {si}"
        at = a + np.where(ok, ix, 0)
        ref_at[..., si, :n] = np.take_along_axis(ref, at, axis=-1)
        cal_at[..., si, :n] = np.take_along_axis(cal, at, axis=-1)
        der_at[..., si, :n] = np.take_along_axis(der, at, axis=-1)
        if si not in tops:
            tops[si] = -np.sort(-ref[..., a:b], axis=-1)[..., :kmax]
        best[..., si, :n] = tops[si][..., :n]
        dead[..., si, :n] = ~ok
    assert (index[dead] == -1).all() and (prob[dead] == 0).all(), f"{what}: an invalid row or a rank beyond the segment is not -1 / 0"
    z = lambda x: np.where(dead, 0.0, x)
    ref_at, cal_at, best = z(ref_at), z(cal_at), z(best)
    r = check_terms(prob, ref_at, cal_at, der_at, what, klass, kind, dead=dead)
    check_index(ref_at, best, rel_part(cal_at, der_at, ref_at, klass), what)
    return r


def oracle_side(q_true, keys, heads, scale, presc=False):
    """for a test that holds its data to reference B: (E (B, H, Lq, Lkv), delta (B, H, Lq, 1)) from the oracle's own LSE"""
    s, T = scores_and_sizes(q_true, keys, heads, scale)
    lse_ref = lse_of(s)
    return elem_scale(T, lse_ref), lse_delta(q_true, keys, scale, lse_ref, presc)[..., None]


# ---- the fp32 emulation of the expression and its planted defects (tests/test_prob_bounds_cpu.py) ----------------------------------
def emulate(q16, keys16, heads, scale, lse32, presc=False, dtype=None, defect=None):
    """csrc/ir_readout.h in plain fp32, float32 (B, H, Lq, Lkv): the 64-term dot product accumulated sequentially over d, scale *
    log2(e) and lse * log2(e) each rounded once, one multiply-add rounded once, ``np.exp2`` in fp32, results below 2^-126 flushed.
    ``q16`` (B, Lq, C): the 16-bit q (or the pre-scaled qs with ``presc``), ``keys16`` (B, Lkv, C), ``lse32`` (B, H, Lq) float32.
    ``defect``: "lse_f16" (the LSE rounded to fp16 before use), "scale_bf16" (scale * log2(e) rounded to bf16), "clamp14" (the
    exponent clamped at -14) or "score16" (the scaled score rounded to ``dtype`` ahead of the exponential)"""
    f32 = np.float32
    q = np.asarray(q16.float().numpy() if isinstance(q16, torch.Tensor) else q16, dtype=f32)
    kk = np.asarray(keys16.float().numpy() if isinstance(keys16, torch.Tensor) else keys16, dtype=f32)
    B, Lq, C = q.shape
    d, lkv = C // heads, kk.shape[1]
    qh = q.reshape(B, Lq, heads, d).transpose(0, 2, 1, 3)                                   # (B, H, Lq, d)
    kh = kk.reshape(B, lkv, heads, d).transpose(0, 2, 1, 3)                                 # (B, H, Lkv, d)
    acc = np.zeros((B, heads, Lq, lkv), dtype=f32)
    for t in range(d):
        acc = acc + qh[..., :, None, t] * kh[..., None, :, t]                              # the product of two 16-bit numbers is exact in fp32
    scale_log2 = f32(1.0) if presc else f32(scale) * f32(LB.LOG2E)
    lse = np.asarray(lse32, dtype=f32)
    if defect == "lse_f16":
        lse = lse.astype(np.float16).astype(f32)
    if defect == "scale_bf16":
        scale_log2 = f32(torch.tensor(float(scale_log2)).to(torch.bfloat16).float().item())
    lse2 = (lse * f32(LB.LOG2E))[..., None]
    if defect == "score16":
        nat = (acc * (f32(LN2) if presc else f32(scale)))
        nat = torch.from_numpy(nat).to(dtype).float().numpy()
        x = ((nat - lse[..., None]).astype(f32) * f32(LB.LOG2E)).astype(f32)
    else:
        x = (acc.astype(np.float64) * np.float64(scale_log2) - lse2.astype(np.float64)).astype(f32)      # one rounding: the fma
    if defect == "clamp14":
        x = np.maximum(x, f32(-14.0))
    with np.errstate(under="ignore"):
        p = np.exp2(x).astype(f32)
    return np.where(p < f32(FLOOR32), f32(0.0), p)


DEFECTS = ("lse_f16", "scale_bf16", "clamp14", "score16")


def case_reference(shape, family, dtype, presc=False):
    """the CPU side of one input set: inputs, q_true, packed keys, float64 scores and sizes, the oracle's LSE"""
    x = LC.inputs(shape, family, dtype)
    qt = LC.q_true(x, presc)
    keys = pack_keys(x.k, x.rk, shape[6])
    s, T = scores_and_sizes(qt, keys, shape[1], LC.SCALE)
    return x, qt, keys, s, T, lse_of(s)
