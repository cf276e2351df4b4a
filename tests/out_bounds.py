"""The bound every oracle comparison of the attention OUTPUT on reference-moving walks is held to - the companion of
tests/lse_bounds.py, which holds the LSE and the by-product masses.

What is held is the fp32 result BEFORE the output rounding (``out_dtype=torch.float32``, IR_FLAG_OUT_F32, which every product
kernel stores), ELEMENT BY ELEMENT per (b, row, h, d), against the float64 oracle on the same 16-bit-rounded inputs and the same
fp32 AdaIN affine (the affine is an input of the attention launch; ``adain_stats`` has tests of its own):

    |O - O_ref| <= u_P * A  +  u_sub * U  +  K_OUT * 2^-23 * row_scale * S            (check_out)

    A[b,i,h,d] = sum_j p_ij * |a_d * v_jd|                  (a = 1 on the self segment and without the fold)
    S[b,i,h,d] = sum_j p_ij * (|a_d * v_jd| + |b_d|)        (b = 0 on the self segment and without the fold)
    U[b,i,h,d] = sum over j with p_ij < 2^-14 max_j p_ij of |a_d * v_jd|,  divided by  l_i = 1 / max_j p_ij      (fp16 only)

First term.  The kernels form O = (sum_j P~_ij v_j) / (sum_j P_ij) with P = exp2(s - reference) in fp32, the row sum taken from
the fp32 P, and P~ = P rounded to the 16-bit type ahead of the P.V matrix product; V is exact in that product, the accumulator is
fp32, and the AdaIN affine of a segment, a_s o acc_s + b_s l_s, is applied in fp32 after the accumulation.  So P~_ij =
P_ij (1 + e_ij) with |e_ij| <= u_P, and the output moves by at most sum_j p_ij |e_ij| |a_d v_jd| <= u_P * A: the coefficient is 1
and nothing else enters at this size - whatever reference the lazy walk happens to use, since a common factor of a row's P
cancels against its row sum.  u_P is the unit roundoff of that conversion for ROUND-TO-NEAREST, 2^-8 for bf16 and 2^-11 for fp16,
read off the kernels: the 32-row and 64-row kernels convert with ``__builtin_convertvector(float -> __bf16 / _Float16)``
(shared_attn_fwd_pipe.hip, shared_attn_fwd_w64.hip, shared_attn_fwd.hip: round to nearest even), the 128-row kernel with
``v_cvt_pk_bf16_f32`` / ``v_cvt_pk_f16_f32`` (csrc/w128/gen.py: nearest even under the default rounding mode, which no kernel
changes).  No form truncates.

The term u_sub * U - fp16 only (u_sub = 2^-25; bf16 has fp32's exponent range, u_sub = 0) - a property of the number format,
given its own term instead of a place in a constant.  P below 2^-14 of the running reference is SUBNORMAL in fp16 and is rounded
at half the subnormal spacing, 2^-25 ABSOLUTE, not at 2^-11 relative.  A row's reference never exceeds its largest score, so in
the reference's frame the row sum is at least l = sum_j exp(s_j - max_j s_j) = 1 / max_j p_ij >= 1, and a reference below the
maximum only makes P larger: the keys that can be subnormal at any time of the walk are among those with p_ij < 2^-14 max_j p_ij,
and each moves the output by at most 2^-25 |a_d v_jd| / l.  The sum is NOT weighted by p, so it is not u_P * A: it shows where one key
carries the row and that key's own value is tiny (A = S ~ 1e-4) while hundreds of weightless keys hold values of ordinary size.
On the MI355X such an element (BIAS form, 479 subnormal P in its row) is off by 1.9e-6 where u_P * A is 5.9e-8 and u_sub * U 2.6e-5: the
rms of 479 independent roundings at 2^-25 is 1.2e-6, and flushing those P to zero would have cost 1.5e-5.  All kernels do this alike: it is
the number format, not a form.
Scaling P up ahead of the fp16 conversion in the kernels would remove it; that is a kernel change with tests of its own.

Third term: everything rounded in fp32.  An exponent that is off by delta moves its probability by |exp(delta) - 1| <= 2 delta,
and the exponents are what tests/lse_bounds.py bounds: delta <= KAPPA * 2^-23 * row_scale (KAPPA 16, class "frame" 8, both
measured there at <= 2.5).  All probabilities of a row moving by 2 delta move the output by at most 2 delta * 2 S (numerator
and row sum).  The fp32 accumulation adds one rounding of the accumulator per 16-key MFMA step and per tile of the walk, one
per move of the reference (accumulator, fold total and row sum are scaled), one per segment for the fold, one per piece for
the merge and the division: with 34 tiles of 64 keys (the longest walk here) about (4 * 34 + 34 + 6 + 2) * 2^-24 * S ~ 90 *
2^-23 * S in the worst case, its square root in the mean.  Starting value: 4 * KAPPA + 90 ~ 154 -> K_OUT = 256 before the
measurement; the measurement below replaces it, per 16-bit type.  The measured constants are 500 to 1000 times smaller, and the
slack is in two factors of this derivation, not in the accumulation count: (1) row_scale is max(|lse|, sum_d |q_d k_jd| scale), 10 ...
70 here, while the fp32 error of an exponent is a few 2^-24 of the score's own partial sums, which cancel to a score of a few units -
and an error common to a row's exponents cancels between numerator and row sum altogether, so delta enters the output through the
DIFFERENCES of the exponent errors only; (2) KAPPA is itself 4x a measured 2.5 of that same overstated unit.  What is left is the
accumulation, ~ sqrt(90) * 2^-24 * |O| in the mean, against a unit of 2^-23 * row_scale * S >= 10 * 2^-23 * |O|: a few hundredths.  A
recalibration that needs K_OUT = 4 would therefore mean exponent errors that no longer cancel within a row (a stale reference applied
to part of a row, a frame change with the wrong factor in the last bits) - 100x what the accumulation can explain - not more roundings.
``row_scale`` is ``lse_bounds.row_scale`` (``frame=True`` for the pre-scaled-Q
forms, as tests/test_gpu_lse.py chooses), extended here by a mask with a query axis for the REGION forms, by the same definition.

The 16-bit launch needs no second bound: tests assert that it equals the fp32 launch rounded to the type, bit for bit.  Rows
without an unmasked key give O == 0 exactly; NaN, Inf and a shape mismatch fail.

How K_OUT was fixed: against the float64 oracle only (IR_OUT_SOFT=1 and IR_PARITY_LOG=<file> on the MI355X), the largest ratio of
what the first two terms leave, r2 = max(0, |err| - u_P * A - u_sub * U) / (2^-23 * row_scale * S), over tests/test_gpu_out_walks.py at three values
of IR_SWEEP_SEED (0, 1, 2); constant = 4 * r2 rounded up to a power of two (a factor 2 for the maximum of a rounding random walk
moving between seeds, a factor 2 for a runtime whose exp2 differs in the last bit - the reasons of tests/lse_bounds.py).  One
constant per 16-bit type, because the two types measure different things.  Never one kernel against another.

Both types: the first terms explain nearly everything.  What they leave (r2 > 0) shows in 136 of 2214 bf16 and 266 of 2214 fp16
comparisons, every one of them on the near-constant style channel of ``lse_cases.styled_values``, where A << S; the fp32 arithmetic of
the kernels is far inside 2^-23 * row_scale * S, because row_scale - sum |q k| - overstates what an exponent of ordinary size loses.

MEASURED on an MI355X (IR_PARITY_LOG records, seeds 0, 1, 2 of tests/test_gpu_out_walks.py, 4428 comparisons; r = |err| / bound with the
constants below, r2 in units of 2^-23 * row_scale * S):
    type   comparisons   r median   r largest   r2 largest   where (r2)                                                        K_OUT
    bf16   2214          0.34       0.974       0.0331       seed 1, 128-row kernel, fold, B3 H2 Lq512 N4 Lr256 no self,       0.25
                                                             at:seg_last, entry 0 row 446 channel 3 (near-constant style)
    fp16   2214          0.35       0.957       0.1144       seed 0, 128-row kernel, fold, valid_refs [1, 3, 0], B3 H2 Lq512   0.5
                                                             N4 Lr256 no self, at:tile_last, entry 0 row 457 channel 67
                                                             (near-constant style); seeds 1, 2: 0.048, 0.044
    r largest (bf16): 32-row kernel, tuning 18, B2 H2 Lq72 N3 Lr40 no self, "peaky", entry 1 row 66 channel 120 - the first term,
    whose coefficient 1 is derived, not calibrated: one key carries the row and its P rounds by nearly 2^-8 (the fp32 emulation
    of tests/test_out_bounds_cpu.py reaches 0.96, and 0.94 of fp16's bound).
    r largest (fp16): 64-row kernel, 4 waves (tuning 12), plain Q, fold, B1 H1 Lq576 N3 Lr192 no self, "peaky", entry 0 row 47
    channel 45: the first term again (r2 there 0.03); fp16 P rounds by nearly 2^-11 where one key carries the row.
    No r2 above half its constant in any seed: the calibrated term is what "no ratio above half the bound" can be asked of - the
    derived first term is met to 0.97 by correct rounding to nearest.
    The two older tests that also hold their fp32 outputs to check_out (test_gpu_round2.py::test_reference_checked_after_the_exponentials, test_gpu_parity.py::
    test_massive_activation_channels; 44 comparisons): bf16 r <= 0.972, r2 <= 0.004; fp16 r <= 0.82, r2 = 0 throughout.

IR_PARITY_LOG=<file> appends one JSON record per comparison (test id, r, r2, max error, where); IR_OUT_SOFT=1 records violations
of the bound without failing (calibration runs only - no committed file sets it; NaN / Inf / shape / dead rows still fail).
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

import lse_bounds as LB

EPS = 2.0 ** -23
K_OUT = {torch.bfloat16: 0.25, torch.float16: 0.5}             # measured, see the table above; the derived starting value was 256
U_P = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U_SUB = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}       # half the spacing of the type's subnormals that P can reach (bf16: none)
SUB_BELOW = 2.0 ** -14                                          # fp16's smallest normal number
MASKED = -1.0e4


def _to64(x):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)


def counts_bias(counts, seg_lens, n_refs):
    """(B, Lkv) float64: -inf on every key t >= clamp(counts[b][n], 0, Lr) of every reference - token counts as a key mask"""
    counts = np.asarray(counts)
    B = counts.shape[0]
    edges = np.concatenate([[0], np.cumsum(seg_lens)])
    first = len(seg_lens) - n_refs
    bias = np.zeros((B, int(edges[-1])))
    for b in range(B):
        for n in range(n_refs):
            lo, hi = int(edges[first + n]), int(edges[first + n + 1])
            bias[b, lo + min(max(int(counts[b][n]), 0), hi - lo):hi] = -np.inf
    return bias


def oracle_out_and_scales(q_true, keys, values, heads, scale, seg_lens, affine=None, bias=None, counts=None, allowed=None):
    """float64, entry by entry, for packed keys and values (B, Lkv, C) in the kernels' key order ([self] ++ ref 0 ++ ... ++ ref N-1,
    ``lse_bounds.pack_keys``) and ``seg_lens``, the segment lengths in that order.

    ``affine``: (a, b), each (B, N, C) or (B, N, H, 64) - the per-segment AdaIN affine of the N LAST segments (the references; a
    self segment in front keeps a = 1, b = 0), taken as given.  At most one of: ``bias`` (B, Lkv) / (B, H, Lkv), added to the
    scaled scores, -inf or <= -1e4 masks a key; ``counts`` (B, N) token counts of the references (keys behind a count do not
    exist); ``allowed`` bool (B, 1, Lq, Lkv), a region rule as ``region_oracle.allowed_np`` returns it.

    Returns a namespace: ``out`` = O_ref, ``A``, ``S``, ``U`` (B, Lq, C) - U = sum over the unmasked keys j with p_ij < 2^-14 max_j p_ij
    of |a_d v_jd|, divided by l = 1 / max_j p_ij, the third term's sum; ``lse`` (B, H, Lq), -inf on rows without an unmasked key;
    ``scale`` and ``scale_frame`` (B, H, Lq), the row scales of tests/lse_bounds.py's classes "fp32" and "frame"."""
    q, kk, vv = _to64(q_true), _to64(keys), _to64(values)
    B, Lq, C = q.shape
    d, lkv = C // heads, kk.shape[1]
    assert sum(seg_lens) == lkv and vv.shape == kk.shape and C == heads * d, (seg_lens, kk.shape, vv.shape)
    assert (bias is not None) + (counts is not None) + (allowed is not None) <= 1, "one of a key bias, token counts, a region rule"
    a_full, b_full = np.ones((B, lkv, C)), np.zeros((B, lkv, C))
    n_refs = 0
    if affine is not None:
        a, b = (_to64(t) for t in affine)
        n_refs = a.shape[1]
        a, b = a.reshape(B, n_refs, C), b.reshape(B, n_refs, C)
        edges = np.concatenate([[0], np.cumsum(seg_lens)])
        first = len(seg_lens) - n_refs
        assert first in (0, 1), (seg_lens, a.shape)
        for n in range(n_refs):
            a_full[:, edges[first + n]:edges[first + n + 1]] = a[:, n, None, :]
            b_full[:, edges[first + n]:edges[first + n + 1]] = b[:, n, None, :]
    if counts is not None:
        nr = np.asarray(counts).shape[1]
        bias = counts_bias(counts, seg_lens, nr)
    kb = None
    if bias is not None:
        kb = _to64(bias)
        kb = np.broadcast_to(kb[:, None, :], (B, heads, lkv)) if kb.ndim == 2 else kb
        assert kb.shape == (B, heads, lkv), kb.shape
    if allowed is not None:
        allowed = np.asarray(allowed, dtype=bool)
        assert allowed.shape == (B, 1, Lq, lkv), allowed.shape
    res = SimpleNamespace(out=np.zeros((B, Lq, C)), A=np.zeros((B, Lq, C)), S=np.zeros((B, Lq, C)), U=np.zeros((B, Lq, C)), lse=np.empty((B, heads, Lq)),
                          scale=np.ones((B, heads, Lq)), scale_frame=np.ones((B, heads, Lq)))
    for b in range(B):
        qh = q[b].reshape(Lq, heads, d).transpose(1, 0, 2)                       # (H, Lq, d)
        kh = kk[b].reshape(lkv, heads, d).transpose(1, 2, 0)                     # (H, d, Lkv)
        s = np.matmul(qh, kh) * scale
        t = np.matmul(np.abs(qh), np.abs(kh)) * abs(scale)
        live = np.ones((heads, Lq, lkv), dtype=bool)
        if kb is not None:
            ok = kb[b] > MASKED
            add = np.where(ok, kb[b], 0.0)[:, None, :]
            s, t = s + add, t + np.abs(add)
            live = np.broadcast_to(ok[:, None, :], s.shape)
        if allowed is not None:
            live = np.broadcast_to(allowed[b], s.shape)
        s = np.where(live, s, -np.inf)
        m = s.max(-1, keepdims=True)
        dead = ~np.isfinite(m)
        e = np.exp(s - np.where(dead, 0.0, m))
        tot = e.sum(-1, keepdims=True)
        p = e / np.where(dead, 1.0, tot)                                         # (H, Lq, Lkv); dead rows: all 0
        with np.errstate(divide="ignore"):
            lse = np.where(dead, -np.inf, m + np.log(np.where(dead, 1.0, tot)))
        res.lse[b] = lse[..., 0]
        av = (a_full[b] * vv[b]).reshape(lkv, heads, d).transpose(1, 0, 2)       # (H, Lkv, d)
        bb = b_full[b].reshape(lkv, heads, d).transpose(1, 0, 2)
        mh = lambda x: np.matmul(p, x).transpose(1, 0, 2).reshape(Lq, C)
        res.out[b], res.A[b] = mh(av + bb), mh(np.abs(av))
        res.S[b] = res.A[b] + mh(np.abs(bb))
        pmax = p.max(-1, keepdims=True)                                          # = 1 / l, l the row sum in the frame of the row max
        sub = np.where(live & (p < SUB_BELOW * pmax), pmax, 0.0)                 # (H, Lq, Lkv): 1 / l on the keys whose P is subnormal
        res.U[b] = np.matmul(sub, np.abs(av)).transpose(1, 0, 2).reshape(Lq, C)
        counts_ = live & ~dead & (s - np.where(dead, 0.0, lse) >= float(np.log(LB.P_FLOOR)))
        t_row = np.where(counts_, t, 0.0).max(-1) if lkv else np.zeros((heads, Lq))
        big = np.where(live & ~dead, np.abs(np.where(live, s, 0.0)), 0.0).max(-1) if lkv else np.zeros((heads, Lq))
        base = np.maximum(1.0, np.where(dead[..., 0], 0.0, np.abs(np.where(dead, 0.0, lse))[..., 0]))
        res.scale[b] = np.maximum(base, t_row)
        res.scale_frame[b] = np.maximum(res.scale[b], big)
    return res


def out_bound(dtype, A, S, scale_rows, heads, U=None):
    """the element-wise bound (B, Lq, C) from A, S, U (B, Lq, C) and the row scales (B, H, Lq)"""
    B, Lq, C = A.shape
    sc = np.repeat(np.asarray(scale_rows).transpose(0, 2, 1), C // heads, axis=2)          # (B, Lq, C)
    first = U_P[dtype] * A + (U_SUB[dtype] * U if U_SUB[dtype] else 0.0)
    return first + K_OUT[dtype] * EPS * sc * S, sc, first


def _soft():
    return os.environ.get("IR_OUT_SOFT") == "1"


def check_out(out, ref, dtype, what, frame=False, enforce=True):
    """``out`` (B, Lq, C): the fp32 result before the output rounding; ``ref``: what ``oracle_out_and_scales`` returned.
    Element-wise |out - ref.out| <= u_P * A + u_sub * U + K_OUT * 2^-23 * row_scale * S, exact zeros on the rows without an unmasked key,
    nothing non-finite.  Returns the largest ratio |err| / bound (``enforce=False``: returns it also where it is above 1 -
    for the tests that plant a defect and want the figure)."""
    got = _to64(out)
    assert got.shape == ref.out.shape, (what, got.shape, ref.out.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    B, Lq, C = got.shape
    heads = ref.lse.shape[1]
    dead = np.repeat(np.isneginf(ref.lse).transpose(0, 2, 1), C // heads, axis=2)
    assert (got[dead] == 0.0).all(), f"{what}: a row without an unmasked key is not exactly 0"
    bnd, sc, first = out_bound(dtype, ref.A, ref.S, ref.scale_frame if frame else ref.scale, heads, ref.U)
    err = np.abs(got - ref.out)
    tiny = np.finfo(np.float64).tiny
    ratio = np.where(dead, 0.0, err / np.maximum(bnd, tiny))
    ratio = np.where((bnd == 0.0) & (err == 0.0), 0.0, ratio)
    r = float(ratio.max()) if ratio.size else 0.0
    r2 = np.where(dead, 0.0, np.maximum(0.0, err - first) / np.maximum(EPS * sc * ref.S, tiny))
    r2 = np.where(err == 0.0, 0.0, r2)
    at = np.unravel_index(int(ratio.argmax()), ratio.shape) if ratio.size else (0, 0, 0)
    at2 = np.unravel_index(int(r2.argmax()), r2.shape) if r2.size else (0, 0, 0)
    log = os.environ.get("IR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"kind": "out", "what": str(what)[:200], "test": os.environ.get("PYTEST_CURRENT_TEST", "")[:200],
                                "class": "frame" if frame else "fp32", "dtype": str(dtype), "r": r, "r2": float(r2.max()) if r2.size else 0.0,
                                "err": float(err.max()) if err.size else 0.0, "at": [int(i) for i in at], "at2": [int(i) for i in at2],
                                "k_out": K_OUT[dtype]}) + "\n")
    if enforce and not _soft() and r > 1.0:
        raise AssertionError(f"{what}: out off by {err[at]:.3e} at (b, row, c) = {tuple(int(i) for i in at)} = {r:.2f} bounds "
                             f"(u_P A {U_P[dtype] * ref.A[at]:.3e}, u_sub U {U_SUB[dtype] * ref.U[at]:.3e}, fp32 term {K_OUT[dtype] * EPS * sc[at] * ref.S[at]:.3e}; reference {ref.out[at]:.6f})")
    return r
