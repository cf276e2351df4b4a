"""The bound every oracle comparison of the attention LSE and of the by-product segment masses is held to.

The forward kernels return the log-sum-exp as an fp32 by-product and six read-outs multiply it into every number they return, so
it is held to fp32 accuracy, ELEMENT BY ELEMENT, against the float64 oracle on the same 16-bit-rounded inputs:

    |lse - lse_ref| <= KAPPA[klass] * 2^-23 * row_scale                            (check_lse)
    |mass - mass_ref| <= KAPPA_MASS * 2^-23 * row_scale         absolute           (check_mass)

    row_scale = max(1, |lse_ref|, T_row)
    T_row     = max over the keys j that carry weight (p_ref >= p_floor = 2^-30) of  scale * sum_d |q_d k_jd| + |bias_j|

``row_scale`` is the size of the largest quantity that is rounded to fp32 on the way to that row's LSE: the LSE itself, and the
partial sums of the score of a key that counts (an fp32 dot product of 64 terms is off by a few 2^-24 of the sum of the terms'
magnitudes, whatever the score's own size; a key bias is added in fp32 as well).  T_row matters where |lse| is small and where a
bias is large.  Rows whose reference is -inf (every key masked, a ragged entry without keys) must be -inf on the device, and
their masses exactly 0; NaN and a shape mismatch fail.  Device-against-device comparisons are held to the SUM of the two sides'
bounds (each side lies within its own bound of the truth): ``check_lse_pair``.

Classes.  "fp32" is every product kernel that sums the fp32 exponentials: the 32-row kernel in its forms 7, 10, 14, 18, tuning 11
and the default dispatch with IR_FLAG_Q_PRESCALED, the 64-row kernels (12, 13), the 128-row kernel (16) and its forms
instantiation, the BIAS and RAGGED forms, the batch-invariant plan and the piece combine.  IR_TUNE_PIPE32_PRESCALE_Q WITHOUT the
flag rounds Q * scale * log2(e) to 16 bit inside the kernel; its reference is formed from the equally rounded Q,
``(q.float() * QC).to(dtype)`` (``q_rounded_like_tuning_11``), and with that reference its ratios are those of the class (70
comparisons, median 0.51, largest 1.43), so it belongs to "fp32" and no "q_rounded" class exists.  The -DIR_ABLATIONS
development kernels get nothing.

"frame" - a finding of the calibration, and a rounding these forms are documented to make ("the running
reference enters through the MFMA C operand").  The pre-scaled-Q forms (IR_FLAG_Q_PRESCALED: 32-row PRESC / POSTCHECK, 64-row,
128-row) form their scores RELATIVE to the running reference inside the matrix pipe, so a score is rounded at the size of that
reference, not at its own.  On the "first tile far below zero" inputs of tests/lse_cases.py (64 keys scoring about -240 that
carry no weight, then ordinary keys) the reference is -240 when the first keys that count arrive, and a row that one of those
keys carries is off by up to one fp32 step at 350 log2 units: the 128-row kernel 3.08e-5 (fp16) / 1.63e-5 (bf16) at B1 H1 Lq128
Ls128 - 17.8 and 10.9 units of 2^-23 * row_scale against at most 1.4 on every other family; the 64-row kernel 2.6, the pieces of
the batch-invariant plan 6.4 (second seed).  The error is diluted by the share of the row's weight that later tiles hold
(tests/test_gpu_round2.py's far_below_zero at 4096 keys: 1.3).  The kernels are left as they are (the frame is what makes their
loop cheap); tests/test_gpu_lse.py holds every pre-scaled-Q call to class "frame", whose row scale (``row_scale(frame=True)``)
also includes the largest |score| over ALL unmasked keys of the row, weight or not.  On ordinary activations the two scales
coincide (|score| <= sum |q_d k_jd|), and with it the "low" family measures like the others (largest 1.41 over 264 comparisons).
The edited files keep class "fp32" with the plain scale for every kernel, pre-scaled or not: their inputs have no such keys.

How the constants were fixed: measured against the float64 oracle only (IR_LSE_SOFT=1 and IR_PARITY_LOG=<file> on the MI355X,
tests/test_gpu_lse.py and every edited file), largest ratio r = |err| / (2^-23 * row_scale) per class, constant = 4 * r rounded
up to a power of two (a factor 2 for the maximum of a rounding random walk over 10^5 ... 10^6 rows moving between seeds, a
factor 2 for a runtime whose exp2 / log2 differ in the last bit), then tests/test_gpu_lse.py again with two further values of
IR_SWEEP_SEED: no ratio above half the constant.  tests/test_lse_bounds_cpu.py shows that plain fp32 arithmetic stays inside
the bound (largest 2.32 over 180 input sets) and that a lost 32-key tile moves every row and a lost key a third of the rows by
more than 4 bounds, where the old gate, 2e-3 * max(1, max|lse_ref|), accepted the lost key in most of them.

MEASURED on an MI355X (IR_PARITY_LOG records; unit: 2^-23 * row_scale):
    class    comparisons   median   largest   where                                                              constant
    fp32     1319          0.73     2.46      tests/test_gpu_item_grid.py, set C zero-filled bf16, tuning 14      16
                                              (valid_refs not given: 2.51e-6 at scale 11.0; tunings 11, 0: 2.45)
    frame    264           0.63     1.41      128-row kernel, B3 H2 Lq512 N4 Lr256 no self, N(0, 1), bf16         8
    mass     867           0.66     1.74      batch-invariant plan, pre-scaled Q, "low", B4 H2 Lq128 N4 Lr256     8 (KAPPA_MASS)
    pairs    148           1.19     2.86      closed form against the walk (tests/test_gpu_valid_refs.py sweep,   sum of the two
                                              case 11) - not used for a constant: device against device           sides' bounds
    Three-seed check of tests/test_gpu_lse.py (IR_SWEEP_SEED 1 and 2; 764 fp32, 932 frame, 1096 mass comparisons): largest
    1.37 / 1.30 / 1.42 - below half of every constant.

IR_PARITY_LOG=<file> appends one JSON record per comparison (test id, class, r, max error, max scale); IR_LSE_SOFT=1 records
violations of the bound without failing (calibration runs only - no committed file sets it; -inf / NaN / shape still fail).
"""
import json
import os

import numpy as np
import torch

EPS = 2.0 ** -23
KAPPA = {"fp32": 16.0, "frame": 8.0}
KAPPA_MASS = 8.0
P_FLOOR = 2.0 ** -30
LOG2E = 1.4426950408889634


def _to64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().float().cpu().numpy().astype(np.float64) if x.dtype != torch.float64 else x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def bound(scale, klass="fp32"):
    """the LSE bound at a row scale (number or array)"""
    return KAPPA[klass] * EPS * scale


def mass_bound(scale):
    return KAPPA_MASS * EPS * scale


def pack_keys(k_self, ref_k, include_self):
    """(B, Lkv, C) float64: [self] ++ ref 0 ++ ... ++ ref N-1, the key order of the kernels"""
    t = lambda x: x.detach().double() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float64))
    segs = []
    if include_self or ref_k is None:
        segs.append(t(k_self))
    if ref_k is not None:
        r = t(ref_k)
        segs.append(r.reshape(r.shape[0], r.shape[1] * r.shape[2], r.shape[3]))
    return torch.cat(segs, dim=1)


def q_rounded_like_tuning_11(q, dtype, scale=0.125):
    """IR_TUNE_PIPE32_PRESCALE_Q without the flag rounds Q * scale * log2(e) to the 16-bit type inside the kernel: the Q its
    scores are formed from, as float64 (B, Lq, C)"""
    qc = scale * LOG2E
    return _to64((q.float() * qc).to(dtype)) / qc


def row_scale(q_true, keys, scale, lse_ref, bias=None, p_floor=P_FLOOR, frame=False):
    """one scale per (b, h, row), float64 (B, H, Lq): max(1, |lse_ref|, T_row).  q_true (B, Lq, C), keys (B, Lkv, C) packed as
    ``pack_keys`` does, lse_ref (B, H, Lq) (-inf rows get 1), bias (B, Lkv) / (B, H, Lkv) or None: -inf or <= -1e4 masks a key.
    ``frame``: the scale of the class "frame" - also the largest |score| over ALL unmasked keys of the row, weight or not"""
    dev = keys.device if isinstance(keys, torch.Tensor) else torch.device("cpu")     # device tensors are evaluated where they live
    t64 = lambda x: (x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=np.float64))).to(dev, torch.float64)
    q, kk, lse_ref = t64(q_true), t64(keys), t64(lse_ref)
    B, H, Lq = lse_ref.shape
    assert q.shape[:2] == (B, Lq) and kk.shape[0] == B and q.shape[2] == kk.shape[2] and q.shape[2] % H == 0, (q.shape, kk.shape, lse_ref.shape)
    d = q.shape[2] // H
    lkv = kk.shape[1]
    kb = None
    if bias is not None:
        kb = t64(bias)
        if kb.dim() == 2:
            kb = kb[:, None, :].expand(B, H, lkv)
        assert kb.shape == (B, H, lkv), kb.shape
    out = torch.ones((B, H, Lq), dtype=torch.float64, device=dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for b in range(B):
        qb = q[b].reshape(Lq, H, d).permute(1, 0, 2)                    # (H, Lq, d)
        kt = kk[b].reshape(lkv, H, d).permute(1, 2, 0)                  # (H, d, Lkv)
        s = torch.matmul(qb, kt) * scale
        t = torch.matmul(qb.abs(), kt.abs()) * abs(scale)
        if kb is not None:
            live = kb[b] > -1.0e4
            add = torch.where(live, kb[b], zero)[:, None, :]
            s = torch.where(live[:, None, :], s + add, zero - float("inf"))
            t = t + add.abs()
        lr = lse_ref[b][..., None]
        alive = torch.isfinite(lr)
        counts = (s - torch.where(alive, lr, zero) >= float(np.log(p_floor))) & alive
        t_row = torch.where(counts, t, zero).amax(-1) if lkv else zero
        if frame and lkv:
            t_row = torch.maximum(t_row, torch.where(torch.isfinite(s) & alive, s.abs(), zero).amax(-1))
        out[b] = torch.clamp(torch.maximum(t_row, torch.where(alive[..., 0], lse_ref[b].abs(), zero)), min=1.0)
    return out.cpu().numpy()


def _record(kind, what, klass, r, err, scale_max, limit):
    log = os.environ.get("IR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"kind": kind, "what": str(what)[:200], "test": os.environ.get("PYTEST_CURRENT_TEST", "")[:200],
                                "class": klass, "r": r, "err": err, "scale_max": scale_max, "kappa": limit}) + "\n")


def _soft():
    return os.environ.get("IR_LSE_SOFT") == "1"


def _ratio(got, ref, scale_rows, live, limit, what, kind, klass):
    """largest |err| / (2^-23 * scale) over the live elements; asserts it against ``limit`` unless in soft mode"""
    err = np.where(live, np.abs(np.where(live, got, 0.0) - np.where(live, ref, 0.0)), 0.0)
    ratio = err / (EPS * scale_rows)
    r = float(ratio.max()) if ratio.size else 0.0
    _record(kind, what, klass, r, float(err.max()) if err.size else 0.0, float(np.max(scale_rows)) if np.size(scale_rows) else 1.0, limit)
    if not _soft() and r > limit:
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{what}: {kind.split('_')[0]} off by {err[at]:.3e} at {tuple(int(i) for i in at)} = {r:.1f} x 2^-23 x its row scale "
                             f"{np.broadcast_to(scale_rows, ratio.shape)[at]:.3f} (bound {limit:g} x; reference {ref[at]:.6f})")
    return r


def check_lse(lse, lse_ref, scale_rows, what, klass="fp32", kappa=None, kind="lse"):
    """elementwise: -inf exactly where the reference is, no NaN, elsewhere |lse - lse_ref| <= KAPPA[klass] * 2^-23 * scale_rows
    (``kappa`` replaces KAPPA[klass]: the sum of two sides' constants in a device-against-device comparison).  Returns the
    largest ratio |err| / (2^-23 * scale_rows)."""
    got, ref, sc = _to64(lse), _to64(lse_ref), _to64(scale_rows)
    assert got.shape == ref.shape == sc.shape, (what, got.shape, ref.shape, sc.shape)
    assert not np.isnan(got).any(), f"{what}: NaN in the LSE"
    assert not np.isnan(ref).any() and not np.isposinf(ref).any(), f"{what}: the reference LSE is not a number"
    live = np.isfinite(ref)
    assert np.array_equal(np.isneginf(got), ~live), f"{what}: the LSE is -inf exactly on the rows without an unmasked key"
    assert np.isfinite(got[live]).all(), f"{what}: non-finite LSE"
    return _ratio(got, ref, sc, live, KAPPA[klass] if kappa is None else kappa, what, kind, klass)


def check_lse_pair(lse_a, lse_b, scale_rows, what, klass_a="fp32", klass_b="fp32"):
    """two device results of the same rows: within the sum of the two sides' bounds"""
    return check_lse(lse_a, lse_b, scale_rows, what, klass=klass_a, kappa=KAPPA[klass_a] + KAPPA[klass_b], kind="lse_pair")


def check_mass(mass, mass_ref, scale_rows, what):
    """mass, mass_ref (..., S), scale_rows (...): |m - m_ref| <= KAPPA_MASS * 2^-23 * scale_rows, absolute, every element; rows
    without any mass in the reference (lse_ref = -inf) carry exactly 0.  Returns the largest ratio."""
    got, ref, sc = _to64(mass), _to64(mass_ref), _to64(scale_rows)
    assert got.shape == ref.shape and sc.shape == ref.shape[:-1], (what, got.shape, ref.shape, sc.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite masses"
    assert np.isfinite(ref).all(), f"{what}: the reference masses are not finite"
    dead = (ref == 0.0).all(-1)
    assert (got[dead] == 0.0).all(), f"{what}: a row without an unmasked key carries mass"
    return _ratio(got, ref, sc[..., None], np.ones(ref.shape, dtype=bool), KAPPA_MASS, what, "mass", "mass")


def case_delta(q_true, k_self, ref_k, heads, scale, include_self, klass="fp32"):
    """delta = bound(largest row scale of a call): every probability formed with the device's LSE is the true one times
    exp(+-delta), and |exp(delta) - 1| <= 2 delta - what a read-out's bound against the oracle alone adds to its bound against
    float64 with the device's LSE.  Derived, not measured."""
    keys = pack_keys(k_self, ref_k, include_self)
    lse_ref = oracle_lse_and_mass(q_true, keys, heads, scale)
    return float(bound(row_scale(q_true, keys, scale, lse_ref).max(), klass))


def oracle_lse_and_mass(q_true, keys, heads, scale, bias=None, seg_lens=None):
    """float64, entry by entry: lse (B, H, Lq) and, with ``seg_lens``, mass (B, H, Lq, S) of packed keys (B, Lkv, C) - the
    arithmetic of tests/item_grid_oracle.py::lse_and_mass and tests/key_bias_oracle.py, for sites that have no oracle call at hand"""
    q, kk = _to64(q_true), _to64(keys)
    B, Lq, C = q.shape
    d, lkv = C // heads, kk.shape[1]
    kb = None
    if bias is not None:
        kb = _to64(bias)
        kb = np.broadcast_to(kb[:, None, :], (B, heads, lkv)) if kb.ndim == 2 else kb
    lse = np.empty((B, heads, Lq))
    edges = None if seg_lens is None else np.concatenate([[0], np.cumsum(seg_lens)])
    mass = None if seg_lens is None else np.zeros((B, heads, Lq, len(seg_lens)))
    for b in range(B):
        s = np.matmul(q[b].reshape(Lq, heads, d).transpose(1, 0, 2), kk[b].reshape(lkv, heads, d).transpose(1, 2, 0)) * scale
        if kb is not None:
            live = kb[b] > -1.0e4
            s = np.where(live[:, None, :], s + np.where(live, kb[b], 0.0)[:, None, :], -np.inf)
        m = s.max(-1, keepdims=True)
        dead = ~np.isfinite(m)
        e = np.exp(s - np.where(dead, 0.0, m))
        tot = e.sum(-1, keepdims=True)
        with np.errstate(divide="ignore"):
            lse[b] = np.where(dead, -np.inf, m + np.log(np.where(dead, 1.0, tot)))[..., 0]
        if mass is not None:
            p = e / np.where(dead, 1.0, tot)
            for i in range(len(seg_lens)):
                mass[b, :, :, i] = p[..., edges[i]:edges[i + 1]].sum(-1)
    return (lse, mass) if seg_lens is not None else lse
