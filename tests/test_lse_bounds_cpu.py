"""tests/lse_bounds.py without a GPU: what the helper accepts and refuses, that plain fp32 arithmetic stays inside the bound on
every input set of tests/test_gpu_lse.py (the bound is not below what fp32 can do), and what the bound sees that the old gate,
``2e-3 * max(1, max|lse_ref|)``, did not: a row sum that lost its last 32-key tile, or only its last key."""
import json

import numpy as np
import pytest
import torch

import lse_bounds as LB
import lse_cases as LC


# ---- helper semantics ----------------------------------------------------------------------------------------------------------
def _ref():
    ref = np.array([[[1.0, -2.0, 12.0, 120.0]]])
    return ref, np.maximum(1.0, np.abs(ref))


def test_exact_and_within_the_bound_pass_and_return_the_ratio():
    ref, sc = _ref()
    assert LB.check_lse(ref.copy(), ref, sc, "exact") == 0.0
    got = ref + 0.5 * LB.bound(sc)
    r = LB.check_lse(got, ref, sc, "half a bound")
    assert abs(r - 0.5 * LB.KAPPA["fp32"]) <= 1e-6 * LB.KAPPA["fp32"]
    assert LB.check_lse(torch.from_numpy(got).float(), ref, sc, "fp32 tensor") <= LB.KAPPA["fp32"]


def test_the_bound_is_elementwise():
    """one row off by twice ITS bound fails although another row's |lse| is ten times larger"""
    ref, sc = _ref()
    got = ref.copy()
    got[0, 0, 2] += 2.0 * LB.bound(sc[0, 0, 2])
    assert 2.0 * LB.bound(sc[0, 0, 2]) < 0.5 * LB.bound(sc[0, 0, 3])          # a batch-wide scale would let it through
    with pytest.raises(AssertionError, match="lse off by"):
        LB.check_lse(got, ref, sc, "one row")
    got = ref.copy()
    got[0, 0, 3] += 0.9 * LB.bound(sc[0, 0, 3])
    LB.check_lse(got, ref, sc, "the large row inside its own bound")


def test_minus_infinity_nan_and_shape():
    ref, sc = _ref()
    ref[0, 0, 1] = -np.inf
    got = ref.copy()
    LB.check_lse(got, ref, sc, "-inf where the reference is")
    bad = got.copy()
    bad[0, 0, 1] = -1e30
    with pytest.raises(AssertionError, match="-inf exactly"):
        LB.check_lse(bad, ref, sc, "finite where the reference is -inf")
    bad = got.copy()
    bad[0, 0, 0] = -np.inf
    with pytest.raises(AssertionError, match="-inf exactly"):
        LB.check_lse(bad, ref, sc, "-inf where the reference is finite")
    bad = got.copy()
    bad[0, 0, 0] = np.inf
    with pytest.raises(AssertionError):
        LB.check_lse(bad, ref, sc, "+inf")
    bad = got.copy()
    bad[0, 0, 2] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        LB.check_lse(bad, ref, sc, "NaN")
    with pytest.raises(AssertionError):
        LB.check_lse(got[..., :3], ref, sc, "shape")
    with pytest.raises(AssertionError):
        LB.check_lse(got, ref, sc[..., :3], "scale shape")


def test_pair_bound_is_the_sum_of_the_two_sides():
    ref, sc = _ref()
    LB.check_lse_pair(ref + 1.9 * LB.bound(sc), ref, sc, "inside two bounds")
    with pytest.raises(AssertionError):
        LB.check_lse_pair(ref + 2.1 * LB.bound(sc), ref, sc, "outside two bounds")


def test_mass_is_absolute_and_dead_rows_are_exactly_zero():
    ref = np.array([[[[0.25, 0.75, 0.0], [0.0, 0.0, 0.0]]]])
    sc = np.array([[[8.0, 1.0]]])
    LB.check_mass(ref.copy(), ref, sc, "exact")
    got = ref.copy()
    got[0, 0, 0, 2] = 0.9 * LB.mass_bound(8.0)                                 # absolute: the reference there is 0
    LB.check_mass(got, ref, sc, "inside")
    got[0, 0, 0, 2] = 1.1 * LB.mass_bound(8.0)
    with pytest.raises(AssertionError, match="mass off by"):
        LB.check_mass(got, ref, sc, "outside")
    got = ref.copy()
    got[0, 0, 1, 0] = 1e-30
    with pytest.raises(AssertionError, match="carries mass"):
        LB.check_mass(got, ref, sc, "a row without keys")
    got = ref.copy()
    got[0, 0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        LB.check_mass(got, ref, sc, "NaN")
    with pytest.raises(AssertionError):
        LB.check_mass(ref[..., :2], ref, sc, "shape")


def test_log_and_soft_mode(tmp_path, monkeypatch):
    ref, sc = _ref()
    log = tmp_path / "lse.jsonl"
    monkeypatch.setenv("IR_PARITY_LOG", str(log))
    LB.check_lse(ref + 0.25 * LB.bound(sc), ref, sc, "logged")
    monkeypatch.setenv("IR_LSE_SOFT", "1")
    r = LB.check_lse(ref + 3.0 * LB.bound(sc), ref, sc, "soft: recorded, not failed")
    assert r > LB.KAPPA["fp32"]
    bad = ref.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        LB.check_lse(bad, ref, sc, "soft mode does not excuse NaN")
    recs = [json.loads(l) for l in log.read_text().splitlines()]
    assert len(recs) == 2 and recs[0]["class"] == "fp32" and recs[0]["kind"] == "lse"
    assert abs(recs[0]["r"] - 0.25 * LB.KAPPA["fp32"]) <= 1e-6 * LB.KAPPA["fp32"] and recs[0]["scale_max"] == 120.0
    assert recs[1]["r"] > recs[1]["kappa"] and recs[1]["err"] > 0


def test_row_scale_is_the_largest_rounded_quantity_of_the_row():
    """T_row counts only keys that carry weight, includes |bias|, and -inf rows get 1"""
    q = np.zeros((1, 2, 64))
    q[0, 0, :] = 1.0
    q[0, 1, 0] = 1.0
    k = np.zeros((1, 3, 64))
    k[0, 0, :32], k[0, 0, 32:] = 4.0, -4.0          # score 0, but sum |q k| = 256: T = 0.125 * 256 = 32
    k[0, 1, :] = -8.0                               # score -64 on row 0: no weight there (p = e^-65); row 1: score -1, T = 1
    lse = LB.oracle_lse_and_mass(q, k, 1, 0.125)
    sc = LB.row_scale(q, k, 0.125, lse)
    assert sc.shape == (1, 1, 2) and sc[0, 0, 0] == 32.0
    assert sc[0, 0, 1] == max(1.0, abs(lse[0, 0, 1]))
    # class "frame": the largest |score| of the row counts too, also of a key without weight (key 1 scores -64 on row 0)
    assert LB.row_scale(q, k, 0.125, lse, frame=True)[0, 0, 0] == 64.0
    bias = np.array([[0.0, 0.0, 40.0]])
    lse_b = LB.oracle_lse_and_mass(q, k, 1, 0.125, bias=bias)
    assert LB.row_scale(q, k, 0.125, lse_b, bias=bias)[0, 0, 1] == 40.0          # key 2 (score 0 + 40) carries row 1
    dead = np.full((1, 3), -np.inf)
    lse_d = LB.oracle_lse_and_mass(q, k, 1, 0.125, bias=dead)
    assert np.isneginf(lse_d).all() and (LB.row_scale(q, k, 0.125, lse_d, bias=dead) == 1.0).all()


# ---- achievability: plain fp32 arithmetic stays inside the bound ------------------------------------------------------------------
def _emulate_fp32(q, keys, heads, scale, bias):
    """what a kernel does, in plain fp32: an fp32 matmul, the exponent s * scale * log2(e) (+ bias * log2(e)), exp2 against the row
    max, row sums by 32-key tiles accumulated in walk order, log2"""
    q32, k32 = torch.from_numpy(q).float(), torch.as_tensor(keys).float()
    B, Lq, C = q32.shape
    d, n = C // heads, k32.shape[1]
    f32 = np.float32
    out = np.empty((B, heads, Lq), dtype=f32)
    for b in range(B):
        s = torch.matmul(q32[b].reshape(Lq, heads, d).permute(1, 0, 2), k32[b].reshape(n, heads, d).permute(1, 2, 0)).numpy()
        x = s * f32(scale * LC.LOG2E)
        if bias is not None:
            kb = np.broadcast_to(bias[b], (heads, n)) if bias.ndim == 2 else bias[b]
            live = kb > -1.0e4
            x = np.where(live[:, None, :], x + (np.where(live, kb, 0.0).astype(f32) * f32(LC.LOG2E))[:, None, :], f32(-np.inf)).astype(f32)
        m = x.max(-1, keepdims=True)
        dead = ~np.isfinite(m)
        p = np.exp2(x - np.where(dead, f32(0), m)).astype(f32)
        pad = (-n) % 32
        tiles = np.pad(p, ((0, 0), (0, 0), (0, pad))).reshape(heads, Lq, -1, 32).sum(-1, dtype=f32)
        tot = np.cumsum(tiles, axis=-1, dtype=f32)[..., -1]
        with np.errstate(divide="ignore"):
            out[b] = np.where(dead[..., 0], f32(-np.inf), (m[..., 0] + np.log2(np.where(dead[..., 0], f32(1), tot)).astype(f32)) * f32(0.6931471805599453))
    return out


SETS = list(LC.cpu_sets())


def test_plain_fp32_arithmetic_is_inside_the_bound():
    worst = (0.0, None)
    for name, q, keys, H, bias, _ in SETS:
        ref = LB.oracle_lse_and_mass(q, keys, H, LC.SCALE, bias=bias)
        sc = LB.row_scale(q, keys, LC.SCALE, ref, bias=bias)
        r = LB.check_lse(_emulate_fp32(q, keys, H, LC.SCALE, bias), ref, sc, f"fp32 emulation on {name}")
        worst = max(worst, (r, name))
    print(f"fp32 emulation: largest ratio {worst[0]:.2f} x 2^-23 x row scale on {worst[1]} ({len(SETS)} sets)")
    assert worst[0] <= LB.KAPPA["fp32"] / 4, "the constant leaves plain fp32 arithmetic less than the calibration's factor 4"


# ---- discriminating power -----------------------------------------------------------------------------------------------------------
def test_a_lost_tile_and_a_lost_key_are_seen_where_the_old_gate_saw_neither():
    """float64, the N(0, 1) and 1.5-scaled sets (the peaky sets are left out: there a tile can carry no weight at all).  Without
    the walk's last 32-key tile EVERY row moves by more than 4 bounds (Lkv <= 1024); without only the last key at least one third
    of the rows do (Lkv <= 576).  Holds for the reference alone as long as KAPPA["fp32"] <= 64.  The old gate accepted the lost
    key in the median row, and in more than half of the rows, of every set (not in EVERY row: a row whose
    last key happens to hold more than 1 ... 2 % of its mass moves by more than 2e-3 * |lse| - up to 1.6 where that key carries
    the row - and such rows exist in every set of a few hundred keys)."""
    assert LB.KAPPA["fp32"] <= 64 and LB.KAPPA_MASS <= 64
    seen = 0
    for name, q, keys, H, bias, fam in SETS:
        n = keys.shape[1]
        if fam not in LC.GAUSSIAN or n > 1024:
            continue
        ref = LB.oracle_lse_and_mass(q, keys, H, LC.SCALE)
        b4 = 4.0 * LB.bound(LB.row_scale(q, keys, LC.SCALE, ref))
        tile = np.abs(LB.oracle_lse_and_mass(q, keys[:, :n - 32], H, LC.SCALE) - ref)
        assert (tile > b4).all(), f"{name}: a lost tile moves a row by {tile.min():.2e}, 4 bounds are {b4.max():.2e}"
        key = np.abs(LB.oracle_lse_and_mass(q, keys[:, :n - 1], H, LC.SCALE) - ref)
        if n <= 576:
            share = float((key > b4).mean())
            assert share >= 1.0 / 3.0, f"{name}: a lost key is seen in {share:.2f} of the rows"
        old = 2e-3 * max(1.0, float(np.abs(ref).max()))
        accepted = float((key <= old).mean())
        assert np.median(key) <= old and accepted >= 0.5, f"{name}: the old gate accepted the lost key in {accepted:.2f} of the rows"
        seen += 1
    assert seen >= 30
