"""Every work item of the attention grid against the oracle: EVERY (b, h, row) of out, LSE and segment masses.

The forward is cut into (batch entry, head, query block) items of 512, 256 or 128 rows that csrc/ir_attn_plan.h hands out: each XCD
owns ix = ceil(items / 8) consecutive ones, whole rounds of its slots run whole items, the rem items of the last round are cut in k
K/V-range pieces whose fp32 partials the combine kernel merges.  The other oracle comparisons either stay inside one partly filled
round (B <= 4) or sample a few rows of the first and last entry; here the item count is what is large (B * H * ceil(Lq / rows) = 282 /
531 / 666, none a multiple of 8) and the K/V walk is short (16 tiles; 64 in bf16, below), so that the float64 reference of every row costs seconds:

    set  kernels (tuning)                   B, H, Lq      items  ix  full  rem  k  grid   the last XCD's chunk
    A    W128 (16), W64X8 (13)              47, 3, 600      282  36    32    4  2   320   30 items: no remainder item exists
    B    W64X4 (12)                         59, 3, 700      531  67    64    3  2   560   62 items: no remainder item exists
    C    32-row forms (7 10 11 14 18, 0)    37, 3, 650      666  84    64   20  2   832   78 items: 14 of 20 remainder items exist

(pinned by the "grid" rows of tests/test_attn_plan_cpu.py; inputs and reference: tests/item_grid_oracle.py; that the gates below
see a wrong map: tests/test_item_grid_oracle_cpu.py).  The thread's scratch is filled with NaN before every call: a partial that
is read without having been written in THIS call shows, and nothing behind the plan's ws_needed bytes may be written.

Gates: fp32 output within the literal 1e-3 of the oracle (parity_bounds.check_before_rounding, per batch entry); the 16-bit output
equal to that fp32 output rounded, bit for bit, and inside parity_bounds.stated_bound (identity + the 1e-3 gate bound the 16-bit
error by 1e-3 + half an output ulp; the regression bound of parity_bounds.py was calibrated on sampled rows and is not applied to
these 5-million-element tensors); every element of the LSE and of the masses within tests/lse_bounds.py (KAPPA * 2^-23 * the row's
own scale: about 2e-5 and 1e-5 here, where the former gates were 2e-3 * max|lse| and 2e-3); masses also within the other three
bounds of tests/test_gpu_seg_mass.py.

bf16 runs on segments FOUR TIMES as long (64 tiles: self 1536 + 2 x 1280 keys, or 4 x 1024; item grids unchanged, up to 64 / 8 = 8
pieces - k = 8, 8 and 3 on sets A, B and C, also pinned in tests/test_attn_plan_cpu.py); fp16, the workspace-size test and the CPU
file keep the 16 tiles.  At 16 tiles every bf16 kernel, whole items included, was 1.4e-3 ... 2.0e-3 from the oracle in a handful
of rows (fp16: 1.8e-4).  That is the rounding of P to 16 bit ahead of P.V and no defect: for the six worst rows of set A,
P = 2^(s - m) with m the FIRST tile's row max (the frame the kernels keep until a tile outgrows it), rounded to nearest-even bf16,
times V in float64 over the exact row sum reproduces the kernel's 64 errors to 3e-7 (correlation 1.000).  The rows are those where
one key holds 10 ... 16 % of the mass beside |v| of 6: half a bf16 ulp of that one weight (2^-8 relative: in the frame of the
row's true max it would be 1.0 and exact) is the error.  The same model on seeded CPU data of set A gives 2.2e-3 at 16 tiles,
8e-4 at 48 and 64; the tail is heavy (one row of set B reached 2.1e-3 at 64 tiles in the model), so the margin below is thin and
a change of the seeds may need still longer segments - not a wider gate.

Measured maxima over all (b, h, row) on an MI355X (IR_ITEM_GRID_LOG=<file> appends one JSON record per gated call); LSE at most
2.5e-6, masses 1.7e-6 from the oracle and 4.1e-6 from the second pass, |sum of a row's masses - 1| = 0 everywhere; in units of
2^-23 * row scale (tests/lse_bounds.py; "lse_r" / "mass_r" of the record): LSE at most 2.46 (bound 16), masses 1.63 (bound 8):

    fp32 output / 16-bit output      bf16 (64 tiles)                      fp16 (16 tiles)
                                     self+fold          noself+plain      self+fold          noself+plain
    set A  tunings 16 and 13         5.2e-4 / 1.45e-3   6.5e-4 / 1.37e-3  1.75e-4 / 3.6e-4   1.62e-4 / 3.7e-4
    set B  tuning 12                 3.5e-4 / 1.20e-3   5.3e-4 / 1.32e-3  1.63e-4 / 4.0e-4   2.25e-4 / 6.2e-4
    set C  tuning 7                  2.0e-4 / 1.13e-3   3.4e-4 / 1.23e-3  5.5e-5 / 2.7e-4    8.6e-5 / 2.6e-4
    set C  tunings 10 and 14         4.2e-4 / 1.15e-3   7.9e-4 / 1.59e-3  1.13e-4 / 3.3e-4   2.32e-4 / 4.5e-4
    set C  tunings 11, 18 and 0      6.0e-4 / 1.18e-3   7.0e-4 / 1.35e-3  1.67e-4 / 3.0e-4   1.88e-4 / 3.4e-4
    zero-filled references (A: 16, 13; C: 11, 14, 0), with or without valid_refs: 5.7e-4 / 1.47e-3 bf16, 1.75e-4 / 3.6e-4 fp16
    batch-invariant plan C' and A':  2.8e-4 / 1.14e-3 and 4.2e-4 / 1.13e-3 bf16, 1.0e-4 / 2.8e-4 and 1.1e-4 / 3.1e-4 fp16
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import item_grid_oracle as G
from lse_bounds import check_lse, check_mass, pack_keys, row_scale
from parity_bounds import check_before_rounding, stated_bound

pytestmark = pytest.mark.gpu

NAN = float("nan")
# tuning -> (input set, pre-scaled Q, what ir_shared_attn_kernel_name must say)
KERNELS = {
    16: ("A", True, "shared_attn_fwd_w128_kernel<"),
    13: ("A", True, "shared_attn_fwd_w64_kernel<64 rows/wave, 8 waves"),
    12: ("B", False, "shared_attn_fwd_w64_kernel<64 rows/wave, 4 waves"),
    7: ("C", False, "shared_attn_fwd_pipe_kernel<4 waves, exact rescale>"),
    10: ("C", False, "shared_attn_fwd_pipe_kernel<4 waves, lazy max>"),
    11: ("C", True, "shared_attn_fwd_pipe_kernel<4 waves, lazy max, pre-scaled Q"),
    14: ("C", False, "shared_attn_fwd_pipe_kernel<4 waves, lazy max, early QK"),
    18: ("C", True, "shared_attn_fwd_pipe_kernel<4 waves, pre-scaled Q, reference checked after the exponentials"),
    0: ("C", True, "shared_attn_fwd_pipe_kernel<4 waves, lazy max, pre-scaled Q"),     # at Lq = 650 the default dispatch stays on the 32-row kernel
}
# bytes of the partials: (set, segments whose masses a piece stores, K/V tiles) - the "grid" literals of tests/test_attn_plan_cpu.py
WS_NEEDED = {("A", 0, 16): 8650752, ("B", 0, 16): 3244032, ("C", 0, 16): 10813440, ("A", 3, 16): 9043968, ("C", 3, 16): 11304960,
             ("A", 0, 64): 34603008, ("B", 0, 64): 12976128, ("C", 0, 64): 16220160, ("A", 3, 64): 36175872, ("C", 3, 64): 16957440}
DTYPES = [torch.bfloat16, torch.float16]
DTYPE_IDS = ["bf16", "f16"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


_INPUTS = {}


def _long(dtype):
    """bf16 runs on segments four times as long (64 tiles): the module docstring says why"""
    return dtype == torch.bfloat16


def _tiles(dtype):
    return 16 * (G.LONG if _long(dtype) else 1)


def _inputs(ops, name, form, dtype, long=None):
    """(q, qs, k, v, rk, rv, AdaIN affine or None) on the device, once per (set, form, dtype, length)"""
    long = _long(dtype) if long is None else long
    key = (name, form, dtype, long)
    if key not in _INPUTS:
        t = G.set_inputs(name, form, dtype, "cuda", long=long)
        _INPUTS[key] = t + ((ops.adain_stats(t[3], t[5], heads=G.SETS[name][1]) if G.FORMS[form][4] else None),)
    return _INPUTS[key]


def _q_eff(q, qs, presc):
    return qs.float() / G.QC if presc else q.float()


def _log(rec):
    print(json.dumps(rec))
    path = os.environ.get("IR_ITEM_GRID_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


_SCALES = {}


def _row_scales(key, q_eff, k, rk, inc, lse_ref):
    """tests/lse_bounds.py::row_scale of every (b, h, row), once per reference (same key as ``G.cached_reference``)"""
    if key not in _SCALES:
        _SCALES[key] = row_scale(q_eff, pack_keys(k, rk, inc), G.SCALE, lse_ref)
        _SCALES[key].setflags(write=False)
    return _SCALES[key]


def _gates(what, dtype, H, ref, scales, out32, lse32, out16, lse16, mass=None, second=None):
    """every element of the results of one call (fp32 output, then 16-bit output) against ``ref`` = (out, lse, mass); ``scales``:
    the row scales of tests/lse_bounds.py"""
    out_ref, lse_ref, mass_ref = ref
    o32 = out32.cpu().numpy().astype(np.float64)
    assert o32.shape == out_ref.shape and np.isfinite(o32).all(), f"{what}: non-finite fp32 output"
    err = np.abs(o32 - out_ref)
    b, row, c = np.unravel_index(int(err.argmax()), err.shape)
    rec = {"what": what, "out32": float(err.max()), "worst_b_h_row": [int(b), int(c) // 64, int(row)]}
    for e in range(o32.shape[0]):
        check_before_rounding(o32[e], out_ref[e], f"{what}: batch entry {e} (worst of the call: {err.max():.3e} at b, h, row {rec['worst_b_h_row']})")
    assert torch.equal(out16, out32.to(dtype)), f"{what}: the 16-bit output is not the fp32 output rounded"
    o16 = out16.float().cpu().numpy().astype(np.float64)
    rec["out16"] = float(np.abs(o16 - out_ref).max())
    assert rec["out16"] <= stated_bound(dtype, float(np.abs(out_ref).max())), (what, rec)
    assert torch.equal(lse16, lse32), f"{what}: the LSE changes with the output format"
    lse = lse32.cpu().numpy().astype(np.float64)
    assert np.isfinite(lse).all(), f"{what}: non-finite LSE"
    rec["lse"] = float(np.abs(lse - lse_ref).max())
    rec["lse_r"] = check_lse(lse, lse_ref, scales, what)
    if mass is not None:
        m = mass.cpu().numpy().astype(np.float64)
        assert m.shape == mass_ref.shape and np.isfinite(m).all(), f"{what}: masses"
        rec["mass"] = float(np.abs(m - mass_ref).max())
        rec["mass_sum"] = float(np.abs(m.sum(-1) - 1.0).max())
        rec["mass_min"] = float(m.min())
        rec["mass_vs_second_pass"] = float((mass - second).abs().max())
        rec["mass_r"] = check_mass(m, mass_ref, scales, what)
        assert rec["mass_sum"] <= 1e-5, (what, rec)
        assert rec["mass_min"] >= -1e-6, (what, rec)
        assert rec["mass_vs_second_pass"] <= 1e-4, (what, rec)
    _log(rec)
    return rec


def _forced_call(ops, what, tuning, name_part, ws_needed, dtype, H, ref, scales, q, k, v, rk, rv, inc, aff, presc, valid=None, want_mass=False):
    """one kernel, forced, twice (fp32 and 16-bit output) on a NaN-filled scratch, through every gate"""
    kw = dict(heads=H, scale=G.SCALE, include_self=inc, adain=aff, q_prescaled=presc, valid_refs=valid)
    ws = ops._workspace(q.device)
    res = []
    prev = ops.set_attn_variant(tuning)
    try:
        name = ops.shared_attention_kernel_name(q, k, v, rk, rv, return_mass=want_mass, **kw)
        assert name_part in name, (what, name)
        for out_dtype in (torch.float32, dtype):
            ws.fill_(NAN)
            res.append(ops.shared_attention(q, k, v, rk, rv, return_lse=True, return_mass=want_mass, out_dtype=out_dtype, **kw))
            assert bool(torch.isnan(ws[ws_needed // 4:]).all()), f"{what}: the scratch was written behind byte {ws_needed}"
    finally:
        ops.set_attn_variant(prev)
    r32, r16 = res
    mass = second = None
    if want_mass:
        assert torch.equal(r32[2], r16[2]), f"{what}: the masses change with the output format"
        mass = r32[2]
        second = ops.attn_segment_mass(q, k, rk, r32[1], heads=H, scale=G.SCALE, include_self=inc, q_prescaled=presc)
    return _gates(what, dtype, H, ref, scales, r32[0], r32[1], r16[0], r16[1], mass, second), r16


def _id(v):
    return DTYPE_IDS[DTYPES.index(v)] if isinstance(v, torch.dtype) else str(v)


@pytest.mark.parametrize("form", list(G.FORMS), ids=_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("tuning", list(KERNELS), ids=lambda t: f"tuning{t}")
def test_every_row_of_every_item_against_the_oracle(ops, tuning, dtype, form):
    name, presc, name_part = KERNELS[tuning]
    _, H, _, _ = G.SETS[name]
    inc, _, _, _, adain = G.FORMS[form]
    q, qs, k, v, rk, rv, aff = _inputs(ops, name, form, dtype)
    ref = G.cached_reference((name, form, dtype, presc), _q_eff(q, qs, presc), k, v, rk, rv, H, adain, inc)
    scales = _row_scales((name, form, dtype, presc), _q_eff(q, qs, presc), k, rk, inc, ref[1])
    _forced_call(ops, f"set {name} {form} {_id(dtype)} tuning {tuning}", tuning, name_part, WS_NEEDED[(name, 0, _tiles(dtype))], dtype, H, ref,
                 scales, qs if presc else q, k, v, rk, rv, inc, aff, presc)


# (b) tuning -> pre-scaled Q.  IR_TUNE_PIPE32_EARLYQK is a plain-Q form; the default dispatch is run with plain Q as well
FORMS_ON_THE_PLAN = {16: True, 13: True, 11: True, 14: False, 0: False}
_ZEROED = {}


def _zero_filled(ops, name, dtype):
    """self+fold inputs with references n >= valid[b] = b % (N + 1) zero-filled, their AdaIN affine, the counts"""
    key = (name, dtype)
    if key not in _ZEROED:
        q, qs, k, v, rk, rv, _ = _inputs(ops, name, "self+fold", dtype)
        B, N = rk.shape[:2]
        valid = torch.tensor([b % (N + 1) for b in range(B)], dtype=torch.int32, device="cuda")
        rkz, rvz = rk.clone(), rv.clone()
        ops.zero_invalid_refs(rkz, rvz, valid, heads=G.SETS[name][1])
        for b in range(B):
            assert float(rkz[b, int(valid[b]):].abs().sum()) == 0.0 and float(rvz[b, int(valid[b]):].abs().sum()) == 0.0
        _ZEROED[key] = (q, qs, k, v, rkz, rvz, ops.adain_stats(v, rvz, heads=G.SETS[name][1]), valid)
    return _ZEROED[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("tuning", list(FORMS_ON_THE_PLAN), ids=lambda t: f"tuning{t}")
def test_valid_refs_and_segment_masses_on_every_item(ops, tuning, dtype):
    """every count 0 ... N of valid references in the middle of the batch; the oracle on the zero-filled tensors (zeroed, not
    masked); then the same tensors without the counts (the kernels walk the zero tiles): the same bounds, no bit equality
    (tests/test_gpu_valid_refs.py: another fp32 summation order)"""
    name, _, name_part = KERNELS[tuning]
    presc = FORMS_ON_THE_PLAN[tuning]
    if tuning == 0 and not presc:
        name_part = KERNELS[14][2]
    _, H, _, _ = G.SETS[name]
    q, qs, k, v, rkz, rvz, aff, valid = _zero_filled(ops, name, dtype)
    ref = G.cached_reference((name, "self+fold", dtype, presc, "zero-filled"), _q_eff(q, qs, presc), k, v, rkz, rvz, H, True, True)
    scales = _row_scales((name, "self+fold", dtype, presc, "zero-filled"), _q_eff(q, qs, presc), k, rkz, True, ref[1])
    for counts in (valid, None):
        _forced_call(ops, f"set {name} zero-filled {_id(dtype)} tuning {tuning} valid_refs {'given' if counts is not None else 'not given'}",
                     tuning, name_part, WS_NEEDED[(name, 3, _tiles(dtype))], dtype, H, ref, scales, qs if presc else q, k, v, rkz, rvz, True, aff, presc,
                     valid=counts, want_mass=True)


def test_callers_workspace_of_the_exact_size_and_one_byte_short(ops):
    """include/instantrestore_hip.h: "a smaller buffer only limits the split" (cap = bytes / piece bytes / 8 pieces per XCD).
    Set A needs 4 items x 2 pieces x 8 XCDs x 135,168 B = 8,650,752 B: with exactly that the cut stays and nothing behind it is
    written; with one byte less 7 pieces per XCD fit, the remainder items run whole and the buffer is not touched"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    need = WS_NEEDED[("A", 0, 16)]
    _, H, _, _ = G.SETS["A"]
    q, qs, k, v, rk, rv, aff = _inputs(ops, "A", "self+fold", torch.bfloat16, long=False)   # bit comparisons only: the 16-tile form
    kw = dict(heads=H, scale=G.SCALE, include_self=True, adain=aff, q_prescaled=True, return_lse=True)
    prev = ops.set_attn_variant(16)
    try:
        assert KERNELS[16][2] in ops.shared_attention_kernel_name(qs, k, v, rk, rv, heads=H, scale=G.SCALE, adain=aff, q_prescaled=True)
        ops._workspace(qs.device).fill_(NAN)
        cut = ops.shared_attention(qs, k, v, rk, rv, **kw)
        whole = ops.shared_attention(qs, k, v, rk, rv, split=False, **kw)
        assert not torch.equal(cut[0], whole[0]), "the remainder split changes no bit of set A: the cases below would show nothing"
        for nbytes, want in ((need, cut), (need - 1, whole)):
            buf = torch.full((need // 4 + 65536,), NAN, dtype=torch.float32, device="cuda")
            out, lse = torch.empty_like(want[0]), torch.empty_like(want[1])
            a = ops._fill_args(qs, k, v, rk, rv, H, G.SCALE, True, aff, out, lse, True, True, None, False)
            assert a.tuning == 16
            a.workspace, a.workspace_bytes = buf.data_ptr(), nbytes
            _lib.check(lib.ir_shared_attn_fwd(C.byref(a), ops._stream()), "ir_shared_attn_fwd")
            torch.cuda.synchronize()
            assert torch.equal(out, want[0]) and torch.equal(lse, want[1]), f"workspace of {nbytes} bytes"
            written = ~torch.isnan(buf)
            if nbytes == need:
                assert not bool(written[need // 4:].any()), "written behind the workspace's last byte"
                assert bool(written[:need // 4].any())
            else:
                assert not bool(written.any()), "one byte short: the split must be off, the buffer untouched"
    finally:
        ops.set_attn_variant(prev)


# (d) B, H, Lq, kernel (IR_TUNE_*), rows per item, items per entry, what the name says, launches with a workspace for two entries
BI_CASES = {
    "C'": (5, 3, 650, 11, 128, 18, "shared_attn_fwd_pipe_kernel<4 waves, lazy max, pre-scaled Q", 3),
    "A'": (3, 3, 4184, 16, 512, 27, "shared_attn_fwd_w128_kernel<", 2),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("case", list(BI_CASES))
def test_batch_invariant_plan_every_row_and_over_several_launches(ops, case, dtype):
    """batch-invariant mode cuts EVERY item in min(ceil(256 / items per entry), tiles / 8) pieces - 2 of the 16 tiles in fp16, 8 of
    the 64 tiles in bf16; with a workspace for two entries' pieces the library runs the batch as several launches whose bytes are
    those of the one launch"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    B, H, Lq, kernel, rows, items, name_part, launches = BI_CASES[case]
    inc, Ls, N, Lr, _ = G.form_shape("self+fold", _long(dtype))
    pieces = min(-(-256 // items), _tiles(dtype) // 8)
    assert pieces == (8 if _long(dtype) else 2)
    q, qs, k, v, rk, rv = G.make_inputs(B, H, Lq, Ls, N, Lr, dtype, 7700 + Lq + (dtype == torch.float16), "cuda")
    valid = torch.tensor([b % (N + 1) for b in range(B)], dtype=torch.int32, device="cuda")
    ops.zero_invalid_refs(rk, rv, valid, heads=H)
    aff = ops.adain_stats(v, rv, heads=H)
    ref = G.cached_reference(("bi", case, dtype), _q_eff(q, qs, True), k, v, rk, rv, H, True, True)
    scales = _row_scales(("bi", case, dtype), _q_eff(q, qs, True), k, rk, True, ref[1])
    plan_kw = dict(len_self=Ls, n_refs=N, len_ref=Lr, dtype=dtype, adain=True, q_prescaled=True, valid_refs=True, return_mass=True)
    plan = ops.shared_attention_plan(B, Lq, H, **plan_kw)
    assert (plan["kernel"], plan["rows_per_item"], plan["items_per_batch"], plan["pieces_per_item"], plan["batch_per_launch"]) == \
        (kernel, rows, items, pieces, B), plan
    kw = dict(heads=H, scale=G.SCALE, include_self=True, adain=aff, q_prescaled=True, valid_refs=valid, batch_invariant=True)
    name = ops.shared_attention_kernel_name(qs, k, v, rk, rv, return_mass=True, **kw)
    assert name_part in name and f"[batch-invariant: {pieces} pieces per {rows}-row item]" in name, name
    r32 = ops.shared_attention(qs, k, v, rk, rv, return_lse=True, return_mass=True, out_dtype=torch.float32, **kw)
    r16 = ops.shared_attention(qs, k, v, rk, rv, return_lse=True, return_mass=True, **kw)
    assert torch.equal(r32[2], r16[2])
    second = ops.attn_segment_mass(qs, k, rk, r32[1], heads=H, scale=G.SCALE, include_self=True, q_prescaled=True)
    _gates(f"batch-invariant {case} {_id(dtype)}", dtype, H, ref, scales, r32[0], r32[1], r16[0], r16[1], r32[2], second)
    # a workspace that holds two entries' pieces, NaN-filled, with a NaN tail behind it that must stay
    for want in (r32, r16):
        out, lse, mass = (torch.empty_like(t) for t in want)
        a = ops._fill_args(qs, k, v, rk, rv, H, G.SCALE, True, aff, out, lse, True, True, valid, True)
        a.seg_mass = mass.data_ptr()
        a2 = ops._fill_args(qs[:2], k[:2], v[:2], rk[:2], rv[:2], H, G.SCALE, True, aff, out[:2], lse[:2], True, True, valid[:2], True)
        a2.seg_mass = mass.data_ptr()
        need2 = int(lib.ir_shared_attn_workspace_bytes_for(C.byref(a2)))
        assert 0 < need2 < int(lib.ir_shared_attn_workspace_bytes_for(C.byref(a))) == plan["workspace_bytes"]
        assert need2 % 4 == 0
        buf = torch.full((need2 // 4 + 65536,), NAN, dtype=torch.float32, device="cuda")
        a.workspace, a.workspace_bytes = buf.data_ptr(), need2
        info = _lib.SharedAttnPlan()
        info.struct_size = C.sizeof(info)
        _lib.check(lib.ir_shared_attn_plan(C.byref(a), C.byref(info)), "ir_shared_attn_plan")
        assert info.batch_per_launch == 2 and info.pieces_per_item == pieces and -(-B // 2) == launches
        _lib.check(lib.ir_shared_attn_fwd(C.byref(a), ops._stream()), "ir_shared_attn_fwd")
        torch.cuda.synchronize()
        for got, w, what in zip((out, lse, mass), want, ("out", "lse", "mass")):
            assert torch.equal(got, w), f"{case}: {what} of {launches} launches differs from the one launch ({want[0].dtype} output)"
        assert bool(torch.isnan(buf[need2 // 4:]).all()), "written behind the workspace's last byte"
