"""Every kernel on tensors and strides whose offsets do not fit 32 bits.

All tensors of a call whose strides the ABI leaves to the caller are views of ONE allocation of 8.5 GiB (``far_placement.place``
chooses their bases under the rule stated there and proved for every layout of this module by tests/test_far_placement_cpu.py:
a truncated offset stays inside the allocation and off every tensor of the call).  The allocation is filled with 0x7FC0 - NaN in
fp16 and in bf16 - before each case, so a kernel that drops a 64-bit term reads NaN or writes where the scan finds it:

* the bytes equal those of the same call on compact copies (and the forward reports the same kernel for both),
* the result is finite and the inputs are untouched,
* every other 16-bit word of the allocation still holds the fill pattern,
* once per entry point the compact result meets the float64 oracle at the bound the suite already uses for it.

``LAYOUTS`` lists every layout without touching the GPU; the tests below run exactly those.  Tensors whose layout the ABI fixes as
contiguous (lse, seg_mass, the affine, row_index, valid_refs, probabilities) are ordinary tensors here; the last two tests make
them large instead."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import far_placement as FP
from test_gpu_ref_table import FAMILIES, LOG2E, SCALE

pytestmark = pytest.mark.gpu

ALLOC_BYTES = 17 << 29                       # 8.5 GiB
FILL = FP.FILL16
D = 1 << 23                                  # what a far stride adds to its power of two: more than any entry here spans
FAR = {"A": (1 << 32) + D,                   # two entries, base near 0: every unsigned truncation, signed ones that wrap positive
       "B": (1 << 31) + D,                   # two entries, base near 2^31 elements: the signed truncations go negative
       "C": (1 << 30) + D}                   # three entries: 2 * stride crosses 2^32 bytes and 2^31 elements
FAR_F32 = (1 << 30) + D                      # fp32 elements: crosses 2^32 bytes
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
LIMIT = 2 ** 31 - 1                          # IR_ATTN_SEG_BYTES_MAX


def far(count, kind):
    return FAR[kind] if count == 2 else FAR["C"]


def seg_stride_max(length):
    """the largest K/V row stride (elements) the forward takes at this segment length (include/instantrestore_hip.h)"""
    return (LIMIT - 128) // (64 * ((length + 63) // 64) * 2) // 8 * 8


def past_4gib_stride(length, cols):
    """a row stride that carries (length - 1) * stride * 2 past 2^32 bytes, by more than the ``cols`` elements in use of a row"""
    return -(-((1 << 31) + (1 << 16) + cols) // (length - 1) // 8) * 8


# ---------------------------------------------------------------------------------------------------------------------------
# layouts: (name, shape, strides[, element size][, (pinned to, element offset)]) lists, no GPU involved
# ---------------------------------------------------------------------------------------------------------------------------
GROUPS = ("batch", "ref_batch", "ref_n", "all")


def attn_layout(shape, group, kind, out_size=2, with_v=True, with_out=True):
    """q, K/V self, K/V references and out of one attention call; ``group`` says which strides are far"""
    B, H, Lq, N, Lr = shape
    Cc = H * 64
    tok = lambda L, sb: ((B, L, Cc), (sb, Cc, 1))
    sb_tok = far(B, kind) if group in ("batch", "all") else None
    if group == "all":
        sb_ref, sn_ref = (1 << 30) + 4 * D, (1 << 29) + D
    else:
        sn_ref = far(N, kind) if group == "ref_n" else Lr * Cc
        sb_ref = far(B, kind) if group == "ref_batch" else (Lr * Cc + 64 if group == "ref_n" else N * Lr * Cc)
    ref = ((B, N, Lr, Cc), (sb_ref, sn_ref, Cc, 1))
    out = [("q",) + tok(Lq, sb_tok or Lq * Cc), ("ks",) + tok(Lq, sb_tok or Lq * Cc)]
    if with_v:
        out.append(("vs",) + tok(Lq, sb_tok or Lq * Cc))
    out.append(("kr",) + ref)
    if with_v:
        out.append(("vr",) + ref)
    if with_out:
        sb_out = (FAR_F32 if out_size == 4 else sb_tok) if sb_tok else Lq * Cc
        out.append(("out",) + tok(Lq, sb_out) + (out_size,))
    return out


def wide_rows_layout(shape, which, stride, with_v=True, with_out=True):
    """K and V (or K alone) as column ranges of the same wide rows: ``which`` = "self" or "ref" has row stride ``stride``"""
    B, H, Lq, N, Lr = shape
    Cc = H * 64
    step = 2 * Cc if with_v else Cc
    out = [("q", (B, Lq, Cc), (Lq * Cc, Cc, 1))]
    if which == "self":
        out.append(("ks", (B, Lq, Cc), (step, stride, 1)))
        if with_v:
            out.append(("vs", (B, Lq, Cc), (step, stride, 1), ("ks", Cc)))
        out.append(("kr", (B, N, Lr, Cc), (N * Lr * Cc, Lr * Cc, Cc, 1)))
        if with_v:
            out.append(("vr", (B, N, Lr, Cc), (N * Lr * Cc, Lr * Cc, Cc, 1)))
    else:
        out.append(("ks", (B, Lq, Cc), (Lq * Cc, Cc, 1)))
        if with_v:
            out.append(("vs", (B, Lq, Cc), (Lq * Cc, Cc, 1)))
        out.append(("kr", (B, N, Lr, Cc), (N * step, step, stride, 1)))
        if with_v:
            out.append(("vr", (B, N, Lr, Cc), (N * step, step, stride, 1), ("kr", Cc)))
    if with_out:
        out.append(("out", (B, Lq, Cc), (Lq * Cc, Cc, 1)))
    return out


FWD_FORMS = [(f[0] + ("" if not (v or m) else "_valid" if v else "_mass"), f[1], f[2], f[3], v, m) for f in FAMILIES for v, m in f[4]]
FWD_VARIANTS = ("fold", "out_f32", "batch_invariant", "no_split", "refs_only")
# the batch-invariant plan chooses its own kernel: the early-QK row would repeat the default row
VARIANT_CASES = [(f, v) for f in FWD_FORMS for v in FWD_VARIANTS if not (v == "batch_invariant" and f[0] == "pipe32_earlyqk")]
LONG_FWD = [f for f in FWD_FORMS if f[0] in ("pipe32_default", "w64x8", "w128")]
READOUT_SHAPE = (2, 2, 200, 3, 72)
READOUTS = ("probs_generic", "probs_lines64", "segment_mass", "rows_none", "rows_head_mean", "rows_map")
ADAIN_OPS = ("adain_stats", "adain_stats_cached", "token_stats", "adain_apply", "zero_invalid_refs")
ADAIN_SHAPE = (2, 2, 300, 3, 300)            # B, H, Ls, N, Lr: two 256-row chunks, the second ragged
# (op, which strides are far, placement); ir_adain_stats_cached reads no reference tensor
ADAIN_CASES = [(op, m, k) for op in ADAIN_OPS for m, k in (("batch", "A"), ("batch", "B"), ("ref", "C"), ("rows", "-"))
               if not (op == "adain_stats_cached" and m == "ref")]
LIN_LD = 4194296                             # the largest leading dimension c_abi.hip takes: 256 * ld * 2 < 2^31
LIN_CASES = [("skinny_k320", 1, 96, 320), ("ksplit_k640", 1, 96, 640)] + \
            [(t, i + 2, 256, 128) for i, t in enumerate(["256x128", "128x128", "128x64", "256x64", "64x128", "128x256", "256x256", "128x128k2"])]
LIN_M = {False: 520, True: 264}              # x in 16 bit / in fp32: the last rows lie beyond 4 GiB from the base
LIN_M_STATS = 576                            # whole 64-row statistics blocks
# At the largest leading dimension 8.5 GiB hold 520 rows: every row block starts below 2^32 bytes and only rows do cross it.  A
# quarter of that leading dimension and four times the rows put the START of the last 256-row block past 2^32 bytes as well
# (2048 rows of 2 101 248 bytes; 2^32 falls 16 KiB short of row 2044, so a wrapped block lands between two rows); ragged M.
LIN_MID_LD = 1050624
LIN_MID_M = {False: 2300, True: 1150}


def adain_layout(op, mode, kind):
    B, H, Ls, N, Lr = ADAIN_SHAPE
    Cc = H * 64
    if mode == "rows":                        # every matrix a column range of the same 300 wide rows
        cols = (B + 2 * B * N) * Cc
        W = past_4gib_stride(Ls, cols)
        vs = ("vs", (B, Ls, Cc), (Cc, W, 1))
        x = lambda name, col, pin: (name, (B, N, Lr, Cc), (N * Cc, Cc, W, 1)) + (((pin, col),) if pin else ())
        return {"adain_stats": [vs, x("vr", B * Cc, "vs")], "adain_stats_cached": [vs], "token_stats": [x("x", 0, None)],
                "adain_apply": [x("x", 0, None), x("y", B * N * Cc, "x")], "zero_invalid_refs": [x("k", 0, None), x("v", B * N * Cc, "k")]}[op]
    if mode == "batch":
        sb, sn = far(B, kind), Lr * Cc
    else:
        sb, sn = Lr * Cc + 64, far(N, kind)
    vs = ("vs", (B, Ls, Cc), (far(B, kind) if mode == "batch" else Ls * Cc, Cc, 1))
    x = lambda name: (name, (B, N, Lr, Cc), (sb, sn, Cc, 1))
    return {"adain_stats": [vs, x("vr")], "adain_stats_cached": [vs], "token_stats": [x("x")], "adain_apply": [x("x"), x("y")],
            "zero_invalid_refs": [x("k"), x("v")]}[op]


def linear_layout(n, k, x_f32, m, y_in_x_rows=False, ld=LIN_LD):
    """``y_in_x_rows``: y's rows start 4096 bytes into x's, with the same distance in bytes from row to row (one footprint: there
    is no room for two of 4.8 GB behind the 2^32 bytes that the signed truncations need in front)"""
    if not y_in_x_rows:
        return [("x", (m, k), (ld, 1), 4 if x_f32 else 2), ("y", (m, n), (ld, 1))]
    return [("x", (m, k), (ld, 1), 4 if x_f32 else 2), ("y", (m, n), (2 * ld if x_f32 else ld, 1), ("x", 2048))]


def _layouts():
    out = {}
    for (name, _, shape, _, _, _), group, kind in itertools.product(FWD_FORMS, GROUPS, "AB"):
        out[f"fwd/{name}/{group}/{kind}"] = attn_layout(shape, group, kind)
    for (name, _, shape, _, _, _), var in VARIANT_CASES:
        out[f"fwd_variant/{name}/{var}"] = attn_layout(shape, "all", "B", out_size=4 if var == "out_f32" else 2)
    for (name, _, shape, _, _, _), which in itertools.product(LONG_FWD, ("self", "ref")):
        B, H, Lq, N, Lr = shape
        out[f"fwd_long/{name}/{which}"] = wide_rows_layout(shape, which, seg_stride_max(Lq if which == "self" else Lr))
    for group, kind in itertools.product(GROUPS, "AB"):
        out[f"readout/{group}/{kind}"] = attn_layout(READOUT_SHAPE, group, kind, with_v=False, with_out=False)
    B, H, Lq, N, Lr = READOUT_SHAPE
    for which in ("self", "ref"):
        out[f"readout_long/{which}"] = wide_rows_layout(READOUT_SHAPE, which, past_4gib_stride(Lq if which == "self" else Lr, (1 + B * N) * H * 64),
                                                        with_v=False, with_out=False)
    for op, mode, kind in ADAIN_CASES:
        out[f"adain/{op}/{mode}/{kind}"] = adain_layout(op, mode, kind)
    for (name, _, n, k), x_f32 in itertools.product(LIN_CASES, (False, True)):
        out[f"linear/{name}/{'f32' if x_f32 else '16'}"] = linear_layout(n, k, x_f32, LIN_M[x_f32])
        out[f"linear_mid/{name}/{'f32' if x_f32 else '16'}"] = linear_layout(n, k, x_f32, LIN_MID_M[x_f32], y_in_x_rows=True, ld=LIN_MID_LD)
    out["linear/stats"] = linear_layout(256, 128, False, LIN_M_STATS, y_in_x_rows=True)
    for kind in "AB":
        out[f"tensor2im/{kind}"] = [("x", (2, 3, 20, 24), (FAR[kind], 20 * 32 + 64, 32, 1))]
        out[f"freeu/{kind}"] = [("x", (2, 256), (FAR[kind], 1)), ("out", (2, 256), (FAR[kind], 1))]
    out["tensor2im/f32"] = [("x", (2, 3, 20, 24), (FAR_F32, 20 * 32 + 64, 32, 1), 4)]
    out["freeu/C"] = [("x", (3, 256), (FAR["C"], 1)), ("out", (3, 256), (FAR["C"], 1))]
    return out


LAYOUTS = _layouts()


# ---------------------------------------------------------------------------------------------------------------------------
# the allocation
# ---------------------------------------------------------------------------------------------------------------------------
class Arena:
    def __init__(self):
        self.buf = torch.empty(ALLOC_BYTES // 2, dtype=torch.int16, device="cuda")

    def fill(self):
        self.buf.fill_(FILL)

    def view(self, p, dtype):
        assert torch.empty(0, dtype=dtype).element_size() == p.elem_size
        return torch.as_strided(self.buf.view(dtype), p.shape, p.strides, p.base)

    def words(self, p):
        """the 16-bit words of a placed tensor"""
        k = p.elem_size // 2
        return torch.as_strided(self.buf, p.shape[:-1] + (p.shape[-1] * k,), tuple(s * k for s in p.strides[:-1]) + (1,), p.base * k)

    def dirty(self):
        """words that do not hold the fill pattern, counted on the device in slices"""
        n = torch.zeros((), dtype=torch.int64, device="cuda")
        step = 1 << 28
        for i in range(0, self.buf.numel(), step):
            n += torch.count_nonzero(self.buf[i:i + step] != FILL)
        return int(n)


_ARENA = []
_PEAK = [0]


def _release_arena():
    _ARENA.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    torch.cuda.reset_peak_memory_stats()
    yield _ops
    _release_arena()
    print(f"\nfar addresses: peak device memory of the module {max(_PEAK[0], torch.cuda.max_memory_allocated()) / 2 ** 30:.2f} GiB")


@pytest.fixture
def arena(ops):
    if not _ARENA:
        _ARENA.append(Arena())
    _ARENA[0].fill()
    return _ARENA[0]


def _put(arena, key, data):
    """place the layout ``key`` and write the compact tensors ``data`` into their far slots: {name: far view}"""
    placed = FP.place(ALLOC_BYTES, 2, LAYOUTS[key])
    views = {}
    for name, p in placed.items():
        if name in data:
            views[name] = arena.view(p, data[name].dtype)
            views[name].copy_(data[name])
    return placed, views


def _settle(arena, placed, data, results, what):
    """the checks every case ends with.  ``data``: compact inputs by name; ``results``: {name: (far view, compact result)} for the
    outputs that live in the allocation"""
    torch.cuda.synchronize()
    for name, (got, want) in results.items():
        assert bool(torch.isfinite(want.float()).all()), f"{what}: the compact call's {name} is not finite"
        assert bool(torch.isfinite(got.float()).all()), f"{what}: {name} is not finite"
        assert torch.equal(got, want), (f"{what}: {name} differs from the compact call, "
                                        f"max |diff| {float((got.float() - want.float()).abs().max()):.3e}")
    for name, p in placed.items():
        if name in data and name not in results:
            assert torch.equal(arena.view(p, data[name].dtype), data[name]), f"{what}: input {name} was written to"
    for p in placed.values():
        arena.words(p).fill_(FILL)
    n = arena.dirty()
    assert n == 0, f"{what}: {n} words outside the call's tensors lost the fill pattern"


def _same_small(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None and b is None:
            continue
        assert bool(torch.isfinite(a.float()).all()), f"{what}: result {i} is not finite"
        assert torch.equal(a, b), f"{what}: result {i} differs from the compact call, max |diff| {float((a.float() - b.float()).abs().max()):.3e}"


_ORACLE_DONE = set()


def _once(key):
    if key in _ORACLE_DONE:
        return False
    _ORACLE_DONE.add(key)
    return True


def _np64(t):
    return t.float().cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# the attention forward
# ---------------------------------------------------------------------------------------------------------------------------
def _attn_data(shape, dtype, presc, seed, zero_last_ref=False):
    B, H, Lq, N, Lr = shape
    Cc = H * 64
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Lq, Cc, generator=g) * (SCALE * LOG2E if presc else 1.0)
    d = {"q": q, "ks": torch.randn(B, Lq, Cc, generator=g), "vs": torch.randn(B, Lq, Cc, generator=g) * 0.9 + 0.2,
         "kr": torch.randn(B, N, Lr, Cc, generator=g) * 1.3 - 0.2, "vr": torch.randn(B, N, Lr, Cc, generator=g) * 1.3 - 0.2}
    if zero_last_ref:                      # the promise of valid_refs: the references behind the count are all-zero
        d["kr"][1, N - 1] = 0
        d["vr"][1, N - 1] = 0
    return {k: v.to("cuda", dtype) for k, v in d.items()}


def _fwd(ops, t, out, *, H, tuning, presc, inc=True, aff=None, valid=None, mass=False, bi=False, split=True, tables=False):
    """one ir_shared_attn_fwd on the tensors ``t`` into ``out``: (kernel name, lse, seg_mass)"""
    from instantrestore_amd import _lib
    B, Lq, _ = t["q"].shape
    rk, rv = t["kr"], t["vr"]
    if tables:
        rk = ops.RefKVTable.from_tensors([[rk[b, n] for n in range(rk.shape[1])] for b in range(B)])
        rv = ops.RefKVTable.from_tensors([[rv[b, n] for n in range(rv.shape[1])] for b in range(B)])
    lse = torch.empty(B, H, Lq, dtype=torch.float32, device="cuda")
    prev = ops.set_attn_variant(tuning)
    try:
        a = ops._fill_args(t["q"], t["ks"] if inc else None, t["vs"] if inc else None, rk, rv, H, SCALE, inc, aff, out, lse, split, presc,
                           valid, bi)
    finally:
        ops.set_attn_variant(prev)
    m = None
    if mass:
        m = torch.empty(B, H, Lq, int(inc) + t["kr"].shape[1], dtype=torch.float32, device="cuda")
        a.seg_mass = m.data_ptr()
    if bi:
        ops._bi_workspace(a, out.device)
    name = _lib.lib().ir_shared_attn_kernel_name(C.byref(a))
    assert name != b"", _lib.lib().ir_last_error_string()
    _lib.check(_lib.lib().ir_shared_attn_fwd(C.byref(a), ops._stream()), "ir_shared_attn_fwd")
    return name, lse, m


def _fwd_case(ops, arena, key, form, dtype, *, inc=True, fold=False, out_dtype=None, bi=False, split=True, tables=False):
    name, tuning, shape, presc, use_valid, mass = form
    B, H, Lq, N, Lr = shape
    data = _attn_data(shape, dtype, presc, seed=len(key) * 7 + (dtype == torch.float16), zero_last_ref=use_valid)
    valid = torch.tensor([N, N - 1], dtype=torch.int32, device="cuda") if use_valid else None
    aff = ops.adain_stats(data["vs"], data["vr"], heads=H) if fold else None
    kw = dict(H=H, tuning=0 if bi else tuning, presc=presc, inc=inc, aff=aff, valid=valid, mass=mass, bi=bi, split=split)
    want = torch.empty(B, Lq, H * 64, dtype=out_dtype or dtype, device="cuda")
    n0, lse0, m0 = _fwd(ops, data, want, **kw)
    placed, far_t = _put(arena, key, data)
    got = arena.view(placed["out"], want.dtype)
    n1, lse1, m1 = _fwd(ops, far_t, got, tables=tables, **kw)
    what = f"{key} {dtype}"
    assert n1 == n0, (what, n0, n1)
    _settle(arena, placed, data, {"out": (got, want)}, what)
    _same_small((lse1, m1), (lse0, m0), what)
    if inc and not use_valid and _once(("fwd", name, fold, dtype, out_dtype)):
        from oracle.shared_attn_oracle import shared_attention_np
        from parity_bounds import check_parity
        from test_gpu_parity import TOL_FACTOR
        qf = _np64(data["q"]) / (SCALE * LOG2E) if presc else _np64(data["q"])
        ref = shared_attention_np(qf, _np64(data["ks"]), _np64(data["vs"]), _np64(data["kr"]), _np64(data["vr"]), H, SCALE, fold, True)
        # the fp32 output rounds to the 16-bit one bit for bit (test_gpu_full_batch) and is held to that output's bounds: the literal
        # 1e-3 before the rounding is the suite's bound from 1024 keys on, and these calls have 416, 456 and 768
        check_parity(want.to(dtype), ref, dtype, what, factor=TOL_FACTOR.get(tuning, 1.0))
    return n0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", "AB")
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("form", FWD_FORMS, ids=[f[0] for f in FWD_FORMS])
def test_forward_with_far_strides(ops, arena, form, group, kind, dtype):
    _fwd_case(ops, arena, f"fwd/{form[0]}/{group}/{kind}", form, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form,variant", VARIANT_CASES, ids=[f"{f[0]}-{v}" for f, v in VARIANT_CASES])
def test_forward_variants_with_every_stride_far(ops, arena, form, variant, dtype):
    """the AdaIN fold, the fp32 output (o_sb in fp32 elements), the batch-invariant plan, the unsplit launch and the call without a
    self segment.  The other tests launch with the default workspace, whose K/V-range pieces start deep inside a segment."""
    name = form[0]
    kw = {"fold": dict(fold=True), "out_f32": dict(out_dtype=torch.float32), "batch_invariant": dict(bi=True), "no_split": dict(split=False),
          "refs_only": dict(inc=False)}[variant]
    _fwd_case(ops, arena, f"fwd_variant/{name}/{variant}", form, dtype, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", "AB")
@pytest.mark.parametrize("form", FWD_FORMS, ids=[f[0] for f in FWD_FORMS])
def test_forward_through_tables_whose_entries_lie_far_apart(ops, arena, form, kind, dtype):
    """the table entries are the far references themselves: neighbouring entries more than 4 GiB (A) or 2 GiB (B) apart"""
    _fwd_case(ops, arena, f"fwd/{form[0]}/{'ref_batch' if kind == 'A' else 'all'}/{kind}", form, dtype, tables=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", ["self", "ref"])
@pytest.mark.parametrize("form", LONG_FWD, ids=[f[0] for f in LONG_FWD])
def test_forward_on_the_longest_segment_it_accepts(ops, arena, form, which, dtype):
    """K and V are two column ranges of the same wide rows, at the largest row stride the validation accepts for the length: the
    offset of the tile behind the segment is within 128 bytes + one stride step of 2^31.  ``ref``: every reference, the last
    one included, has that stride."""
    B, H, Lq, N, Lr = form[2]
    length = Lq if which == "self" else Lr
    s = seg_stride_max(length)
    assert 64 * ((length + 63) // 64) * s * 2 + 128 <= LIMIT < 64 * ((length + 63) // 64) * (s + 8) * 2 + 128
    for fold in (False, True):
        _fwd_case(ops, arena, f"fwd_long/{form[0]}/{which}", form, dtype, fold=fold)
        arena.fill()


# ---------------------------------------------------------------------------------------------------------------------------
# the read-outs
# ---------------------------------------------------------------------------------------------------------------------------
def _readout(ops, entry, t, lse, H, rows):
    kw = dict(heads=H, scale=SCALE, include_self=True)
    if entry.startswith("probs_"):
        return ops.attn_probs(t["q"], t["ks"], t["kr"], lse, kernel=entry[6:], **kw)
    if entry == "segment_mass":
        return ops.attn_segment_mass(t["q"], t["ks"], t["kr"], lse, **kw)
    return ops.attn_rows(t["q"], t["ks"], t["kr"], lse, rows, reduce=entry[5:], **kw)


def _readout_case(ops, arena, key, dtype):
    from oracle.shared_attn_oracle import shared_attention_np
    import test_gpu_attn_rows as TR
    import test_gpu_probs as TP
    B, H, Lq, N, Lr = READOUT_SHAPE
    data = _attn_data(READOUT_SHAPE, dtype, False, seed=len(key))
    _, lse = ops.shared_attention(data["q"], data["ks"], data["vs"], data["kr"], data["vr"], heads=H, scale=SCALE, return_lse=True)
    rows = torch.tensor([[0, 5, Lq - 1, 64], [64, 3, 3, 199]])
    placed, far_t = _put(arena, key, data)
    p_ref = None                          # (ops takes the far views as they are: channel stride 1, every other a multiple of 8)
    for entry in READOUTS:
        want, got = _readout(ops, entry, data, lse, H, rows), _readout(ops, entry, far_t, lse, H, rows)
        _same_small((got,), (want,), f"{key} {entry} {dtype}")
        if _once((entry, dtype)):
            if p_ref is None:
                _, p_ref = shared_attention_np(*(_np64(data[n]) for n in ("q", "ks", "vs", "kr", "vr")), H, SCALE, False, True, return_probs=True)
            w = want.float().cpu().numpy()
            picked = np.stack([p_ref[b][:, rows[b].numpy()] for b in range(B)])                 # (B, H, R, Lkv)
            if entry.startswith("probs_"):
                assert np.abs(w - p_ref).max() <= TP.TOL[dtype]
            elif entry == "segment_mass":
                edges = [0, Lq] + [Lq + (n + 1) * Lr for n in range(N)]
                m_ref = np.stack([p_ref[..., a:b].sum(-1) for a, b in zip(edges[:-1], edges[1:])], axis=-1)
                import lse_bounds as LB                                    # the bound of test_gpu_probs.test_segment_mass
                keys = LB.pack_keys(data["ks"], data["kr"], True)
                sc = LB.row_scale(data["q"], keys, SCALE, LB.oracle_lse_and_mass(_np64(data["q"]), keys, H, SCALE))
                LB.check_mass(w, m_ref.reshape(w.shape), sc, f"{key} {entry} {dtype}")
            elif entry == "rows_none":
                assert np.abs(w - picked).max() <= TR.TOL[dtype]
            elif entry == "rows_head_mean":
                assert np.abs(w - picked.mean(1)).max() <= TR.TOL[dtype]
            else:
                assert np.abs(w - picked.mean(1).sum(1)).max() <= rows.shape[1] * TR.TOL[dtype]
    _settle(arena, placed, data, {}, f"{key} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", "AB")
@pytest.mark.parametrize("group", GROUPS)
def test_readouts_with_far_strides(ops, arena, group, kind, dtype):
    _readout_case(ops, arena, f"readout/{group}/{kind}", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", ["self", "ref"])
def test_readouts_on_segments_longer_than_the_forward_takes(ops, arena, which, dtype):
    """the read-outs address K through 64-bit pointers: a K segment whose rows reach past 2^32 bytes is theirs to read, while the
    forward refuses the same arguments"""
    from instantrestore_amd import _lib
    key = f"readout_long/{which}"
    spec = {t[0]: t for t in LAYOUTS[key]}
    k = spec["ks" if which == "self" else "kr"]
    assert (k[1][-2] - 1) * k[2][-2] * 2 >= 1 << 32
    _readout_case(ops, arena, key, dtype)
    a = _lib.SharedAttnArgs()
    a.struct_size = C.sizeof(a)
    a.dtype, a.batch, a.heads, a.len_q, a.len_self, a.n_refs, a.len_ref, a.flags, a.scale = 1, 2, 2, 200, 200, 3, 72, 1, SCALE
    a.q = a.k_self = a.v_self = a.k_ref = a.v_ref = a.out = 4096
    a.q_sb = a.ks_sb = a.vs_sb = a.o_sb = a.kr_sn = a.vr_sn = 200 * 128
    a.kr_sb = a.vr_sb = 3 * 200 * 128
    a.q_sl = a.ks_sl = a.vs_sl = a.o_sl = a.kr_sl = a.vr_sl = 128
    a.q_sh = a.ks_sh = a.vs_sh = a.o_sh = a.kr_sh = a.vr_sh = 64
    setattr(a, "ks_sl" if which == "self" else "kr_sl", k[2][-2])
    assert _lib.lib().ir_shared_attn_kernel_name(C.byref(a)) == b"" and b"IR_ATTN_SEG_BYTES_MAX" in _lib.lib().ir_last_error_string()


# ---------------------------------------------------------------------------------------------------------------------------
# AdaIN statistics, token statistics, the affine's application, the zero fill
# ---------------------------------------------------------------------------------------------------------------------------
def _adain_call(ops, op, t, H, aux):
    """the op on the tensors ``t`` (compact or far): the small fp32 results; in-place and strided outputs are in ``t``"""
    from instantrestore_amd import _lib
    if op == "adain_stats":
        return ops.adain_stats(t["vs"], t["vr"], heads=H)
    if op == "adain_stats_cached":
        return ops.adain_stats_cached(t["vs"], aux["mean"], aux["std"], heads=H)
    if op == "token_stats":
        return ops.token_stats(t["x"], heads=H)
    if op == "adain_apply":
        x, y = t["x"], t["y"]
        B, N, L, _ = x.shape
        rc = _lib.lib().ir_adain_apply(ops._dtype_code(x), B, H, N, L, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), 64,
                                       aux["a"].data_ptr(), aux["b"].data_ptr(), y.data_ptr(), y.stride(0), y.stride(1), y.stride(2), 64, ops._stream())
        _lib.check(rc, "ir_adain_apply")
        return ()
    ops.zero_invalid_refs(t["k"], t["v"], aux["valid"], heads=H)
    return ()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op,mode,kind", ADAIN_CASES, ids=["-".join(c).rstrip("-") for c in ADAIN_CASES])
def test_adain_family_with_far_strides(ops, arena, op, mode, kind, dtype):
    """``rows``: a token-row stride that carries len * stride * 2 past 4 GiB at 300 tokens (two 256-row chunks, one ragged)"""
    import oracle.shared_attn_oracle as O
    key = f"adain/{op}/{mode}/{kind}"
    B, H, Ls, N, Lr = ADAIN_SHAPE
    Cc = H * 64
    g = torch.Generator().manual_seed(len(key))
    mk = lambda shape, s, m: (torch.randn(shape, generator=g) * s + m).to("cuda", dtype)
    names = [t[0] for t in LAYOUTS[key]]
    data = {n: mk((B, Ls, Cc), 0.7, 1.0) if n == "vs" else mk((B, N, Lr, Cc), 1.5, -0.5) for n in names if n != "y"}
    aux = {"mean": torch.randn(B, N, H, 64, generator=g).cuda(), "std": (torch.rand(B, N, H, 64, generator=g) + 0.5).cuda(),
           "a": (torch.rand(B, N, H, 64, generator=g) + 0.5).cuda(), "b": torch.randn(B, N, H, 64, generator=g).cuda(), "valid": [N - 1, 0]}
    compact = {n: v.clone() for n, v in data.items()}
    if op == "adain_apply":
        compact["y"] = torch.empty_like(compact["x"])
    want = _adain_call(ops, op, compact, H, aux)
    placed, far_t = _put(arena, key, data)
    if op == "adain_apply":
        far_t["y"] = arena.view(placed["y"], dtype)
    got = _adain_call(ops, op, far_t, H, aux)
    what = f"{key} {dtype}"
    _same_small(got, want, what)
    written = {"adain_apply": ["y"], "zero_invalid_refs": ["k", "v"]}.get(op, [])
    _settle(arena, placed, data, {n: (far_t[n], compact[n]) for n in written}, what)
    if op == "zero_invalid_refs":          # exactly the invalid references are zero, the others keep their data
        for n in ("k", "v"):
            keep = data[n].clone()
            keep[0, N - 1:] = 0
            keep[1] = 0
            assert torch.equal(compact[n], keep), what
    if _once((op, dtype)):
        from parity_bounds import check_parity
        if op in ("adain_stats", "adain_stats_cached"):
            a_ref, b_ref = O.adain_affine_np(_np64(data["vs"]), _np64(data["vr"]), H) if op == "adain_stats" else (None, None)
            if a_ref is not None:          # the tolerances of test_gpu_parity.test_adain_stats_and_apply
                np.testing.assert_allclose(want[0].cpu().numpy().reshape(B, N, Cc), a_ref, rtol=2e-4, atol=1e-6)
                np.testing.assert_allclose(want[1].cpu().numpy().reshape(B, N, Cc), b_ref, rtol=2e-4, atol=2e-4)
            else:                          # bit-identical to ir_adain_stats on the statistics of the same tensors (test_gpu_adain_cached)
                rv = mk((B, N, Lr, Cc), 1.7, -0.2)
                m, sd = ops.token_stats(rv, heads=H)
                a1, b1 = ops.adain_stats_cached(data["vs"], m, sd, heads=H)
                a0, b0 = ops.adain_stats(data["vs"], rv, heads=H)
                assert torch.equal(a0, a1) and torch.equal(b0, b1)
        elif op == "token_stats":
            x = _np64(data["x"]).reshape(B * N, Lr, Cc)
            m_ref, s_ref = O.token_stats_np(x)
            rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())      # 1e-5 relative: the bar of test_gpu_fused_stats
            assert rel(want[0].cpu().numpy().reshape(B * N, 1, Cc), m_ref) <= 1e-5 and rel(want[1].cpu().numpy().reshape(B * N, 1, Cc), s_ref) <= 1e-5
        elif op == "adain_apply":
            a, b = _np64(aux["a"]).reshape(B, N, 1, Cc), _np64(aux["b"]).reshape(B, N, 1, Cc)
            check_parity(compact["y"], _np64(data["x"]) * a + b, dtype, what)


# ---------------------------------------------------------------------------------------------------------------------------
# the projection GEMMs
# ---------------------------------------------------------------------------------------------------------------------------
def _linear_call(ops, x, w, bias, y, kernel, stats=None):
    from instantrestore_amd import _lib
    m, k = x.shape
    n = w.shape[0]
    head = (ops._dtype_code(w), 1 if x.dtype == torch.float32 else 0, m, n, k, x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0),
            bias.data_ptr(), y.data_ptr(), y.stride(0), 64, 0.5)
    if stats is None:
        _lib.check(_lib.lib().ir_linear_fwd_ex(*head, kernel, ops._stream()), "ir_linear_fwd_ex")
        return None
    ws = torch.zeros(m // 64, n // 64, 128, dtype=torch.float32, device="cuda")
    if stats == "auto":
        rc = _lib.lib().ir_linear_fwd_stats(*head, 0, n, ws.data_ptr(), ws.numel() * 4, ops._stream())
    else:
        rc = _lib.lib().ir_linear_fwd_stats_ex(*head, 0, n, ws.data_ptr(), ws.numel() * 4, _lib.IR_LIN_BATCH_INVARIANT, ops._stream())
    _lib.check(rc, "ir_linear_fwd_stats")
    return ws


def _linear_case(ops, arena, key, dtype, n, k, x_f32, m, kernel, stats=None):
    from test_gpu_linear import TOL
    g = torch.Generator().manual_seed(n + k + m)
    x = torch.randn(m, k, generator=g)
    x = x.cuda() if x_f32 else x.to("cuda", dtype)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to("cuda", dtype)
    bias = torch.randn(n, generator=g).to("cuda", dtype)
    want = torch.empty(m, n, dtype=dtype, device="cuda")
    s0 = _linear_call(ops, x, w, bias, want, kernel, stats)
    placed, far_t = _put(arena, key, {"x": x})
    px = placed["x"]
    assert (px.entries[-1] - px.base) * px.elem_size >= 1 << 32
    if key.startswith("linear_mid"):       # the last 256-row block STARTS past 2^32 bytes
        assert (px.entries[(m - 1) // 256 * 256] - px.base) * px.elem_size >= 1 << 32
    got = arena.view(placed["y"], dtype)
    s1 = _linear_call(ops, far_t["x"], w, bias, got, kernel, stats)
    what = f"{key} {dtype}"
    _settle(arena, placed, {"x": x}, {"y": (got, want)}, what)
    if stats is not None:
        _same_small((s1,), (s0,), what)
    rows = sorted({0, 1, 63, 64, 255, 256, 257, m // 2, m // 2 + 1, m - 65, m - 2, m - 1})        # first, middle and last row blocks
    xr = x[rows].to(dtype).double().cpu().numpy()
    ref = xr @ w.double().cpu().numpy().T
    ref[:, :64] *= np.float32(0.5)                                                                # scale_cols = 64, col_scale = 0.5
    ref += bias.double().cpu().numpy()
    err = np.abs(want[rows].double().cpu().numpy() - ref)
    assert (err <= TOL[dtype] * np.maximum(1.0, np.abs(ref))).all(), (what, err.max())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("x_f32", [False, True], ids=["x16", "x32"])
@pytest.mark.parametrize("case", LIN_CASES, ids=[c[0] for c in LIN_CASES])
def test_linear_with_leading_dimensions_at_the_limit(ops, arena, case, x_f32, dtype):
    """x_ld and y_ld are the largest c_abi.hip takes; the last rows of X (and of Y with 16-bit X) lie beyond 4 GiB from the base"""
    name, kernel, n, k = case
    _linear_case(ops, arena, f"linear/{name}/{'f32' if x_f32 else '16'}", dtype, n, k, x_f32, LIN_M[x_f32], kernel)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("x_f32", [False, True], ids=["x16", "x32"])
@pytest.mark.parametrize("case", LIN_CASES, ids=[c[0] for c in LIN_CASES])
def test_linear_with_row_blocks_that_start_past_4_gib(ops, arena, case, x_f32, dtype):
    name, kernel, n, k = case
    _linear_case(ops, arena, f"linear_mid/{name}/{'f32' if x_f32 else '16'}", dtype, n, k, x_f32, LIN_MID_M[x_f32], kernel)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("stats", ["auto", "batch_invariant"])
def test_linear_statistics_tail_with_leading_dimensions_at_the_limit(ops, arena, stats, dtype):
    _linear_case(ops, arena, "linear/stats", dtype, 256, 128, False, LIN_M_STATS, 0, stats)


# ---------------------------------------------------------------------------------------------------------------------------
# image output and the FreeU filter
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("A", torch.float16), ("B", torch.bfloat16), ("f32", torch.float32)], ids=["A_f16", "B_bf16", "f32"])
def test_tensor2im_with_a_far_batch_stride(ops, arena, case):
    kind, dtype = case
    key = f"tensor2im/{kind}"
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 3, 20, 24, generator=g) * 2.4 - 1.2).to("cuda", dtype)
    want = ops.tensor2im_u8(x)
    placed, far_t = _put(arena, key, {"x": x})
    got = ops.tensor2im_u8(far_t["x"])
    _settle(arena, placed, {"x": x}, {}, key)
    assert torch.equal(got, want), key
    if dtype != torch.bfloat16:            # bit-exact against the restated tensor2im (test_gpu_parity.test_tensor2im_bytes_are_identical)
        from oracle.shared_attn_oracle import tensor2im_np
        for b in range(2):
            assert np.array_equal(want[b].cpu().numpy(), tensor2im_np(x[b].cpu().numpy()))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", "ABC")
def test_freeu_filter_with_far_plane_strides(ops, arena, kind, dtype):
    from instantrestore_amd import _lib
    from oracle.image_oracle import fourier_filter_np
    key = f"freeu/{kind}"
    planes = LAYOUTS[key][0][1][0]
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(planes, 256, generator=g) * 1.5 + 0.3).to("cuda", dtype)
    want = ops.freeu_fourier_filter(x.view(1, planes, 16, 16), 1, 0.2).view(planes, 256)
    placed, far_t = _put(arena, key, {"x": x})
    got = arena.view(placed["out"], dtype)
    rc = _lib.lib().ir_freeu_fourier_filter(ops._dtype_code(x), planes, 16, 16, far_t["x"].data_ptr(), far_t["x"].stride(0), got.data_ptr(),
                                            got.stride(0), 1, 0.2, ops._stream())
    _lib.check(rc, "ir_freeu_fourier_filter")
    _settle(arena, placed, {"x": x}, {"out": (got, want)}, f"{key} {dtype}")
    if _once(("freeu", dtype)):            # the tolerance of test_gpu_image.test_randomised_freeu_filter_shapes
        ref = fourier_filter_np(x.float().cpu().numpy().reshape(1, planes, 16, 16), 1, 0.2).reshape(planes, 256)
        amax = max(1.0, np.abs(ref).max(), float(x.float().abs().max()))
        tol = {torch.float16: 2.0 ** -11 + 4e-6, torch.bfloat16: 2.0 ** -8 + 4e-6}[dtype] * amax
        assert np.abs(want.float().cpu().numpy().astype(np.float64) - ref).max() <= tol


# ---------------------------------------------------------------------------------------------------------------------------
# tensors that are large by size alone
# ---------------------------------------------------------------------------------------------------------------------------
BIG = dict(B=5, H=4, L=4096, N=7)


def _big_inputs():
    B, H, L, N = BIG["B"], BIG["H"], BIG["L"], BIG["N"]
    g = torch.Generator(device="cuda").manual_seed(2)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return (r(B, L, H * 64) * 1.2).half(), r(B, L, H * 64).half(), r(B, L, H * 64).half(), r(B, N, L, H * 64).half(), r(B, N, L, H * 64).half()


def test_probability_matrix_beyond_2_to_the_32_bytes(ops):
    """(5, 4, 4096, 32768) fp16 probabilities: 2.7 G elements, 5.4 GB.  Row sums, about 40 rows against the float64 oracle (first and
    last (b, h), both sides of element 2^31 = byte 2^32), the generic kernel against the line kernel on a band of the last (b, h),
    and the same call's seg_mass against the band's block sums."""
    from oracle.shared_attn_oracle import shared_attention_np
    from test_gpu_probs import TOL
    _release_arena()
    torch.cuda.synchronize()
    _PEAK[0] = max(_PEAK[0], torch.cuda.max_memory_allocated())
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dtype = torch.float16
    B, H, L, N = BIG["B"], BIG["H"], BIG["L"], BIG["N"]
    Lkv = (1 + N) * L
    q, k, v, rk, rv = _big_inputs()
    _, lse, mass = ops.shared_attention(q, k, v, rk, rv, heads=H, scale=SCALE, include_self=True, return_lse=True, return_mass=True)
    probs = ops.attn_probs(q, k, rk, lse, heads=H, scale=SCALE, include_self=True, kernel="lines64")      # a line kernel by name, not by the AUTO rule
    assert probs.shape == (B, H, L, Lkv) and probs.numel() * 2 > 1 << 32 and mass.numel() == B * H * L * (1 + N)
    for b in range(B):
        for h in range(H):
            sums = probs[b, h].sum(-1, dtype=torch.float32)
            assert float((sums - 1).abs().max()) <= 4 * TOL[dtype], (b, h)
    mark = (1 << 31) // Lkv                                              # the first row that starts at element 2^31 / byte 2^32
    assert mark * Lkv == 1 << 31 and mark < B * H * L
    rng = np.random.default_rng(1)
    flat = sorted(set(rng.integers(0, B * H * L, 28).tolist() + [0, 1, L - 1, B * H * L - L, B * H * L - 1, mark - 2, mark - 1, mark, mark + 1,
                                                                  (1 << 30) // Lkv - 1, (1 << 30) // Lkv]))
    worst = 0.0
    for b in range(B):
        mine = [r for r in flat if r // (H * L) == b]
        if not mine:
            continue
        rows = sorted({r % L for r in mine})
        _, p_ref = shared_attention_np(_np64(q[b:b + 1, rows]), _np64(k[b:b + 1]), _np64(v[b:b + 1]), _np64(rk[b:b + 1]), _np64(rv[b:b + 1]),
                                       H, SCALE, False, True, return_probs=True)
        for r in mine:
            h, i = (r // L) % H, r % L
            worst = max(worst, float(np.abs(probs[b, h, i].float().cpu().numpy() - p_ref[0, h, rows.index(i)]).max()))
    print(f"\nprobability rows against the oracle: {len(flat)} rows, worst |err| {worst:.3e} (bound {TOL[dtype]:.1e})")
    assert worst <= TOL[dtype]
    band = slice(L - 512 - 64, L - 64)
    b, h = B - 1, H - 1
    qb, kb, rkb = q[b:, band, h * 64:(h + 1) * 64].contiguous(), k[b:, :, h * 64:(h + 1) * 64].contiguous(), rk[b:, :, :, h * 64:(h + 1) * 64].contiguous()
    lse_b = lse[b:, h:, band].contiguous()
    gen = ops.attn_probs(qb, kb, rkb, lse_b, heads=1, scale=SCALE, include_self=True, kernel="generic")
    assert torch.equal(gen[0, 0], probs[b, h, band])
    blocks = gen[0, 0].float().reshape(512, 1 + N, L).sum(-1)
    assert float((mass[b, h, band] - blocks).abs().max()) <= 4 * TOL[dtype]           # fp32 sums of 16-bit probabilities (test_gpu_probs)
    assert float((mass.sum(-1) - 1).abs().max()) <= 2e-3
    peak = torch.cuda.max_memory_allocated()
    print(f"peak device memory {peak / 2 ** 30:.2f} GiB ({base / 2 ** 30:.2f} GiB held before the test)")
    assert peak < 8 << 30


def test_attn_rows_output_beyond_2_to_the_32_bytes(ops):
    """IR_ROWS_NONE at the smallest n_rows whose (B, H, n_rows, Lkv) output crosses 2^32 bytes: its rows are the dump's rows"""
    _release_arena()
    B, H, L, N = BIG["B"], BIG["H"], BIG["L"], BIG["N"]
    Lkv = (1 + N) * L
    R = (1 << 32) // (B * H * Lkv * 2) + 1
    assert B * H * R * Lkv * 2 > 1 << 32 >= B * H * (R - 1) * Lkv * 2 and R <= L
    q, k, v, rk, rv = _big_inputs()
    _, lse = ops.shared_attention(q, k, v, rk, rv, heads=H, scale=SCALE, include_self=True, return_lse=True)
    idx = torch.stack([torch.randperm(L, generator=torch.Generator().manual_seed(b))[:R] for b in range(B)])
    got = ops.attn_rows(q, k, rk, lse, idx, heads=H, scale=SCALE, include_self=True, reduce="none")
    assert got.shape == (B, H, R, Lkv)
    for b in range(B):                     # the dump of this entry's rows, one batch entry at a time
        sel = idx[b].cuda()
        want = ops.attn_probs(q[b:b + 1, sel].contiguous(), k[b:b + 1], rk[b:b + 1], lse[b:b + 1][:, :, sel].contiguous(), heads=H, scale=SCALE,
                              include_self=True)
        assert torch.equal(got[b], want[0]), b
        assert float((got[b].sum(-1, dtype=torch.float32) - 1).abs().max()) <= 4e-3
