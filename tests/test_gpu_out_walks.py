"""The attention OUTPUT of every forward form on walks that MOVE the lazy softmax reference, EVERY element, against the float64
oracle on the same 16-bit-rounded inputs, held to tests/out_bounds.py: |O - O_ref| <= u_P * A + u_sub * U + K_OUT * 2^-23 * row_scale * S
per (b, row, h, d) on the fp32 result before the output rounding (u_sub * U: fp16's subnormal P, zero for bf16); the 16-bit launch must
be that result rounded to the type, bit for bit; rows without an unmasked key are exact zeros.

Why: the kernels rescale lazily - the running reference of a row moves only when the row max outgrows it by 2^6 (the forms that
check after the exponentials: when a partial row sum exceeds 2^11).  What runs at a move - the accumulator scaling, the frame
change of the AdaIN fold (the LDS total with its lazy scale in the 32-row kernel, the ratio frame of the 64-row and 128-row
kernels), the (O, m, l) merge of K/V-range pieces, and the copies of all of it in the BIAS, RAGGED and REGION forms - is dead
after the first tile on N(0, 1) inputs (tests/test_out_bounds_cpu.py asserts that, and that every family here moves the reference
on at least 10 % of the rows).  tests/test_gpu_lse.py holds the row SUM's rescale on such inputs; this file holds the output.

Inputs (tests/lse_cases.py, the smallest shapes at which each path exists): the families "peaky", "ramp", "spike", "low" and the
boundary spikes "at:<where>" - one dominant key as the last key of a tile, the first of the next, the last of a segment, the first
of the next, the last existing key of a ragged tail, the first key of the second K/V-range piece, and for the masked forms an
allowed key directly behind a fully masked tile.  Values are ``styled_values``: AdaIN scales that differ by 20x and 80x between
neighbouring segments and a near-constant style channel, so a fold in the wrong frame leaves the bound by orders of magnitude.
A dominant key that is masked, disallowed or beyond its count must be inert: the same bytes as without it.  A few cases run without
being relied on to move the reference ("low" where its block does not fill the first tile, "spike" - one key times 6 - where it is too
weak, "spike" and "peaky" under the 2^11 rule; ``lse_cases.relied_on``): their printed labels and IR_PARITY_LOG records say so.
So for the forms that check after the exponentials (tuning 18, 13 with the flag, the 128-row kernel) the reference-moving inputs
relied on are "ramp", "low" and the boundary spikes "at:*" (one key times 16) only.

Reference: ``out_bounds.oracle_out_and_scales`` (cross-checked against oracle.shared_attn_oracle, tests/key_bias_oracle.py and
tests/region_oracle.py in tests/test_out_bounds_cpu.py) with the fp32 affine the launch is given; q_true = q16 / QC under the
pre-scaled flag; tuning 11 WITHOUT the flag rounds Q * scale * log2(e) inside the kernel and is held against the equally rounded Q.
The kernel that ran is asserted by name.  IR_SWEEP_SEED offsets every seed.

Measured on an MI355X (seeds 0, 1, 2; tests/out_bounds.py has the table): bf16 largest 0.974 of the bound (median 0.34) - the derived
first term, where one key carries a row; what it leaves is at most 0.033 x 2^-23 x row_scale x S (K_OUT 0.25).  fp16: largest 0.957 of
the bound (median 0.35); what the first two terms leave is at most 0.114 of that unit (K_OUT 0.5).  Every 16-bit launch was its fp32
launch rounded, every masked dominant key inert, no form needed a fix."""
import numpy as np
import pytest
import torch

import lse_bounds as LB
import lse_cases as LC
import out_bounds as OB
from region_oracle import allowed_np

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
PIPE = "shared_attn_fwd_pipe_kernel<"
NAMES = {7: PIPE + "4 waves, exact rescale>", 10: PIPE + "4 waves, lazy max>", 11: PIPE + "4 waves, lazy max, pre-scaled Q",
         14: PIPE + "4 waves, lazy max, early QK", 18: PIPE + "4 waves, pre-scaled Q, reference checked after the exponentials",
         12: "shared_attn_fwd_w64_kernel<64 rows/wave, 4 waves", 13: "shared_attn_fwd_w64_kernel<64 rows/wave, 8 waves",
         16: "shared_attn_fwd_w128_kernel<"}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


_DEV, _AFF, _REF = {}, {}, {}


def _dev(x):
    if id(x) not in _DEV:
        d = lambda t: None if t is None else t.cuda()
        _DEV[id(x)] = (x, tuple(map(d, (x.q, x.qs, x.k, x.v, x.rk, x.rv))))
    return _DEV[id(x)][1]


def _affine(ops, x):
    """the fp32 affine of the launch (device) and the same numbers for the oracle"""
    if id(x) not in _AFF:
        q, qs, k, v, rk, rv = _dev(x)
        aff = ops.adain_stats(v, rv, heads=x.shape[1])
        B, N = rv.shape[:2]
        _AFF[id(x)] = (aff, tuple(t.cpu().double().numpy().reshape(B, N, -1) for t in aff))
    return _AFF[id(x)]


def _reference(ops, x, q_kind, fold, mask_key=None, bias=None, counts=None, allowed=None):
    """the oracle's output and scales, once per (inputs, which Q, fold, mask) and left unchanged.  q_kind: "plain", "presc" (q16 / QC)
    or "rounded" (what tuning 11 without the flag forms its scores from)"""
    key = (id(x), q_kind, fold, mask_key)
    if key not in _REF:
        q = {"plain": lambda: LC.np64(x.q), "presc": lambda: LC.np64(x.qs) / LC.QC,
             "rounded": lambda: LB.q_rounded_like_tuning_11(x.q, x.dtype, LC.SCALE)}[q_kind]()
        inc = x.shape[6]
        ref = OB.oracle_out_and_scales(q, LB.pack_keys(x.k, x.rk, inc), LB.pack_keys(x.v, x.rv, inc), x.shape[1], LC.SCALE, LC.seg_lens(x.shape),
                                       affine=_affine(ops, x)[1] if fold else None, bias=bias, counts=counts, allowed=allowed)
        for a in vars(ref).values():
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _launch(ops, x, tuning, presc, fold, name_part, **kw):
    """the forced call with the store before the output rounding; the 16-bit launch must be its rounding, bit for bit"""
    q, qs, k, v, rk, rv = _dev(x)
    H, inc = x.shape[1], x.shape[6]
    args = dict(heads=H, scale=LC.SCALE, include_self=inc, adain=_affine(ops, x)[0] if fold else None, q_prescaled=presc, **kw)
    first = lambda r: r[0] if isinstance(r, tuple) else r
    prev = ops.set_attn_variant(tuning)
    try:
        name = ops.shared_attention_kernel_name(qs if presc else q, k, v, rk, rv, **args)
        out32 = first(ops.shared_attention(qs if presc else q, k, v, rk, rv, out_dtype=torch.float32, **args))
        out16 = first(ops.shared_attention(qs if presc else q, k, v, rk, rv, **args))
    finally:
        ops.set_attn_variant(prev)
    assert all(part in name for part in ([name_part] if isinstance(name_part, str) else name_part)), (tuning, name)
    assert out32.dtype == torch.float32 and out16.dtype == x.dtype
    assert torch.equal(out32.to(x.dtype), out16), f"[{name}]: the 16-bit launch is not the fp32 result rounded to the type"
    return out32, name


def _hold(ops, x, ref, tuning, presc, fold, name_part, what, **kw):
    out, name = _launch(ops, x, tuning, presc, fold, name_part, **kw)
    what = f"{what} {'fold' if fold else 'plain'} [{name}]"
    r = OB.check_out(out, ref, x.dtype, what, frame=presc)
    print(f"{what}: out ratio {r:.3f}")
    return out


def _mark(shape, family, kind="plain", which=None, rule11=False):
    """what a comparison's label and record carry where the case is NOT relied on to move the reference (``lse_cases.relied_on``;
    ``rule11``: the form checks after the exponentials - the 2^11 partial-sum rule): it runs all the same, as an ordinary walk"""
    return "" if LC.relied_on(shape, family, kind, which, rule11) else " (NOT relied on to move the reference)"


def _folds(x):
    B, H, Lq, Ls, N, Lr, inc = x.shape
    return (False, True) if N and Lr >= 8 else (False,)


def _params(shapes, **kw):
    return [pytest.param(s, f, id=f"{LC.sid(s)}-{f}") for s in shapes for f in LC.walk_families(s, **kw)]


# tuning, pre-scaled flag, which Q the reference is formed from
PIPE32_FORMS = [(7, False, "plain"), (10, False, "plain"), (14, False, "plain"), (11, True, "presc"), (18, True, "presc"), (0, True, "presc"),
                (11, False, "rounded")]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,family", _params(LC.PIPE32))
def test_32_row_forms(ops, shape, family, dtype):
    """the plain-Q forms 7 / 10 / 14, tuning 11, 18 and the default dispatch with the flag, and tuning 11 without it (Q rounded
    inside the kernel; reference from the equally rounded Q): ragged tiles, a partial row block"""
    x = LC.inputs(shape, family, dtype, style=True)
    for tuning, presc, q_kind in PIPE32_FORMS:
        for fold in _folds(x):
            _hold(ops, x, _reference(ops, x, q_kind, fold), tuning, presc, fold,
                  "Q rounded in the kernel" if q_kind == "rounded" else NAMES[11 if tuning == 0 else tuning],
                  f"{LC.sid(shape)} {family}{_mark(shape, family, rule11=tuning == 18)} tuning {tuning} Q {q_kind}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,family", _params(LC.W64))
def test_64_row_kernels(ops, shape, family, dtype):
    """4 waves (12) and 8 waves (13) with the plain Q, 13 pre-scaled (reference checked after the exponentials; ratio frame of the fold)"""
    x = LC.inputs(shape, family, dtype, style=True)
    for tuning, presc in ((12, False), (13, False), (13, True)):
        for fold in _folds(x):
            _hold(ops, x, _reference(ops, x, "presc" if presc else "plain", fold), tuning, presc, fold, NAMES[tuning],
                  f"{LC.sid(shape)} {family}{_mark(shape, family, rule11=presc)} tuning {tuning} {'prescq' if presc else 'plainq'}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,family", _params(LC.W128))
def test_128_row_kernel_and_its_forms(ops, shape, family, dtype):
    """the plain instantiation, the forms instantiation with ``return_mass``, and - where the case has zero-filled references - with
    ``valid_refs`` on the zero-filled tensors (the closed form of the zero suffix against the oracle that walks the zeros)"""
    x = LC.inputs(shape, family, dtype, style=True)
    what = f"{LC.sid(shape)} {family}{_mark(shape, family, rule11=True)} tuning 16"
    for fold in _folds(x):
        ref = _reference(ops, x, "presc", fold)
        _hold(ops, x, ref, 16, True, fold, NAMES[16], what + " plain instantiation")
        _hold(ops, x, ref, 16, True, fold, NAMES[16], what + " with masses", return_mass=True)
    valid = LC.W128_VALID.get(shape)
    if valid is not None:
        xz = LC.inputs(shape, family, dtype, valid, style=True)
        vt = torch.tensor(valid, dtype=torch.int32, device="cuda")
        for fold in _folds(xz):
            ref = _reference(ops, xz, "presc", fold)
            _hold(ops, xz, ref, 16, True, fold, NAMES[16], what + f" valid_refs {valid}", return_mass=True, valid_refs=vt)
            _hold(ops, xz, ref, 16, True, fold, NAMES[16], what + f" valid_refs {valid}, no masses", valid_refs=vt)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,family", _params(LC.PIECES))
def test_kv_range_pieces_and_the_combine(ops, shape, family, dtype):
    """the batch-invariant plan cuts every item in 2 K/V-range pieces whose fp32 partials (O, m, l) the combine kernel merges; the
    boundary spike "piece_first" is the first key of the second piece.  The default dispatch with the flag may pick a form that checks
    the reference after the exponentials, so the pre-scaled comparisons are labelled under the 2^11 rule, as the 64-row test's are"""
    B, H, Lq, Ls, N, Lr, inc = shape
    x = LC.inputs(shape, family, dtype, style=True)
    for presc in (True, False):
        for fold in _folds(x):
            for od in (torch.float32, None):
                plan = ops.shared_attention_plan(B, Lq, H, len_self=Ls, n_refs=N, len_ref=Lr, dtype=dtype, include_self=inc, adain=fold,
                                                 q_prescaled=presc, out_dtype=od)
                assert plan["pieces_per_item"] == 2, plan
            _hold(ops, x, _reference(ops, x, "presc" if presc else "plain", fold), 0, presc, fold, "[batch-invariant: 2 pieces per",
                  f"{LC.sid(shape)} {family}{_mark(shape, family, rule11=presc)} plan {'prescq' if presc else 'plainq'}", batch_invariant=True)


def _masked_cases(kind):
    return [pytest.param(s, f, w, id=f"{f}-{w}" if w else f) for s, f, k, w in LC.out_walk_cases() if k == kind]


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,family,pattern", _masked_cases("bias"))
def test_bias_forms(ops, shape, family, pattern, dtype, presc):
    """a finite bias of both signs, a -inf mask over scattered keys, and a fully masked tile with the dominant key directly behind it"""
    bias, _, _ = LC.case_mask(shape, "bias", pattern, family)
    x = LC.inputs(shape, family, dtype, style=True)
    for fold in (False, True):
        ref = _reference(ops, x, "presc" if presc else "plain", fold, mask_key=(pattern, family), bias=bias.double().numpy())
        _hold(ops, x, ref, 0, presc, fold, ["pipe_kernel", "key bias"], f"bias {pattern} {family}{_mark(shape, family, 'bias', pattern, presc)} {'prescq' if presc else 'plainq'}",
              key_bias=bias.cuda())


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,family,_w", _masked_cases("counts"))
def test_ragged_forms(ops, shape, family, _w, dtype, presc):
    """per-reference token counts (full, absent, one key past a tile / a single key, a whole tile, ragged): "at:tail_last" is every
    entry's last existing key, "at:seg_first" sits directly behind entry 0's absent reference"""
    x = LC.inputs(shape, family, dtype, style=True, counts=LC.COUNTS)
    lens = torch.tensor(LC.COUNTS, dtype=torch.int32, device="cuda")
    for fold in (False, True):
        ref = _reference(ops, x, "presc" if presc else "plain", fold, mask_key="counts", counts=LC.COUNTS)
        _hold(ops, x, ref, 0, presc, fold, ["pipe_kernel", "ragged refs"], f"counts {family}{_mark(shape, family, 'counts', None, presc)} {'prescq' if presc else 'plainq'}",
              ref_lens=lens)


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,family,_w", _masked_cases("region"))
def test_region_forms(ops, shape, family, _w, dtype, presc):
    """a rule that masks some segments for some rows only (the fold's frames differ per row of one block), a tile that is nobody's with
    the dominant key directly behind it, two rows that may attend nothing"""
    qa, kr = LC.region_rule(shape)
    allowed = allowed_np(qa.numpy(), kr.numpy())
    x = LC.inputs(shape, family, dtype, style=True)
    for fold in (False, True):
        ref = _reference(ops, x, "presc" if presc else "plain", fold, mask_key="region", allowed=allowed)
        assert np.isneginf(ref.lse[:, :, 7]).all()
        _hold(ops, x, ref, 0, presc, fold, ["pipe_kernel", "regions"], f"regions {family}{_mark(shape, family, 'region', None, presc)} {'prescq' if presc else 'plainq'}",
              q_allow=qa.cuda(), key_region=kr.cuda())


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["bias", "counts", "region"])
def test_a_dominant_key_that_is_masked_is_inert(ops, kind, dtype, presc):
    """one key times SPIKE_X inside the masked tile (BIAS, REGION: nobody's) or directly behind its reference's count (RAGGED): output, LSE
    and masses are the same bytes as without it, fold on and off"""
    shape = LC.REGION if kind == "region" else LC.BIASED
    B, H, Lq, Ls, N, Lr, inc = shape
    x = LC.inputs(shape, "spike", dtype, style=True)
    q, qs, k, v, rk, rv = _dev(x)
    bias, counts, region = LC.case_mask(shape, kind, "masked_tile")
    rk2 = rk.clone()
    flat = rk2.view(B, N * Lr, -1)
    if kind == "counts":
        kw = dict(ref_lens=torch.tensor(counts, dtype=torch.int32, device="cuda"))
        for b in range(B):
            flat[b, (N - 1) * Lr + counts[b][N - 1]] *= LC.SPIKE_X
    else:
        kw = dict(key_bias=bias.cuda()) if kind == "bias" else dict(q_allow=region[0].cuda(), key_region=region[1].cuda())
        flat[:, LC.masked_tile(shape)[0] + 5 - Ls] *= LC.SPIKE_X
    assert not torch.equal(rk2, rk)
    for fold in (False, True):
        args = dict(heads=H, scale=LC.SCALE, include_self=inc, adain=_affine(ops, x)[0] if fold else None, q_prescaled=presc,
                    return_lse=True, return_mass=True, out_dtype=torch.float32, **kw)
        want = ops.shared_attention(qs if presc else q, k, v, rk, rv, **args)
        got = ops.shared_attention(qs if presc else q, k, v, rk2, rv, **args)
        for a, b_, what in zip(got, want, ("out", "lse", "mass")):
            assert torch.equal(a, b_) or (what == "lse" and torch.equal(torch.nan_to_num(a, neginf=-1e30), torch.nan_to_num(b_, neginf=-1e30))), \
                f"{kind} {'fold' if fold else 'plain'}: {what} changed with a dominant key that is masked"
