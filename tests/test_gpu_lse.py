"""The log-sum-exp and the by-product segment masses of every product forward kernel, EVERY element, against the float64 oracle
on the same 16-bit-rounded inputs, held to tests/lse_bounds.py: |lse - lse_ref| <= KAPPA * 2^-23 * max(1, |lse_ref|, T_row) per
(b, h, row), masses to the same scale absolutely.  The six read-outs (probabilities, segment masses, rows, match, transfer,
received) multiply exp(-lse) into everything they return and their own tests use the DEVICE's LSE in the reference, so this is
where a row sum that is off by a fraction of a percent - a stale lazy reference in a rescale, a K/V-range piece combined with the
wrong weight, a cumulative sum stored one tile early, a zero-suffix closed form that miscounts a segment - shows
(tests/test_lse_bounds_cpu.py: a lost key moves a third of the rows by more than 4 bounds).

Shapes (tests/lse_cases.py) are the smallest at which each path exists; the kernel that ran is asserted by name.  Reference:
``lse_bounds.oracle_lse_and_mass`` - the arithmetic of oracle.shared_attn_oracle / tests/key_bias_oracle.py (m + log sum exp(s - m),
block sums of exp(s - lse)), cross-checked against both in ``test_the_reference_is_the_oracles``; q_true = q16 / QC under the
pre-scaled flag.  IR_TUNE_PIPE32_PRESCALE_Q (11) WITHOUT the flag rounds Q * scale * log2(e) to 16 bit inside the kernel: its
reference is formed from the equally rounded Q.  IR_SWEEP_SEED offsets every seed."""
import numpy as np
import pytest
import torch

import lse_bounds as LB
import lse_cases as LC
from key_bias_oracle import biased_attention_np
from oracle import shared_attn_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
MASS_TUNINGS = (0, 11, 13, 14, 16)          # the kernels that carry the by-product instantiation
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


_DEV, _REF = {}, {}


def _dev(x):
    if id(x) not in _DEV:
        d = lambda t: None if t is None else t.cuda()
        _DEV[id(x)] = (x, tuple(map(d, (x.q, x.qs, x.k, x.v, x.rk, x.rv))))
    return _DEV[id(x)][1]


def _seg_lens(shape):
    B, H, Lq, Ls, N, Lr, inc = shape
    return ([Ls] if inc or N == 0 else []) + [Lr] * N


def _reference(x, q_kind, bias=None, bias_key=None):
    """(lse_ref, mass_ref, row scales), float64, once per (inputs, which Q, bias) and left unchanged.  q_kind: "plain", "presc"
    (q16 / QC) or "rounded" (what tuning 11 without the flag forms its scores from)"""
    key = (id(x), q_kind, bias_key)
    if key not in _REF:
        shape = x.shape
        q = {"plain": lambda: LC.np64(x.q), "presc": lambda: LC.np64(x.qs) / LC.QC,
             "rounded": lambda: LB.q_rounded_like_tuning_11(x.q, x.dtype, LC.SCALE)}[q_kind]()
        assert bias is None
        keys = LB.pack_keys(x.k, x.rk, shape[6])
        lse, mass = LB.oracle_lse_and_mass(q, keys, shape[1], LC.SCALE, bias=bias, seg_lens=_seg_lens(shape))
        sc = LB.row_scale(q, keys, LC.SCALE, lse, bias=bias)
        sc_frame = LB.row_scale(q, keys, LC.SCALE, lse, bias=bias, frame=True)
        for a in (lse, mass, sc, sc_frame):
            a.setflags(write=False)
        _REF[key] = (lse, mass, sc, sc_frame)
    return _REF[key]


def _klass(name, presc):
    """the pre-scaled-Q forms (IR_FLAG_Q_PRESCALED: 32-row PRESC / POSTCHECK, 64-row, 128-row) take minus the running reference
    through the MFMA C operand: class "frame" (tests/lse_bounds.py)"""
    return "frame" if presc else "fp32"


def _call(ops, x, tuning, presc, fold, want_mass, name_part, **kw):
    """the forced call: (lse, mass or None)"""
    q, qs, k, v, rk, rv = _dev(x)
    H, inc = x.shape[1], x.shape[6]
    aff = ops.adain_stats(v, rv, heads=H) if fold else None
    args = dict(heads=H, scale=LC.SCALE, include_self=inc, adain=aff, q_prescaled=presc, **kw)
    prev = ops.set_attn_variant(tuning)
    try:
        name = ops.shared_attention_kernel_name(qs if presc else q, k, v, rk, rv, return_mass=want_mass, **args)
        res = ops.shared_attention(qs if presc else q, k, v, rk, rv, return_lse=True, return_mass=want_mass, **args)
    finally:
        ops.set_attn_variant(prev)
    assert name_part in name, (tuning, name)
    return res[1], (res[2] if want_mass else None), name


def _hold(ops, x, tuning, presc, fold, name_part, what, q_kind=None, want_mass=None, **kw):
    want_mass = (tuning in MASS_TUNINGS) if want_mass is None else want_mass
    lse, mass, name = _call(ops, x, tuning, presc, fold, want_mass, name_part, **kw)
    lse_ref, mass_ref, sc, sc_frame = _reference(x, q_kind or ("presc" if presc else "plain"))
    what = f"{what} {'fold' if fold else 'plain'} [{name}]"
    klass = _klass(name, presc)
    if klass == "frame":
        sc = sc_frame
    r = LB.check_lse(lse, lse_ref, sc, what, klass=klass)
    rm = LB.check_mass(mass, mass_ref, sc, what) if want_mass else None
    print(f"{what}: lse ratio {r:.2f}" + ("" if rm is None else f", mass ratio {rm:.2f}"))
    return lse, mass


def _folds(x):
    B, H, Lq, Ls, N, Lr, inc = x.shape
    return (False, True) if N and Lr >= 8 else (False,)


def test_the_reference_is_the_oracles():
    """``lse_bounds.oracle_lse_and_mass`` against oracle.shared_attn_oracle (probabilities -> block sums, scores -> LSE) and
    tests/key_bias_oracle.biased_attention_np on one small case each: the same float64 numbers to 1e-12"""
    x = LC.inputs(LC.PIPE32[0], "n15", torch.bfloat16)
    B, H, Lq, Ls, N, Lr, inc = x.shape
    f = LC.np64
    lse, mass = LB.oracle_lse_and_mass(f(x.q), LB.pack_keys(x.k, x.rk, inc), H, LC.SCALE, seg_lens=_seg_lens(x.shape))
    _, p = O.shared_attention_np(f(x.q), f(x.k), f(x.v), f(x.rk), f(x.rv), H, LC.SCALE, False, inc, return_probs=True)
    p = p.reshape(B, H, Lq, -1)
    edges = np.concatenate([[0], np.cumsum(_seg_lens(x.shape))])
    assert np.abs(np.stack([p[..., a:b].sum(-1) for a, b in zip(edges[:-1], edges[1:])], -1) - mass).max() <= 1e-12
    qh = O.head_to_batch_dim_np(f(x.q), H)
    ek, _ = O.extended_kv_np(f(x.k), f(x.v), f(x.rk), f(x.rv), H, False, inc)
    s = np.matmul(qh, ek.transpose(0, 2, 1)) * LC.SCALE
    assert np.abs((s.max(-1) + np.log(np.exp(s - s.max(-1, keepdims=True)).sum(-1))).reshape(B, H, Lq) - lse).max() <= 1e-12
    xb = LC.inputs(LC.BIASED, "n1", torch.bfloat16)
    bias = LC.bias_patterns(LC.BIASED)["finite_one_entry_masked"].double().numpy()
    lse_b, mass_b = LB.oracle_lse_and_mass(f(xb.q), LB.pack_keys(xb.k, xb.rk, True), 2, LC.SCALE, bias=bias, seg_lens=_seg_lens(LC.BIASED))
    _, rl, rm = biased_attention_np(f(xb.q), f(xb.k), f(xb.v), f(xb.rk), f(xb.rv), 2, LC.SCALE, bias, seg_lens=_seg_lens(LC.BIASED))
    assert np.array_equal(np.isneginf(rl), np.isneginf(lse_b)) and np.isneginf(rl[1]).all()
    assert np.abs(rl[0] - lse_b[0]).max() <= 1e-12 and np.abs(rm - mass_b).max() <= 1e-12


# tuning, pre-scaled flag, which Q the reference is formed from
PIPE32_FORMS = [(7, False, "plain"), (10, False, "plain"), (14, False, "plain"), (11, True, "presc"), (18, True, "presc"), (0, True, "presc"),
                (11, False, "rounded")]


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", LC.PIPE32, ids=LC.sid)
def test_32_row_forms(ops, shape, dtype, family):
    """ragged tiles, a partial row block: every named form of the 32-row kernel, tuning 11 and the default dispatch with the flag,
    and tuning 11 without it (Q rounded inside the kernel; reference from the equally rounded Q)"""
    x = LC.inputs(shape, family, dtype)
    for tuning, presc, q_kind in PIPE32_FORMS:
        for fold in _folds(x):
            _hold(ops, x, tuning, presc, fold, "Q rounded in the kernel" if q_kind == "rounded" else NAMES[11 if tuning == 0 else tuning], f"{LC.sid(shape)} {family} tuning {tuning} Q {q_kind}",
                  q_kind=q_kind)


UNALIGNED = [(s, 0, p) for s in LC.ODD + LC.TAILS for p in (False, True)] + [(LC.TAILS[0], 14, False)]   # 14 is a plain-Q form


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape,tuning,presc", UNALIGNED, ids=[f"{LC.sid(s)}-tuning{t}-{'prescq' if p else 'plainq'}" for s, t, p in UNALIGNED])
def test_unaligned_lengths_and_key_tails(ops, shape, tuning, presc, dtype):
    """nothing aligned, a one-token reference, key tails of 8 / 48 keys: the default dispatch; the tails also on tuning 14"""
    x = LC.inputs(shape, "n15", dtype)
    for fold in _folds(x):
        _hold(ops, x, tuning, presc, fold, NAMES[14] if tuning == 14 else PIPE, f"{LC.sid(shape)} tuning {tuning} {'prescq' if presc else 'plainq'}")


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", LC.W64, ids=LC.sid)
def test_64_row_kernels(ops, shape, dtype, family):
    x = LC.inputs(shape, family, dtype)
    for tuning, presc in ((12, False), (13, False), (13, True)):
        for fold in _folds(x):
            _hold(ops, x, tuning, presc, fold, NAMES[tuning], f"{LC.sid(shape)} {family} tuning {tuning} {'prescq' if presc else 'plainq'}")


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", LC.W128, ids=LC.sid)
def test_128_row_kernel_and_its_forms(ops, shape, dtype, family):
    """the plain instantiation (no by-product, no counts) and the forms instantiation: return_mass, and valid_refs where the case
    has zero-filled references (the closed form of the zero suffix against the oracle on the zero-filled tensors)"""
    valid = LC.W128_VALID.get(shape)
    x = LC.inputs(shape, family, dtype, valid)
    what = f"{LC.sid(shape)} {family} tuning 16"
    for fold in _folds(x):
        plain, _ = _hold(ops, x, 16, True, fold, NAMES[16], what + " plain instantiation", want_mass=False)
        forms, _ = _hold(ops, x, 16, True, fold, NAMES[16], what + " with masses", want_mass=True)
        if valid is not None:
            vt = torch.tensor(valid, dtype=torch.int32, device="cuda")
            _hold(ops, x, 16, True, fold, NAMES[16], what + f" valid_refs {valid}", want_mass=True, valid_refs=vt)
            _hold(ops, x, 16, True, fold, NAMES[16], what + f" valid_refs {valid}, no masses", want_mass=False, valid_refs=vt)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", LC.PIECES, ids=LC.sid)
def test_kv_range_pieces_and_the_combine(ops, shape, dtype, family):
    """batch-invariant mode cuts every item in K/V-range pieces (2 here, as tests/test_gpu_ref_lens.py asserts of this shape) whose
    fp32 partials - row max, row sum, cumulative sums at the segment boundaries - the combine kernel merges"""
    B, H, Lq, Ls, N, Lr, inc = shape
    x = LC.inputs(shape, family, dtype)
    for presc in (True, False):
        for fold in _folds(x):
            plan = ops.shared_attention_plan(B, Lq, H, len_self=Ls, n_refs=N, len_ref=Lr, dtype=dtype, include_self=inc, adain=fold,
                                             q_prescaled=presc, return_mass=True)
            assert plan["pieces_per_item"] == 2, plan
            _hold(ops, x, 0, presc, fold, "[batch-invariant: 2 pieces per", f"{LC.sid(shape)} {family} plan {'prescq' if presc else 'plainq'}",
                  want_mass=True, batch_invariant=True)


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("pattern", ["scatter", "finite", "finite_one_entry_masked"])
def test_bias_forms(ops, pattern, dtype, presc):
    """a -inf mask over scattered keys, a finite bias of both signs (|bias| up to 6: T_row carries it), one fully masked entry"""
    x = LC.inputs(LC.BIASED, "n1", dtype)
    bias = LC.bias_patterns(LC.BIASED)[pattern]
    q, qs, k, v, rk, rv = _dev(x)
    B, H, Lq, Ls, N, Lr, inc = LC.BIASED
    q_kind = "presc" if presc else "plain"
    key = (id(x), q_kind, pattern)
    if key not in _REF:
        qt = LC.q_true(x, presc)
        _, lse_ref, mass_ref = biased_attention_np(qt, LC.np64(x.k), LC.np64(x.v), LC.np64(x.rk), LC.np64(x.rv), H, LC.SCALE,
                                                   bias.double().numpy(), train_input=inc, seg_lens=_seg_lens(LC.BIASED))
        _REF[key] = (lse_ref, mass_ref, LB.row_scale(qt, LB.pack_keys(x.k, x.rk, inc), LC.SCALE, lse_ref, bias=bias))
    lse_ref, mass_ref, sc = _REF[key]
    for fold in (False, True):
        aff = ops.adain_stats(v, rv, heads=H) if fold else None
        kw = dict(heads=H, scale=LC.SCALE, include_self=inc, adain=aff, q_prescaled=presc, key_bias=bias.cuda())
        name = ops.shared_attention_kernel_name(qs if presc else q, k, v, rk, rv, return_mass=True, **kw)
        assert "pipe_kernel" in name and "key bias" in name, name
        _, lse, mass = ops.shared_attention(qs if presc else q, k, v, rk, rv, return_lse=True, return_mass=True, **kw)
        what = f"bias {pattern} {'prescq' if presc else 'plainq'} {'fold' if fold else 'plain'} [{name}]"
        print(what, "lse ratio", LB.check_lse(lse, lse_ref, sc, what), "mass ratio", LB.check_mass(mass, mass_ref, sc, what))
        if pattern == "finite_one_entry_masked":
            assert bool(torch.isneginf(lse[B - 1]).all()) and float(mass[B - 1].abs().max()) == 0.0


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ragged_forms(ops, dtype, presc):
    """per-reference token counts: full, absent, one key past a tile / a single key, a whole tile, ragged"""
    x = LC.inputs(LC.BIASED, "n1", dtype)
    q, qs, k, v, rk, rv = _dev(x)
    B, H, Lq, Ls, N, Lr, inc = LC.BIASED
    bias = LC.tail_bias(LC.BIASED, LC.COUNTS)
    key = (id(x), "presc" if presc else "plain", "counts")
    if key not in _REF:
        qt = LC.q_true(x, presc)
        _, lse_ref, mass_ref = biased_attention_np(qt, LC.np64(x.k), LC.np64(x.v), LC.np64(x.rk), LC.np64(x.rv), H, LC.SCALE, bias,
                                                   train_input=inc, seg_lens=_seg_lens(LC.BIASED))
        _REF[key] = (lse_ref, mass_ref, LB.row_scale(qt, LB.pack_keys(x.k, x.rk, inc), LC.SCALE, lse_ref, bias=bias))
    lse_ref, mass_ref, sc = _REF[key]
    lens = torch.tensor(LC.COUNTS, dtype=torch.int32, device="cuda")
    for fold in (False, True):
        aff = ops.adain_stats(v, rv, heads=H) if fold else None
        kw = dict(heads=H, scale=LC.SCALE, include_self=inc, adain=aff, q_prescaled=presc, ref_lens=lens)
        name = ops.shared_attention_kernel_name(qs if presc else q, k, v, rk, rv, return_mass=True, **kw)
        assert "pipe_kernel" in name and "ragged refs" in name, name
        _, lse, mass = ops.shared_attention(qs if presc else q, k, v, rk, rv, return_lse=True, return_mass=True, **kw)
        what = f"counts {'prescq' if presc else 'plainq'} {'fold' if fold else 'plain'} [{name}]"
        print(what, "lse ratio", LB.check_lse(lse, lse_ref, sc, what), "mass ratio", LB.check_mass(mass, mass_ref, sc, what))
