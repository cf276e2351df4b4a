"""Every read-out probability on the GPU against float64, element by element, under the relative fp32 bound of
tests/prob_bounds.py (its docstring has the bound, the two references and the measured table).

Inputs: ``lse_cases.inputs(shape, family, dtype)`` with the families and shapes of ``prob_bounds.cases()`` - the smallest shapes at
which each store shape and each gather path of the read-outs exists:

    LC.PIPE32 (both entries)            72 rows; ragged 64-key steps; a partial row block
    LC.ODD (both entries)               nothing aligned, so the 2-byte-store kernel; a one-key reference
    LC.TAILS[0]                         rows not a multiple of 32; key tails of 8 and 48 keys
    LC.W64[1]                           576 rows, 3 x 192 keys, no self segment; more than one 256-row workgroup
    (2, 1, 64, 64, 8, 64, True)         eight references
    (1, 2, 96, 96, 0, 0, True)          no references
    (1, 1, 1024, 1024, 4, 1024, True)   family "n15" only; key chunks cut the segments

What is held, each against reference A (float64 with the device's LSE) and reference B (the oracle, with the per-row delta of
tests/lse_bounds.py):
  * ``attn_probs`` kernel "generic": every element under the 16-bit bound; "auto" and the five line kernels ``torch.equal`` to it;
  * ``attn_rows``: 1, 5 and 68 rows with duplicates and out-of-range indices, and all rows; form "none" under the 16-bit bound,
    "head_mean" and "map" under the reduced-form bounds;
  * ``attn_match`` (both forms), ``attn_topk`` (k = 1, 3, 8; both forms), ``attn_key_match`` (both forms): ``prob`` at the returned
    index under the fp32 bound (the head mean under its own), the index under the index rule, index -1 / prob 0 for an invalid row;
  * ``attn_received`` with one-hot weights, 8 rows per call: every key of those rows under the fp32 bound, and rounded to the 16-bit
    type ``torch.equal`` to the dump's rows;
  * ``attn_transfer`` with one-hot payload channels at 8 keys of a segment (its first and last among them): the fp32 bound at those
    keys, exactly 0 in the other segments;
  * IR_FLAG_Q_PRESCALED (the LSE of the pre-scaled forward, reference A from ln2 * <qs, k>): probs, rows, match and received at
    ``prob_bounds.PRESC_SHAPES``.
Pointer tables are held to the dense bytes elsewhere.  The inputs, the LSE and the references of a (shape, family, dtype, flag) are
computed once and never changed.  Each comparison prints its largest ratio before it asserts (``pytest -s``); IR_PARITY_LOG=<file>
appends a record per comparison."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lse_cases as LC
import prob_bounds as PB
from test_gpu_attn_rows import _indices
from test_gpu_probs import LINE_KERNELS

pytestmark = pytest.mark.gpu

DT = {torch.float16: "f16", torch.bfloat16: "bf16"}
PLAIN = [(s, f, False) for (s, f) in PB.cases()]
ALL = PLAIN + [(s, f, True) for (s, f) in PB.presc_cases()]
FORMS = ("none", "head_mean")
KS = (1, 3, 8)


def _cid(c):
    return f"{LC.sid(c[0])}-{c[1]}-{'prescq' if c[2] else 'plainq'}"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


@functools.lru_cache(maxsize=None)
def _setup(shape, family, presc, dtype):
    """device tensors, the LSE of the fused forward and both float64 references of one input set: computed once, never changed"""
    from instantrestore_amd import ops
    B, H, Lq, Ls, N, Lr, inc = shape
    x, qt, keys, s, T, lse_ref = PB.case_reference(shape, family, dtype, presc)
    d = lambda t: None if t is None else t.cuda()
    q, k, v, rk, rv = d(x.qs if presc else x.q), d(x.k), d(x.v), d(x.rk), d(x.rv)
    kw = dict(heads=H, scale=LC.SCALE, include_self=inc, **({"q_prescaled": True} if presc else {}))
    _, lse = ops.shared_attention(q, k, v, rk, rv, return_lse=True, **kw)
    lse_dev = lse.double().cpu().numpy()
    assert lse_dev.shape == lse_ref.shape and np.isfinite(lse_dev).all()
    delta = np.broadcast_to(PB.lse_delta(qt, keys, LC.SCALE, lse_ref, presc)[..., None], s.shape)
    refs = {"A": (PB.probs_given_lse(s, lse_dev), PB.elem_scale(T, lse_dev), None),
            "B": (PB.probs_given_lse(s, lse_ref), PB.elem_scale(T, lse_ref), delta)}
    lens = LC.seg_lens(shape)
    return SimpleNamespace(q=q, k=k, rk=rk, lse=lse, kw=kw, refs=refs, edges=[0] + list(np.cumsum(lens)), lens=lens, klass=PB.klass_of(presc),
                           B=B, H=H, Lq=Lq, lkv=s.shape[-1], what=f"{_cid((shape, family, presc))} {DT[dtype]}")


@functools.lru_cache(maxsize=None)
def _dump(shape, family, presc, dtype):
    from instantrestore_amd import ops
    c = _setup(shape, family, presc, dtype)
    return ops.attn_probs(c.q, c.k, c.rk, c.lse, kernel="generic", **c.kw)


def _row_lists(B, Lq):
    """(B, R) int32 index lists: 1, 5 and 68 rows with forced duplicates - the longer two with an index of Lq and, in the last
    entry, of -1 - and every row"""
    out = []
    for R in sorted({min(r, Lq) for r in (1, 5, 68)}):
        idx = _indices(B, Lq, R, seed=100 + R)
        if R >= 5:
            idx[:, 3] = Lq
            idx[B - 1, 4] = -1
        out.append(idx)
    return out + [torch.arange(Lq, dtype=torch.int32).expand(B, -1).contiguous()]


def _rows_of(arr, idx, fill):
    """(B, H, Lq, Lkv) -> (B, H, R, Lkv): the rows ``idx`` (B, R) of every entry, ``fill`` on the rows of an invalid index"""
    Lq = arr.shape[2]
    ok = (idx >= 0) & (idx < Lq)
    safe = np.where(ok, idx, 0)
    out = np.stack([arr[b][:, safe[b]] for b in range(arr.shape[0])])
    return np.where(ok[:, None, :, None], out, fill)


def _row_refs(c, idx):
    """name -> (ref, E, delta) on the rows ``idx``, and the (B, R) mask of the invalid ones"""
    idx = idx.numpy().astype(np.int64)
    bad = (idx < 0) | (idx >= c.Lq)
    refs = {}
    for name, (p, E, delta) in c.refs.items():
        refs[name] = (_rows_of(p, idx, 0.0), _rows_of(E, idx, 1.0), None if delta is None else _rows_of(delta, idx, 0.0))
    return refs, bad


def _hm(terms3, ref):
    return PB.head_mean_terms(terms3[0], terms3[1], ref, axis=1)


def _held(c, dtype, got, take, what, dtype_out=None):
    """one device result of per-head probabilities against both references; ``take`` cuts the (B, H, Lq, Lkv) arrays to its shape"""
    for name, (p, E, delta) in c.refs.items():
        PB.check_probs(got, take(p), take(E), dtype_out, f"{c.what} {what} ref {name}", delta=None if delta is None else take(delta), klass=c.klass)


# ---- the dump -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PB.DTYPES, ids=list(DT.values()))
@pytest.mark.parametrize("case", ALL, ids=[_cid(c) for c in ALL])
def test_probs_generic_every_element_and_the_other_kernels_equal_it(ops, case, dtype):
    c = _setup(*case, dtype)
    dump = _dump(*case, dtype)
    assert tuple(dump.shape) == (c.B, c.H, c.Lq, c.lkv) and dump.dtype == dtype
    _held(c, dtype, dump, lambda a: a, "attn_probs generic", dtype_out=dtype)
    assert torch.equal(ops.attn_probs(c.q, c.k, c.rk, c.lse, **c.kw), dump), f"{c.what}: auto differs from the 2-byte-store kernel"
    if all(n % 8 == 0 for n in c.lens):
        for kern in LINE_KERNELS:
            assert torch.equal(ops.attn_probs(c.q, c.k, c.rk, c.lse, kernel=kern, **c.kw), dump), f"{c.what}: {kern} differs from the 2-byte-store kernel"


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PB.DTYPES, ids=list(DT.values()))
@pytest.mark.parametrize("case", ALL, ids=[_cid(c) for c in ALL])
def test_rows_three_forms(ops, case, dtype):
    c = _setup(*case, dtype)
    for idx in _row_lists(c.B, c.Lq):
        R = idx.shape[1]
        refs, bad = _row_refs(c, idx)
        got = {f: ops.attn_rows(c.q, c.k, c.rk, c.lse, idx.cuda(), reduce=f, **c.kw) for f in ("none", "head_mean", "map")}
        assert got["none"].dtype == dtype and got["head_mean"].dtype == torch.float32 and got["map"].dtype == torch.float32
        for name, (p, E, delta) in refs.items():
            what = f"{c.what} attn_rows R={R} ref {name}"
            PB.check_probs(got["none"], p, E, dtype, what + " none", delta=delta, klass=c.klass, dead=bad[:, None, :, None])
            cal, der, ref = _hm(PB.terms(p, E, None, delta, c.klass), p)
            PB.check_terms(got["head_mean"], ref, cal, der, what + " head_mean", c.klass, "head_mean" + name, dead=bad[:, :, None])
            cal2, der2, ref2 = PB.map_terms(cal, der, ref, axis=1)
            PB.check_terms(got["map"], ref2, cal2, der2, what + " map", c.klass, "map" + name)


# ---- match, topk, key_match: the value at the returned index, and the index --------------------------------------------------------------
def _ranked_both_forms(c, refs, bad, calls, edges, what, kind):
    """``calls``: label -> ``call(form)`` -> (index, prob) with the rank axis last (at most max(KS) ranks), held in both forms
    against every reference in ``refs``; the terms and the sorted references of a (form, reference) are formed once"""
    for form in FORMS:
        got = {label: call(form) for label, call in calls.items()}
        for name, (p, E, delta) in refs.items():
            cal, der = PB.terms(p, E, None, delta, c.klass)
            ref, b = p, np.broadcast_to(bad[:, None], p.shape[:-1])
            if form == "head_mean":
                cal, der, ref = PB.head_mean_terms(cal, der, p, axis=1)
                b = bad
            tops = {}
            for label, (index, prob) in got.items():
                assert index.dtype == torch.int32 and prob.dtype == torch.float32
                PB.check_ranked(index, prob, ref, cal, der, edges, b, f"{what}{label} {form} ref {name}", c.klass, f"{kind}_{form}{name}", tops)


@pytest.mark.parametrize("dtype", PB.DTYPES, ids=list(DT.values()))
@pytest.mark.parametrize("case", ALL, ids=[_cid(c) for c in ALL])
def test_match_value_and_index(ops, case, dtype):
    c = _setup(*case, dtype)
    lists = _row_lists(c.B, c.Lq)
    for n, idx in enumerate(lists):
        refs, bad = _row_refs(c, idx)
        rows = None if n == len(lists) - 1 else idx.cuda()                  # the last list is every row: the call's own default
        call = lambda form: tuple(t[..., None] for t in ops.attn_match(c.q, c.k, c.rk, c.lse, rows, reduce=form, **c.kw))
        _ranked_both_forms(c, refs, bad, {"": call}, c.edges, f"{c.what} attn_match R={idx.shape[1]}", "match")


@pytest.mark.parametrize("dtype", PB.DTYPES, ids=list(DT.values()))
@pytest.mark.parametrize("case", PLAIN, ids=[_cid(c) for c in PLAIN])
def test_topk_values_and_indices(ops, case, dtype):
    c = _setup(*case, dtype)
    lists = _row_lists(c.B, c.Lq)
    for n, idx in enumerate(lists):
        refs, bad = _row_refs(c, idx)
        rows = None if n == len(lists) - 1 else idx.cuda()
        calls = {f" k={k}": (lambda form, k=k: ops.attn_topk(c.q, c.k, c.rk, c.lse, rows, k=k, reduce=form, **c.kw)) for k in KS}
        _ranked_both_forms(c, refs, bad, calls, c.edges, f"{c.what} attn_topk R={idx.shape[1]}", "topk")


@pytest.mark.parametrize("dtype", PB.DTYPES, ids=list(DT.values()))
@pytest.mark.parametrize("case", PLAIN, ids=[_cid(c) for c in PLAIN])
def test_key_match_value_and_index(ops, case, dtype):
    """the query axis takes the place of the key axis: one segment of Lq rows per key"""
    c = _setup(*case, dtype)
    t = lambda a: None if a is None else np.swapaxes(a, -1, -2)             # (B, H, Lkv, Lq)
    refs = {name: (t(p), t(E), t(delta)) for name, (p, E, delta) in c.refs.items()}
    bad = np.zeros((c.B, c.lkv), dtype=bool)
    call = lambda form: tuple(x[..., None, None] for x in ops.attn_key_match(c.q, c.k, c.rk, c.lse, reduce=form, **c.kw))
    _ranked_both_forms(c, refs, bad, {"": call}, [0, c.Lq], f"{c.what} attn_key_match", "key_match")


# ---- received and transfer: the fp32 window on P ---------------------------------------------------------------------------------------
def _window_rows(Lq, seed):
    """8 rows: 0, 31, 32, the last, the first and last rows of the partial (else the last whole) 32-row block, then seeded rows"""
    first = (Lq // 32) * 32 if Lq % 32 else Lq - 32
    rows = [r for r in dict.fromkeys([0, 31, 32, Lq - 1, first]) if 0 <= r < Lq]
    rng = np.random.default_rng(seed)
    while len(rows) < 8:
        rows.append(int(rng.integers(0, Lq)))
    return rows


@pytest.mark.parametrize("dtype", PB.DTYPES, ids=list(DT.values()))
@pytest.mark.parametrize("case", ALL, ids=[_cid(c) for c in ALL])
def test_received_one_hot_rows(ops, case, dtype):
    c = _setup(*case, dtype)
    rows = _window_rows(c.Lq, seed=7 + c.Lq + LC.seed_offset())
    w = torch.zeros(1, c.Lq, 8, device="cuda")
    for ch, r in enumerate(rows):
        w[0, r, ch] = 1.0
    recv = ops.attn_received(c.q, c.k, c.rk, c.lse, w, reduce="none", **c.kw)              # (B, H, Lkv, 8)
    assert tuple(recv.shape) == (c.B, c.H, c.lkv, 8) and recv.dtype == torch.float32
    p32 = recv.transpose(-1, -2).contiguous()                                               # (B, H, 8, Lkv): whole rows of the fp32 P
    _held(c, dtype, p32, lambda a: a[:, :, rows], f"attn_received rows {rows}")
    assert torch.equal(p32.to(dtype), _dump(*case, dtype)[:, :, rows]), f"{c.what}: the fp32 rows rounded to the 16-bit type are not the dump's rows"


@pytest.mark.parametrize("dtype", PB.DTYPES, ids=list(DT.values()))
@pytest.mark.parametrize("case", PLAIN, ids=[_cid(c) for c in PLAIN])
def test_transfer_one_hot_keys(ops, case, dtype):
    c = _setup(*case, dtype)
    rng = np.random.default_rng(11 + c.lkv + LC.seed_offset())
    S = len(c.lens)
    for si, (a, b) in enumerate(zip(c.edges[:-1], c.edges[1:])):
        keys = [a, b - 1] + [int(j) for j in rng.integers(a, b, size=6)]                   # the segment's first and last key among them
        payload = torch.zeros(c.lkv, 8, device="cuda")
        for ch, j in enumerate(keys):
            payload[j, ch] = 1.0
        sums, mass = ops.attn_transfer(c.q, c.k, c.rk, c.lse, payload, reduce="none", **c.kw)   # (B, H, Lq, S, 8)
        assert tuple(sums.shape) == (c.B, c.H, c.Lq, S, 8) and sums.dtype == torch.float32
        _held(c, dtype, sums[..., si, :], lambda x: x[..., keys], f"attn_transfer segment {si} keys {keys}")
        others = [s for s in range(S) if s != si]
        assert bool((sums[..., others, :] == 0).all()), f"{c.what}: a payload inside segment {si} shows in another segment"
