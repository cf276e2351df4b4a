"""``ir_attn_key_match`` on the GPU: per key, the largest attention probability over ALL query rows and the lowest row that attains it.

What is held to what:
  1. the library's own read-outs, with NO tolerance.  Head mean: ``prob`` is the maximum over the rows of
     ``attn_rows(all rows, reduce="head_mean")`` with ``torch.equal`` and ``index`` its first argmax (``_first_argmax`` of
     tests/test_gpu_attn_match.py: no library's tie rule).  Per head, at the smallest cases: the whole fp32 matrix is assembled bit
     for bit from ``attn_received`` with one-hot weight channels, 8 rows per call, and ``prob`` / ``index`` equal its column maximum /
     first argmax.  Per head, every case: ``prob`` rounded to the 16-bit type is ``attn_probs(...).max(-2)`` and the dump's element
     at ``index`` is that maximum;
  2. the float64 oracle, with ``TOL`` of tests/test_gpu_attn_rows.py used as tests/test_gpu_attn_match.py uses it:
     ``|prob - p64[index, j]| <= TOL`` and ``p64[index, j] >= max_i p64[i, j] - 2 TOL``; and under the relative fp32 bound of
     tests/prob_bounds.py (reference B): ``prob`` at the returned row element by element, the row under its index rule;
  3. planted cases with exact indices: ties between rows (the LSE is written, not computed), the winner in the last row before the
     padding, a column of zeros, one query row;
  4. ``torch.equal`` with the plain call: pointer tables, pre-scaled Q, ``batch_invariant``, an entry of a batch alone, a replayed
     graph, the processor attribute, one placement beyond 32-bit element offsets;
  5. the mutual check end to end against the NumPy restatement on the assembled fp32 matrix.
The inputs, the LSE and the float64 probabilities of a (case, dtype) are computed once and shared by the tests that need them."""
import functools

import numpy as np
import pytest
import torch

import oracle_ops_key_match as K
from test_gpu_attn_match import _first_argmax
import prob_bounds as PB
from test_gpu_attn_rows import CASES, ODD_CASES, TOL, _case_inputs, _gpu_lse, _ids, _oracle_probs, _oracle_side, _rand
from test_gpu_ref_table import _pool_grid, _stack

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["f16", "bf16"]
FORMS = ("none", "head_mean")
LN2 = 0.6931471805599453

# B, H, Lq, Ls, N, Lr, include_self: what CASES / ODD_CASES leave out of len_q 1 / 33 / 40 / 100, segment lengths 1 / 40 / 96 / 97 /
# 200 (a 64-key group: one whole, one and a half, one and a key, three and a quarter), with and without the self block, no
# references at 77 keys (the cross-attention shape) and 3, H 1 / 5 / 20
SMALL_CASES = [
    (1, 1, 1, 1, 3, 40, True),         # one query row, a self segment of one key
    (2, 5, 33, 97, 3, 96, True),       # one row behind a whole block; 64 + 33 keys; a reference of whole blocks
    (1, 2, 40, 200, 3, 1, True),       # references of one key each
    (1, 1, 100, 77, 0, 0, True),       # no references, 77 keys
    (1, 20, 40, 40, 1, 97, True),      # twenty heads at a tiny shape
    (2, 5, 100, 96, 3, 200, False),    # without the self block
    (1, 1, 1, 40, 3, 97, False),       # one query row without the self block
]
ALL_CASES = CASES + ODD_CASES + SMALL_CASES
EXACT_CASES = ODD_CASES + SMALL_CASES                       # the whole fp32 matrix is assembled for these


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


@functools.lru_cache(maxsize=None)
def _setup(case, dtype):
    """device tensors, the LSE of the fused forward and the oracle's float64 probabilities of one case: computed once, never changed"""
    from instantrestore_amd import ops
    B, H, Lq, Ls, N, Lr, inc = case
    q, k, v, rk, rv = _case_inputs(case, dtype)
    qd, kd, rkd, lse = _gpu_lse(ops, q, k, v, rk, rv, H, inc)
    E, delta = _oracle_side(q, k, rk, H, inc)
    return dict(q=qd, k=kd, rk=rkd, lse=lse, p64=_oracle_probs(q, k, v, rk, rv, H, inc), E=E, delta=delta, edges=K.segment_edges(Ls, N, Lr, inc),
                kw=dict(heads=H, scale=0.125, include_self=inc))


def _fp32_matrix(ops, q, k, rk, lse, **kw):
    """the fp32 p of every (row, key), (B, H, Lq, Lkv), bit for bit: a one-hot weight channel at row i makes ``attn_received`` return
    that row's fp32 probabilities at every key (its header: adding exact zeros changes nothing); 8 rows per call"""
    B, Lq = q.shape[0], q.shape[1]
    parts = []
    for i0 in range(0, Lq, 8):
        n = min(8, Lq - i0)
        w = torch.zeros(1, Lq, n, device="cuda")                 # three axes: (L, C) would read as (B, L) where both fit
        w[0, i0:i0 + n] = torch.eye(n, device="cuda")
        parts.append(ops.attn_received(q, k, rk, lse, w, reduce="none", **kw).transpose(-1, -2))      # (B, H, n, Lkv)
    return torch.cat(parts, dim=2)


@functools.lru_cache(maxsize=None)
def _exact(case, dtype):
    from instantrestore_amd import ops
    s = _setup(case, dtype)
    return _fp32_matrix(ops, s["q"], s["k"], s["rk"], s["lse"], **s["kw"])


def _inv_h(H):
    """1.0f / (float)H, one fp32 division"""
    return torch.tensor(1.0, dtype=torch.float32, device="cuda") / torch.tensor(float(H), dtype=torch.float32, device="cuda")


def _col_first_argmax(x):
    """(..., L, Lkv) -> (column maximum, the lowest row that holds it), both (..., Lkv)"""
    return _first_argmax(x.transpose(-1, -2))


def _check_shapes(index, prob, B, H, Lq, lkv, form, what):
    shape = (B, H, lkv) if form == "none" else (B, lkv)
    assert tuple(index.shape) == shape and tuple(prob.shape) == shape, what
    assert index.dtype == torch.int32 and prob.dtype == torch.float32 and index.is_contiguous() and prob.is_contiguous()
    assert int(index.min()) >= 0 and int(index.max()) < Lq, f"{what}: index outside [0, len_q)"
    assert bool(torch.isfinite(prob).all()) and float(prob.min()) >= 0


# ---- 1: the library's own read-outs, no tolerance ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_head_mean_is_the_column_maximum_of_the_rows_readout_bit_for_bit(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    what = f"{_ids([case])[0]} {dtype}"
    hm = ops.attn_rows(s["q"], s["k"], s["rk"], s["lse"], torch.arange(Lq), reduce="head_mean", **s["kw"])      # (B, Lq, Lkv) fp32
    index, prob = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce="head_mean", **s["kw"])
    _check_shapes(index, prob, B, H, Lq, s["edges"][-1], "head_mean", what)
    m, first = _col_first_argmax(hm)
    assert torch.equal(prob, m), f"{what}: head-mean prob is not the maximum of the head-mean rows bit for bit"
    assert torch.equal(index.long(), first), f"{what}: head-mean index is not the first argmax"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", EXACT_CASES, ids=_ids(EXACT_CASES))
def test_per_head_equals_the_assembled_fp32_matrix(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    what = f"{_ids([case])[0]} {dtype}"
    p32 = _exact(case, dtype)
    assert tuple(p32.shape) == (B, H, Lq, s["edges"][-1]) and p32.dtype == torch.float32
    index, prob = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce="none", **s["kw"])
    _check_shapes(index, prob, B, H, Lq, s["edges"][-1], "none", what)
    m, first = _col_first_argmax(p32)
    assert torch.equal(prob, m), f"{what}: per-head prob is not the column maximum of the fp32 matrix"
    assert torch.equal(index.long(), first), f"{what}: per-head index is not the first argmax of the fp32 matrix"
    # the head mean of that matrix, formed as the interface states it, gives the head-mean form as well
    acc = torch.zeros_like(p32[:, 0])
    for h in range(H):
        acc = acc + p32[:, h]
    m1, first1 = _col_first_argmax(acc * _inv_h(H))
    i1, p1 = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce="head_mean", **s["kw"])
    assert torch.equal(p1, m1) and torch.equal(i1.long(), first1), f"{what}: head mean of the fp32 matrix"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_per_head_against_the_dump(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    what = f"{_ids([case])[0]} {dtype}"
    dump = ops.attn_probs(s["q"], s["k"], s["rk"], s["lse"], **s["kw"])                                   # (B, H, Lq, Lkv)
    index, prob = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce="none", **s["kw"])
    _check_shapes(index, prob, B, H, Lq, s["edges"][-1], "none", what)
    best = dump.max(-2).values
    assert torch.equal(prob.to(dtype), best), f"{what}: prob rounded to the 16-bit type is not the dump's column maximum"
    assert torch.equal(dump.gather(-2, index.long()[:, :, None, :])[:, :, 0], best), f"{what}: the dump's element at index is not the maximum"


# ---- 2: the float64 oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_against_the_float64_oracle(ops, case, dtype):
    s = _setup(case, dtype)
    tol = TOL[dtype]
    for form in FORMS:
        index, prob = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce=form, **s["kw"])
        index, prob = index.cpu().numpy().astype(np.int64), prob.cpu().numpy().astype(np.float64)
        x = s["p64"].mean(axis=1) if form == "head_mean" else s["p64"]
        best, _ = K.key_match_of_matrix_np(x)
        at = np.take_along_axis(x, index[..., None, :], axis=-2)[..., 0, :]                       # p64[index, j]
        worst_v, worst_gap = float(np.abs(prob - at).max()), float((best - at).max())
        print(f"attn_key_match {_ids([case])[0]} {dtype} {form}: max |prob - p64[index, j]| {worst_v:.3e} (bound {tol:.0e}), "
              f"max (max_i p64 - p64[index, j]) {worst_gap:.3e} (bound {2 * tol:.0e})")
        assert worst_v <= tol and worst_gap <= 2 * tol, (form, worst_v, worst_gap)
        t = lambda a: np.swapaxes(a, -1, -2)                                  # the query axis as the one segment of every key
        cal, der, ref = (*PB.terms(t(s["p64"]), t(s["E"]), None, t(s["delta"])), t(s["p64"]))
        if form == "head_mean":
            cal, der, ref = PB.head_mean_terms(cal, der, ref)
        PB.check_ranked(index[..., None, None], prob[..., None, None], ref, cal, der, [0, s["p64"].shape[2]], np.zeros(ref.shape[:-1], dtype=bool),
                        f"attn_key_match {_ids([case])[0]} {dtype} {form}", kind=f"key_match_{form}B")


# ---- 3: planted cases, exact indices ---------------------------------------------------------------------------------------------
def _plant_rows(dtype, B, H, Lq, Ls, N, Lr, rows_keys, seed):
    """quiet query rows (randn * 0.5) except the planted ones (randn * 1.5); for every (row, self keys, reference keys) the keys are
    copies of that query row on every head: its score there is |q|^2 / 8, about 18, against a spread of 2.25 elsewhere in the row -
    the row hands nearly all of its attention to its few planted keys - while a quiet row's score on them spreads by 0.75 under an
    LSE near log(Lkv): a planted row wins its keys' columns by a factor of five or more, in every head and so in the head mean"""
    gen = torch.Generator().manual_seed(seed)
    Cc = H * 64
    q = _rand((B, Lq, Cc), dtype, gen, 0.5)
    k, v = _rand((B, Ls, Cc), dtype, gen, 1.5), _rand((B, Ls, Cc), dtype, gen)
    rk, rv = _rand((B, N, Lr, Cc), dtype, gen, 1.5), _rand((B, N, Lr, Cc), dtype, gen)
    for row, self_keys, ref_keys in rows_keys:
        q[:, row] = _rand((B, Cc), dtype, gen, 1.5)
        for j in self_keys:
            k[:, j] = q[:, row]
        for j in ref_keys:
            rk[:, :, j] = q[:, row, None]
    return tuple(t.cuda() for t in (q, k, v, rk, rv))


TIE_PAIRS = [(3, 35), (4, 5), (6, 22), (7, 71)]      # same lane in the next block; neighbouring lanes; across the last butterfly step; two blocks on


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ties_go_to_the_lowest_row_in_both_forms(ops, dtype):
    B, H, Lq, Ls, N, Lr = 2, 2, 100, 100, 2, 97
    # pair n owns self keys 5 + n, 40 + n, 70 + n and reference keys n, 33 + n, 96 - n: both half-waves, both key blocks of a
    # group, the second group and its partial last block
    plan = [(i1, [5 + n, 40 + n, 70 + n], [n, 33 + n, 96 - n]) for n, (i1, _) in enumerate(TIE_PAIRS)]
    q, k, v, rk, rv = _plant_rows(dtype, B, H, Lq, Ls, N, Lr, plan, seed=47)
    for i1, i2 in TIE_PAIRS:
        q[:, i2] = q[:, i1]
    kw = dict(heads=H, scale=0.125, include_self=True)
    _, lse = ops.shared_attention(q, k, v, rk, rv, return_lse=True, **kw)
    lse = lse.clone()
    for i1, i2 in TIE_PAIRS:
        lse[:, :, i2] = lse[:, :, i1]                   # identical q and identical lse: identical fp32 probabilities at every key
    p32 = _fp32_matrix(ops, q, k, rk, lse, **kw)
    for i1, i2 in TIE_PAIRS:
        assert torch.equal(p32[:, :, i1], p32[:, :, i2])                                          # the tie is real
    for form in FORMS:
        index, prob = ops.attn_key_match(q, k, rk, lse, reduce=form, **kw)
        assert not any(bool((index == i2).any()) for _, i2 in TIE_PAIRS), f"{form}: the higher row of a tied pair was chosen somewhere"
        for (i1, i2), (_, self_keys, ref_keys) in zip(TIE_PAIRS, plan):
            cols = self_keys + [Ls + n * Lr + j for n in range(N) for j in ref_keys]
            got = index[..., cols]
            assert bool((got == i1).all()), f"{form} pair {(i1, i2)}: got rows {got.unique().tolist()} at its keys"
            assert float(prob[..., cols].min()) > 0.05, f"{form} pair {(i1, i2)}: the planted pair does not own its keys"
    m, first = _col_first_argmax(p32)
    i0, p0 = ops.attn_key_match(q, k, rk, lse, reduce="none", **kw)
    assert torch.equal(p0, m) and torch.equal(i0.long(), first)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_winner_in_the_last_row_before_the_padding(ops, dtype):
    """len_q 33: row 32 is the only row of the second 32-row block; the 31 padded rows beside it read it again and never take part"""
    B, H, Lq, Ls, N, Lr = 1, 2, 33, 40, 2, 97
    self_keys, ref_keys = [0, 17, 39], [15, 64, 96]
    q, k, v, rk, rv = _plant_rows(dtype, B, H, Lq, Ls, N, Lr, [(32, self_keys, ref_keys)], seed=53)
    kw = dict(heads=H, scale=0.125, include_self=True)
    _, lse = ops.shared_attention(q, k, v, rk, rv, return_lse=True, **kw)
    cols = self_keys + [Ls + n * Lr + j for n in range(N) for j in ref_keys]
    for form in FORMS:
        index, prob = ops.attn_key_match(q, k, rk, lse, reduce=form, **kw)
        assert bool((index[..., cols] == 32).all()), (form, index[..., cols].unique().tolist())
        assert int(index.max()) == 32 and int(index.min()) >= 0 and float(prob[..., cols].min()) > 0.05


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_a_column_of_zeros_gives_row_zero_and_probability_zero(ops, dtype):
    """lse = +200 on every row: every exponent is far below the smallest fp32 number, every probability is 0"""
    for case in (ODD_CASES[0], SMALL_CASES[1], SMALL_CASES[5]):
        s = _setup(case, dtype)
        lse = torch.full_like(s["lse"], 200.0)
        for form in FORMS:
            index, prob = ops.attn_key_match(s["q"], s["k"], s["rk"], lse, reduce=form, **s["kw"])
            assert bool((prob == 0).all()) and bool((index == 0).all()), (case, form)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_one_query_row(ops, dtype):
    for case in (SMALL_CASES[0], SMALL_CASES[6]):
        s = _setup(case, dtype)
        row = torch.zeros(1, dtype=torch.int32)
        i0, p0 = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce="none", **s["kw"])
        i1, p1 = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce="head_mean", **s["kw"])
        assert bool((i0 == 0).all()) and bool((i1 == 0).all())
        assert torch.equal(p0.to(dtype), ops.attn_rows(s["q"], s["k"], s["rk"], s["lse"], row, reduce="none", **s["kw"])[:, :, 0])
        assert torch.equal(p1, ops.attn_rows(s["q"], s["k"], s["rk"], s["lse"], row, reduce="head_mean", **s["kw"])[:, 0])
        assert torch.equal(p0, _exact(case, dtype)[:, :, 0])


# ---- 4: torch.equal with the plain call ------------------------------------------------------------------------------------------
def _same(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_pointer_tables_equal_the_dense_call(ops, dtype):
    B, H, Lq, N, Lr = 2, 2, 100, 3, 97
    g = torch.Generator().manual_seed(13)
    q, ks, vs = (torch.randn(B, Lq, H * 64, generator=g).to("cuda", dtype) for _ in range(3))
    gk, gv = _pool_grid(g, B, N, Lr, H * 64, dtype)
    dk, dv = _stack(gk), _stack(gv)
    tk = ops.RefKVTable.from_tensors(gk)
    for inc in (True, False):
        kw = dict(heads=H, scale=0.125, include_self=inc)
        _, lse = ops.shared_attention(q, ks, vs, dk, dv, return_lse=True, **kw)
        for form in FORMS:
            _same(ops.attn_key_match(q, ks, tk, lse, reduce=form, **kw), ops.attn_key_match(q, ks, dk, lse, reduce=form, **kw), (form, inc))


def test_graph_replay_follows_q_and_the_table(ops):
    dtype = torch.bfloat16
    B, H, Lq, N, Lr = 2, 2, 100, 3, 72
    g = torch.Generator().manual_seed(9)
    q0, q1, ks, vs = (torch.randn(B, Lq, H * 64, generator=g).to("cuda", dtype) for _ in range(4))
    gk0, gv0 = _pool_grid(g, B, N, Lr, H * 64, dtype)
    gk1, gv1 = _pool_grid(g, B, N, Lr, H * 64, dtype, scale=0.7, shift=0.1)
    kw = dict(heads=H, scale=0.125, include_self=True)
    lse0 = ops.shared_attention(q0, ks, vs, _stack(gk0), _stack(gv0), return_lse=True, **kw)[1]
    lse1 = ops.shared_attention(q1, ks, vs, _stack(gk1), _stack(gv1), return_lse=True, **kw)[1]
    for form in FORMS:
        tk = ops.RefKVTable.from_tensors(gk0)
        static_q, static_lse = q0.clone(), lse0.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.attn_key_match(static_q, ks, tk, static_lse, reduce=form, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.attn_key_match(static_q, ks, tk, static_lse, reduce=form, **kw)
        graph.replay()
        torch.cuda.synchronize()
        want0 = ops.attn_key_match(q0, ks, _stack(gk0), lse0, reduce=form, **kw)
        _same(out, want0, form)
        static_q.copy_(q1)
        static_lse.copy_(lse1)
        tk.fill_(gk1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want1 = ops.attn_key_match(q1, ks, _stack(gk1), lse1, reduce=form, **kw)
        _same(out, want1, form)
        assert not torch.equal(want0[0], want1[0])
        del graph


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_prescaled_q(ops, dtype):
    """IR_FLAG_Q_PRESCALED: the products of the pre-scaled query and k ARE the exponents.  The plain call on that rounded query
    with scale = ln 2 forms scale * log2(e) = 1 in fp32 and so the same bytes; the flagged head mean agrees with the rows read-out
    under the flag"""
    B, H, L, N, Lr = 2, 2, 72, 3, 40
    gen = torch.Generator().manual_seed(11)
    q = _rand((B, L, H * 64), dtype, gen, 1.5)
    qs = (q.float() * (0.125 * 1.4426950408889634)).to(dtype).cuda()
    k, v = _rand((B, L, H * 64), dtype, gen, 1.5).cuda(), _rand((B, L, H * 64), dtype, gen).cuda()
    rk, rv = _rand((B, N, Lr, H * 64), dtype, gen, 1.5).cuda(), _rand((B, N, Lr, H * 64), dtype, gen).cuda()
    _, lse = ops.shared_attention(qs, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True, q_prescaled=True)
    for form in FORMS:
        flagged = ops.attn_key_match(qs, k, rk, lse, heads=H, scale=0.125, include_self=True, reduce=form, q_prescaled=True)
        _same(flagged, ops.attn_key_match(qs, k, rk, lse, heads=H, scale=LN2, include_self=True, reduce=form), form)
    hm = ops.attn_rows(qs, k, rk, lse, torch.arange(L), heads=H, scale=0.125, include_self=True, reduce="head_mean", q_prescaled=True)
    m, first = _col_first_argmax(hm)
    assert torch.equal(flagged[1], m) and torch.equal(flagged[0].long(), first)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_batch_invariance(ops, dtype):
    """entry b of a batch of 3 equals the same entry run alone, in both forms, with and without the (accepted, inert) flag"""
    case = (3, 2, 72, 72, 3, 40, True)
    B = case[0]
    s = _setup(case, dtype)
    for form in FORMS:
        a = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce=form, **s["kw"])
        _same(a, ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce=form, batch_invariant=True, **s["kw"]), form)
        for b in range(B):
            one = ops.attn_key_match(s["q"][b:b + 1].contiguous(), s["k"][b:b + 1].contiguous(), s["rk"][b:b + 1].contiguous(),
                                     s["lse"][b:b + 1].contiguous(), reduce=form, **s["kw"])
            assert torch.equal(one[0][0], a[0][b]) and torch.equal(one[1][0], a[1][b]), (form, b)


def test_through_the_plugin_surface(ops, monkeypatch):
    """``attention_key_match_reduce`` on a shared layer: the result is ``ops.attn_key_match`` on that layer's q / k / lse (caught on
    their way into the call), agrees with the dump of the same forward, and leaves the layer output as it was bit for bit"""
    import instantrestore_amd.attn_processors as ap
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    from instantrestore_amd.attn_maps import mutual_matches
    seen = []
    real = ops.attn_key_match

    def spy(*a, **kw):
        seen.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ap._ops, "attn_key_match", spy)
    torch.manual_seed(4)
    B, H, L, N = 2, 2, 256, 3
    Cc = H * 64
    for train_input in (True, False):
        proc = SharedAttnProcessor(self_attn_idx=0, use_adain=True, train_input=train_input)
        attn = Attention(query_dim=Cc, heads=H, dim_head=64, processor=proc).cuda()
        x = torch.randn(B, L, Cc, device="cuda")
        rk = torch.randn(B, N, L, Cc, device="cuda", dtype=torch.bfloat16)
        rv = torch.randn(B, N, L, Cc, device="cuda", dtype=torch.bfloat16)
        run = lambda: attn(x, ref_keys=[rk], ref_values=[rv])
        S = N + int(train_input)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y0 = run()
            assert proc.attention_key_match is None and not seen
            proc.attention_key_match_reduce = "head_mean"
            y1 = run()
            assert len(seen) == 1
            (a, kw) = seen.pop()
            assert kw["reduce"] == "head_mean"
            index, prob = proc.attention_key_match
            want = real(*a, **kw)
            assert index.shape == (B, S * L) and torch.equal(index, want[0]) and torch.equal(prob, want[1]) and torch.equal(y0, y1)
            proc.attention_key_match_reduce, proc.save_self_attentions = "none", True
            proc.attention_match_index, proc.attention_match_reduce = "all", "none"
            run()
            seen.clear()
            i0, p0 = proc.attention_key_match
            dump = proc.attention_probs
            assert dump.shape == (B, H, L, S * L) and i0.shape == (B, H, S * L)
            best = dump.max(-2).values
            assert torch.equal(p0.to(dump.dtype), best) and torch.equal(dump.gather(-2, i0.long()[:, :, None, :])[:, :, 0], best)
            mutual = mutual_matches(proc.attention_match[0], i0, L, N, L, train_input)
            assert mutual.shape == (B, H, L, S) and mutual.is_cuda and bool(mutual.any()) and not bool(mutual.all())


def test_batch_stride_beyond_32_bit_element_offsets(ops):
    """q, K self and the references are views of one 8.5 GiB allocation whose batch strides exceed 2^32 elements, placed by
    tests/far_placement.py as tests/test_gpu_far_addresses.py places the other read-outs: a truncated offset reads fill pattern (NaN)
    inside the allocation, never another tensor and never outside it"""
    import test_gpu_far_addresses as FA
    dtype = torch.bfloat16
    B, H, Lq, N, Lr = FA.READOUT_SHAPE
    key = "readout/batch/A"
    assert FA.LAYOUTS[key][0][2][0] > 2 ** 32                       # q's batch stride in elements
    data = FA._attn_data(FA.READOUT_SHAPE, dtype, False, seed=len(key))
    _, lse = ops.shared_attention(data["q"], data["ks"], data["vs"], data["kr"], data["vr"], heads=H, scale=FA.SCALE, return_lse=True)
    arena = FA.Arena()
    try:
        arena.fill()
        placed, far_t = FA._put(arena, key, data)
        kw = dict(heads=H, scale=FA.SCALE, include_self=True)
        for form in FORMS:
            want = ops.attn_key_match(data["q"], data["ks"], data["kr"], lse, reduce=form, **kw)
            got = ops.attn_key_match(far_t["q"], far_t["ks"], far_t["kr"], lse, reduce=form, **kw)
            FA._same_small(got, want, f"{key} attn_key_match {form}")
        FA._settle(arena, placed, data, {}, f"{key} attn_key_match")
    finally:
        del arena
        torch.cuda.empty_cache()


# ---- 5: the mutual check end to end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [ODD_CASES[0], SMALL_CASES[1], SMALL_CASES[5]], ids=_ids([ODD_CASES[0], SMALL_CASES[1], SMALL_CASES[5]]))
def test_mutual_check_end_to_end(ops, case, dtype):
    from instantrestore_amd.attn_maps import mutual_matches
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    p32 = _exact(case, dtype)
    acc = torch.zeros_like(p32[:, 0])
    for h in range(H):
        acc = acc + p32[:, h]
    matrices = {"none": p32, "head_mean": acc * _inv_h(H)}
    for form in FORMS:
        mi, _ = ops.attn_match(s["q"], s["k"], s["rk"], s["lse"], None, reduce=form, **s["kw"])
        ki, _ = ops.attn_key_match(s["q"], s["k"], s["rk"], s["lse"], reduce=form, **s["kw"])
        got = mutual_matches(mi, ki, Ls, N, Lr, inc)
        x = matrices[form].cpu().numpy()
        want = K.mutual_np(K.match_of_matrix_np(x, s["edges"]), K.key_match_of_matrix_np(x)[1], s["edges"])
        assert got.is_cuda and got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), form
        assert want.any() and not want.all()
