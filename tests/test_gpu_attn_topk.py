"""``ir_attn_topk`` on the GPU: per K/V segment, the k largest attention probabilities of chosen query tokens and the keys that
attain them, under the total order (probability descending, key ascending).

What is held to what:
  1. ``ir_attn_match``, with NO tolerance: rank 0 IS the match of the same call, index and prob, in both forms;
  2. the library's own rows, with NO tolerance: the head-mean ranks are a stable descending sort of ``attn_rows(reduce="head_mean")``'s
     row segment, values and indices; the per-head ``prob`` rounded to the 16-bit format holds ``torch.topk`` of
     ``attn_rows(reduce="none")``'s segment (rounding is monotone: the k largest rounded values are the rounded k largest), the row
     gathered at ``index`` has exactly that value, the indices are distinct and in range, the fp32 ``prob`` does not increase over the
     ranks and among equal fp32 ``prob`` the indices ascend.  Ranks beyond the segment's keys are ``-1`` / ``0``;
  3. the float64 oracle, with ``TOL`` of tests/test_gpu_probs.py (1e-3 fp16 / 8e-3 bf16, the project's stated bound for
     probabilities): for every rank t ``|prob_t - p64[index_t]| <= TOL`` and ``p64[index_t] >= (t-th largest p64) - 2 TOL`` (every
     key is within TOL, and an order statistic moves by at most the sup-norm error - hence twice); and under the relative fp32
     bound of tests/prob_bounds.py (reference B): every ``prob_t`` at its returned index, every index under the index rule;
  4. planted graded winners and ties: exact indices; row groups against calls of one row; invalid rows;
  5. pointer tables, pre-scaled Q, graph replay, batch invariance, the processor, repeated calls: ``torch.equal`` with the plain call.
The inputs, the LSE and the float64 probabilities of a (case, dtype) are computed once and shared by the tests that need them.

Measured on an MI355X, the worst over every case, row list and k: ``|prob_t - p64[index_t]|`` 1.0e-6 (fp16) / 8.4e-7 (bf16) per
head, 6.7e-7 / 8.4e-7 of the head mean; ``(t-th largest p64) - p64[index_t]`` 1.5e-9 (fp16, per head), 0 everywhere else."""
import functools

import numpy as np
import pytest
import torch

import oracle_ops_topk as M
from test_gpu_attn_match import _plant, _planted_inputs
import prob_bounds as PB
from test_gpu_attn_rows import CASES, ODD_CASES, TOL, _case_inputs, _gpu_lse, _ids, _indices, _oracle_probs, _oracle_side, _rand
from test_gpu_ref_table import _pool_grid, _stack

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
FORMS = ("none", "head_mean")
KS = (1, 2, 3, 5, 8)
LN2 = 0.6931471805599453
# len < k with several heads and a key tail (the list of the issue): a 5-key reference beside a 40-key self segment
TOPK_CASES = CASES + ODD_CASES + [(1, 2, 40, 40, 2, 5, True)]


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
    return dict(q=qd, k=kd, rk=rkd, lse=lse, p64=_oracle_probs(q, k, v, rk, rv, H, inc), E=E, delta=delta, edges=M.segment_edges(Ls, N, Lr, inc),
                kw=dict(heads=H, scale=0.125, include_self=inc))


def _row_lists(B, Lq):
    """1, 5 and 68 rows with forced duplicates, and every row (None)"""
    return [_indices(B, Lq, R, seed=100 + R) for R in sorted({min(r, Lq) for r in (1, 5, 68)})] + [None]


def _idx_np(idx, B, Lq):
    return np.broadcast_to(np.arange(Lq), (B, Lq)) if idx is None else idx.numpy()


def _what(case, dtype, idx, form=None, k=None):
    return f"{_ids([case])[0]} {dtype} R={'all' if idx is None else idx.shape[1]}" + (f" {form}" if form else "") + (f" k={k}" if k else "")


def _topk(ops, s, idx, form, k):
    return ops.attn_topk(s["q"], s["k"], s["rk"], s["lse"], None if idx is None else idx.cuda(), k=k, reduce=form, **s["kw"])


def _stable_desc(x):
    """(..., n) -> (values, positions) of a stable descending sort: equal values in ascending position"""
    order = torch.sort(x, dim=-1, descending=True, stable=True)
    return order.values, order.indices


# ---- 1: rank 0 is attn_match ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", TOPK_CASES, ids=_ids(TOPK_CASES))
def test_rank_zero_is_attn_match(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    S = len(s["edges"]) - 1
    for idx in _row_lists(B, Lq):
        R = Lq if idx is None else idx.shape[1]
        for form in FORMS:
            mi, mp = ops.attn_match(s["q"], s["k"], s["rk"], s["lse"], None if idx is None else idx.cuda(), reduce=form, **s["kw"])
            for k in KS:
                index, prob = _topk(ops, s, idx, form, k)
                shape = (B, H, R, S, k) if form == "none" else (B, R, S, k)
                assert index.shape == shape and prob.shape == shape and index.dtype == torch.int32 and prob.dtype == torch.float32
                assert index.is_contiguous() and prob.is_contiguous()
                assert torch.equal(index[..., 0], mi) and torch.equal(prob[..., 0], mp), _what(case, dtype, idx, form, k)


# ---- 2, 3: against the library's rows, no tolerance ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", TOPK_CASES, ids=_ids(TOPK_CASES))
def test_head_mean_is_a_stable_sort_of_the_head_mean_rows(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    for idx in _row_lists(B, Lq):
        rows = torch.arange(Lq, dtype=torch.int32).expand(B, -1).contiguous() if idx is None else idx
        HM = ops.attn_rows(s["q"], s["k"], s["rk"], s["lse"], rows.cuda(), reduce="head_mean", **s["kw"])
        sorts = [_stable_desc(HM[..., a:b]) for a, b in zip(s["edges"][:-1], s["edges"][1:])]
        for k in KS:
            index, prob = _topk(ops, s, idx, "head_mean", k)
            for si, (vals, pos) in enumerate(sorts):
                n = min(k, vals.shape[-1])
                what = (_what(case, dtype, idx, "head_mean", k), si)
                assert torch.equal(prob[..., si, :n], vals[..., :n]), what
                assert torch.equal(index[..., si, :n].long(), pos[..., :n]), what
                assert bool((index[..., si, n:] == -1).all()) and bool((prob[..., si, n:] == 0).all()), what


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", TOPK_CASES, ids=_ids(TOPK_CASES))
def test_per_head_against_the_rows_readout(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    for idx in _row_lists(B, Lq):
        rows = torch.arange(Lq, dtype=torch.int32).expand(B, -1).contiguous() if idx is None else idx
        P0 = ops.attn_rows(s["q"], s["k"], s["rk"], s["lse"], rows.cuda(), reduce="none", **s["kw"])
        tops = [torch.topk(P0[..., a:b], min(max(KS), b - a), dim=-1).values for a, b in zip(s["edges"][:-1], s["edges"][1:])]
        for k in KS:
            index, prob = _topk(ops, s, idx, "none", k)
            for si, (a, b) in enumerate(zip(s["edges"][:-1], s["edges"][1:])):
                n = min(k, b - a)
                what = (_what(case, dtype, idx, "none", k), si)
                ix, pr = index[..., si, :n].long(), prob[..., si, :n]
                want = tops[si][..., :n]                                                            # torch.topk(segment, n).values
                assert torch.equal(pr.to(dtype), want), what                                          # the k largest rounded values
                assert int(ix.min()) >= 0 and int(ix.max()) < b - a, what
                assert torch.equal(P0[..., a:b].gather(-1, ix), want), what                          # ... sit at the reported keys
                if n > 1:
                    assert bool((torch.sort(ix, dim=-1).values.diff(dim=-1) > 0).all()), what           # distinct
                    d = pr.diff(dim=-1)
                    assert bool((d <= 0).all()), what                                                  # fp32 prob does not increase
                    assert bool((ix.diff(dim=-1)[d == 0] > 0).all()), what                             # equal prob: ascending keys
                assert bool((index[..., si, n:] == -1).all()) and bool((prob[..., si, n:] == 0).all()), what


# ---- 4: the float64 oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", TOPK_CASES, ids=_ids(TOPK_CASES))
def test_against_the_float64_oracle(ops, case, dtype):
    """bounds: TOL and 2 TOL (module docstring, which also has the largest figures seen).  The worst figures of every case and row
    list are printed before they are asserted"""
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    tol = TOL[dtype]
    for idx in _row_lists(B, Lq):
        p_rows = M.gather_rows(s["p64"], _idx_np(idx, B, Lq))
        E_rows, d_rows = M.gather_rows(s["E"], _idx_np(idx, B, Lq)), M.gather_rows(s["delta"], _idx_np(idx, B, Lq))
        for form in FORMS:
            x = p_rows.mean(axis=1) if form == "head_mean" else p_rows
            best, _ = M.topk_np(p_rows, s["edges"], max(KS), form == "head_mean")                # (..., S, 8): the t-th largest p64
            cal, der, ref = (*PB.terms(p_rows, E_rows, None, d_rows), p_rows)
            if form == "head_mean":
                cal, der, ref = PB.head_mean_terms(cal, der, p_rows)
            tops = {}
            worst_v = worst_gap = 0.0
            for k in KS:
                index, prob = _topk(ops, s, idx, form, k)
                index, prob = index.cpu().numpy().astype(np.int64), prob.cpu().numpy().astype(np.float64)
                PB.check_ranked(index, prob, ref, cal, der, s["edges"], np.zeros(ref.shape[:-1], dtype=bool),
                                f"attn_topk {_what(case, dtype, idx, form)} k={k}", kind=f"topk_{form}B", tops=tops)
                for si, (a, b) in enumerate(zip(s["edges"][:-1], s["edges"][1:])):
                    n = min(k, b - a)
                    at = np.take_along_axis(x, a + index[..., si, :n], axis=-1)                  # p64[index_t]
                    worst_v = max(worst_v, float(np.abs(prob[..., si, :n] - at).max()))
                    worst_gap = max(worst_gap, float((best[..., si, :n] - at).max()))
            print(f"attn_topk {_what(case, dtype, idx, form)} k in {KS}: max |prob_t - p64[index_t]| {worst_v:.3e} (bound {tol:.0e}), "
                  f"max (t-th largest p64 - p64[index_t]) {worst_gap:.3e} (bound {2 * tol:.0e})")
            assert worst_v <= tol and worst_gap <= 2 * tol, (form, worst_v, worst_gap)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_rank_prefixes_agree(ops, dtype):
    """the ranks of a call with a smaller k are the first ranks of the call with k = 8, across the compiled capacities"""
    case = CASES[3]
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    for idx in (None, _indices(B, Lq, 68, seed=12)):
        for form in FORMS:
            i8, p8 = _topk(ops, s, idx, form, 8)
            for k in range(1, 8):
                ik, pk = _topk(ops, s, idx, form, k)
                assert torch.equal(ik, i8[..., :k]) and torch.equal(pk, p8[..., :k]), (form, k)


# ---- 5: planted order ----------------------------------------------------------------------------------------------------------------------
# every boundary of the walk inside a 200-key segment (no multiple of 32): key 0, the lane groups of 16, the 32-key blocks, the 64-key
# steps of the per-head walk, the 128-key steps of the head-mean walk, the last key
POSITIONS = [0, 15, 16, 31, 32, 63, 64, 127, 128, 199]
PLANT = dict(B=2, H=2, Lq=72, Ls=200, N=2, Lr=200)


def _planted(dtype, seed):
    c = PLANT
    q, k, v, rk, rv, win = _planted_inputs(dtype, c["B"], c["H"], c["Lq"], c["Ls"], c["N"], c["Lr"], seed=seed)
    return q, k, v, rk, rv, win, dict(heads=c["H"], scale=0.125, include_self=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_planted_graded_winners_come_out_in_their_order(ops, dtype):
    """keys c_t * u_h, c = 3.0, 2.9, ... 2.1, at the positions above in shuffled order, on every head: a step of 0.1 in c is a step
    of 0.8 a_i >= 0.4 in the logit of every row, an order of magnitude above what rounding the key to 16 bits moves it"""
    q, k, v, rk, rv, win, kw = _planted(dtype, seed=45)
    H = PLANT["H"]
    order = np.random.default_rng(7).permutation(len(POSITIONS))                # POSITIONS[order[t]] holds the t-th largest key
    k2, rk2 = k.clone(), rk.clone()
    for t, o in enumerate(order):
        graded = (win.float() * ((3.0 - 0.1 * t) / 3.0)).to(dtype)
        k2, rk2 = _plant(k2, rk2, graded, range(H), [POSITIONS[o]], [POSITIONS[o]])
    want_all = [POSITIONS[o] for o in order]
    _, lse = ops.shared_attention(q, k2, v, rk2, rv, return_lse=True, **kw)
    for form in FORMS:
        for rows in (None, _indices(PLANT["B"], PLANT["Lq"], 5, seed=3).cuda()):
            for kk in KS:
                index, prob = ops.attn_topk(q, k2, rk2, lse, rows, k=kk, reduce=form, **kw)
                want = torch.tensor(want_all[:kk], dtype=torch.int32, device="cuda").expand_as(index)
                assert torch.equal(index, want), f"{form} k={kk}: got {index.reshape(-1, kk).unique(dim=0).tolist()}, want {want_all[:kk]}"
                assert bool((prob[..., :-1] > prob[..., 1:]).all()) if kk > 1 else True


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_planted_ties_come_out_in_ascending_key_order(ops, dtype):
    """the SAME winner at 11 positions, k = 8: the 8 lowest positions, ascending, with values identical bit for bit; and at 15 and 16
    only - the two half-waves' first shared block - k = 2: [15, 16]"""
    q, k, v, rk, rv, win, kw = _planted(dtype, seed=47)
    H = PLANT["H"]
    eleven = sorted(POSITIONS + [96])
    for pos, kk in ((eleven, 8), ([15, 16], 2)):
        k2, rk2 = _plant(k, rk, win, range(H), pos, pos)
        _, lse = ops.shared_attention(q, k2, v, rk2, rv, return_lse=True, **kw)
        want_list = sorted(pos)[:kk]
        for form in FORMS:
            for rows in (None, _indices(PLANT["B"], PLANT["Lq"], 5, seed=4).cuda()):
                index, prob = ops.attn_topk(q, k2, rk2, lse, rows, k=kk, reduce=form, **kw)
                want = torch.tensor(want_list, dtype=torch.int32, device="cuda").expand_as(index)
                assert torch.equal(index, want), f"{pos} {form}: got {index.reshape(-1, kk).unique(dim=0).tolist()}"
                assert torch.equal(prob, prob[..., :1].expand_as(prob)), (pos, form)           # one value in every rank
                assert float(prob.min()) > 0


# ---- 6: row groups ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_row_groups_equal_calls_of_one_row(ops, dtype):
    """R = 100 and 200: more than one group of 96 rows; R = 33: a partial second 32-row block.  Row for row the result of a call
    that holds that row alone"""
    case = CASES[3]                                # Lq = 300, key tails of 8 / 48 keys
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    k = 8
    idx = _indices(B, Lq, 200, seed=77)
    single = {form: [_topk(ops, s, idx[:, r:r + 1].contiguous(), form, k) for r in range(200)] for form in FORMS}
    for R in (33, 100, 200):
        for form in FORMS:
            index, prob = _topk(ops, s, idx[:, :R].contiguous(), form, k)
            one_i = torch.cat([single[form][r][0] for r in range(R)], dim=-3)
            one_p = torch.cat([single[form][r][1] for r in range(R)], dim=-3)
            assert torch.equal(index, one_i) and torch.equal(prob, one_p), (R, form)


# ---- 7: invalid rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_invalid_rows_give_minus_one_and_zero_and_are_never_read(ops, dtype):
    """indices -1 and len_q on the device: index -1, prob 0 in every rank.  q is a view into a larger NaN-filled buffer, so the rows
    those indices would address hold NaN - and nothing changes for the other rows"""
    case = CASES[0]
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    buf = torch.full((B, Lq + 2, H * 64), float("nan"), dtype=dtype, device="cuda")
    buf[:, 1:Lq + 1] = s["q"]
    qv = buf[:, 1:Lq + 1]                                           # rows -1 and Lq of this view are NaN
    R = 40
    idx = _indices(B, Lq, R, seed=9)
    bad = idx.clone()
    bad[:, 3], bad[:, 17], bad[:, R - 1] = -1, Lq, Lq
    bad[1, 20] = -1
    keep = (bad == idx).cuda()
    for form in FORMS:
        for k in (1, 3, 8):
            i_ok, p_ok = ops.attn_topk(s["q"], s["k"], s["rk"], s["lse"], idx.cuda(), k=k, reduce=form, **s["kw"])
            i_bad, p_bad = ops.attn_topk(qv, s["k"], s["rk"], s["lse"], bad.cuda(), k=k, reduce=form, **s["kw"])
            sel = keep[:, None, :, None, None] if form == "none" else keep[:, :, None, None]
            sel = sel.expand_as(i_ok)
            assert torch.equal(i_bad[sel], i_ok[sel]) and torch.equal(p_bad[sel], p_ok[sel]), (form, k)
            assert bool((i_bad[~sel] == -1).all()) and bool((p_bad[~sel] == 0).all()), (form, k)
            assert bool(torch.isfinite(p_bad).all())


# ---- 8: torch.equal with the plain call ------------------------------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_pointer_tables_equal_the_dense_call(ops, dtype):
    B, H, Lq, N, Lr = 2, 2, 128, 2, 72
    g = torch.Generator().manual_seed(13)
    q, ks, vs = (torch.randn(B, Lq, H * 64, generator=g).to("cuda", dtype) for _ in range(3))
    gk, gv = _pool_grid(g, B, N, Lr, H * 64, dtype)
    dk, dv = _stack(gk), _stack(gv)
    tk = ops.RefKVTable.from_tensors(gk)
    kw = dict(heads=H, scale=0.125, include_self=True)
    _, lse = ops.shared_attention(q, ks, vs, dk, dv, return_lse=True, **kw)
    for form in FORMS:
        for rows in (None, torch.tensor([[0, 5, 127], [64, 3, 3]])):
            for k in (2, 8):
                assert _same(ops.attn_topk(q, ks, tk, lse, rows, k=k, reduce=form, **kw), ops.attn_topk(q, ks, dk, lse, rows, k=k, reduce=form, **kw)), (form, k)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_prescaled_q(ops, dtype):
    """IR_FLAG_Q_PRESCALED: the products of the pre-scaled query and k ARE the exponents.  The plain call on that rounded query
    with scale = ln 2 forms scale * log2(e) = 1 in fp32 and so the same bytes; rank 0 is the flagged match"""
    B, H, L, N, Lr = 2, 2, 72, 3, 40
    gen = torch.Generator().manual_seed(11)
    q = _rand((B, L, H * 64), dtype, gen, 1.5)
    qs = (q.float() * (0.125 * 1.4426950408889634)).to(dtype).cuda()
    k, v = _rand((B, L, H * 64), dtype, gen, 1.5).cuda(), _rand((B, L, H * 64), dtype, gen).cuda()
    rk, rv = _rand((B, N, Lr, H * 64), dtype, gen, 1.5).cuda(), _rand((B, N, Lr, H * 64), dtype, gen).cuda()
    _, lse = ops.shared_attention(qs, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True, q_prescaled=True)
    for idx in (None, _indices(B, L, 68, seed=31).cuda()):
        for form in FORMS:
            flagged = ops.attn_topk(qs, k, rk, lse, idx, k=5, heads=H, scale=0.125, include_self=True, reduce=form, q_prescaled=True)
            plain = ops.attn_topk(qs, k, rk, lse, idx, k=5, heads=H, scale=LN2, include_self=True, reduce=form)
            assert _same(flagged, plain), form
            mi, mp = ops.attn_match(qs, k, rk, lse, idx, heads=H, scale=0.125, include_self=True, reduce=form, q_prescaled=True)
            assert torch.equal(flagged[0][..., 0], mi) and torch.equal(flagged[1][..., 0], mp), form


def test_graph_replay_follows_the_index_tensor_and_the_table(ops):
    dtype = torch.bfloat16
    B, H, Lq, N, Lr, R = 2, 2, 200, 3, 72, 68
    g = torch.Generator().manual_seed(9)
    q, ks, vs = (torch.randn(B, Lq, H * 64, generator=g).to("cuda", dtype) for _ in range(3))
    gk0, gv0 = _pool_grid(g, B, N, Lr, H * 64, dtype)
    gk1, gv1 = _pool_grid(g, B, N, Lr, H * 64, dtype, scale=0.7, shift=0.1)
    kw = dict(heads=H, scale=0.125, include_self=True)
    lse0 = ops.shared_attention(q, ks, vs, _stack(gk0), _stack(gv0), return_lse=True, **kw)[1]
    lse1 = ops.shared_attention(q, ks, vs, _stack(gk1), _stack(gv1), return_lse=True, **kw)[1]
    idx0, idx1 = _indices(B, Lq, R, seed=1).cuda(), _indices(B, Lq, R, seed=2).cuda()
    for form in FORMS:
        tk = ops.RefKVTable.from_tensors(gk0)
        static_idx, static_lse = idx0.clone(), lse0.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.attn_topk(q, ks, tk, static_lse, static_idx, k=4, reduce=form, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.attn_topk(q, ks, tk, static_lse, static_idx, k=4, reduce=form, **kw)
        graph.replay()
        torch.cuda.synchronize()
        want0 = ops.attn_topk(q, ks, _stack(gk0), lse0, idx0, k=4, reduce=form, **kw)
        assert _same(out, want0), form
        static_idx.copy_(idx1)
        static_lse.copy_(lse1)
        tk.fill_(gk1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want1 = ops.attn_topk(q, ks, _stack(gk1), lse1, idx1, k=4, reduce=form, **kw)
        assert _same(out, want1), form
        assert not torch.equal(want0[0], want1[0])
        del graph


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_batch_invariance_and_repeated_calls(ops, dtype):
    """entry b of a batch of 3 equals the same entry run alone, in both forms, with and without the (accepted, inert) flag; a
    repeated call gives the same bytes"""
    case = (3, 2, 72, 72, 3, 40, True)
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    for idx in (None, _indices(B, Lq, 68, seed=21).cuda()):
        for form in FORMS:
            for k in (3, 8):
                a = ops.attn_topk(s["q"], s["k"], s["rk"], s["lse"], idx, k=k, reduce=form, **s["kw"])
                f = ops.attn_topk(s["q"], s["k"], s["rk"], s["lse"], idx, k=k, reduce=form, batch_invariant=True, **s["kw"])
                assert _same(a, f)
                for _ in range(3):
                    assert _same(a, ops.attn_topk(s["q"], s["k"], s["rk"], s["lse"], idx, k=k, reduce=form, **s["kw"]))
                for b in range(B):
                    one = ops.attn_topk(s["q"][b:b + 1].contiguous(), s["k"][b:b + 1].contiguous(), s["rk"][b:b + 1].contiguous(),
                                        s["lse"][b:b + 1].contiguous(), None if idx is None else idx[b:b + 1].contiguous(), k=k, reduce=form, **s["kw"])
                    assert torch.equal(one[0][0], a[0][b]) and torch.equal(one[1][0], a[1][b]), (form, k, b)


def test_through_the_plugin_surface(ops, monkeypatch):
    """``attention_topk_index = "all"`` on a shared layer: the result is ``ops.attn_topk`` on that layer's q / k / lse (caught on
    their way into the call), its rank 0 is ``attention_match`` of the same forward, and the layer output stays as it was bit for bit"""
    import instantrestore_amd.attn_processors as ap
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    seen = []
    real = ops.attn_topk

    def spy(*a, **kw):
        seen.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ap._ops, "attn_topk", spy)
    torch.manual_seed(4)
    B, H, L, N = 2, 2, 256, 4
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
            assert proc.attention_topk is None and not seen
            proc.attention_topk_index, proc.attention_match_index = "all", "all"
            y1 = run()
            assert len(seen) == 1
            (a, kw) = seen.pop()
            assert a[4] is None and kw["reduce"] == "head_mean" and kw["k"] == 4
            index, prob = proc.attention_topk
            assert index.shape == (B, L, S, 4) and _same((index, prob), real(*a, **kw)) and torch.equal(y0, y1)
            assert torch.equal(index[..., 0], proc.attention_match[0]) and torch.equal(prob[..., 0], proc.attention_match[1])
            rows = _indices(B, L, 68, seed=6)
            proc.attention_topk_index, proc.attention_topk_reduce, proc.attention_topk_k = rows, "none", 8
            proc.attention_match_index, proc.attention_match_reduce = rows, "none"
            run()
            (a, kw) = seen.pop()
            index, prob = proc.attention_topk
            assert index.shape == (B, H, 68, S, 8) and _same((index, prob), real(*a, **kw))
            assert torch.equal(index[..., 0], proc.attention_match[0]) and torch.equal(prob[..., 0], proc.attention_match[1])


def test_helpers_on_device_results(ops):
    """the ``attn_maps`` helpers on a device result: coverage from the forward's own segment masses lies in [0, 1] and grows with k;
    ``keep_from_topk`` keeps exactly the reference tokens the ranks name"""
    from instantrestore_amd import attn_maps as am
    case = CASES[2]                                # (1, 3, 256, 256, 4, 256, True)
    B, H, Lq, Ls, N, Lr, inc = case
    dtype = torch.bfloat16
    s = _setup(case, dtype)
    q, k, v, rk, rv = _case_inputs(case, dtype)
    _, mass = ops.shared_attention(q.cuda(), k.cuda(), v.cuda(), rk.cuda(), rv.cuda(), return_mass=True, **s["kw"])
    prev = None
    for kk in (2, 8):
        index, prob = _topk(ops, s, None, "none", kk)
        cov = am.topk_coverage(prob, mass)
        assert cov.shape == (B, H, Lq, N + 1) and float(cov.min()) > 0 and float(cov.max()) <= 1
        assert prev is None or bool((cov >= prev).all())
        prev = cov
        amb = am.match_ambiguity(prob)
        assert float(amb.min()) >= 0 and float(amb.max()) <= 1
        y, x = am.topk_coordinates(index, 16)
        assert torch.equal(y * 16 + x, index.long())
        keep = am.keep_from_topk(index, N, Lr, inc)
        want = torch.zeros(B, N, Lr, dtype=torch.bool, device="cuda")
        for n in range(N):
            want[0, n, index[0, :, :, 1 + n].reshape(-1).long().unique()] = True
        assert keep.shape == (B, N, Lr) and torch.equal(keep, want)


def test_example_topk_switch(capsys):
    """examples/synthetic_inference.py --topk K --prune-topk: every shared layer prints its per-reference figures"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "synthetic_inference.py")
    spec = importlib.util.spec_from_file_location("synthetic_inference_topk", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--identities", "2", "--refs", "3", "--px", "256", "--small", "--topk", "4", "--prune-topk", "--dtype", "bf16"])
    text = capsys.readouterr().out
    assert out.shape == (2, 256, 256, 3)
    assert text.count(": top-4 (2, ") == 9 and "top-4 (2, 1024, 4, 4)" in text, text
    assert text.count("mean ambiguity per reference") == 9 and text.count("mean coverage of the 4 best keys per reference") == 9
    assert text.count("fraction of reference tokens keep_from_topk keeps") == 9
