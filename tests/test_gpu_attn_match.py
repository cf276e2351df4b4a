"""``ir_attn_match`` on the GPU: per K/V segment, the largest attention probability of chosen query tokens and the key that attains it.

What is held to what:
  1. the library's own read-outs, with NO tolerance: ``prob`` rounded to the 16-bit format is the maximum of ``attn_rows(reduce="none")``
     over the segment and the row gathered at ``index`` has that value; the head-mean ``prob`` is the maximum of
     ``attn_rows(reduce="head_mean")`` bit for bit and ``index`` its first argmax (same expression, same order, monotone rounding);
  2. the float64 oracle, with ``TOL`` of tests/test_gpu_probs.py (1e-3 fp16 / 8e-3 bf16, the project's stated bound for
     probabilities): ``|prob - p64[index]| <= TOL`` and ``p64[index] >= max_j p64[j] - 2 TOL`` (every key's probability is within
     TOL, so the chosen key is a maximiser up to twice that); and under the relative fp32 bound of tests/prob_bounds.py
     (reference B): ``prob`` at the returned index element by element, the index under its index rule;
  3. planted winners, ties, invalid rows: exact indices;
  4. pointer tables, graph replay, pre-scaled Q, batch invariance, the processor: ``torch.equal`` with the plain call.
The inputs, the LSE and the float64 probabilities of a (case, dtype) are computed once and shared by the tests that need them."""
import functools

import numpy as np
import pytest
import torch

import oracle_ops_match as M
import prob_bounds as PB
from test_gpu_attn_rows import CASES, ODD_CASES, TOL, _case_inputs, _gpu_lse, _ids, _indices, _oracle_probs, _oracle_side, _rand
from test_gpu_ref_table import _pool_grid, _stack

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
FORMS = ("none", "head_mean")
LN2 = 0.6931471805599453


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


def _first_argmax(x):
    """(..., n) -> (max, the lowest position that holds it), without relying on a library's tie rule"""
    m = x.max(-1).values
    pos = torch.arange(x.shape[-1], device=x.device).expand_as(x)
    first = torch.where(x == m[..., None], pos, torch.full_like(pos, x.shape[-1])).min(-1).values
    return m, first


def _check_against_rows(ops, q, k, rk, lse, idx, edges, dtype, what, **kw):
    """item 1 of the module docstring on one row list"""
    B, Lq = q.shape[0], q.shape[1]
    rows = torch.arange(Lq, dtype=torch.int32).expand(B, -1).contiguous() if idx is None else idx
    dev_idx = None if idx is None else idx.cuda()
    P0 = ops.attn_rows(q, k, rk, lse, rows.cuda(), reduce="none", **kw)
    HM = ops.attn_rows(q, k, rk, lse, rows.cuda(), reduce="head_mean", **kw)
    i0, p0 = ops.attn_match(q, k, rk, lse, dev_idx, reduce="none", **kw)
    i1, p1 = ops.attn_match(q, k, rk, lse, dev_idx, reduce="head_mean", **kw)
    R, S = rows.shape[1], len(edges) - 1
    H = P0.shape[1]
    assert i0.shape == (B, H, R, S) and p0.shape == (B, H, R, S) and i1.shape == (B, R, S) and p1.shape == (B, R, S), what
    assert i0.dtype == torch.int32 and i1.dtype == torch.int32 and p0.dtype == torch.float32 and p1.dtype == torch.float32
    for s, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        seg0 = P0[..., a:b]
        assert int(i0[..., s].min()) >= 0 and int(i0[..., s].max()) < b - a, (what, s)
        assert torch.equal(p0[..., s].to(dtype), seg0.max(-1).values), f"{what}: per-head prob of segment {s} is not the maximum of the rows"
        assert torch.equal(seg0.gather(-1, i0[..., s:s + 1].long())[..., 0], seg0.max(-1).values), f"{what}: per-head index of segment {s} does not attain the maximum"
        m1, first1 = _first_argmax(HM[..., a:b])
        assert torch.equal(p1[..., s], m1), f"{what}: head-mean prob of segment {s} is not the maximum of the head-mean rows bit for bit"
        assert torch.equal(i1[..., s].long(), first1), f"{what}: head-mean index of segment {s} is not the first argmax"
    return (i0, p0), (i1, p1)


# ---- 1, 2: every case against the library's read-outs and against the oracle -----------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES + ODD_CASES, ids=_ids(CASES + ODD_CASES))
def test_against_the_rows_readout_bit_for_bit(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    for idx in _row_lists(B, Lq):
        _check_against_rows(ops, s["q"], s["k"], s["rk"], s["lse"], idx, s["edges"], dtype, f"{_ids([case])[0]} {dtype} R={'all' if idx is None else idx.shape[1]}", **s["kw"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES + ODD_CASES, ids=_ids(CASES + ODD_CASES))
def test_against_the_float64_oracle(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    tol = TOL[dtype]
    for idx in _row_lists(B, Lq):
        p_rows = M.gather_rows(s["p64"], _idx_np(idx, B, Lq))
        E_rows, d_rows = M.gather_rows(s["E"], _idx_np(idx, B, Lq)), M.gather_rows(s["delta"], _idx_np(idx, B, Lq))
        dev_idx = None if idx is None else idx.cuda()
        for form in FORMS:
            index, prob = ops.attn_match(s["q"], s["k"], s["rk"], s["lse"], dev_idx, reduce=form, **s["kw"])
            index, prob = index.cpu().numpy().astype(np.int64), prob.cpu().numpy().astype(np.float64)
            cal, der, ref = (*PB.terms(p_rows, E_rows, None, d_rows), p_rows)
            if form == "head_mean":
                cal, der, ref = PB.head_mean_terms(cal, der, p_rows)
            PB.check_ranked(index[..., None], prob[..., None], ref, cal, der, s["edges"], np.zeros(ref.shape[:-1], dtype=bool),
                            f"attn_match {_ids([case])[0]} {dtype} R={'all' if idx is None else idx.shape[1]} {form}", kind=f"match_{form}B")
            x = p_rows.mean(axis=1) if form == "head_mean" else p_rows
            best, _, _ = M.match_np(p_rows, s["edges"], form == "head_mean")
            worst_v = worst_gap = 0.0
            for si, a in enumerate(s["edges"][:-1]):
                at = np.take_along_axis(x, (a + index[..., si])[..., None], axis=-1)[..., 0]        # p64[index]
                worst_v = max(worst_v, float(np.abs(prob[..., si] - at).max()))
                worst_gap = max(worst_gap, float((best[..., si] - at).max()))
            print(f"attn_match {_ids([case])[0]} {dtype} R={'all' if idx is None else idx.shape[1]} {form}: max |prob - p64[index]| {worst_v:.3e} "
                  f"(bound {tol:.0e}), max (max_j p64 - p64[index]) {worst_gap:.3e} (bound {2 * tol:.0e})")
            assert worst_v <= tol and worst_gap <= 2 * tol, (form, worst_v, worst_gap)


# ---- 3, 4: planted winners and ties ---------------------------------------------------------------------------------------------
def _planted_inputs(dtype, B, H, Lq, Ls, N, Lr, seed):
    """every query row is a positive multiple of one direction u_h per head (q_i = a_i * u_h, a_i in [0.5, 1.5]): a key 3 * u_h then
    has the largest score of EVERY row - 24 a_i against a_i * N(0, 1.5) of the random keys - so one planted key per segment is the
    clear winner for every (row, segment) at once, while the rows (and their LSEs) still differ"""
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(H, 64, generator=gen)
    u = u * (8.0 / u.norm(dim=-1, keepdim=True))                          # |u|^2 = 64
    a = 0.5 + torch.rand(B, Lq, 1, 1, generator=gen)
    q = (a * u).reshape(B, Lq, H * 64).to(dtype)
    k = _rand((B, Ls, H * 64), dtype, gen, 1.5)
    v = _rand((B, Ls, H * 64), dtype, gen)
    rk = _rand((B, N, Lr, H * 64), dtype, gen, 1.5)
    rv = _rand((B, N, Lr, H * 64), dtype, gen)
    win = (3.0 * u).to(dtype)                                              # (H, 64)
    return q.cuda(), k.cuda(), v.cuda(), rk.cuda(), rv.cuda(), win.cuda()


def _plant(k, rk, win, heads, self_pos, ref_pos):
    """copies of K with the winner written at ``self_pos`` of the self segment and ``ref_pos`` of every reference, on ``heads``"""
    k2, rk2 = k.clone(), rk.clone()
    for h in heads:
        for pos in self_pos:
            k2[:, pos, h * 64:(h + 1) * 64] = win[h]
        for pos in ref_pos:
            rk2[:, :, pos, h * 64:(h + 1) * 64] = win[h]
    return k2, rk2


# (Lq, Ls, N, Lr, positions in the self segment, positions in the references): key 0, the edges of the 16-key lane groups, of the
# 32-key blocks and of the 64-key steps, the last key of a 40-, 136- and 1032-key segment, the last key before a 256-key boundary
PLANT_SHAPES = [
    (72, 40, 2, 136, [0, 15, 16, 31, 32, 39], [0, 15, 16, 31, 32, 63, 64, 135]),
    (40, 1032, 1, 300, [0, 63, 64, 255, 256, 511, 767, 1023, 1031], [255, 256, 299]),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", PLANT_SHAPES, ids=["Ls40Lr136", "Ls1032Lr300"])
def test_planted_winners_are_found_at_their_exact_position(ops, shape, dtype):
    Lq, Ls, N, Lr, self_pos, ref_pos = shape
    B, H, head = 1, 2, 1
    q, k, v, rk, rv, win = _planted_inputs(dtype, B, H, Lq, Ls, N, Lr, seed=41)
    kw = dict(heads=H, scale=0.125, include_self=True)
    for turn in range(max(len(self_pos), len(ref_pos))):
        sp, rp = self_pos[turn % len(self_pos)], ref_pos[turn % len(ref_pos)]
        k2, rk2 = _plant(k, rk, win, [head], [sp], [rp])
        _, lse = ops.shared_attention(q, k2, v, rk2, rv, return_lse=True, **kw)
        for rows in (None, _indices(B, Lq, 5, seed=turn).cuda()):
            index, prob = ops.attn_match(q, k2, rk2, lse, rows, reduce="none", **kw)
            want = torch.tensor([sp] + [rp] * N, dtype=torch.int32, device="cuda").expand_as(index[:, head])
            assert torch.equal(index[:, head], want), f"planted at self {sp} / ref {rp}: got {index[:, head].unique(dim=1).tolist()}"
            assert float(prob[:, head].min()) > 0.05             # one winner per segment, S = 3: each holds about a third of the row


TIES = [
    ("lane-local pair", (3, 7)),
    ("pair across the half-waves", (5, 20)),
    ("pair across the half-waves, the lower key in the upper half", (20, 33)),
    ("pair across 32-key blocks", (10, 45)),
    ("pair across 64-key steps", (20, 100)),
    ("three: one lane, the other half-wave, the next block", (7, 20, 45)),
    ("three across steps, the last key of the segment among them", (64, 70, 135)),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_ties_go_to_the_lowest_key_in_both_forms(ops, dtype):
    B, H, Lq, Ls, N, Lr = 1, 2, 72, 136, 2, 136
    q, k, v, rk, rv, win = _planted_inputs(dtype, B, H, Lq, Ls, N, Lr, seed=43)
    kw = dict(heads=H, scale=0.125, include_self=True)
    for what, pos in TIES:
        k2, rk2 = _plant(k, rk, win, range(H), pos, pos)       # identical K rows on every head: the head mean ties too
        _, lse = ops.shared_attention(q, k2, v, rk2, rv, return_lse=True, **kw)
        for form in FORMS:
            for rows in (None, _indices(B, Lq, 5, seed=3).cuda()):
                index, prob = ops.attn_match(q, k2, rk2, lse, rows, reduce=form, **kw)
                assert bool((index == pos[0]).all()), f"{what} {pos} {form}: got {index.unique().tolist()}"
        # the tie is real: the rows read-out holds the same fp32 head mean at every planted key
        hm = ops.attn_rows(q, k2, rk2, lse, torch.arange(Lq), reduce="head_mean", **kw)
        for p in pos[1:]:
            assert torch.equal(hm[..., pos[0]], hm[..., p]) and torch.equal(hm[..., Ls + pos[0]], hm[..., Ls + p]), (what, p)


# ---- 5: invalid rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_invalid_rows_give_minus_one_and_zero_and_are_never_read(ops, dtype):
    """indices -1 and len_q on the device: index -1, prob 0.  q is a view into a larger NaN-filled buffer, so the rows those
    indices would address hold NaN - and nothing changes for the other rows"""
    case = CASES[0]
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    buf = torch.full((B, Lq + 2, H * 64), float("nan"), dtype=dtype, device="cuda")
    buf[:, 1:Lq + 1] = s["q"]
    qv = buf[:, 1:Lq + 1]                                           # rows -1 and Lq of this view are NaN
    assert torch.equal(qv, s["q"]) and bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, Lq + 1]).all())
    R = 40
    idx = _indices(B, Lq, R, seed=9)
    bad = idx.clone()
    bad[:, 3], bad[:, 17], bad[:, R - 1] = -1, Lq, Lq
    bad[1, 20] = -1
    keep = (bad == idx).cuda()
    for form in FORMS:
        i_ok, p_ok = ops.attn_match(s["q"], s["k"], s["rk"], s["lse"], idx.cuda(), reduce=form, **s["kw"])
        i_bad, p_bad = ops.attn_match(qv, s["k"], s["rk"], s["lse"], bad.cuda(), reduce=form, **s["kw"])
        sel = keep[:, None, :, None] if form == "none" else keep[:, :, None]
        sel = sel.expand_as(i_ok)
        assert torch.equal(i_bad[sel], i_ok[sel]) and torch.equal(p_bad[sel], p_ok[sel]), form
        assert bool((i_bad[~sel] == -1).all()) and bool((p_bad[~sel] == 0).all()), form
        assert bool(torch.isfinite(p_bad).all())


# ---- 6, 7: pointer tables, graph replay --------------------------------------------------------------------------------------------
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
            a = ops.attn_match(q, ks, tk, lse, rows, reduce=form, **kw)
            b = ops.attn_match(q, ks, dk, lse, rows, reduce=form, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (form, rows is None)


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
            ops.attn_match(q, ks, tk, static_lse, static_idx, reduce=form, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.attn_match(q, ks, tk, static_lse, static_idx, reduce=form, **kw)
        graph.replay()
        torch.cuda.synchronize()
        want0 = ops.attn_match(q, ks, _stack(gk0), lse0, idx0, reduce=form, **kw)
        assert torch.equal(out[0], want0[0]) and torch.equal(out[1], want0[1]), form
        static_idx.copy_(idx1)
        static_lse.copy_(lse1)
        tk.fill_(gk1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want1 = ops.attn_match(q, ks, _stack(gk1), lse1, idx1, reduce=form, **kw)
        assert torch.equal(out[0], want1[0]) and torch.equal(out[1], want1[1]), form
        assert not torch.equal(want0[0], want1[0])
        del graph


# ---- 8, 9: pre-scaled Q, batch invariance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_prescaled_q(ops, dtype):
    """IR_FLAG_Q_PRESCALED: the products of the pre-scaled query and k ARE the exponents.  The plain call on that rounded query
    with scale = ln 2 forms scale * log2(e) = 1 in fp32 and so the same bytes; both agree with the rows read-out under the flag"""
    B, H, L, N, Lr = 2, 2, 72, 3, 40
    gen = torch.Generator().manual_seed(11)
    q = _rand((B, L, H * 64), dtype, gen, 1.5)
    qs = (q.float() * (0.125 * 1.4426950408889634)).to(dtype).cuda()
    k, v = _rand((B, L, H * 64), dtype, gen, 1.5).cuda(), _rand((B, L, H * 64), dtype, gen).cuda()
    rk, rv = _rand((B, N, Lr, H * 64), dtype, gen, 1.5).cuda(), _rand((B, N, Lr, H * 64), dtype, gen).cuda()
    _, lse = ops.shared_attention(qs, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True, q_prescaled=True)
    edges = M.segment_edges(L, N, Lr, True)
    for idx in (None, _indices(B, L, 68, seed=31)):
        flagged = _check_against_rows(ops, qs, k, rk, lse, idx, edges, dtype, f"prescaled {dtype}", heads=H, scale=0.125, include_self=True,
                                      q_prescaled=True)
        for form, (fi, fp) in zip(FORMS, flagged):
            pi, pp = ops.attn_match(qs, k, rk, lse, None if idx is None else idx.cuda(), heads=H, scale=LN2, include_self=True, reduce=form)
            assert torch.equal(pi, fi) and torch.equal(pp, fp), form


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_batch_invariance(ops, dtype):
    """entry b of a batch of 3 equals the same entry run alone, in both forms, with and without the (accepted, inert) flag"""
    case = (3, 2, 72, 72, 3, 40, True)
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    for idx in (None, _indices(B, Lq, 68, seed=21).cuda()):
        for form in FORMS:
            a = ops.attn_match(s["q"], s["k"], s["rk"], s["lse"], idx, reduce=form, **s["kw"])
            f = ops.attn_match(s["q"], s["k"], s["rk"], s["lse"], idx, reduce=form, batch_invariant=True, **s["kw"])
            assert torch.equal(a[0], f[0]) and torch.equal(a[1], f[1])
            for b in range(B):
                one = ops.attn_match(s["q"][b:b + 1].contiguous(), s["k"][b:b + 1].contiguous(), s["rk"][b:b + 1].contiguous(),
                                     s["lse"][b:b + 1].contiguous(), None if idx is None else idx[b:b + 1].contiguous(), reduce=form, **s["kw"])
                assert torch.equal(one[0][0], a[0][b]) and torch.equal(one[1][0], a[1][b]), (form, b)


# ---- 10: the processor ----------------------------------------------------------------------------------------------------------------
def test_through_the_plugin_surface(ops, monkeypatch):
    """``attention_match_index = "all"`` on a shared layer: the result is ``ops.attn_match`` on that layer's q / k / lse (caught on
    their way into the call), agrees with the dump of the same forward, and leaves ``attention_rows``, ``attention_mass`` and the
    layer output as they were bit for bit"""
    import instantrestore_amd.attn_processors as ap
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    seen = []
    real = ops.attn_match

    def spy(*a, **kw):
        seen.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ap._ops, "attn_match", spy)
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
            proc.attention_rows_index, proc.save_attention_mass = _indices(B, L, 68, seed=6), True
            y0 = run()
            rows0, mass0 = proc.attention_rows.clone(), proc.attention_mass.clone()
            assert proc.attention_match is None and not seen
            proc.attention_match_index, proc.save_self_attentions = "all", True
            y1 = run()
            assert len(seen) == 1
            (a, kw) = seen.pop()
            assert a[4] is None and kw["reduce"] == "head_mean"
            index, prob = proc.attention_match
            want = real(*a, **kw)
            assert index.shape == (B, L, S) and torch.equal(index, want[0]) and torch.equal(prob, want[1])
            assert torch.equal(proc.attention_rows, rows0) and torch.equal(proc.attention_mass, mass0) and torch.equal(y0, y1)
            proc.attention_match_reduce = "none"
            run()
            seen.clear()
            i0, p0 = proc.attention_match
            dump = proc.attention_probs
            assert dump.shape == (B, H, L, S * L) and i0.shape == (B, H, L, S)
            for s in range(S):
                seg = dump[..., s * L:(s + 1) * L]
                assert torch.equal(p0[..., s].to(dump.dtype), seg.max(-1).values)
                assert torch.equal(seg.gather(-1, i0[..., s:s + 1].long())[..., 0], seg.max(-1).values)


# ---- 11: one real-shape slice ---------------------------------------------------------------------------------------------------------
def test_1024px_layer_one_identity_one_head(ops):
    """the 1024-px top shared layer for one identity and one head (L = Ls = Lr = 16384, N = 4, bf16, 68 rows): the shape the dump
    cannot serve, held to the rows read-out bit for bit"""
    dtype = torch.bfloat16
    B, H, L, N, R = 1, 1, 16384, 4, 68
    g = torch.Generator(device="cuda").manual_seed(2)
    q = (torch.randn(B, L, 64, device="cuda", generator=g) * 1.2).to(dtype)
    k = torch.randn(B, L, 64, device="cuda", generator=g).to(dtype)
    v = torch.randn(B, L, 64, device="cuda", generator=g).to(dtype)
    rk = torch.randn(B, N, L, 64, device="cuda", generator=g).to(dtype)
    rv = torch.randn(B, N, L, 64, device="cuda", generator=g).to(dtype)
    _, lse = ops.shared_attention(q, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True)
    _check_against_rows(ops, q, k, rk, lse, _indices(B, L, R, seed=5), M.segment_edges(L, N, L, True), dtype, "1024px", heads=H, scale=0.125,
                        include_self=True)


def test_example_matches_switch(capsys):
    """examples/synthetic_inference.py --matches: every shared layer prints its per-reference figures"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "synthetic_inference.py")
    spec = importlib.util.spec_from_file_location("synthetic_inference_match", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--identities", "2", "--refs", "3", "--px", "256", "--small", "--matches", "--dtype", "bf16"])
    text = capsys.readouterr().out
    assert out.shape == (2, 256, 256, 3)
    assert text.count(": match (2, ") == 9 and "match (2, 1024, 4)" in text and "match (2, 64, 4)" in text, text
    assert text.count("mean best probability per reference") == 9 and text.count("share of tokens whose best match lies in each reference") == 9
