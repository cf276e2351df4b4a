"""``ir_attn_received`` on the GPU: per key of the packed key axis, the sum over ALL query rows of the attention times a per-row
payload - the column sums of P without the dump.

What is held to what:
  1. the library's own read-outs, with NO tolerance: a one-hot channel at row ``i`` rounded to the 16-bit format is row ``i`` of
     ``attn_rows(reduce="none")`` over all of ``Lkv``; of the head mean it is ``attn_rows(reduce="head_mean")``'s row bit for bit;
     ``weights=None`` IS a channel of ones; duplicated channels are equal; the head-mean output IS the ascending fold of the
     per-head output times ``float32(1 / H)``; 1, 2, 3, 5 and 8 channels agree channel by channel with single-channel calls;
  2. ``ops.attn_segment_mass``: per (b, h, segment) the received mass summed over the segment's keys against the masses summed
     over the rows, both in float64: ``<= 1e-4 * len_q`` - the per-row bound the project holds between its two mass
     computations (tests/test_gpu_attn_transfer.py item 2), once per row;
  3. the adjoint of ``ops.attn_transfer``: ``<recv(w), y>`` against ``<w, transfer(y)>``, both contracted in float64, within the sum
     of the two sides' own bounds;
  4. float64, weights of both signs and magnitudes up to 64, with ``A[b,h,j,c] = sum_i p64[i,j] |w[i,c]|`` and
     ``floor = len_q * 2^-126 * max|w|`` (flushed subnormals): ``|recv - ref| <= 1e-4 * A + floor`` against float64 probabilities
     recomputed from the 16-bit inputs and the DEVICE's LSE, ``<= (1e-4 + 2 delta) * A + floor`` against the oracle alone.  The 1e-4 is the
     constant of tests/test_gpu_attn_transfer.py item 3 (about 5e-6 relative per probability plus a summation chain of
     ``(len_q / 32 + 6) * 2^-24 <= 3.1e-5`` up to 16 384 rows); delta = ``lse_bounds.bound`` at the case's largest row scale: the
     device's LSE is within delta of the truth (tests/test_gpu_lse.py), an LSE error multiplies every probability of a row by
     exp(+-delta) and |exp(delta) - 1| <= 2 delta, so both carry over as relative bounds (derived, nothing measured);
  5. addressing and plumbing - weight strides, NaN padding, a batch stride beyond 2^32 elements, NaN behind every segment of K,
     pointer tables, graph replay, batch invariance, pre-scaled Q, the processor, the example: ``torch.equal`` with the plain call;
  6. one identity, one head at the 1024-px layer (16 384 rows: the longest summation chain), item 4's device-LSE bound.
The inputs, the LSE and the float64 probabilities of a (case, dtype) are computed once (shared with tests/test_gpu_attn_match.py)
and never changed."""

import numpy as np
import pytest
import torch

import oracle_ops_received as R
from lse_bounds import case_delta
from test_gpu_attn_match import _setup
from test_gpu_attn_rows import CASES, ODD_CASES, _ids, _rand
from test_gpu_ref_table import _pool_grid, _stack

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
FORMS = ("none", "head_mean")
LN2 = 0.6931471805599453
ALL = CASES + ODD_CASES
TINY = 2.0 ** -126


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


def _call(ops, s, w, form, **extra):
    return ops.attn_received(s["q"], s["k"], s["rk"], s["lse"], w, reduce=form, **s["kw"], **extra)


def _onehot_rows(Lq, want=8):
    """`want` distinct query rows: row 0, the last row, rows 31 / 32 (two row blocks), the first and the last row of a partial last
    block, filled up with further rows"""
    cand = [0, Lq - 1, 31, 32]
    if Lq % 32:
        cand += [Lq // 32 * 32, Lq - 1]
    cand += [Lq // 2, 1, Lq - 2, 33, 63, 64] + list(range(Lq))
    rows = []
    for c in cand:
        if 0 <= c < Lq and c not in rows:
            rows.append(c)
        if len(rows) == want:
            break
    return rows


def _rand_weights(B, Lq, Cn, seed):
    """both signs, magnitudes up to 64 (one element exactly 64)"""
    w = (torch.rand(B, Lq, Cn, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * 64
    w[0, 0, 0] = 64.0
    return w


def _received64(q, k, rk, lse, w, H, inc, scale=0.125, chunk=2048):
    """float64 ``(ref, A)`` on the device, ``(B, H, Lkv, C)`` each: ``sum_i p64[i, j] * w[i, c]`` and ``sum_i p64[i, j] * |w[i, c]|`` with
    probabilities from the 16-bit inputs and the DEVICE's LSE, formed a chunk of rows at a time"""
    B, Lq = q.shape[:2]
    parts = ([k] if inc else []) + ([rk.flatten(1, 2)] if rk is not None else [])
    kk = torch.cat(parts, dim=1).double().reshape(B, -1, H, 64)
    wd = (w if w.dim() == 3 else w[None]).double().expand(B, -1, -1)
    ref = torch.zeros(B, H, kk.shape[1], wd.shape[-1], dtype=torch.float64, device=q.device)
    A = torch.zeros_like(ref)
    for i0 in range(0, Lq, chunk):
        qq = q[:, i0:i0 + chunk].double().reshape(B, -1, H, 64)
        p = torch.exp(torch.einsum("bihd,bjhd->bhij", qq, kk) * scale - lse[:, :, i0:i0 + chunk].double()[..., None])
        ref += torch.einsum("bhij,bic->bhjc", p, wd[:, i0:i0 + chunk])
        A += torch.einsum("bhij,bic->bhjc", p, wd[:, i0:i0 + chunk].abs())
        del p
    return ref, A


def _fold(per_head):
    H = per_head.shape[1]
    inv_h = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32)).to(per_head.device)
    acc = torch.zeros_like(per_head[:, 0])
    for h in range(H):
        acc = acc + per_head[:, h]
    return acc * inv_h


# ---- 1: no tolerance, against the library itself ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_one_hot_channels_are_the_rows_of_attn_rows_bit_for_bit(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    lkv = s["edges"][-1]
    rows = _onehot_rows(Lq)
    w = torch.zeros(Lq, len(rows))
    for c, i in enumerate(rows):
        w[i, c] = 1.0
    w = w.cuda()
    idx = torch.tensor(rows, dtype=torch.int32).expand(B, -1).contiguous().cuda()
    P0 = ops.attn_rows(s["q"], s["k"], s["rk"], s["lse"], idx, reduce="none", **s["kw"])          # (B, H, R, Lkv) in dtype
    HM = ops.attn_rows(s["q"], s["k"], s["rk"], s["lse"], idx, reduce="head_mean", **s["kw"])     # (B, R, Lkv) fp32
    r0, r1 = _call(ops, s, w, "none"), _call(ops, s, w, "head_mean")
    assert r0.shape == (B, H, lkv, len(rows)) and r1.shape == (B, lkv, len(rows)) and r0.dtype == r1.dtype == torch.float32
    assert float(P0.float().max()) > 0
    for c, i in enumerate(rows):
        assert torch.equal(r0[..., c].to(dtype), P0[:, :, c]), f"per-head one-hot channel {c} (row {i}) is not the row of attn_rows"
        assert torch.equal(r1[..., c], HM[:, c]), f"head-mean one-hot channel {c} (row {i}) is not the head-mean row bit for bit"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_ones_duplicates_fold_and_channel_counts(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    lkv = s["edges"][-1]
    # no weights IS a channel of ones, in (L,), (L, 1) and (B, L, 1) clothes
    for form in FORMS:
        plain = _call(ops, s, None, form)
        assert plain.shape[-2:] == (lkv, 1)
        for ones in (torch.ones(Lq, device="cuda"), torch.ones(Lq, 1, device="cuda"), torch.ones(B, Lq, 1, device="cuda")):
            assert torch.equal(_call(ops, s, ones, form), plain), (form, tuple(ones.shape))
        assert float(plain.min()) > 0
    w8 = _rand_weights(B, Lq, 8, seed=41).cuda()
    full = {form: _call(ops, s, w8, form) for form in FORMS}
    # the head mean is the ascending fold of the per-head output
    assert torch.equal(_fold(full["none"]), full["head_mean"]), "the head-mean output is not the fold of the per-head output"
    assert torch.equal(_fold(_call(ops, s, None, "none")), _call(ops, s, None, "head_mean"))
    for form in FORMS:
        # 1, 2, 3, 5 channels: the leading channels of the 8-channel call; every single channel on its own
        for Cn in (1, 2, 3, 5):
            got = _call(ops, s, w8[..., :Cn].contiguous(), form)
            assert torch.equal(got, full[form][..., :Cn]), f"{form}: {Cn} channels disagree with the 8-channel call"
        for c in range(8):
            got = _call(ops, s, w8[..., c].contiguous(), form)
            assert torch.equal(got[..., 0], full[form][..., c]), f"{form}: channel {c} alone disagrees with the 8-channel call"
        # duplicated channels are equal, wherever they stand
        dup = torch.stack([w8[..., 3], w8[..., 0], w8[..., 3], w8[..., 3], w8[..., 0]], dim=-1).contiguous()
        got = _call(ops, s, dup, form)
        assert torch.equal(got[..., 0], got[..., 2]) and torch.equal(got[..., 0], got[..., 3]) and torch.equal(got[..., 1], got[..., 4])
        assert torch.equal(got[..., 0], full[form][..., 3]) and torch.equal(got[..., 1], full[form][..., 0])


# ---- 2: against attn_segment_mass ---------------------------------------------------------------------------------------------------
# The head-mean form shares the heads of an item among the waves of a workgroup, at most 8, in rounds: the case lists above stop at 3
# heads (one round).  8 heads: one full round; 9: two rounds of 5 waves, the second one short; 10 / 20: the model's 2 x 5 and 3 x 7
# with a short last round; 17: three rounds of 6, the last one of 5.  Thin shapes: a partial row block, a key tail, two key groups.
MANY_HEADS = [(2, H, 40, 40, 2, 100, True) for H in (8, 9, 10, 17, 20)]


@pytest.mark.parametrize("case", MANY_HEADS, ids=_ids(MANY_HEADS))
def test_head_mean_with_more_heads_than_waves(ops, case):
    """the fold of the per-head output and the head-mean rows of attn_rows, bit for bit, whatever the number of rounds; all
    channel paddings"""
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, torch.bfloat16)
    w8 = _rand_weights(B, Lq, 8, seed=43).cuda()
    for w in (None, w8[..., :1].contiguous(), w8[..., :2].contiguous(), w8[..., :3].contiguous(), w8[..., :4].contiguous(), w8):
        assert torch.equal(_fold(_call(ops, s, w, "none")), _call(ops, s, w, "head_mean")), None if w is None else tuple(w.shape)
    rows = _onehot_rows(Lq)
    w = torch.zeros(Lq, len(rows))
    for c, i in enumerate(rows):
        w[i, c] = 1.0
    idx = torch.tensor(rows, dtype=torch.int32).expand(B, -1).contiguous().cuda()
    HM = ops.attn_rows(s["q"], s["k"], s["rk"], s["lse"], idx, reduce="head_mean", **s["kw"])     # (B, R, Lkv) fp32
    r1 = _call(ops, s, w.cuda(), "head_mean")
    for c, i in enumerate(rows):
        assert torch.equal(r1[..., c], HM[:, c]), f"head-mean one-hot channel {c} (row {i}) is not the head-mean row bit for bit"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_received_mass_against_segment_mass(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    edges = s["edges"]
    mass = ops.attn_segment_mass(s["q"], s["k"], s["rk"], s["lse"], **s["kw"]).double().sum(dim=2)      # (B, H, S)
    recv = _call(ops, s, None, "none")[..., 0].double()                                                    # (B, H, Lkv)
    got = torch.stack([recv[..., a:b].sum(-1) for a, b in zip(edges[:-1], edges[1:])], dim=-1)
    d = float((got - mass).abs().max())
    print(f"attn_received {_ids([case])[0]} {dtype}: max |sum_j recv - sum_i mass| per segment {d:.3e} (bound {1e-4 * Lq:.1e})")
    assert d <= 1e-4 * Lq


# ---- 3: the adjoint of attn_transfer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_adjoint_of_attn_transfer(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    lkv = s["edges"][-1]
    gen = torch.Generator().manual_seed(29)
    w = ((torch.rand(B, Lq, 1, generator=gen) * 2 - 1) * 64).cuda()
    y = ((torch.rand(B, lkv, 1, generator=gen) * 2 - 1) * 64).cuda()
    recv = _call(ops, s, w, "none")[..., 0].double()                                                       # (B, H, Lkv)
    sums, _ = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], y, None, reduce="none", **s["kw"])     # (B, H, Lq, S, 1)
    lhs = torch.einsum("bhj,bj->bh", recv, y[..., 0].double())
    rhs = torch.einsum("bi,bhi->bh", w[..., 0].double(), sums[..., 0].double().sum(-1))
    _, A = _received64(s["q"], s["k"], s["rk"], s["lse"], w, H, inc)
    floor = Lq * TINY * float(w.abs().max())
    ymax = y.abs().amax(dim=(1, 2)).double()                                                                # (B,)
    bound = 1e-4 * ymax[:, None] * w[..., 0].double().abs().sum(-1)[:, None] + \
        torch.einsum("bhj,bj->bh", 1e-4 * A[..., 0] + floor, y[..., 0].double().abs())
    ratio = float(((lhs - rhs).abs() / bound).max())
    print(f"attn_received {_ids([case])[0]} {dtype}: adjoint |<recv, y> - <w, transfer>| / bound {ratio:.3e}")
    assert bool(((lhs - rhs).abs() <= bound).all()), ratio


# ---- 4: float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_float64_parity(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    ob = 1e-4 + 2 * case_delta(s["q"], s["k"], s["rk"], H, 0.125, inc)      # against the oracle alone: the device-LSE bound + 2 delta
    for n, Cn in enumerate((1, 2, 5, 8)):
        w = _rand_weights(B, Lq, Cn, seed=50 + n)
        wmax = float(w.abs().max())
        floor = Lq * TINY * wmax
        wd = w.cuda()
        ref, A = _received64(s["q"], s["k"], s["rk"], s["lse"], wd, H, inc)
        o0, o1 = R.received_np(s["p64"], w)
        oA0, oA1 = R.received_np(s["p64"], w.abs())
        for form, r, a, oo, oa in (("none", ref, A, o0, oA0), ("head_mean", ref.mean(1), A.mean(1), o1, oA1)):
            got = _call(ops, s, wd, form).double()
            ra = float(((got - r).abs() / (1e-4 * a + floor)).max())
            gn = got.cpu().numpy()
            rb = float((np.abs(gn - oo) / (ob * oa + floor)).max())
            print(f"attn_received {_ids([case])[0]} {dtype} C={Cn} {form}: largest |recv - ref| / bound: {ra:.3e} vs float64 with the device's LSE "
                  f"(1e-4 * A + floor), {rb:.3e} vs the oracle ({ob:.2e} * A + floor)")
            assert bool(((got - r).abs() <= 1e-4 * a + floor).all()), (form, Cn, ra)
            assert bool((np.abs(gn - oo) <= ob * oa + floor).all()), (form, Cn, rb)


# ---- 5: addressing and plumbing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_weight_shapes_and_strides(ops, dtype):
    case = CASES[0]                                                          # 72 rows: a partial row block behind len_q
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    Cn = 3
    gen = torch.Generator().manual_seed(3)
    w2 = ((torch.rand(Lq, Cn, generator=gen) * 2 - 1) * 64).cuda()
    wb = ((torch.rand(B, Lq, Cn, generator=gen) * 2 - 1) * 64).cuda()
    for form in FORMS:
        want = _call(ops, s, w2[None].expand(B, -1, -1).contiguous(), form)
        for w in (w2, w2[None], w2[None].expand(B, -1, -1)):                  # a stride-0 batch
            assert torch.equal(_call(ops, s, w, form), want), (form, tuple(w.shape), w.stride())
        # rows of a wider buffer, NaN in the padding between the rows, before the first row and behind len_q (40 more rows)
        want = _call(ops, s, wb, form)
        buf = torch.full((B, Lq + 41, 8), float("nan"), device="cuda")
        buf[:, 1:Lq + 1, 2:2 + Cn] = wb
        view = buf[:, 1:Lq + 1, 2:2 + Cn]
        assert view.stride() == ((Lq + 41) * 8, 8, 1) and torch.equal(view, wb)
        got = _call(ops, s, view, form)
        assert torch.equal(got, want) and bool(torch.isfinite(got).all()), form
        # one channel as a column of that buffer
        assert torch.equal(_call(ops, s, buf[:, 1:Lq + 1, 3], form)[..., 0], want[..., 1]), form


def test_weight_batch_stride_beyond_32_bits(ops):
    """ONE allocation of 2^32 + 64 + Lq * C floats, NaN-filled, viewed as (2, Lq, C) with a batch stride of 2^32 + 64 elements and
    different rows per entry: every 32-bit truncation of entry 1's offset, in elements or bytes, signed or unsigned, lands inside
    the allocation - on entry 0's rows or on the fill - so a 32-bit offset shows as a mismatch, never as a fault"""
    dtype = torch.bfloat16
    case = CASES[0]
    B, H, Lq, Ls, N, Lr, inc = case
    assert B == 2
    s = _setup(case, dtype)
    Cn = 4
    far = 2 ** 32 + 64
    assert Lq * Cn > 64
    w = ((torch.rand(B, Lq, Cn, generator=torch.Generator().manual_seed(5)) * 2 - 1) * 64).cuda()
    buf = torch.full((far + Lq * Cn,), float("nan"), device="cuda")
    view = buf.as_strided((B, Lq, Cn), (far, Cn, 1))
    view.copy_(w)
    assert torch.equal(view, w) and view.stride(0) == far
    for form in FORMS:
        assert torch.equal(_call(ops, s, view, form), _call(ops, s, w, form)), form
    del buf, view


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], ODD_CASES[0], ODD_CASES[2]], ids=_ids([CASES[0], CASES[3], ODD_CASES[0], ODD_CASES[2]]))
def test_nan_behind_every_segment_and_behind_the_last_row(ops, case, dtype):
    """K and Q as views into larger NaN-filled buffers: the key behind every segment's last key and the row behind the last query
    row hold NaN - a tail that was read and counted would show"""
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    Cc = H * 64
    kbuf = torch.full((B, Ls + 1, Cc), float("nan"), dtype=dtype, device="cuda")
    kbuf[:, :Ls] = s["k"]
    rbuf = torch.full((B, N, Lr + 1, Cc), float("nan"), dtype=dtype, device="cuda")
    rbuf[:, :, :Lr] = s["rk"]
    qbuf = torch.full((B, Lq + 1, Cc), float("nan"), dtype=dtype, device="cuda")
    qbuf[:, :Lq] = s["q"]
    kv, rv, qv = kbuf[:, :Ls], rbuf[:, :, :Lr], qbuf[:, :Lq]
    assert kv.data_ptr() == kbuf.data_ptr() and rv.data_ptr() == rbuf.data_ptr() and qv.data_ptr() == qbuf.data_ptr()    # views, no copies
    w = _rand_weights(B, Lq, 2, seed=61).cuda()
    for form in FORMS:
        for ww in (None, w):
            want = _call(ops, s, ww, form)
            got = ops.attn_received(qv, kv, rv, s["lse"], ww, reduce=form, **s["kw"])
            assert torch.equal(got, want) and bool(torch.isfinite(got).all()), (form, ww is None)


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
    w = ((torch.rand(B, Lq, 2, generator=g) * 2 - 1) * 64).cuda()
    for form in FORMS:
        for ww in (None, w):
            a = ops.attn_received(q, ks, tk, lse, ww, reduce=form, **kw)
            b = ops.attn_received(q, ks, dk, lse, ww, reduce=form, **kw)
            assert torch.equal(a, b), (form, ww is None)


def test_graph_replay_follows_the_weights_and_the_table(ops):
    dtype = torch.bfloat16
    B, H, Lq, N, Lr = 2, 2, 200, 3, 72
    g = torch.Generator().manual_seed(9)
    q, ks, vs = (torch.randn(B, Lq, H * 64, generator=g).to("cuda", dtype) for _ in range(3))
    gk0, gv0 = _pool_grid(g, B, N, Lr, H * 64, dtype)
    gk1, gv1 = _pool_grid(g, B, N, Lr, H * 64, dtype, scale=0.7, shift=0.1)
    kw = dict(heads=H, scale=0.125, include_self=True)
    lse0 = ops.shared_attention(q, ks, vs, _stack(gk0), _stack(gv0), return_lse=True, **kw)[1]
    lse1 = ops.shared_attention(q, ks, vs, _stack(gk1), _stack(gv1), return_lse=True, **kw)[1]
    w0, w1 = (((torch.rand(B, Lq, 3, generator=g) * 2 - 1) * 64).cuda() for _ in range(2))
    for form in FORMS:
        tk = ops.RefKVTable.from_tensors(gk0)
        static_lse, static_w = lse0.clone(), w0.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.attn_received(q, ks, tk, static_lse, static_w, reduce=form, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.attn_received(q, ks, tk, static_lse, static_w, reduce=form, **kw)
        graph.replay()
        torch.cuda.synchronize()
        want0 = ops.attn_received(q, ks, _stack(gk0), lse0, w0, reduce=form, **kw)
        assert torch.equal(out, want0), form
        static_lse.copy_(lse1)
        static_w.copy_(w1)
        tk.fill_(gk1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want1 = ops.attn_received(q, ks, _stack(gk1), lse1, w1, reduce=form, **kw)
        assert torch.equal(out, want1), form
        assert not torch.equal(want0, want1)
        del graph


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_batch_invariance(ops, dtype):
    """an entry's bytes are the same alone and at another position of a larger batch, in both forms, with and without the
    (accepted, inert) flag"""
    case = (3, 2, 72, 72, 3, 40, True)
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    w = _rand_weights(B, Lq, 2, seed=8).cuda()
    take = [2, 0, 1, 0]                                                                # entry b of the batch of 3 at position i of a batch of 4
    c = lambda t: t.contiguous()
    for ww in (None, w):
        for form in FORMS:
            a = _call(ops, s, ww, form)
            assert torch.equal(_call(ops, s, ww, form, batch_invariant=True), a)
            for b in range(B):
                one = ops.attn_received(c(s["q"][b:b + 1]), c(s["k"][b:b + 1]), c(s["rk"][b:b + 1]), c(s["lse"][b:b + 1]),
                                        None if ww is None else c(ww[b:b + 1]), reduce=form, **s["kw"])
                assert torch.equal(one[0], a[b]), (form, b)
            big = ops.attn_received(c(s["q"][take]), c(s["k"][take]), c(s["rk"][take]), c(s["lse"][take]),
                                    None if ww is None else c(ww[take]), reduce=form, **s["kw"])
            for i, b in enumerate(take):
                assert torch.equal(big[i], a[b]), (form, i, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_prescaled_q(ops, dtype):
    """IR_FLAG_Q_PRESCALED: the one-hot identity under the flag, and the plain call on that query with scale = ln 2 gives the same bytes"""
    B, H, L, N, Lr = 2, 2, 72, 3, 40
    gen = torch.Generator().manual_seed(11)
    q = _rand((B, L, H * 64), dtype, gen, 1.5)
    qs = (q.float() * (0.125 * 1.4426950408889634)).to(dtype).cuda()
    k, v = _rand((B, L, H * 64), dtype, gen, 1.5).cuda(), _rand((B, L, H * 64), dtype, gen).cuda()
    rk, rv = _rand((B, N, Lr, H * 64), dtype, gen, 1.5).cuda(), _rand((B, N, Lr, H * 64), dtype, gen).cuda()
    _, lse = ops.shared_attention(qs, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True, q_prescaled=True)
    rows = _onehot_rows(L)
    w = torch.zeros(L, len(rows))
    for c, i in enumerate(rows):
        w[i, c] = 1.0
    w = w.cuda()
    idx = torch.tensor(rows, dtype=torch.int32).expand(B, -1).contiguous().cuda()
    kw = dict(heads=H, scale=0.125, include_self=True, q_prescaled=True)
    P0 = ops.attn_rows(qs, k, rk, lse, idx, reduce="none", **kw)
    HM = ops.attn_rows(qs, k, rk, lse, idx, reduce="head_mean", **kw)
    r0 = ops.attn_received(qs, k, rk, lse, w, reduce="none", **kw)
    r1 = ops.attn_received(qs, k, rk, lse, w, reduce="head_mean", **kw)
    for c in range(len(rows)):
        assert torch.equal(r0[..., c].to(dtype), P0[:, :, c]) and torch.equal(r1[..., c], HM[:, c]), c
    for form, a in (("none", r0), ("head_mean", r1)):
        b = ops.attn_received(qs, k, rk, lse, w, heads=H, scale=LN2, include_self=True, reduce=form)
        assert torch.equal(a, b), form


def test_through_the_plugin_surface(ops, monkeypatch):
    """``attention_received_weights`` on a shared layer: the result is ``ops.attn_received`` on that layer's q / k / lse (caught on
    their way into the call), agrees with the dump of the same forward, and leaves ``attention_mass`` and the layer output as they
    were bit for bit"""
    import instantrestore_amd.attn_processors as ap
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    seen = []
    real = ops.attn_received

    def spy(*a, **kw):
        seen.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ap._ops, "attn_received", spy)
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
        lkv = (N + int(train_input)) * L
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            proc.save_attention_mass = True
            y0 = run()
            mass0 = proc.attention_mass.clone()
            assert proc.attention_received is None and not seen
            proc.attention_received_weights, proc.save_self_attentions = "ones", True
            y1 = run()
            assert len(seen) == 1
            (a, kw) = seen.pop()
            assert a[4] is None and kw["reduce"] == "head_mean"
            recv = proc.attention_received
            assert recv.shape == (B, lkv, 1) and torch.equal(recv, real(*a, **kw))
            assert torch.equal(proc.attention_mass, mass0) and torch.equal(y0, y1)
            # every probability of the dump carries one bf16 rounding (2^-9 relative): 2^-9 * the column sum
            dump = proc.attention_probs.double()
            ref = dump.sum(dim=-2).mean(dim=1)
            assert bool(((recv[..., 0].double() - ref).abs() <= 2.0 ** -9 * ref + 1e-4 * L).all())
            w = torch.rand(B, L, 3, device="cuda")
            proc.attention_received_weights, proc.attention_received_reduce = w, "none"
            run()
            (a, kw) = seen.pop()
            assert a[4] is w and kw["reduce"] == "none"
            r2 = proc.attention_received
            assert r2.shape == (B, H, lkv, 3) and torch.equal(r2, real(*a, **kw))
            ref = torch.einsum("bhij,bic->bhjc", proc.attention_probs.double(), w.double())
            assert bool(((r2.double() - ref).abs() <= 2.0 ** -9 * ref + 1e-4 * L).all())


def test_example_received_switch(capsys):
    """examples/synthetic_inference.py --received --prune: every shared layer prints its per-reference received mass, and the
    route warm-up frame -> keep_from_received -> compact_refs -> counted call runs"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "synthetic_inference.py")
    spec = importlib.util.spec_from_file_location("synthetic_inference_received", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--identities", "2", "--refs", "3", "--px", "256", "--small", "--received", "--prune", "0.5", "--dtype", "bf16"])
    text = capsys.readouterr().out
    assert out.shape == (2, 256, 256, 3)
    assert text.count(": received (2, ") == 9 and "received (2, 4096, 1)" in text and "received (2, 256, 1)" in text, text
    assert text.count("received mass [self?] ++ references") == 9
    assert text.count("pruned to [512, 512, 512] of 1024 tokens by received attention") == 2, text


# ---- 6: one real-shape slice ---------------------------------------------------------------------------------------------------------
def test_1024px_layer_one_identity_one_head(ops):
    """the 1024-px top shared layer for one identity and one head (L = Ls = Lr = 16384, N = 4, bf16, 1 and 2 channels): the shape the
    dump cannot serve and the longest summation chain (512 row blocks per lane), held to float64 with the device's LSE"""
    dtype = torch.bfloat16
    B, H, L, N = 1, 1, 16384, 4
    g = torch.Generator(device="cuda").manual_seed(2)
    q = (torch.randn(B, L, 64, device="cuda", generator=g) * 1.2).to(dtype)
    k = torch.randn(B, L, 64, device="cuda", generator=g).to(dtype)
    v = torch.randn(B, L, 64, device="cuda", generator=g).to(dtype)
    rk = torch.randn(B, N, L, 64, device="cuda", generator=g).to(dtype)
    rv = torch.randn(B, N, L, 64, device="cuda", generator=g).to(dtype)
    kw = dict(heads=H, scale=0.125, include_self=True)
    _, lse = ops.shared_attention(q, k, v, rk, rv, return_lse=True, **kw)
    w = _rand_weights(B, L, 2, seed=71).cuda()
    floor = L * TINY * float(w.abs().max())
    ref, A = _received64(q, k, rk, lse, w, H, True, chunk=1024)
    for Cn in (1, 2):
        for form in FORMS:
            got = ops.attn_received(q, k, rk, lse, w[..., :Cn].contiguous(), reduce=form, **kw).double()
            r, a = (ref[..., :Cn], A[..., :Cn]) if form == "none" else (ref[..., :Cn].mean(1), A[..., :Cn].mean(1))
            ratio = float(((got - r).abs() / (1e-4 * a + floor)).max())
            print(f"attn_received 1024px C={Cn} {form}: largest |recv - ref| / (1e-4 * A + floor) vs float64 with the device's LSE {ratio:.3e}")
            assert bool(((got - r).abs() <= 1e-4 * a + floor).all()), (form, Cn, ratio)
