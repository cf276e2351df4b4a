"""``ir_attn_transfer`` on the GPU: per K/V segment, the attention-weighted sums of a per-key payload and the segment's mass for
chosen query tokens.

What is held to what:
  1. the library's own read-outs, with NO tolerance: a one-hot channel rounded to the 16-bit format is the element of
     ``attn_rows(reduce="none")`` at its key and exactly 0 in every other segment; the head-mean sums of a one-hot channel are the
     element of ``attn_rows(reduce="head_mean")`` bit for bit; a channel of ones IS the mass; the head-mean output IS the ascending
     fold of the per-head output times ``float32(1 / H)``;
  2. the mass against ``ops.attn_segment_mass``: 1e-4, the bound the project holds between its two mass computations
     (tests/test_gpu_seg_mass.py: the same fp32 arithmetic in another summation order);
  3. float64, payloads of both signs and magnitudes up to 64 (coordinates): ``|sums - ref| <= 1e-4 * max|y|`` against float64
     probabilities recomputed from the 16-bit inputs and the DEVICE's LSE (only fp32 rounding separates the two: about 5e-6
     relative per probability plus the summation, the 1e-4 of item 2), and ``<= (1e-4 + 2 delta) * max|y|`` against the oracle alone
     (mass: ``1e-4 + 2 delta``), delta = ``lse_bounds.bound`` at the case's largest row scale: the device's LSE is within delta of
     the truth (tests/test_gpu_lse.py), so every device-LSE probability is the true one times exp(+-delta), |exp(delta) - 1| <=
     2 delta - derived, nothing measured (delta is about 1e-5 where the former constant was 2e-3);
  4. tails, payload addressing (strides, NaN padding, a batch stride beyond 2^32 elements), invalid rows, pointer tables, graph
     replay, batch invariance, the processor: ``torch.equal`` with the plain call.
The inputs, the LSE and the float64 probabilities of a (case, dtype) are computed once (shared with tests/test_gpu_attn_match.py)
and never changed."""

import numpy as np
import pytest
import torch

import oracle_ops_transfer as T
from lse_bounds import case_delta
from test_gpu_attn_match import _setup
from test_gpu_attn_rows import CASES, ODD_CASES, _case_inputs, _gpu_lse, _ids, _indices, _oracle_probs, _rand  # noqa: F401
from test_gpu_ref_table import _pool_grid, _stack

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
FORMS = ("none", "head_mean")
LN2 = 0.6931471805599453
ALL = CASES + ODD_CASES


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


def _row_lists(B, Lq):
    """1, 5, 68 and min(200, Lq) rows (more than 96: two row groups of three 32-row blocks) with forced duplicates, and every
    row (None)"""
    return [_indices(B, Lq, R, seed=100 + R) for R in sorted({min(r, Lq) for r in (1, 5, 68, 200)})] + [None]


def _rows_of(idx, B, Lq):
    return torch.arange(Lq, dtype=torch.int32).expand(B, -1).contiguous() if idx is None else idx


def _dev(idx):
    return None if idx is None else idx.cuda()


def _onehot_keys(edges, want=8):
    """`want` keys of the packed key axis: the first and the last key of segments, keys 15 / 16 and 31 / 32 of a block, a key of a
    partial last block, keys of different segments - as many of those as the case has, filled up with further keys"""
    S = len(edges) - 1
    lens = [b - a for a, b in zip(edges[:-1], edges[1:])]
    cand = [edges[0], edges[1] - 1]                                                        # first and last key of segment 0
    big = max(range(S), key=lambda s: (lens[s], s))                                        # the (last) longest segment
    cand += [edges[big] + j for j in (15, 16, 31, 32) if j < lens[big]]
    last = S - 1
    cand += [edges[last + 1] - 1]                                                          # the last key of the key axis
    if lens[last] % 32 > 1:
        cand += [edges[last + 1] - (lens[last] % 32)]                                      # the first key of the partial last block
    cand += [edges[s] + lens[s] // 2 for s in range(S)]                                    # one key inside every segment
    cand += list(range(edges[-1]))
    keys = []
    for c in cand:
        if 0 <= c < edges[-1] and c not in keys:
            keys.append(c)
        if len(keys) == want:
            break
    return keys


def _onehot_payload(keys, lkv):
    y = torch.zeros(lkv, len(keys))
    for c, key in enumerate(keys):
        y[key, c] = 1.0
    return y.cuda()


def _seg_of(key, edges):
    return max(s for s in range(len(edges) - 1) if edges[s] <= key)


def _check_onehot(ops, q, k, rk, lse, idx, edges, dtype, what, **kw):
    """item 1 of the module docstring (one-hot channels) on one row list"""
    B, Lq = q.shape[0], q.shape[1]
    rows = _rows_of(idx, B, Lq).cuda()
    keys = _onehot_keys(edges)
    y = _onehot_payload(keys, edges[-1])
    P0 = ops.attn_rows(q, k, rk, lse, rows, reduce="none", **kw)
    HM = ops.attn_rows(q, k, rk, lse, rows, reduce="head_mean", **kw)
    s0, m0 = ops.attn_transfer(q, k, rk, lse, y, _dev(idx), reduce="none", **kw)
    s1, m1 = ops.attn_transfer(q, k, rk, lse, y, _dev(idx), reduce="head_mean", **kw)
    R, S, H = rows.shape[1], len(edges) - 1, P0.shape[1]
    assert s0.shape == (B, H, R, S, len(keys)) and m0.shape == (B, H, R, S) and s1.shape == (B, R, S, len(keys)) and m1.shape == (B, R, S), what
    assert s0.dtype == m0.dtype == s1.dtype == m1.dtype == torch.float32
    for c, key in enumerate(keys):
        own = _seg_of(key, edges)
        assert torch.equal(s0[..., own, c].to(dtype), P0[..., key]), f"{what}: per-head one-hot channel {c} (key {key}) is not the rows' element"
        assert torch.equal(s1[..., own, c], HM[..., key]), f"{what}: head-mean one-hot channel {c} (key {key}) is not the head-mean rows' element bit for bit"
        for s in range(S):
            if s != own:
                assert not bool(s0[..., s, c].any()) and not bool(s1[..., s, c].any()), f"{what}: channel {c} (key {key}) leaks into segment {s}"


# ---- 1: one-hot payloads, no tolerance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_one_hot_payloads_are_the_rows_elements_bit_for_bit(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    for idx in _row_lists(B, Lq):
        _check_onehot(ops, s["q"], s["k"], s["rk"], s["lse"], idx, s["edges"], dtype,
                      f"{_ids([case])[0]} {dtype} R={'all' if idx is None else idx.shape[1]}", **s["kw"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_one_hot_payloads_with_a_prescaled_q(ops, dtype):
    """IR_FLAG_Q_PRESCALED: the same identities under the flag, and the plain call on that query with scale = ln 2 gives the same bytes"""
    B, H, L, N, Lr = 2, 2, 72, 3, 40
    gen = torch.Generator().manual_seed(11)
    q = _rand((B, L, H * 64), dtype, gen, 1.5)
    qs = (q.float() * (0.125 * 1.4426950408889634)).to(dtype).cuda()
    k, v = _rand((B, L, H * 64), dtype, gen, 1.5).cuda(), _rand((B, L, H * 64), dtype, gen).cuda()
    rk, rv = _rand((B, N, Lr, H * 64), dtype, gen, 1.5).cuda(), _rand((B, N, Lr, H * 64), dtype, gen).cuda()
    _, lse = ops.shared_attention(qs, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True, q_prescaled=True)
    edges = T.segment_edges(L, N, Lr, True)
    y = _onehot_payload(_onehot_keys(edges), edges[-1])
    for idx in (None, _indices(B, L, 68, seed=31)):
        _check_onehot(ops, qs, k, rk, lse, idx, edges, dtype, f"prescaled {dtype}", heads=H, scale=0.125, include_self=True, q_prescaled=True)
        for form in FORMS:
            a = ops.attn_transfer(qs, k, rk, lse, y, _dev(idx), heads=H, scale=0.125, include_self=True, q_prescaled=True, reduce=form)
            b = ops.attn_transfer(qs, k, rk, lse, y, _dev(idx), heads=H, scale=LN2, include_self=True, reduce=form)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), form


# ---- 2, 3: the mass contract, the head mean as the fold of the per-head output ------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_mass_contract_and_head_mean_fold(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    lkv = s["edges"][-1]
    full = ops.attn_segment_mass(s["q"], s["k"], s["rk"], s["lse"], **s["kw"])                # (B, H, Lq, S)
    gen = torch.Generator().manual_seed(17)
    inv_h = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32)
    for n, idx in enumerate(_row_lists(B, Lq)):
        rows = _rows_of(idx, B, Lq).cuda()
        Cn = (8, 3, 1, 5, 2)[n % 5]
        # a payload of ones: every channel IS the mass
        ones = torch.ones(lkv, Cn, device="cuda")
        out = {form: ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], ones, _dev(idx), reduce=form, **s["kw"]) for form in FORMS}
        for form in FORMS:
            sums, mass = out[form]
            for c in range(Cn):
                assert torch.equal(sums[..., c], mass), f"{form}: channel {c} of an all-ones payload is not the mass"
        want = torch.stack([full[b][:, rows[b].long()] for b in range(B)])                      # (B, H, R, S)
        d = float((out["none"][1] - want).abs().max())
        print(f"attn_transfer {_ids([case])[0]} {dtype} R={rows.shape[1]}: max |mass - attn_segment_mass| {d:.3e} (bound 1e-4)")
        assert d <= 1e-4
        # the head mean is the ascending fold of the per-head output, for sums and mass, on a random payload
        y = ((torch.rand(B, lkv, Cn, generator=gen) * 2 - 1) * 64).cuda()
        s0, m0 = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], y, _dev(idx), reduce="none", **s["kw"])
        s1, m1 = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], y, _dev(idx), reduce="head_mean", **s["kw"])
        for per_head, mean in ((s0, s1), (m0, m1)):
            acc = torch.zeros_like(per_head[:, 0])
            for h in range(H):
                acc = acc + per_head[:, h]
            assert torch.equal(acc * inv_h.cuda(), mean), "the head-mean output is not the fold of the per-head output"


# ---- 4: float64 parity ------------------------------------------------------------------------------------------------------------
def _p64_device_lse(q, k, rk, lse, rows, H, inc, scale=0.125):
    """float64 probabilities of the rows ``rows`` (B, R) from the 16-bit inputs and the DEVICE's LSE: (B, H, R, Lkv) on the device"""
    B = q.shape[0]
    parts = ([k] if inc else []) + ([rk.flatten(1, 2)] if rk is not None else [])
    kk = torch.cat(parts, dim=1).double().reshape(B, -1, H, 64)
    qq = torch.stack([q[b, rows[b].long()] for b in range(B)]).double().reshape(B, -1, H, 64)
    ll = torch.stack([lse[b][:, rows[b].long()] for b in range(B)]).double()                       # (B, H, R)
    return torch.exp(torch.einsum("brhd,bjhd->bhrj", qq, kk) * scale - ll[..., None])


def _transfer64(p, y, edges):
    """float64 sums and masses per segment of (B, H, R, Lkv) probabilities on the device; y (B | 1, Lkv, C) or (Lkv, C)"""
    y = (y if y.dim() == 3 else y[None]).double().expand(p.shape[0], -1, -1)
    sums = torch.stack([torch.einsum("bhrj,bjc->bhrc", p[..., a:b], y[:, a:b]) for a, b in zip(edges[:-1], edges[1:])], dim=-2)
    mass = torch.stack([p[..., a:b].sum(-1) for a, b in zip(edges[:-1], edges[1:])], dim=-1)
    return sums, mass


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_float64_parity(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    edges, lkv = s["edges"], s["edges"][-1]
    gen = torch.Generator().manual_seed(23)
    ob = 1e-4 + 2 * case_delta(s["q"], s["k"], s["rk"], H, 0.125, inc)      # against the oracle alone: the device-LSE bound + 2 delta
    for n, idx in enumerate(_row_lists(B, Lq)):
        rows = _rows_of(idx, B, Lq).cuda()
        Cn = (2, 5, 8, 3, 4)[n % 5]
        y = ((torch.rand(B, lkv, Cn, generator=gen) * 2 - 1) * 64)
        y[0, 0, 0] = 64.0
        ymax = float(y.abs().max())
        yd = y.cuda()
        ref_s, ref_m = _transfer64(_p64_device_lse(s["q"], s["k"], s["rk"], s["lse"], rows, H, inc), yd, edges)
        o_s, o_m, o_shm, o_mhm = T.transfer_np(T.gather_rows(s["p64"], rows.cpu().numpy()), y, edges)
        got = {form: ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], yd, _dev(idx), reduce=form, **s["kw"]) for form in FORMS}
        for form, r_s, r_m, oo_s, oo_m in (("none", ref_s, ref_m, o_s, o_m), ("head_mean", ref_s.mean(1), ref_m.mean(1), o_shm, o_mhm)):
            sums, mass = got[form]
            da = float((sums.double() - r_s).abs().max())
            dm = float((mass.double() - r_m).abs().max())
            db = float(np.abs(sums.cpu().numpy().astype(np.float64) - oo_s).max())
            dbm = float(np.abs(mass.cpu().numpy().astype(np.float64) - oo_m).max())
            print(f"attn_transfer {_ids([case])[0]} {dtype} R={rows.shape[1]} C={Cn} {form}: vs float64 with the device's LSE sums {da:.3e} "
                  f"(bound {1e-4 * ymax:.1e}) mass {dm:.3e} (1e-4); vs the oracle sums {db:.3e} (bound {ob * ymax:.1e}) mass {dbm:.3e} ({ob:.2e})")
            assert da <= 1e-4 * ymax and dm <= 1e-4, (form, da, dm)
            assert db <= ob * ymax and dbm <= ob, (form, db, dbm)
            ns, nm = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], yd, _dev(idx), reduce=form, normalize=True, **s["kw"])
            want = torch.where(mass[..., None] > 0, sums / mass[..., None], torch.zeros_like(sums))
            assert torch.equal(ns, want) and torch.equal(nm, mass), f"{form}: normalize=True is not sums / mass of the plain call"


# ---- 5: tails do not count twice -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("length", [33, 37, 40, 1])
def test_tails_do_not_count_twice(ops, length, dtype):
    """the payload is 0 everywhere except the last key of each segment, where load_k's clamp would read the same key again for
    every missing key of the block: the result is the one-hot value, not a multiple of it"""
    case = (1, 2, 40, length, 2, length, True)
    B, H, Lq, Ls, N, Lr, inc = case
    q, k, v, rk, rv = _case_inputs(case, dtype, seed=7)
    qd, kd, rkd, lse = _gpu_lse(ops, q, k, v, rk, rv, H, inc)
    kw = dict(heads=H, scale=0.125, include_self=inc)
    edges = T.segment_edges(Ls, N, Lr, inc)
    y = torch.zeros(edges[-1], 1)
    for e in edges[1:]:
        y[e - 1, 0] = 1.0
    rows = torch.arange(Lq, dtype=torch.int32).expand(B, -1).contiguous().cuda()
    P0 = ops.attn_rows(qd, kd, rkd, lse, rows, reduce="none", **kw)
    HM = ops.attn_rows(qd, kd, rkd, lse, rows, reduce="head_mean", **kw)
    s0, m0 = ops.attn_transfer(qd, kd, rkd, lse, y.cuda(), None, reduce="none", **kw)
    s1, _ = ops.attn_transfer(qd, kd, rkd, lse, y.cuda(), None, reduce="head_mean", **kw)
    full = ops.attn_segment_mass(qd, kd, rkd, lse, **kw)
    for si, e in enumerate(edges[1:]):
        assert float(P0[..., e - 1].float().max()) > 0
        assert torch.equal(s0[..., si, 0].to(dtype), P0[..., e - 1]) and torch.equal(s1[..., si, 0], HM[..., e - 1]), (length, si)
    assert float((m0 - full).abs().max()) <= 1e-4                                        # (a mass that counts a tail twice is off by a probability)


# ---- 6: payload addressing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_payload_shapes_and_strides(ops, dtype):
    case = CASES[0]
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    lkv, Cn = s["edges"][-1], 3
    gen = torch.Generator().manual_seed(3)
    y2 = ((torch.rand(lkv, Cn, generator=gen) * 2 - 1) * 64).cuda()
    yb = ((torch.rand(B, lkv, Cn, generator=gen) * 2 - 1) * 64).cuda()
    idx = _indices(B, Lq, 68, seed=4).cuda()
    for form in FORMS:
        call = lambda y: ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], y, idx, reduce=form, **s["kw"])
        want = call(y2[None].expand(B, -1, -1).contiguous())
        for y in (y2, y2[None]):
            got = call(y)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (form, tuple(y.shape))
        # a row stride wider than C, NaN in the padding, before the first row and after the last
        want = call(yb)
        buf = torch.full((B, lkv + 2, 8), float("nan"), device="cuda")
        buf[:, 1:lkv + 1, 2:2 + Cn] = yb
        view = buf[:, 1:lkv + 1, 2:2 + Cn]
        assert view.stride() == ((lkv + 2) * 8, 8, 1) and torch.equal(view, yb)
        got = call(view)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), form
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


def test_payload_batch_stride_beyond_32_bits(ops):
    """ONE allocation of 2^32 + 64 + Lkv * C floats, NaN-filled, viewed as (2, Lkv, C) with a batch stride of 2^32 + 64 elements and
    different rows per entry: every 32-bit truncation of entry 1's offset, in elements or bytes, signed or unsigned, lands inside
    the allocation - on entry 0's rows or on the fill - so a 32-bit offset shows as a mismatch, never as a fault"""
    dtype = torch.bfloat16
    case = CASES[0]
    B, H, Lq, Ls, N, Lr, inc = case
    assert B == 2
    s = _setup(case, dtype)
    lkv, Cn = s["edges"][-1], 4
    far = 2 ** 32 + 64
    assert lkv * Cn > 64
    gen = torch.Generator().manual_seed(5)
    y = ((torch.rand(B, lkv, Cn, generator=gen) * 2 - 1) * 64).cuda()
    buf = torch.full((far + lkv * Cn,), float("nan"), device="cuda")
    view = buf.as_strided((B, lkv, Cn), (far, Cn, 1))
    view.copy_(y)
    assert torch.equal(view, y) and view.stride(0) == far
    idx = _indices(B, Lq, 68, seed=6).cuda()
    for form in FORMS:
        want = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], y, idx, reduce=form, **s["kw"])
        got = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], view, idx, reduce=form, **s["kw"])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), form
    del buf, view


# ---- 7: invalid rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_invalid_rows_give_zeros_and_leave_their_neighbours_alone(ops, dtype):
    """indices -1 and len_q on the device: sums 0, mass 0.  q is a view into a larger NaN-filled buffer, so the rows those indices
    would address hold NaN - and nothing changes for the other rows"""
    case = CASES[0]
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    buf = torch.full((B, Lq + 2, H * 64), float("nan"), dtype=dtype, device="cuda")
    buf[:, 1:Lq + 1] = s["q"]
    qv = buf[:, 1:Lq + 1]
    R = 40
    idx = _indices(B, Lq, R, seed=9)
    bad = idx.clone()
    bad[:, 3], bad[:, 17], bad[:, R - 1] = -1, Lq, Lq
    bad[1, 20] = -1
    keep = (bad == idx).cuda()
    y = ((torch.rand(s["edges"][-1], 5, generator=torch.Generator().manual_seed(2)) * 2 - 1) * 64).cuda()
    for form in FORMS:
        s_ok, m_ok = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], y, idx.cuda(), reduce=form, **s["kw"])
        s_bad, m_bad = ops.attn_transfer(qv, s["k"], s["rk"], s["lse"], y, bad.cuda(), reduce=form, **s["kw"])
        sel = (keep[:, None, :, None] if form == "none" else keep[:, :, None]).expand_as(m_ok)
        assert torch.equal(m_bad[sel], m_ok[sel]) and torch.equal(s_bad[sel], s_ok[sel]), form
        assert bool((m_bad[~sel] == 0).all()) and bool((s_bad[~sel] == 0).all()), form
        assert bool(torch.isfinite(s_bad).all()) and bool(torch.isfinite(m_bad).all())
        assert float(m_ok.min()) > 0


# ---- 8: plumbing ------------------------------------------------------------------------------------------------------------------------
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
    y = ((torch.rand(B, Lq + N * Lr, 2, generator=g) * 2 - 1) * 64).cuda()
    for form in FORMS:
        for rows in (None, torch.tensor([[0, 5, 127], [64, 3, 3]])):
            a = ops.attn_transfer(q, ks, tk, lse, y, rows, reduce=form, **kw)
            b = ops.attn_transfer(q, ks, dk, lse, y, rows, reduce=form, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (form, rows is None)


def test_graph_replay_follows_the_payload_the_index_tensor_and_the_table(ops):
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
    y0, y1 = (((torch.rand(B, Lq + N * Lr, 3, generator=g) * 2 - 1) * 64).cuda() for _ in range(2))
    for form in FORMS:
        tk = ops.RefKVTable.from_tensors(gk0)
        static_idx, static_lse, static_y = idx0.clone(), lse0.clone(), y0.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.attn_transfer(q, ks, tk, static_lse, static_y, static_idx, reduce=form, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.attn_transfer(q, ks, tk, static_lse, static_y, static_idx, reduce=form, **kw)
        graph.replay()
        torch.cuda.synchronize()
        want0 = ops.attn_transfer(q, ks, _stack(gk0), lse0, y0, idx0, reduce=form, **kw)
        assert torch.equal(out[0], want0[0]) and torch.equal(out[1], want0[1]), form
        static_idx.copy_(idx1)
        static_lse.copy_(lse1)
        static_y.copy_(y1)
        tk.fill_(gk1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want1 = ops.attn_transfer(q, ks, _stack(gk1), lse1, y1, idx1, reduce=form, **kw)
        assert torch.equal(out[0], want1[0]) and torch.equal(out[1], want1[1]), form
        assert not torch.equal(want0[0], want1[0])
        del graph


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_batch_invariance(ops, dtype):
    """an entry's bytes are the same alone and at another position of a larger batch, in both forms, with and without the
    (accepted, inert) flag"""
    case = (3, 2, 72, 72, 3, 40, True)
    B, H, Lq, Ls, N, Lr, inc = case
    s = _setup(case, dtype)
    y = ((torch.rand(B, s["edges"][-1], 2, generator=torch.Generator().manual_seed(8)) * 2 - 1) * 64).cuda()
    take = [2, 0, 1, 0]                                                                # entry b of the batch of 3 at position i of a batch of 4
    for idx in (None, _indices(B, Lq, 68, seed=21).cuda()):
        for form in FORMS:
            a = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], y, idx, reduce=form, **s["kw"])
            f = ops.attn_transfer(s["q"], s["k"], s["rk"], s["lse"], y, idx, reduce=form, batch_invariant=True, **s["kw"])
            assert torch.equal(a[0], f[0]) and torch.equal(a[1], f[1])
            for b in range(B):
                one = ops.attn_transfer(s["q"][b:b + 1].contiguous(), s["k"][b:b + 1].contiguous(), s["rk"][b:b + 1].contiguous(),
                                        s["lse"][b:b + 1].contiguous(), y[b:b + 1].contiguous(), None if idx is None else idx[b:b + 1].contiguous(),
                                        reduce=form, **s["kw"])
                assert torch.equal(one[0][0], a[0][b]) and torch.equal(one[1][0], a[1][b]), (form, b)
            big = ops.attn_transfer(s["q"][take].contiguous(), s["k"][take].contiguous(), s["rk"][take].contiguous(), s["lse"][take].contiguous(),
                                    y[take].contiguous(), None if idx is None else idx[take].contiguous(), reduce=form, **s["kw"])
            for i, b in enumerate(take):
                assert torch.equal(big[0][i], a[0][b]) and torch.equal(big[1][i], a[1][b]), (form, i, b)


# ---- 9: the plugin surface -----------------------------------------------------------------------------------------------------------
def test_through_the_plugin_surface(ops, monkeypatch):
    """``attention_transfer_payload`` on a shared layer: the result is ``ops.attn_transfer`` on that layer's q / k / lse (caught on
    their way into the call), agrees with the dump of the same forward, and leaves ``attention_match``, ``attention_mass`` and the
    layer output as they were bit for bit"""
    import instantrestore_amd.attn_processors as ap
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    from instantrestore_amd.attn_maps import coordinate_payload
    seen = []
    real = ops.attn_transfer

    def spy(*a, **kw):
        seen.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ap._ops, "attn_transfer", spy)
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
        payload = coordinate_payload(L, N, L, train_input, device="cuda")
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            proc.attention_match_index, proc.save_attention_mass = "all", True
            y0 = run()
            (mi0, mp0), mass0 = proc.attention_match, proc.attention_mass.clone()
            assert proc.attention_transfer is None and not seen
            proc.attention_transfer_payload, proc.save_self_attentions = payload, True
            y1 = run()
            assert len(seen) == 1
            (a, kw) = seen.pop()
            assert a[4] is payload and a[5] is None and kw["reduce"] == "head_mean"
            sums, mass = proc.attention_transfer
            want = real(*a, **kw)
            assert sums.shape == (B, L, S, 2) and mass.shape == (B, L, S) and torch.equal(sums, want[0]) and torch.equal(mass, want[1])
            assert torch.equal(proc.attention_match[0], mi0) and torch.equal(proc.attention_match[1], mp0)
            assert torch.equal(proc.attention_mass, mass0) and torch.equal(y0, y1)
            proc.attention_transfer_reduce, proc.attention_transfer_index = "none", torch.tensor([7, 0, 255])
            run()
            seen.clear()
            s0, m0 = proc.attention_transfer
            dump = proc.attention_probs[:, :, [7, 0, 255]].double()                            # the 16-bit dump of the same forward
            assert s0.shape == (B, H, 3, S, 2) and m0.shape == (B, H, 3, S)
            for si in range(S):
                seg = dump[..., si * L:(si + 1) * L]
                ref = torch.einsum("bhrj,jc->bhrc", seg, payload[0, si * L:(si + 1) * L].double())
                # every probability of the dump carries one bf16 rounding (2^-9 relative): 2^-9 * mass * max|y|
                assert float((s0[..., si, :].double() - ref).abs().max()) <= 2.0 ** -9 * 15 + 1e-4
                assert float((m0[..., si].double() - seg.sum(-1)).abs().max()) <= 2.0 ** -9 + 1e-4


def test_example_transfer_switch(capsys):
    """examples/synthetic_inference.py --transfer: every shared layer prints its per-reference figures"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "synthetic_inference.py")
    spec = importlib.util.spec_from_file_location("synthetic_inference_transfer", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--identities", "2", "--refs", "3", "--px", "256", "--small", "--transfer", "--dtype", "bf16"])
    text = capsys.readouterr().out
    assert out.shape == (2, 256, 256, 3)
    assert text.count(": transfer (2, ") == 9 and "transfer (2, 1024, 4, 2)" in text and "transfer (2, 64, 4, 2)" in text, text
    assert text.count("mean soft displacement per reference") == 9 and text.count("mean mass per reference") == 9
    assert text.count("share of tokens whose rounded expected position is the hard match") == 9


# ---- 10: one real-shape slice --------------------------------------------------------------------------------------------------------
def test_1024px_layer_one_identity_one_head(ops):
    """the 1024-px top shared layer for one identity and one head (L = Ls = Lr = 16384, N = 4, bf16, 68 rows): the shape the dump
    cannot serve, with the coordinate payload, held to float64 with the device's LSE"""
    from instantrestore_amd.attn_maps import coordinate_payload
    dtype = torch.bfloat16
    B, H, L, N, R = 1, 1, 16384, 4, 68
    g = torch.Generator(device="cuda").manual_seed(2)
    q = (torch.randn(B, L, 64, device="cuda", generator=g) * 1.2).to(dtype)
    k = torch.randn(B, L, 64, device="cuda", generator=g).to(dtype)
    v = torch.randn(B, L, 64, device="cuda", generator=g).to(dtype)
    rk = torch.randn(B, N, L, 64, device="cuda", generator=g).to(dtype)
    rv = torch.randn(B, N, L, 64, device="cuda", generator=g).to(dtype)
    kw = dict(heads=H, scale=0.125, include_self=True)
    _, lse = ops.shared_attention(q, k, v, rk, rv, return_lse=True, **kw)
    y = coordinate_payload(L, N, L, True, device="cuda")                                     # (1, Lkv, 2), values 0 ... 127
    ymax = float(y.max())
    idx = _indices(B, L, R, seed=5).cuda()
    edges = T.segment_edges(L, N, L, True)
    ref_s, ref_m = _transfer64(_p64_device_lse(q, k, rk, lse, idx, H, True), y, edges)
    for form in FORMS:
        sums, mass = ops.attn_transfer(q, k, rk, lse, y, idx, reduce=form, **kw)
        r_s, r_m = (ref_s, ref_m) if form == "none" else (ref_s.mean(1), ref_m.mean(1))
        da, dm = float((sums.double() - r_s).abs().max()), float((mass.double() - r_m).abs().max())
        print(f"attn_transfer 1024px {form}: vs float64 with the device's LSE sums {da:.3e} (bound {1e-4 * ymax:.1e}) mass {dm:.3e} (1e-4)")
        assert da <= 1e-4 * ymax and dm <= 1e-4, (form, da, dm)
