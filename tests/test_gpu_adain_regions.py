"""Per-region AdaIN on the MI355X: ``ir_token_stats_labelled`` / ``ir_adain_apply_labelled`` through ``ops``, the affine table and
the processor branch.

Bit for bit: region ``r`` of ``token_stats_regions`` == ``token_stats_weighted`` with the weights ``(labels == r)`` (mean, std,
count == wsum), for random, raster, empty, single-token, one-region and out-of-range label patterns; shared labels == expanded
labels; a token of region ``r`` out of ``adain_apply_regions`` == the same token out of ``adain_apply`` with slot ``r``'s affine;
in place == out of place; an entry of a batch == the same entry alone; eager == hipGraph replay, which follows in-place changes of
the labels; a fallen-back slot of the table == the ordinary affine.

Against the float64 oracle of tests/adain_regions_oracle.py: mean / std / (a, b) to the bounds of
tests/test_gpu_adain_weighted.py (``RTOL`` 2e-4, ``MEAN_ATOL`` 2e-5, ``STD_ATOL`` 1e-6, ``A_ATOL`` 1e-6, ``B_ATOL`` 2e-4), whose
docstring derives them; the arithmetic per region is that of the weighted pass, so no new constant is needed.  The fused result:
(a) the attention over the device's own renormalised V against the float64 attention over the same 16-bit V meets both bounds of
tests/parity_bounds.py; (b) end to end, against the float64 oracle on the UN-rounded renormalised V, the stated tolerance only -
V' carries one 16-bit rounding the fold does not have, which the regression bound was not calibrated for; the ratio to the
regression bound is printed."""
import itertools

import numpy as np
import pytest
import torch

from adain_regions_oracle import region_adain_attention_np, region_affine_table_np, region_token_stats_np
from oracle.shared_attn_oracle import shared_attention_np
from parity_bounds import check_parity, regression_bound, stated_bound

pytestmark = pytest.mark.gpu

LENS = [1, 2, 31, 33, 255, 256, 257, 600]      # the chunk is 256 rows, a wave covers 32 row slots
SHAPES = list(itertools.product((1, 3), (1, 5), (1, 2)))     # H, M, B
REGIONS = [1, 3, 8, 32]
DTYPES = [torch.float16, torch.bfloat16]
PATTERNS = ["random", "raster", "empty", "single", "one", "outside"]
RTOL, A_ATOL, B_ATOL, MEAN_ATOL, STD_ATOL = 2e-4, 1e-6, 2e-4, 2e-5, 1e-6


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


def _x(B, M, L, H, dtype, seed):
    """N(0.3, 1) as a strided (B, M, L, C) view of a wider buffer"""
    g = torch.Generator().manual_seed(seed)
    C = H * 64
    buf = (torch.randn((B, M + 1, L + 2, C + 64), generator=g) + 0.3).to(dtype).cuda()
    x = buf[:, 1:, 1:L + 1, 64:]
    assert x.stride(2) == C + 64 and x.data_ptr() % 16 == 0 and x.data_ptr() != buf.data_ptr()
    return x


def _np64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _same(a, b):
    return all(s.shape == t.shape and torch.equal(s.contiguous().view(torch.int32), t.contiguous().view(torch.int32)) for s, t in zip(a, b))


def _labels(pattern, B, M, L, R, seed):
    """int32 (B, M, L) on the host"""
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(0, R, (B, M, L), generator=g, dtype=torch.int32)
    if pattern == "random":
        return rnd
    if pattern == "raster":                                   # contiguous blocks, as a parsing map gives them
        return ((torch.arange(L) * R) // L).to(torch.int32).expand(B, M, L).contiguous()
    if pattern == "empty":                                    # region R - 1 has no token (R == 1: no token has a region)
        return torch.where(rnd == R - 1, torch.full_like(rnd, 0 if R > 1 else -1), rnd)
    if pattern == "single":                                   # region R - 1 has exactly one token
        lab = torch.where(rnd == R - 1, torch.full_like(rnd, 0 if R > 1 else -1), rnd)
        lab[:, :, (seed * 7) % L] = R - 1
        return lab
    if pattern == "one":
        return torch.full((B, M, L), R - 1, dtype=torch.int32)
    return torch.randint(-1, R + 1, (B, M, L), generator=g, dtype=torch.int32)      # -1 and R mixed in


def _weighted_route(ops, x, labels, H, R):
    """what exists without the kernel: R weighted passes with one-hot weights -> (B, R, M, ...) like the one-pass op"""
    parts = [ops.token_stats_weighted(x, heads=H, weights=(labels == r).float(), return_wsum=True) for r in range(R)]
    return tuple(torch.stack([p[i] for p in parts], dim=1) for i in range(3))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("L", LENS)
def test_every_region_is_the_weighted_pass_bit_for_bit(ops, dtype, L):
    for (H, M, B), R in itertools.product(SHAPES, REGIONS):
        x = _x(B, M, L, H, dtype, 10 * L + H + M + B)
        for pattern in PATTERNS:
            lab = _labels(pattern, B, M, L, R, L + R + len(pattern)).cuda()
            got = ops.token_stats_regions(x, lab, heads=H, n_regions=R, return_count=True)
            assert got[0].shape == (B, R, M, H, 64) and got[2].shape == (B, R, M)
            assert _same(got, _weighted_route(ops, x, lab, H, R)), (pattern, H, M, B, R)
            assert _same(got[:2], ops.token_stats_regions(x, lab, heads=H, n_regions=R))
            in_range = ((lab >= 0) & (lab < R)).sum(-1).float()
            assert torch.equal(got[2].sum(1), in_range), (pattern, H, M, B, R)              # exact integers
            if pattern == "one" and L >= 2 and R > 1:                                        # everything in one region: ir_token_stats
                assert _same((got[0][:, R - 1], got[1][:, R - 1]), ops.token_stats(x, heads=H))
                assert not got[0][:, :R - 1].any() and not got[2][:, :R - 1].any()
        # labels shared across the batch (lb_sb = 0) equal the expanded labels
        lab = _labels("outside", 1, M, L, R, L + R).cuda()
        assert _same(ops.token_stats_regions(x, lab, heads=H, n_regions=R, return_count=True),
                     ops.token_stats_regions(x, lab.expand(B, M, L).contiguous(), heads=H, n_regions=R, return_count=True)), (H, M, B, R)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_tokens_of_no_region_are_inert_and_the_empty_and_single_token_rules(ops, dtype):
    B, M, L, H, R = 2, 5, 600, 3, 8
    x = _x(B, M, L, H, dtype, 5).contiguous()
    g = torch.Generator().manual_seed(9)
    lab = torch.randint(-2, R + 2, (B, M, L), generator=g, dtype=torch.int32)
    lab[0, 0][lab[0, 0] == 3] = R                                 # (0, 0): region 3 is empty
    lab[1, 2][lab[1, 2] == 5] = -1
    lab[1, 2, 300] = 5                                            # (1, 2): region 5 has exactly one token
    lab[1, 4] = 40                                                # (1, 4): no token has a region
    ld = lab.cuda()
    clean = ops.token_stats_regions(x, ld, heads=H, n_regions=R, return_count=True)
    dead = (ld < 0) | (ld >= R)
    junk = torch.tensor([float("nan"), float("inf"), -float("inf"), 6e4], dtype=dtype, device="cuda")
    fill = junk[torch.randint(0, 4, (B, M, L), generator=g).cuda()][..., None].expand(B, M, L, H * 64)
    dirty = torch.where(dead[..., None], fill, x)
    assert not torch.isfinite(dirty.float()).all()
    got = ops.token_stats_regions(dirty, ld, heads=H, n_regions=R, return_count=True)
    assert all(torch.isfinite(t).all() for t in got) and _same(clean, got)
    mean, std, count = (t.cpu() for t in clean)
    assert not mean[0, 3, 0].any() and not std[0, 3, 0].any() and float(count[0, 3, 0]) == 0.0
    assert not mean[1, :, 4].any() and not std[1, :, 4].any() and not count[1, :, 4].any()
    assert torch.equal(mean[1, 5, 2].reshape(-1), x[1, 2, 300].float().cpu()) and not std[1, 5, 2].any() and float(count[1, 5, 2]) == 1.0
    want = torch.stack([(lab == r).sum(-1) for r in range(R)], dim=1).float()
    assert torch.equal(count, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("L", LENS[1:])
def test_statistics_and_table_against_the_float64_oracle(ops, dtype, L):
    worst = {"mean": 0.0, "std": 0.0, "a": 0.0, "b": 0.0}
    for (H, M, B), R in zip(SHAPES, [r for r in REGIONS * 2 if r <= L // 2] * 8):
        x = _x(B, M, L, H, dtype, 3 * L + H + M + B)
        g = torch.Generator().manual_seed(L + R)
        lab = torch.stack([torch.stack([torch.randperm(L, generator=g) % R for _ in range(M)]) for _ in range(B)]).to(torch.int32)
        what = f"L={L} R={R} H={H} M={M} B={B} {dtype}"
        mean, std, count = ops.token_stats_regions(x, lab.cuda(), heads=H, n_regions=R, return_count=True)
        m_ref, s_ref, c_ref = region_token_stats_np(_np64(x), lab.numpy(), R)
        assert c_ref.min() >= 2, what                              # every region of every matrix has at least two tokens
        np.testing.assert_array_equal(_np64(count), c_ref, err_msg=what)
        got_m, got_s = _np64(mean).reshape(B, R, M, -1), _np64(std).reshape(B, R, M, -1)
        worst["mean"] = max(worst["mean"], float((np.abs(got_m - m_ref) / (MEAN_ATOL + RTOL * np.abs(m_ref))).max()))
        worst["std"] = max(worst["std"], float((np.abs(got_s - s_ref) / (STD_ATOL + RTOL * np.abs(s_ref))).max()))
        np.testing.assert_allclose(got_m, m_ref, rtol=RTOL, atol=MEAN_ATOL, err_msg=what)
        np.testing.assert_allclose(got_s, s_ref, rtol=RTOL, atol=STD_ATOL, err_msg=what)
        # the table: x's matrices are the references, another tensor gives the style; min_tokens = 2, so every slot is regional
        v = (torch.randn((B, L, H * 64), generator=g) * 0.7 + 0.3).to(dtype).cuda()
        ql = torch.stack([torch.randperm(L, generator=g) % R for _ in range(B)]).to(torch.int32)
        style = ops.token_stats_regions(v.unsqueeze(1), ql.cuda().unsqueeze(1), heads=H, n_regions=R, return_count=True)
        a, b = ops.adain_affine_regions(style, (mean, std, count), ops.token_stats_weighted(v.unsqueeze(1), heads=H),
                                        ops.token_stats_weighted(x, heads=H), min_tokens=2)
        a_ref, b_ref, regional = region_affine_table_np(_np64(v), _np64(x), ql.numpy(), lab.numpy(), R, min_tokens=2)
        assert regional.all() and a.shape == (B, M, R + 1, H, 64), what
        got_a, got_b = _np64(a).reshape(B, M, R + 1, -1), _np64(b).reshape(B, M, R + 1, -1)
        worst["a"] = max(worst["a"], float((np.abs(got_a - a_ref) / (A_ATOL + RTOL * np.abs(a_ref))).max()))
        worst["b"] = max(worst["b"], float((np.abs(got_b - b_ref) / (B_ATOL + RTOL * np.abs(b_ref))).max()))
        np.testing.assert_allclose(got_a, a_ref, rtol=RTOL, atol=A_ATOL, err_msg=what)
        np.testing.assert_allclose(got_b, b_ref, rtol=RTOL, atol=B_ATOL, err_msg=what)
    print(f"L={L} {dtype}: largest error / bound  " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def _table(B, N, R, H, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(B, N, R + 1, H, 64, generator=g) + 0.5).cuda()
    b = (torch.randn(B, N, R + 1, H, 64, generator=g) * 0.5).cuda()
    return a, b


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("L", [1, 33, 257])
def test_apply_picks_the_affine_per_token(ops, dtype, L):
    for (H, N, B), R in zip(SHAPES, REGIONS * 2):
        x = _x(B, N, L, H, dtype, L + H + N + B)
        a, b = _table(B, N, R, H, L + R)
        lab = _labels("outside", B, N, L, R, L + R).cuda()
        lab[0, 0, 0] = -5
        y = ops.adain_apply_regions(x, lab, a, b, heads=H)
        assert y.shape == x.shape and y.is_contiguous() and y.dtype == dtype
        slot = torch.where((lab >= 0) & (lab < R), lab, torch.full_like(lab, R))
        for s in range(R + 1):                                   # slot R: the tokens of no region
            want = ops.adain_apply(x, a[:, :, s].contiguous(), b[:, :, s].contiguous(), heads=H)
            sel = slot == s
            assert torch.equal(y[sel].view(torch.int16), want[sel].view(torch.int16)), (H, N, B, R, s)
        # against float64 a * x + b, the bounds tests/test_gpu_parity.py holds ir_adain_apply to
        bi, ni = torch.arange(B, device="cuda")[:, None, None], torch.arange(N, device="cuda")[None, :, None]
        ref = _np64(x) * _np64(a[bi, ni, slot.long()]).reshape(B, N, L, -1) + _np64(b[bi, ni, slot.long()]).reshape(B, N, L, -1)
        check_parity(y, ref, dtype, f"adain_apply_regions L={L} H={H} N={N} B={B} R={R}")
        # labels shared by the batch
        assert torch.equal(ops.adain_apply_regions(x, lab[:1], a, b, heads=H).view(torch.int16),
                           ops.adain_apply_regions(x, lab[:1].expand(B, N, L).contiguous(), a, b, heads=H).view(torch.int16))
        # in place equals out of place (on the strided view: the bytes around it stay)
        C = H * 64
        buf = torch.full((B, N + 1, L + 2, C + 64), 7.0, dtype=dtype, device="cuda")
        view = buf[:, 1:, 1:L + 1, 64:]
        view.copy_(x)
        before = buf.clone()
        assert ops.adain_apply_regions(view, lab, a, b, heads=H, out=view) is view
        assert torch.equal(view.contiguous().view(torch.int16), y.view(torch.int16))
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:, 1:, 1:L + 1, 64:] = False
        assert torch.equal(buf[outside].view(torch.int16), before[outside].view(torch.int16))
        # a strided y of its own leaves the bytes around it untouched
        buf2 = torch.full((B, N, L + 3, C + 128), -3.0, dtype=dtype, device="cuda")
        y2 = buf2[:, :, 2:L + 2, 128:]
        before2 = buf2.clone()
        ops.adain_apply_regions(x, lab, a, b, heads=H, out=y2)
        assert torch.equal(y2.contiguous().view(torch.int16), y.view(torch.int16))
        outside2 = torch.ones_like(buf2, dtype=torch.bool)
        outside2[:, :, 2:L + 2, 128:] = False
        assert torch.equal(buf2[outside2].view(torch.int16), before2[outside2].view(torch.int16))


def test_fallback_slots_are_the_ordinary_affine_bit_for_bit(ops):
    B, N, L, H, R = 2, 3, 256, 2, 4
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(31)
    v = (torch.randn(B, L, H * 64, generator=g) * 0.8 + 0.2).to(dtype).cuda()
    rv = (torch.randn(B, N, L, H * 64, generator=g) * 1.3 - 0.4).to(dtype).cuda()
    ql = torch.stack([torch.randperm(L, generator=g) % R for _ in range(B)]).to(torch.int32)
    rl = torch.stack([torch.stack([torch.randperm(L, generator=g) % R for _ in range(N)]) for _ in range(B)]).to(torch.int32)
    rl[0, 1][rl[0, 1] == 2] = 0                                    # reference (0, 1) lacks region 2
    ql[1][ql[1] == 1] = 3                                          # query picture 1 lacks region 1
    rl[1, 2][rl[1, 2] == 0] = 3
    rl[1, 2, :7] = 0                                               # 7 tokens of region 0: below min_tokens = 8
    fallen = {(0, 1, 2), (1, 0, 1), (1, 1, 1), (1, 2, 1), (1, 2, 0)}
    v1 = v.unsqueeze(1)
    style_g, content_g = ops.token_stats(v1, heads=H), ops.token_stats(rv, heads=H)
    style = ops.token_stats_regions(v1, ql.cuda().unsqueeze(1), heads=H, n_regions=R, return_count=True)
    content = ops.token_stats_regions(rv, rl.cuda(), heads=H, n_regions=R, return_count=True)
    a, b = ops.adain_affine_regions(style, content, style_g, content_g)
    assert a.shape == (B, N, R + 1, H, 64) and torch.isfinite(a).all() and torch.isfinite(b).all()
    ag, bg = ops.adain_affine(style_g, content_g)
    assert _same((ag, bg), ops.adain_stats(v, rv, heads=H))        # ... which is the affine the plain layer uses
    assert _same((a[:, :, R], b[:, :, R]), (ag, bg))
    for r in range(R):
        ar, br = ops.adain_affine((style[0][:, r, 0].contiguous(), style[1][:, r, 0].contiguous()),
                                  (content[0][:, r].contiguous(), content[1][:, r].contiguous()))
        for bb in range(B):
            for n in range(N):
                want = (ag[bb, n], bg[bb, n]) if (bb, n, r) in fallen else (ar[bb, n], br[bb, n])
                assert _same((a[bb, n, r], b[bb, n, r]), want), (bb, n, r)
                assert ((bb, n, r) in fallen) or not _same((a[bb, n, r],), (ag[bb, n],))
    # an absent region never produces the eps / sigma affine of (0, 0) statistics: the largest scale stays that of real statistics
    assert float(a.max()) < 10.0


def test_batch_entries_alone_and_graph_replay_follow_the_labels(ops):
    B, M, L, H, R = 2, 5, 600, 3, 8
    x = _x(B, M, L, H, torch.bfloat16, 77)
    g = torch.Generator().manual_seed(4)
    lab = torch.randint(-1, R + 1, (B, M, L), generator=g, dtype=torch.int32).cuda()
    a, b = _table(B, M, R, H, 5)
    run = lambda: ops.token_stats_regions(x, lab, heads=H, n_regions=R, return_count=True) + (ops.adain_apply_regions(x, lab, a, b, heads=H),)
    eager = [t.clone() for t in run()]
    # an entry alone equals the same entry inside the batch, whatever its neighbours
    for bb, m in ((0, 0), (B - 1, M - 1)):
        alone = ops.token_stats_regions(x[bb:bb + 1, m:m + 1], lab[bb:bb + 1, m:m + 1].contiguous(), heads=H, n_regions=R, return_count=True)
        assert _same((eager[0][bb, :, m], eager[1][bb, :, m], eager[2][bb, :, m]), (alone[0][0, :, 0], alone[1][0, :, 0], alone[2][0, :, 0]))
        y1 = ops.adain_apply_regions(x[bb:bb + 1, m:m + 1], lab[bb:bb + 1, m:m + 1].contiguous(), a[bb:bb + 1, m:m + 1].contiguous(),
                                     b[bb:bb + 1, m:m + 1].contiguous(), heads=H)
        assert torch.equal(y1[0, 0].view(torch.int16), eager[3][bb, m].view(torch.int16))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        run()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):            # a linear graph: four launches in a row
            static = run()
    torch.cuda.current_stream().wait_stream(stream)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager[:3], static[:3]) and torch.equal(eager[3].view(torch.int16), static[3].view(torch.int16))
    lab.copy_(torch.randint(-1, R + 1, (B, M, L), generator=g, dtype=torch.int32))     # in place: the replay reads them when it runs
    graph.replay()
    torch.cuda.synchronize()
    second = [t.clone() for t in static]
    again = run()
    assert _same(second[:3], again[:3]) and torch.equal(second[3].view(torch.int16), again[3].view(torch.int16))
    assert not _same(second[:1], eager[:1]) and not torch.equal(second[3].view(torch.int16), eager[3].view(torch.int16))


def _regional_case(dtype, seed=21):
    """L 64, N 2, H 2, R 3; the references' regions have deliberately different statistics (shift and scale per region)"""
    B, H, L, N, R = 2, 2, 64, 2, 3
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0, sh=0.0: torch.randn(s, generator=g) * sc + sh
    ql = torch.stack([torch.randperm(L, generator=g) % R for _ in range(B)]).to(torch.int32)
    rl = torch.stack([torch.stack([torch.randperm(L, generator=g) % R for _ in range(N)]) for _ in range(B)]).to(torch.int32)
    scale, shift = torch.tensor([0.5, 1.0, 2.5]), torch.tensor([-2.0, 0.0, 3.0])
    v_scale, v_shift = torch.tensor([1.5, 0.6, 1.0]), torch.tensor([0.8, -0.5, 0.2])
    q, k = r(B, L, H * 64).to(dtype), r(B, L, H * 64).to(dtype)
    v = (r(B, L, H * 64) * v_scale[ql.long()][..., None] + v_shift[ql.long()][..., None]).to(dtype)
    rk = r(B, N, L, H * 64).to(dtype)
    rv = (r(B, N, L, H * 64) * scale[rl.long()][..., None] + shift[rl.long()][..., None]).to(dtype)
    return B, H, L, N, R, q, k, v, rk, rv, ql, rl


def _op_level_route(ops, v, rv, ql, rl, H, R, min_tokens=8):
    v1 = v.unsqueeze(1)
    style = ops.token_stats_regions(v1, ql.unsqueeze(1), heads=H, n_regions=R, return_count=True)
    content = ops.token_stats_regions(rv, rl, heads=H, n_regions=R, return_count=True)
    a, b = ops.adain_affine_regions(style, content, ops.token_stats(v1, heads=H), ops.token_stats(rv, heads=H), min_tokens=min_tokens)
    return ops.adain_apply_regions(rv, rl, a, b, heads=H), (a, b)


@pytest.mark.parametrize("train_input", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_fused_attention_on_the_regionally_renormalised_values(ops, dtype, train_input):
    B, H, L, N, R, q, k, v, rk, rv, ql, rl = _regional_case(dtype)
    c = lambda t: t.cuda()
    rv2, _ = _op_level_route(ops, c(v), c(rv), c(ql), c(rl), H, R)
    out = ops.shared_attention(c(q), c(k), c(v), c(rk), rv2, heads=H, scale=0.125, include_self=train_input)
    # (a) the attention over the device's own V' against the float64 attention over the same 16-bit V': both bounds
    same_v = shared_attention_np(_np64(q), _np64(k), _np64(v), _np64(rk), _np64(rv2), H, 0.125, False, train_input)
    check_parity(out, same_v, dtype, f"attention over the device's renormalised V train_input={train_input}")
    # (b) end to end against the oracle on the un-rounded renormalised V: the stated tolerance only
    ref = region_adain_attention_np(_np64(q), _np64(k), _np64(v), _np64(rk), _np64(rv), ql.numpy(), rl.numpy(), R, H, 0.125, train_input)
    err, rmax = float(np.abs(_np64(out) - ref).max()), float(np.abs(ref).max())
    print(f"per-region AdaIN end to end {dtype} train_input={train_input}: max|err| {err:.3e}, max|ref| {rmax:.3f}, stated bound "
          f"{stated_bound(dtype, rmax):.3e}, regression bound {regression_bound(dtype, rmax):.3e}, err / regression {err / regression_bound(dtype, rmax):.2f}")
    assert np.isfinite(_np64(out)).all() and err <= stated_bound(dtype, rmax)
    # (c) whole-face AdaIN is visibly another function at this size
    plain = ops.shared_attention(c(q), c(k), c(v), c(rk), c(rv), heads=H, scale=0.125, include_self=train_input,
                                 adain=ops.adain_stats(c(v), c(rv), heads=H))
    assert float((plain.float() - out.float()).abs().max()) > 0.05


class _Recorder:
    """``ops`` with the arguments and the result of every ``shared_attention`` call kept"""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def shared_attention(self, *a, **kw):
        res = self._ops.shared_attention(*a, **kw)
        self.calls.append((a, kw, res))
        return res


def test_processor_equals_the_op_level_route_and_is_unchanged_without_the_kwarg(ops, monkeypatch):
    import instantrestore_amd.attn_processors as ap
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    from instantrestore_amd import attn_maps
    B, H, L, N, R = 2, 2, 256, 2, 4
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(8)
    torch.manual_seed(8)
    proc = SharedAttnProcessor(self_attn_idx=0, use_adain=True, train_input=True)
    attn = Attention(query_dim=H * 64, heads=H, dim_head=64, processor=proc).cuda()
    x = torch.randn(B, L, H * 64, generator=g).cuda()
    rk = torch.randn(B, N, L, H * 64, generator=g).to(dtype).cuda()
    rv = (torch.randn(B, N, L, H * 64, generator=g) * 1.3 - 0.4).to(dtype).cuda()
    q_pic = torch.randint(0, R, (B, 32, 32), generator=g).cuda()                  # pictures: sampled on the 16 x 16 grid
    r_pic = torch.randint(-1, R + 1, (B, N, 32, 32), generator=g).cuda()
    rec = _Recorder(ops)
    monkeypatch.setattr(ap, "_ops", rec)
    refs = {"ref_keys": [rk], "ref_values": [rv]}
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        y_plain = attn(x, **refs)
        y = attn(x, adain_regions=(q_pic, r_pic), adain_n_regions=R, **refs)
        y_both = attn(x, adain_regions=(q_pic, r_pic), adain_n_regions=R, region_labels=(q_pic, r_pic.clamp(0, R - 1)),
                      region_allow=torch.eye(R, dtype=torch.bool), **refs)
        y_again = attn(x, **refs)
    (a0, kw0, res0), (a1, kw1, res1), (a2, kw2, res2), (a3, kw3, res3) = rec.calls
    # without the kwarg: the parent's route - ops.adain_stats on this layer's V and the dense references, the same bytes again
    assert _same(kw0["adain"], ops.adain_stats(a0[2], rv, heads=H)) and a0[4].data_ptr() == rv.data_ptr() and torch.equal(y_plain, y_again) and a3[4].data_ptr() == rv.data_ptr()
    # with it: the op-level route, bit for bit
    q, k, v = a1[:3]
    ql = attn_maps.token_labels(q_pic, 16).int()
    rl = attn_maps.token_labels(r_pic, 16).int().reshape(B, N, L)
    rv2, _ = _op_level_route(ops, v, rv, ql, rl, H, R)
    assert kw1.get("adain") is None and kw1.get("valid_refs") is None and torch.equal(a1[4], rv2)
    mine = ops.shared_attention(q, k, v, rk, rv2, **kw1)
    assert torch.equal(mine, res1) and torch.isfinite(y.float()).all() and not torch.equal(y, y_plain)
    # composes with region_labels: the region pair rides the same call
    assert kw2.get("adain") is None and kw2["q_allow"] is not None and kw2["key_region"] is not None and torch.equal(a2[4], rv2)
    both = ops.shared_attention(q, k, v, rk, rv2, **kw2)
    assert torch.equal(both, res2) and torch.isfinite(y_both.float()).all() and not torch.equal(y_both, y)


def test_example_adain_regions_switch(capsys):
    """examples/synthetic_inference.py --adain-regions: nine shared layers build a table, and the output moves"""
    import importlib.util
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "synthetic_inference.py")
    spec = importlib.util.spec_from_file_location("synthetic_inference_adain_regions", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--identities", "2", "--refs", "3", "--px", "256", "--small", "--adain-regions", "4", "--dtype", "bf16"])
    text = capsys.readouterr().out
    assert out.shape == (2, 256, 256, 3)
    m = re.search(r"--adain-regions 4: 9 shared layers, (\d+) of (\d+) \(reference, class\) slots carry regional statistics.*largest change of the "
                  r"output ([0-9.]+)", text)
    assert m, text
    assert int(m.group(2)) == 9 * 2 * 3 * 4 and int(m.group(1)) == int(m.group(2)) and float(m.group(3)) > 0.0, text
