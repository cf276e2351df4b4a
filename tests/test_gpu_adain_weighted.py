"""Mask-aware AdaIN on the MI355X: ``ir_token_stats_weighted`` / ``ir_adain_affine_from_stats`` through ``ops``.

Bit for bit: NULL == all-ones == ``lens == len`` == ``ir_token_stats``; ``ir_token_stats`` + ``ir_adain_affine_from_stats`` ==
``ir_adain_stats_cached``; an entry of a batch == the same matrix alone; eager == hipGraph replay, which follows in-place changes
of the weights and the counts.  Against the float64 oracle of tests/adain_weighted_oracle.py: (a, b) to the bounds
tests/test_gpu_parity.py holds ``ops.adain_stats`` to (rtol 2e-4; atol 1e-6 for a, 2e-4 for b), mean / std to the same rtol.  The
absolute terms of mean / std come from the format, not from the kernel: a mean is a sum of at most 600 products whose partial
sums pass ~45 fp32 roundings (8 per thread, 32 row slots, 3 chunks) of values up to |x - K| < 10, 45 * 2^-24 * 10 = 2.7e-5 at
the very worst - ``MEAN_ATOL`` 2e-5 is below that worst case; a std is positive and of order 1, so it gets the 1e-6 of ``a``.
The rules (zero-weight tokens are inert, no token gives (0, 0), one token gives (x, 0), ``wsum``), the fused attention with the
weighted affine against a float64 attention on kept-token statistics (tests/parity_bounds.py), and the processor."""
import itertools

import numpy as np
import pytest
import torch

from adain_weighted_oracle import effective_weights_np, weighted_adain_affine_np, weighted_adain_attention_np, weighted_token_stats_np
from parity_bounds import check_parity

pytestmark = pytest.mark.gpu

LENS = [1, 2, 31, 33, 255, 256, 257, 600]      # the chunk is 256 rows, a wave covers 32 row slots
SHAPES = list(itertools.product((1, 3), (1, 5), (1, 2)))     # H, M, B
DTYPES = [torch.float16, torch.bfloat16]
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
    return all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(a, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("L", LENS)
def test_unit_weights_and_full_counts_are_token_stats_bit_for_bit(ops, dtype, L):
    for H, M, B in SHAPES:
        x = _x(B, M, L, H, dtype, 10 * L + H + M + B)
        plain = ops.token_stats_weighted(x, heads=H)
        ones = ops.token_stats_weighted(x, heads=H, weights=torch.ones(B, M, L, device="cuda"))
        shared = ops.token_stats_weighted(x, heads=H, weights=torch.ones(1, M, L, device="cuda"))         # w_sb = 0
        full = ops.token_stats_weighted(x, heads=H, lens=torch.full((B, M), L, dtype=torch.int32, device="cuda"))
        over = ops.token_stats_weighted(x, heads=H, lens=torch.full((B, M), L + 7, dtype=torch.int32, device="cuda"),
                                        weights=torch.ones(B, M, L, dtype=torch.bool, device="cuda"))       # clamped; bool converted
        for other in (ones, shared, full, over):
            assert _same(plain, other), (H, M, B)
        if L >= 2:
            assert _same(plain, ops.token_stats(x, heads=H)), (H, M, B)
        else:                                                     # one token: (x, 0) where ir_token_stats says NaN
            assert torch.equal(plain[0].reshape(B, M, -1), x[:, :, 0].float()) and not plain[1].any()
        # an entry of the batch is the same matrix alone, whatever its neighbours
        w = (torch.rand(B, M, L, generator=torch.Generator().manual_seed(L)) < 0.7).float().cuda()
        lens = torch.randint(0, L + 1, (B, M), generator=torch.Generator().manual_seed(L + 1), dtype=torch.int32).cuda()
        mean, std, W = ops.token_stats_weighted(x, heads=H, weights=w, lens=lens, return_wsum=True)
        for b, m in ((0, 0), (B - 1, M - 1)):
            alone = ops.token_stats_weighted(x[b:b + 1, m:m + 1], heads=H, weights=w[b:b + 1, m:m + 1], lens=lens[b:b + 1, m:m + 1].contiguous(),
                                             return_wsum=True)
            assert _same((mean[b, m], std[b, m], W[b, m]), (alone[0][0, 0], alone[1][0, 0], alone[2][0, 0])), (H, M, B, b, m)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("L", [2, 33, 256, 600])
def test_token_stats_then_affine_is_adain_stats_cached_bit_for_bit(ops, dtype, L):
    for H, N, B in SHAPES:
        g = torch.Generator().manual_seed(L + H)
        v = (torch.randn((B, L, H * 64), generator=g) + 0.3).to(dtype).cuda()
        rv = (torch.randn((B, N, 40, H * 64), generator=g) * 1.3 - 0.4).to(dtype).cuda()
        rv[0, 0, :, 5] = 0.75                                    # a constant reference channel
        rv[B - 1, N - 1] = 0                                     # a zero-filled reference
        cm, cs = ops.token_stats(rv, heads=H)
        assert float(cs[0, 0].reshape(-1)[5]) == 0.0 and not cs[B - 1, N - 1].any()
        want = ops.adain_stats_cached(v, cm, cs, heads=H)
        style = ops.token_stats(v.unsqueeze(1), heads=H)
        assert _same(want, ops.adain_affine(style, (cm, cs))), (H, N, B)
        assert _same(want, ops.adain_affine((style[0][:, 0].contiguous(), style[1][:, 0].contiguous()), (cm, cs)))
        assert _same(want, ops.adain_affine(ops.token_stats_weighted(v.unsqueeze(1), heads=H), (cm, cs)))
        a = want[0]
        assert torch.isfinite(a).all() and torch.isfinite(want[1]).all()


def test_graph_replay_equals_eager_and_follows_in_place_updates(ops):
    B, M, L, H = 2, 5, 600, 3
    x = _x(B, M, L, H, torch.bfloat16, 77)
    g = torch.Generator().manual_seed(4)
    w = torch.rand(B, M, L, generator=g).cuda()
    lens = torch.randint(2, L + 1, (B, M), generator=g, dtype=torch.int32).cuda()
    run = lambda: ops.token_stats_weighted(x, heads=H, weights=w, lens=lens, return_wsum=True)
    eager = [t.clone() for t in run()]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        run()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            static = run()
    torch.cuda.current_stream().wait_stream(stream)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager, static)
    w.copy_((torch.rand(B, M, L, generator=g) < 0.5).float())     # in place: the replay reads them when it runs
    graph.replay()
    torch.cuda.synchronize()
    second = [t.clone() for t in static]
    assert _same(second, run()) and not _same(second[:1], eager[:1])
    lens.copy_(torch.randint(2, L // 2, (B, M), generator=g, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(static, run()) and not _same(static[:1], second[:1])


def _weights_case(case, B, M, L, seed):
    """(weights or None, lens or None) on the host; every (b, m) keeps at least 2 effective tokens"""
    g = torch.Generator().manual_seed(seed)
    w = lens = None
    if case.startswith("keep"):
        w = (torch.rand(B, M, L, generator=g) < float(case[4:])).float()
        w[..., :2] = torch.where(w.sum(-1, keepdim=True) < 2, torch.ones(B, M, 2), w[..., :2])
    elif case == "soft":
        w = torch.rand(B, M, L, generator=g)
        w[w < 0.15] = 0.0
        w[..., :2] = w[..., :2].clamp(min=0.25)
    elif case == "counts":
        lens = torch.randint(2, L + 1, (B, M), generator=g, dtype=torch.int32)
    else:
        lens = torch.randint(2, L + 1, (B, M), generator=g, dtype=torch.int32)
        w = torch.rand(B, M, L, generator=g)
        w[..., :2] = w[..., :2].clamp(min=0.25)
    return w, lens


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("L", LENS[1:])
def test_statistics_and_affine_against_the_float64_oracle(ops, dtype, L):
    for (H, M, B), case in zip(SHAPES * 2, ["keep0.1", "keep0.5", "keep0.9", "soft", "counts", "counts_weights"] * 3):
        x = _x(B, M, L, H, dtype, 3 * L + H + M + B)
        w, lens = _weights_case(case, B, M, L, L + len(case))
        d = lambda t: None if t is None else t.cuda()
        mean, std, W = ops.token_stats_weighted(x, heads=H, weights=d(w), lens=d(lens), return_wsum=True)
        n = lambda t: None if t is None else t.numpy()
        m_ref, s_ref, w_ref = weighted_token_stats_np(_np64(x), n(w), n(lens))
        what = f"{case} L={L} H={H} M={M} B={B} {dtype}"
        assert (effective_weights_np((B, M, L), n(w), n(lens)) > 0).sum(-1).min() >= 2, what
        m_err = np.abs(_np64(mean).reshape(B, M, -1) - m_ref)
        s_err = np.abs(_np64(std).reshape(B, M, -1) - s_ref)
        print(f"{what}: mean err {m_err.max():.2e} (rel {(m_err / np.maximum(np.abs(m_ref), 1e-30)).max():.2e}), "
              f"std err {s_err.max():.2e} (rel {(s_err / np.maximum(s_ref, 1e-30)).max():.2e})")
        np.testing.assert_allclose(_np64(mean).reshape(B, M, -1), m_ref, rtol=RTOL, atol=MEAN_ATOL, err_msg=what)
        np.testing.assert_allclose(_np64(std).reshape(B, M, -1), s_ref, rtol=RTOL, atol=STD_ATOL, err_msg=what)
        np.testing.assert_allclose(_np64(W), w_ref, rtol=1e-6, err_msg=what)
        # the affine: x's matrices are the references, a weighted self pass gives the style
        g = torch.Generator().manual_seed(L)
        v = (torch.randn((B, L, H * 64), generator=g) * 0.7 + 0.3).to(dtype).cuda()
        sw = torch.rand(B, L, generator=g)
        sw[:, :2] = sw[:, :2].clamp(min=0.25)
        style = ops.token_stats_weighted(v.unsqueeze(1), heads=H, weights=sw.cuda().unsqueeze(1))
        a, b = ops.adain_affine(style, (mean, std))
        a_ref, b_ref = weighted_adain_affine_np(_np64(v), _np64(x), sw.numpy(), n(w), None, n(lens))
        a_err, b_err = np.abs(_np64(a).reshape(B, M, -1) - a_ref), np.abs(_np64(b).reshape(B, M, -1) - b_ref)
        print(f"{what}: a err/bound {(a_err / (A_ATOL + RTOL * np.abs(a_ref))).max():.2e}, b err/bound {(b_err / (B_ATOL + RTOL * np.abs(b_ref))).max():.2e}")
        np.testing.assert_allclose(_np64(a).reshape(B, M, -1), a_ref, rtol=RTOL, atol=A_ATOL, err_msg=what)
        np.testing.assert_allclose(_np64(b).reshape(B, M, -1), b_ref, rtol=RTOL, atol=B_ATOL, err_msg=what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_zero_weight_tokens_are_inert_and_the_empty_and_single_token_rules(ops, dtype):
    B, M, L, H = 2, 5, 600, 3
    x = _x(B, M, L, H, dtype, 5).contiguous()
    g = torch.Generator().manual_seed(9)
    w = torch.rand(B, M, L, generator=g)
    w[w < 0.4] = 0.0
    lens = torch.randint(2, L + 1, (B, M), generator=g, dtype=torch.int32)
    w[0, 0] = 0.0                                                 # W == 0 by the weights
    lens[0, 1] = 0                                                # ... and by the count
    w[1, 0] = 0.0
    w[1, 0, 300] = 0.5                                            # one effective token, weight 0.5
    lens[1, 0] = L
    lens[1, 1] = 1
    w[1, 1, 0] = 1.0                                              # one token by the count
    wd, ld = w.cuda(), lens.cuda()
    clean = ops.token_stats_weighted(x, heads=H, weights=wd, lens=ld, return_wsum=True)
    dead = (wd == 0) | (torch.arange(L, device="cuda")[None, None] >= ld[:, :, None])
    dirty = x.clone()
    junk = torch.tensor([float("nan"), float("inf"), -float("inf"), 6e4], dtype=dtype, device="cuda")
    fill = junk[torch.randint(0, 4, (B, M, L), generator=g).cuda()][..., None].expand(B, M, L, H * 64)
    dirty = torch.where(dead[..., None], fill, dirty)
    assert not torch.isfinite(dirty.float()).all()
    got = ops.token_stats_weighted(dirty, heads=H, weights=wd, lens=ld, return_wsum=True)
    assert all(torch.isfinite(t).all() for t in got) and _same(clean, got)
    mean, std, W = (t.cpu() for t in clean)
    for b, m in ((0, 0), (0, 1)):
        assert not mean[b, m].any() and not std[b, m].any() and float(W[b, m]) == 0.0
    assert torch.equal(mean[1, 0].reshape(-1), x[1, 0, 300].float().cpu()) and not std[1, 0].any() and float(W[1, 0]) == 0.5
    assert torch.equal(mean[1, 1].reshape(-1), x[1, 1, 0].float().cpu()) and not std[1, 1].any() and float(W[1, 1]) == 1.0
    eff = torch.where(dead.cpu(), torch.zeros(()), w)
    np.testing.assert_allclose(W.numpy(), eff.double().sum(-1).numpy(), rtol=1e-6)
    # the statistics of nothing are those of a zero-filled reference: the affine carries the style mean alone
    v = (torch.randn((B, 64, H * 64), generator=g) + 0.3).to(dtype).cuda()
    style = ops.token_stats(v.unsqueeze(1), heads=H)
    a, b = ops.adain_affine(style, clean[:2])
    zero = ops.adain_affine(style, ops.token_stats(torch.zeros_like(x), heads=H))
    assert _same((a[0, 0], b[0, 0]), (zero[0][0, 0], zero[1][0, 0])) and torch.equal(b[0, 0], style[0][0, 0])


@pytest.mark.parametrize("train_input", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_fused_attention_with_the_weighted_affine(ops, dtype, train_input):
    B, H, L, N = 2, 2, 64, 2
    g = torch.Generator().manual_seed(21)
    r = lambda *s, sc=1.0, sh=0.0: (torch.randn(s, generator=g) * sc + sh).to(dtype)
    q, k, v = r(B, L, H * 64), r(B, L, H * 64), r(B, L, H * 64, sc=0.8, sh=0.2)
    rk, rv = r(B, N, L, H * 64), r(B, N, L, H * 64, sc=1.3, sh=-0.4)
    sw = (torch.rand(B, L, generator=g) < 0.6).float()
    rw = (torch.rand(B, N, L, generator=g) < 0.4).float()
    rv = torch.where(rw[..., None] > 0, rv, (rv.float() * 3 + 2).to(dtype))      # the dropped tokens would pollute the statistics
    c = lambda t: t.cuda()
    style = ops.token_stats_weighted(c(v).unsqueeze(1), heads=H, weights=c(sw).unsqueeze(1))
    affine = ops.adain_affine(style, ops.token_stats_weighted(c(rv), heads=H, weights=c(rw)))
    out = ops.shared_attention(c(q), c(k), c(v), c(rk), c(rv), heads=H, scale=0.125, include_self=train_input, adain=affine)
    ref = weighted_adain_attention_np(_np64(q), _np64(k), _np64(v), _np64(rk), _np64(rv), H, 0.125, sw.numpy(), rw.numpy(), train_input)
    check_parity(out, ref, dtype, f"weighted AdaIN attention train_input={train_input}")
    unmasked = ops.shared_attention(c(q), c(k), c(v), c(rk), c(rv), heads=H, scale=0.125, include_self=train_input,
                                    adain=ops.adain_stats(c(v), c(rv), heads=H))
    assert float((unmasked.float() - out.float()).abs().max()) > 0.05       # the masks matter at this size


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
    B, H, L, N = 2, 2, 256, 2
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(8)
    torch.manual_seed(8)
    proc = SharedAttnProcessor(self_attn_idx=0, use_adain=True, train_input=True)
    attn = Attention(query_dim=H * 64, heads=H, dim_head=64, processor=proc).cuda()
    x = torch.randn(B, L, H * 64, generator=g).cuda()
    rk = torch.randn(B, N, L, H * 64, generator=g).to(dtype).cuda()
    rv = (torch.randn(B, N, L, H * 64, generator=g) * 1.3 - 0.4).to(dtype).cuda()
    keep = (torch.rand(B, N, L, generator=g) < 0.5).cuda()
    self_w = (torch.rand(B, 32, 32, generator=g) < 0.7).cuda()                   # a picture: sampled on the 16 x 16 grid
    rec = _Recorder(ops)
    monkeypatch.setattr(ap, "_ops", rec)
    from instantrestore_amd import attn_maps
    refs = {"ref_keys": [rk], "ref_values": [rv]}
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        y_plain = attn(x, **refs)
        y = attn(x, adain_weights=(self_w, attn_maps.weights_from_keep(keep)), ref_token_keep=keep, **refs)
    (a0, kw0, res0), (a1, kw1, res1) = rec.calls
    q, k, v = a1[:3]
    # without the kwarg: the parent's route - ops.adain_stats on this layer's V and the dense references
    assert _same(kw0["adain"], ops.adain_stats(a0[2], rv, heads=H)) and kw0.get("key_bias") is None
    # with it: the op-level route, bit for bit
    style = ops.token_stats_weighted(v.unsqueeze(1), heads=H, weights=attn_maps.token_weights(self_w, 16).unsqueeze(1))
    affine = ops.adain_affine(style, ops.token_stats_weighted(rv, heads=H, weights=attn_maps.weights_from_keep(keep)))
    assert _same(kw1["adain"], affine)
    bias = ops.key_bias(B, L, N, L, True, ref_token_keep=keep, device=q.device)
    assert torch.equal(kw1["key_bias"], bias)
    mine = ops.shared_attention(q, k, v, rk, rv, **{**kw1, "adain": affine, "key_bias": bias})
    assert torch.equal(mine, res1) and torch.isfinite(y.float()).all()
    assert not torch.equal(y, y_plain)
