"""Per-region AdaIN on the CPU-only box: the float64 oracle's tie to the weighted oracle, the fallback rule of
``ops.adain_affine_regions``, the refusals of ``ir_token_stats_labelled`` / ``ir_adain_apply_labelled`` in their stated order
(validation happens before any launch; device pointers are never dereferenced), the ops' argument checks, and the host logic of
the processors through a CPU stand-in for ``ops`` (as tests/test_adain_weighted_cpu.py)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from adain_regions_oracle import region_affine_table_np, region_apply_np, region_token_stats_np
from adain_weighted_oracle import affine_from_stats_np, weighted_token_stats_np

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def test_oracle_is_the_weighted_oracle_with_one_hot_weights():
    rng = np.random.default_rng(0)
    B, M, L, Cn, R = 2, 3, 50, 8, 5
    x = rng.normal(0.3, 1.0, (B, M, L, Cn))
    labels = rng.integers(-1, R + 1, (B, M, L))                    # -1 and R: no region
    labels[0, 0][labels[0, 0] == 2] = 0                            # an empty region
    labels[1, 2] = np.where(labels[1, 2] == 3, 1, labels[1, 2])
    labels[1, 2, 7] = 3                                            # a region of exactly one token
    mean, std, count = region_token_stats_np(x, labels, R)
    assert mean.shape == (B, R, M, Cn) and count.shape == (B, R, M)
    for r in range(R):
        m, s, w = weighted_token_stats_np(x, (labels == r).astype(np.float64))
        np.testing.assert_allclose(mean[:, r], m, rtol=0, atol=1e-12)
        np.testing.assert_allclose(std[:, r], s, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(count[:, r], w)
    assert count[0, 2, 0] == 0 and not mean[0, 2, 0].any() and not std[0, 2, 0].any()
    assert count[1, 3, 2] == 1 and np.array_equal(mean[1, 3, 2], x[1, 2, 7]) and not std[1, 3, 2].any()
    assert count.sum() == ((labels >= 0) & (labels < R)).sum()
    # a batch of 1 is shared by the batch
    shared = region_token_stats_np(x, labels[:1], R)
    np.testing.assert_array_equal(shared[0][0], mean[0])
    # the bytes of a token of no region never matter
    dirty = np.where(((labels < 0) | (labels >= R))[..., None], np.nan, x)
    for got, want in zip(region_token_stats_np(dirty, labels, R), (mean, std, count)):
        np.testing.assert_array_equal(got, want)


def test_oracle_table_falls_back_on_both_sides_and_applies_per_token():
    rng = np.random.default_rng(1)
    B, N, L, Cn, R = 2, 2, 40, 4, 3
    v, rv = rng.normal(0.2, 0.8, (B, L, Cn)), rng.normal(-0.4, 1.3, (B, N, L, Cn))
    ql, rl = rng.integers(0, R, (B, L)), rng.integers(0, R, (B, N, L))
    rl[0, 1][rl[0, 1] == 2] = 0                                    # reference (0, 1) lacks region 2
    ql[1][ql[1] == 1] = 0                                          # picture 1 lacks region 1
    a, b, regional = region_affine_table_np(v, rv, ql, rl, R, min_tokens=2)
    assert not regional[0, 1, 2] and not regional[1, :, 1].any() and regional.sum() == B * N * R - 3
    for bb, n, r in ((0, 1, 2), (1, 0, 1), (1, 1, 1)):
        np.testing.assert_array_equal(a[bb, n, r], a[bb, n, R])
        np.testing.assert_array_equal(b[bb, n, r], b[bb, n, R])
    # slot R is the ordinary affine; a regional slot renormalises its tokens to the style statistics of the region
    from oracle.shared_attn_oracle import adain_affine_np
    a0, b0 = adain_affine_np(v, rv, 1)
    np.testing.assert_allclose(a[:, :, R], a0, rtol=1e-12)
    np.testing.assert_allclose(b[:, :, R], b0, rtol=1e-12, atol=1e-12)
    out = region_apply_np(rv, rl, a, b)
    sel_r, sel_q = rl[0, 0] == 1, ql[0] == 1
    np.testing.assert_allclose(out[0, 0][sel_r].mean(0), v[0][sel_q].mean(0), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out[0, 0][sel_r].std(0, ddof=1), v[0][sel_q].std(0, ddof=1), rtol=1e-4)
    lab = rl.copy()
    lab[0, 0, :5] = (-1, R, 99, -7, R + 1)                         # tokens of no region take slot R
    np.testing.assert_array_equal(region_apply_np(rv, lab, a, b)[0, 0, :5], rv[0, 0, :5] * a[0, 0, R] + b[0, 0, R])


# ---- ops.adain_affine_regions: the fallback rule ----------------------------------------------------------------------------------
def _affine_stand_in(log=None):
    def adain_affine(style, content, *, eps=1e-5):
        B, N, H, _ = content[0].shape
        if log is not None:
            log.append((B, N))
        g = lambda t, n: t.double().numpy().reshape(*((B, N) if n else (B,)), H * 64)
        a, b = affine_from_stats_np((g(style[0], 0), g(style[1], 0)), (g(content[0], 1), g(content[1], 1)), eps)
        f = lambda t: torch.from_numpy(t).float().reshape(B, N, H, 64)
        return f(a), f(b)
    return adain_affine


def _stats_torch(x, labels, R, H):
    mean, std, count = region_token_stats_np(x.double().numpy(), labels.numpy(), R)
    B, M = x.shape[:2]
    f = lambda t: torch.from_numpy(t).float().reshape(B, R, M, H, 64)
    return f(mean), f(std), torch.from_numpy(count).float()


def test_affine_regions_fallback_rule_on_the_device_without_a_sync(monkeypatch):
    from instantrestore_amd import ops
    log = []
    monkeypatch.setattr(ops, "adain_affine", _affine_stand_in(log))
    B, N, L, H, R = 2, 3, 128, 2, 4
    g = torch.Generator().manual_seed(2)
    v, rv = torch.randn(B, L, H * 64, generator=g) * 0.8 + 0.2, torch.randn(B, N, L, H * 64, generator=g) * 1.3 - 0.4
    ql, rl = torch.randint(0, R, (B, L), generator=g), torch.randint(0, R, (B, N, L), generator=g)
    rl[0, 1][rl[0, 1] == 2] = 0                                    # absent on one reference
    ql[1][ql[1] == 1] = 3                                          # absent on one query picture
    rl[1, 2, :] = torch.where(rl[1, 2] == 0, 3, rl[1, 2])
    rl[1, 2, :7] = 0                                               # 7 tokens: below the default min_tokens of 8
    import oracle_ops
    style_g, content_g = oracle_ops.token_stats(v.unsqueeze(1), heads=H), oracle_ops.token_stats(rv, heads=H)
    style, content = _stats_torch(v.unsqueeze(1), ql.unsqueeze(1), R, H), _stats_torch(rv, rl, R, H)
    a, b = ops.adain_affine_regions(style, content, style_g, content_g)
    assert a.shape == b.shape == (B, N, R + 1, H, 64) and a.is_contiguous() and b.is_contiguous()
    assert log == [(B * R * N, 1), (B, N)]                         # two affine calls
    ag, bg = _affine_stand_in()((style_g[0][:, 0], style_g[1][:, 0]), content_g)
    assert torch.equal(a[:, :, R], ag) and torch.equal(b[:, :, R], bg)
    fallen = {(0, 1, 2), (1, 0, 1), (1, 1, 1), (1, 2, 1), (1, 2, 0)}
    for bb in range(B):
        for n in range(N):
            for r in range(R):
                same = torch.equal(a[bb, n, r], ag[bb, n]) and torch.equal(b[bb, n, r], bg[bb, n])
                assert same == ((bb, n, r) in fallen), (bb, n, r)
    # a regional slot is the affine of the regional pair
    ar, br = _affine_stand_in()((style[0][:, 1, 0], style[1][:, 1, 0]), (content[0][:, 1], content[1][:, 1]))
    assert torch.equal(a[0, :, 1], ar[0]) and torch.equal(b[0, :, 1], br[0])
    # the oracle's table
    a_ref, b_ref, regional = region_affine_table_np(v.double().numpy(), rv.double().numpy(), ql.numpy(), rl.numpy(), R)
    assert {tuple(i) for i in np.argwhere(~regional)} == fallen
    np.testing.assert_allclose(a.double().numpy().reshape(B, N, R + 1, -1), a_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(b.double().numpy().reshape(B, N, R + 1, -1), b_ref, rtol=1e-4, atol=1e-4)
    # min_tokens is the caller's: 7 lets the 7-token region through; an absent region (count 0) never does, not even at 0 ... 1
    a7, _ = ops.adain_affine_regions(style, content, style_g, content_g, min_tokens=7)
    assert not torch.equal(a7[1, 2, 0], ag[1, 2]) and torch.equal(a7[0, 1, 2], ag[0, 1])
    a1, b1 = ops.adain_affine_regions(style, content, style_g, content_g, min_tokens=1)
    assert torch.equal(a1[0, 1, 2], ag[0, 1]) and torch.isfinite(a1).all() and torch.isfinite(b1).all()
    # shapes are checked before anything else
    for bad, word in (((style[0][:, :, :, :1], style[1], style[2]), "style statistics"), ((style[0], style[1], style[2][:, :1]), "counts"),
                      ((style[0][:1], style[1][:1], style[2][:1]), "style statistics")):
        with pytest.raises(ValueError, match=word):
            ops.adain_affine_regions(bad, content, style_g, content_g)
    with pytest.raises(ValueError, match="content statistics"):
        ops.adain_affine_regions(style, (content[0][0], content[1][0], content[2]), style_g, content_g)
    with pytest.raises(ValueError, match="content_global"):
        ops.adain_affine_regions(style, content, style_g, (content_g[0][:, :1], content_g[1][:, :1]))
    with pytest.raises(ValueError, match="style_global"):
        ops.adain_affine_regions(style, content, content_g, content_g)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def _host_ptr():
    buf = (C.c_char * 4096)()
    return buf, C.addressof(buf) + (64 - C.addressof(buf) % 64)        # a 64-byte aligned host address (never dereferenced)


def _ordered(call, err, cases):
    for over, status, word in cases:
        assert call(**over) == status, (over, err())
        assert word in err(), (over, err())
    # the order of the checks: each pair breaks two rules, the EARLIER one answers
    for i in range(len(cases) - 1):
        for j in range(i + 1, len(cases)):
            both = dict(cases[j][0], **cases[i][0])
            if len(both) < len(cases[i][0]) + len(cases[j][0]):
                continue                                  # the same argument twice
            assert call(**both) == cases[i][1] and cases[i][2] in err(), (cases[i][0], cases[j][0], err())


def _stats_args(ptr, **over):
    a = dict(dtype=1, batch=2, heads=3, n_mats=5, len=600, n_regions=8, x=ptr, x_sb=5 * 600 * 192, x_sn=600 * 192, x_sl=192, x_sh=64,
             labels=ptr, lb_sb=5 * 600, lb_sn=600, mean=ptr, std=ptr, count=ptr, workspace=ptr, workspace_bytes=1 << 40)
    a.update(over)
    return [a[k] for k in ("dtype", "batch", "heads", "n_mats", "len", "n_regions", "x", "x_sb", "x_sn", "x_sl", "x_sh", "labels", "lb_sb",
                           "lb_sn", "mean", "std", "count", "workspace", "workspace_bytes")] + [None]


def test_token_stats_regions_refusals_name_the_argument_and_come_in_order():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    keep, ptr = _host_ptr()
    err = lambda: lib.ir_last_error_string().decode()
    call = lambda **over: lib.ir_token_stats_labelled(*_stats_args(ptr, **over))
    cases = [
        (dict(dtype=2), UNSUPPORTED, "dtype"),
        (dict(batch=0), INVALID, "batch"), (dict(heads=-1), INVALID, "heads"), (dict(n_mats=0), INVALID, "n_mats"), (dict(len=0), INVALID, "len"),
        (dict(n_regions=0), INVALID, "n_regions"),
        (dict(x=None), INVALID, "x is NULL"), (dict(labels=None), INVALID, "labels is NULL"), (dict(mean=None), INVALID, "mean is NULL"),
        (dict(std=None), INVALID, "std is NULL"), (dict(workspace=None), INVALID, "workspace is NULL"),
        (dict(x=ptr + 8), UNSUPPORTED, "x must be 16-byte aligned"), (dict(x_sl=196), UNSUPPORTED, "x stride"), (dict(x_sb=-192), UNSUPPORTED, "x stride"),
        (dict(lb_sn=599), INVALID, "lb_sn"), (dict(lb_sb=-1), INVALID, "lb_sb"),
        (dict(labels=ptr + 2), UNSUPPORTED, "labels"), (dict(mean=ptr + 2), UNSUPPORTED, "mean"),
        (dict(std=ptr + 2), UNSUPPORTED, "std"), (dict(count=ptr + 2), UNSUPPORTED, "count"),
        (dict(workspace_bytes=lib.ir_token_stats_labelled_workspace_bytes(2, 3, 5, 600, 8) - 1), WORKSPACE, "workspace"),
    ]
    _ordered(call, err, cases)
    assert call(n_regions=33) == INVALID and "n_regions" in err()
    assert call(n_regions=32, workspace_bytes=0) == WORKSPACE and call(n_regions=1, workspace_bytes=0) == WORKSPACE
    assert call(batch=13108, workspace_bytes=0) == UNSUPPORTED and "grid" in err()          # 13108 * 5 > 65535
    assert call(heads=65536, workspace_bytes=0) == UNSUPPORTED and "grid" in err()
    assert call(count=None, lb_sb=0, workspace_bytes=0) == WORKSPACE                        # optional count, shared labels
    del keep


def test_regions_workspace_bytes_grow_with_chunks_heads_matrices_and_regions():
    from instantrestore_amd import _lib
    assert _lib.IR_ADAIN_REGIONS_MAX == _lib.IR_REGION_MAX == 32
    L = _lib.lib()
    ws = L.ir_token_stats_labelled_workspace_bytes
    one = ws(1, 1, 1, 1, 1)
    assert one == L.ir_token_stats_weighted_workspace_bytes(1, 1, 1, 1) and one >= (128 + 1) * 4
    assert ws(1, 1, 1, 256, 1) == one and ws(1, 1, 1, 257, 1) == 2 * one and ws(1, 1, 1, 1, 32) == 32 * one
    assert ws(2, 3, 5, 600, 8) == 2 * 3 * 5 * 3 * 8 * one
    assert ws(0, 1, 1, 1, 1) == 0 and ws(1, 1, 1, 0, 1) == 0 and ws(1, 1, 1, 1, 0) == 0 and ws(1, 1, 1, 1, 33) == 0
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "instantrestore_hip.h")).read()
    assert "#define IR_ADAIN_REGIONS_MAX 32" in hdr and "#define IR_ABI_VERSION 10" in hdr
    for sym in ("ir_token_stats_labelled_workspace_bytes", "ir_token_stats_labelled", "ir_adain_apply_labelled"):
        assert re.search(r"\b%s\(" % sym, hdr) and sym in _lib.SYMBOLS


def _apply_args(ptr, **over):
    a = dict(dtype=1, batch=2, heads=3, n_refs=4, len=600, n_regions=8, x=ptr, x_sb=4 * 600 * 192, x_sn=600 * 192, x_sl=192, x_sh=64,
             labels=ptr, lb_sb=4 * 600, lb_sn=600, a=ptr, b=ptr, y=ptr, y_sb=4 * 600 * 192, y_sn=600 * 192, y_sl=192, y_sh=64)
    a.update(over)
    return [a[k] for k in ("dtype", "batch", "heads", "n_refs", "len", "n_regions", "x", "x_sb", "x_sn", "x_sl", "x_sh", "labels", "lb_sb",
                           "lb_sn", "a", "b", "y", "y_sb", "y_sn", "y_sl", "y_sh")] + [None]


def test_adain_apply_regions_refusals_name_the_argument_and_come_in_order():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    keep, ptr = _host_ptr()
    err = lambda: lib.ir_last_error_string().decode()
    call = lambda **over: lib.ir_adain_apply_labelled(*_apply_args(ptr, **over))
    cases = [
        (dict(dtype=3), UNSUPPORTED, "dtype"),
        (dict(batch=0), INVALID, "batch"), (dict(heads=0), INVALID, "heads"), (dict(n_refs=-2), INVALID, "n_refs"), (dict(len=0), INVALID, "len"),
        (dict(n_regions=33), INVALID, "n_regions"),
        (dict(x=None), INVALID, "x is NULL"), (dict(y=None), INVALID, "y is NULL"), (dict(a=None), INVALID, "a / b is NULL"),
        (dict(labels=None), INVALID, "labels is NULL"),
        (dict(y=ptr + 8), UNSUPPORTED, "16-byte aligned"), (dict(y_sl=196), UNSUPPORTED, "stride"), (dict(x_sn=-8), UNSUPPORTED, "stride"),
        (dict(lb_sn=599), INVALID, "lb_sn"), (dict(lb_sb=-1), INVALID, "lb_sb"),
        (dict(labels=ptr + 2), UNSUPPORTED, "4-byte"),
    ]
    _ordered(call, err, cases)
    assert call(b=None) == INVALID and "a / b is NULL" in err() and call(n_regions=0) == INVALID
    assert call(a=ptr + 1) == UNSUPPORTED and call(b=ptr + 2) == UNSUPPORTED and call(x=ptr + 2) == UNSUPPORTED
    del keep


# ---- ops --------------------------------------------------------------------------------------------------------------------------
def test_ops_have_no_cpu_path_and_check_their_arguments_before_any_launch(monkeypatch):
    from instantrestore_amd import ops
    x = torch.zeros(2, 3, 16, 128, dtype=torch.bfloat16)
    lab = torch.zeros(2, 3, 16, dtype=torch.int32)
    a = torch.zeros(2, 3, 5, 2, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_stats_regions(x, lab, heads=2, n_regions=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adain_apply_regions(x, lab, a, a, heads=2)
    # with the device check out of the way every shape / dtype error still comes before the library is touched
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    monkeypatch.setattr(ops._lib, "lib", lambda: pytest.fail("a launch was attempted"))
    bad = [
        (dict(labels=lab[:, :, :15]), ValueError, "labels"), (dict(labels=lab[:, 0]), ValueError, "labels"),
        (dict(labels=torch.zeros(3, 3, 16, dtype=torch.int32)), ValueError, "labels"), (dict(labels=lab.long()), TypeError, "labels"),
        (dict(n_regions=0), ValueError, "n_regions"), (dict(n_regions=33), ValueError, "n_regions"),
    ]
    for kw, exc, word in bad:
        args = dict(labels=lab, n_regions=4)
        args.update(kw)
        with pytest.raises(exc, match=word):
            ops.token_stats_regions(x, args["labels"], heads=2, n_regions=args["n_regions"])
    with pytest.raises(ValueError, match="expected"):
        ops.token_stats_regions(x[0], lab, heads=2, n_regions=4)
    for kw, exc, word in bad[:4]:
        with pytest.raises(exc, match=word):
            ops.adain_apply_regions(x, kw["labels"], a, a, heads=2)
    with pytest.raises(ValueError, match="a, b"):
        ops.adain_apply_regions(x, lab, a[:, :2], a[:, :2], heads=2)
    with pytest.raises(ValueError, match="a, b"):
        ops.adain_apply_regions(x, lab, a[:, :, :1], a[:, :, :1], heads=2)          # R + 1 slots with R >= 1
    with pytest.raises(ValueError, match="a, b"):
        ops.adain_apply_regions(x, lab, a, a[:, :, :4], heads=2)
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.adain_apply_regions(x, lab, a.double(), a.double(), heads=2)
    with pytest.raises(ValueError, match="n_regions"):
        ops.adain_apply_regions(x, lab, torch.zeros(2, 3, 34, 2, 64), torch.zeros(2, 3, 34, 2, 64), heads=2)
    with pytest.raises(ValueError, match="out"):
        ops.adain_apply_regions(x, lab, a, a, heads=2, out=torch.zeros(2, 3, 16, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="out"):
        ops.adain_apply_regions(x, lab, a, a, heads=2, out=torch.zeros(2, 3, 16, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="out"):
        ops.adain_apply_regions(x, lab, a, a, heads=2, out=torch.zeros(2, 3, 16, 132, dtype=torch.bfloat16)[..., 4:])
    for fn in (ops.token_stats_regions, ops.adain_apply_regions, ops.adain_affine_regions):
        assert fn.__doc__


# ---- the processors' host logic (CPU stand-in) ------------------------------------------------------------------------------------
class _RegionShim:
    """tests/oracle_ops.py plus float64 stand-ins of the new ops and a call log"""

    def __init__(self):
        import oracle_ops
        self._o = oracle_ops
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._o, name)

    def linear_supported(self, x, w, b):
        return False

    def key_bias(self, *a, **kw):
        from instantrestore_amd import ops
        return ops.key_bias(*a, **kw)

    def region_masks(self, *a, **kw):
        from instantrestore_amd import ops
        return ops.region_masks(*a, **kw)

    def token_stats(self, x, *, heads):
        self.calls.append(("token_stats", dict(shape=tuple(x.shape))))
        return self._o.token_stats(x, heads=heads)

    def adain_stats(self, *a, **kw):
        self.calls.append(("adain_stats", None))
        return self._o.adain_stats(*a, **kw)

    def adain_stats_cached(self, v_self, content_mean, content_std, *, heads, eps=1e-5):
        self.calls.append(("adain_stats_cached", None))
        B, L, _ = v_self.shape
        v = v_self.double().view(B, L, heads, 64)
        a = (v.std(dim=1) + eps).unsqueeze(1) / (content_std.double() + eps)
        return a.float().contiguous(), (v.mean(dim=1).unsqueeze(1) - content_mean.double() * a).float().contiguous()

    def adain_apply(self, *a, **kw):
        self.calls.append(("adain_apply", None))
        return self._o.adain_apply(*a, **kw)

    def token_stats_regions(self, x, labels, *, heads, n_regions, return_count=False):
        self.calls.append(("token_stats_regions", dict(shape=tuple(x.shape), labels=labels.clone(), n_regions=n_regions, count=return_count)))
        assert labels.dtype == torch.int32
        res = _stats_torch(x, labels, n_regions, heads)
        return res if return_count else res[:2]

    def adain_affine_regions(self, style, content, style_global, content_global, *, min_tokens=8, eps=1e-5):
        from instantrestore_amd import ops
        self.calls.append(("adain_affine_regions", dict(min_tokens=min_tokens, style=style, content=content)))
        real, ops.adain_affine = ops.adain_affine, _affine_stand_in()
        try:
            return ops.adain_affine_regions(style, content, style_global, content_global, min_tokens=min_tokens, eps=eps)
        finally:
            ops.adain_affine = real

    def adain_apply_regions(self, x, labels, a, b, *, heads, out=None):
        self.calls.append(("adain_apply_regions", dict(shape=tuple(x.shape), labels=labels.clone(), table=tuple(a.shape))))
        B, N, L, Cn = x.shape
        y = region_apply_np(x.double().numpy(), labels.numpy(), a.double().numpy().reshape(B, N, -1, Cn), b.double().numpy().reshape(B, N, -1, Cn))
        return torch.from_numpy(y).to(x.dtype)

    def shared_attention(self, q, k_self, v_self, ref_k=None, ref_v=None, *, key_bias=None, q_allow=None, key_region=None, **kw):
        self.calls.append(("shared_attention", dict(adain=kw.get("adain"), key_bias=key_bias, q_allow=q_allow, valid_refs=kw.get("valid_refs"),
                                                    ref_v=ref_v)))
        return self._o.shared_attention(q, k_self, v_self, ref_k, ref_v, **kw)     # (bias and regions themselves are not the subject here)


@pytest.fixture()
def shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    s = _RegionShim()
    monkeypatch.setattr(ap, "_ops", s)
    ap._BIAS_ROWS.clear()
    ap._REGION_PAIRS.clear()
    ap._ADAIN_REGION_LABELS.clear()
    return s


def _shared_layer(heads=2, L=16, N=3, adain=True, idx=0):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    g = torch.Generator().manual_seed(3)
    proc = SharedAttnProcessor(self_attn_idx=idx, use_adain=adain, train_input=True)
    attn = Attention(query_dim=64 * heads, heads=heads, dim_head=64, processor=proc)
    x = torch.randn(2, L, 64 * heads, generator=g)
    rk, rv = torch.randn(2, N, L, 64 * heads, generator=g), torch.randn(2, N, L, 64 * heads, generator=g) + 0.3
    return attn, proc, x, {"ref_keys": [rk], "ref_values": [rv]}


def _names(shim, start=0):
    return [c[0] for c in shim.calls[start:]]


REGIONAL = ["token_stats", "token_stats_regions", "token_stats", "token_stats_regions", "adain_affine_regions", "adain_apply_regions",
            "shared_attention"]


def test_processor_takes_the_regional_branch_only_when_asked(shim, monkeypatch):
    import instantrestore_amd.attn_processors as ap
    attn, proc, x, refs = _shared_layer()
    B, L, N, H, R = 2, 16, 3, 2, 2
    g = torch.Generator().manual_seed(5)
    ql = torch.randint(0, R, (B, L), generator=g)
    rl = torch.randint(0, R, (B, N, L), generator=g)
    rl[0, 0, :3] = torch.tensor([-1, R, 7])
    want = []
    real = ap._project_qkv
    monkeypatch.setattr(ap, "_project_qkv", lambda attn_, st, want_stats=False, bi=False: (want.append(want_stats), real(attn_, st, want_stats=want_stats, bi=bi))[1])
    rv = refs["ref_values"][0]
    full = (rv.view(B, N, L, H, 64).mean(2), rv.view(B, N, L, H, 64).std(2))
    with torch.no_grad():
        # without the kwarg (or with None): the recorded calls are those of the parent
        plain = attn(x, **refs)
        assert _names(shim) == ["adain_stats", "shared_attention"]
        n = len(shim.calls)
        assert torch.equal(attn(x, adain_regions=None, adain_n_regions=R, adain_region_min_tokens=2, **refs), plain)
        assert _names(shim, n) == ["adain_stats", "shared_attention"]
        n = len(shim.calls)
        attn(x, ref_stats=[full], **refs)
        assert _names(shim, n) == ["adain_stats_cached", "shared_attention"] and want[-1] is True

        # with it: global + regional statistics of this layer's V and of the dense references, the table, the apply, then an
        # attention WITHOUT an affine and without valid_refs on the renormalised V
        n = len(shim.calls)
        valid = torch.tensor([3, 3], dtype=torch.int32)
        y = attn(x, adain_regions=(ql, rl), adain_n_regions=R, adain_region_min_tokens=2, ref_valid=valid, **refs)
        assert _names(shim, n) == REGIONAL and want[-1] is False             # the GEMM's statistics tail is off
        sg, sr, cg, cr, tab, app, att = (c[1] for c in shim.calls[n:])
        assert sg["shape"] == sr["shape"] == (B, 1, L, H * 64) and cg["shape"] == cr["shape"] == (B, N, L, H * 64)
        assert sr["n_regions"] == cr["n_regions"] == R and sr["count"] and cr["count"]
        assert torch.equal(sr["labels"], ql.int().unsqueeze(1)) and torch.equal(cr["labels"], rl.int())
        assert tab["min_tokens"] == 2 and tab["style"][0].shape == (B, R, 1, H, 64) and tab["content"][0].shape == (B, R, N, H, 64)
        assert app["shape"] == (B, N, L, H * 64) and app["table"] == (B, N, R + 1, H, 64) and torch.equal(app["labels"], rl.int())
        assert att["adain"] is None and att["valid_refs"] is None and att["ref_v"] is not rv and not torch.equal(att["ref_v"], rv)
        assert not torch.equal(y, plain) and torch.isfinite(y).all()
        # the default min_tokens follows FOLD_MIN_REF_TOKENS; ref_stats is not consulted
        n = len(shim.calls)
        attn(x, adain_regions=(ql, rl), adain_n_regions=R, ref_stats=[full], **refs)
        assert _names(shim, n) == REGIONAL and shim.calls[n + 4][1]["min_tokens"] == ap.FOLD_MIN_REF_TOKENS == 8 and want[-1] is False
        # one region holding every token is whole-face AdaIN applied to V
        n = len(shim.calls)
        one = attn(x, adain_regions=(torch.zeros(B, L, dtype=torch.int64), torch.zeros(B, N, L, dtype=torch.int64)), adain_n_regions=1, **refs)
        torch.testing.assert_close(one, plain, atol=2e-5, rtol=1e-5)
        # ... and so is a call whose every label is "no region"
        none = attn(x, adain_regions=(torch.full((B, L), -1), torch.full((B, N, L), 40)), adain_n_regions=R, **refs)
        torch.testing.assert_close(none, plain, atol=2e-5, rtol=1e-5)

        # composes: a key bias and the region masks reach the attention beside the renormalised V
        attn(x, adain_regions=(ql, rl), adain_n_regions=R, ref_token_keep=torch.rand(B, N, L, generator=g) < 0.6, ref_weights=torch.ones(B, N), **refs)
        assert shim.calls[-1][1]["key_bias"] is not None and shim.calls[-1][1]["adain"] is None
        attn(x, adain_regions=(ql, rl), adain_n_regions=R, region_labels=(ql, rl), region_allow=torch.eye(R, dtype=torch.bool), **refs)
        assert shim.calls[-1][1]["q_allow"] is not None and shim.calls[-1][1]["adain"] is None
        proc.save_attention_mass = True
        attn(x, adain_regions=(ql, rl), adain_n_regions=R, **refs)
        assert proc.attention_mass.shape[-1] == N + 1
        proc.save_attention_mass = False

        # label pictures are sampled at the layer's token centres, once per geometry, cached by identity and version
        pic_q, pic_r = torch.randint(0, R, (B, 32, 32), generator=g), torch.randint(0, R, (B, N, 32, 32), generator=g)
        calls = []
        from instantrestore_amd import attn_maps
        real_tl = attn_maps.token_labels
        monkeypatch.setattr(attn_maps, "token_labels", lambda p, s: (calls.append(s), real_tl(p, s))[1])
        n = len(shim.calls)
        attn(x, adain_regions=(pic_q, pic_r), adain_n_regions=R, **refs)
        attn(x, adain_regions=(pic_q, pic_r), adain_n_regions=R, **refs)
        assert calls == [4, 4]                                           # the second call hit the cache
        assert torch.equal(shim.calls[n + 1][1]["labels"], real_tl(pic_q, 4).int().unsqueeze(1))
        assert torch.equal(shim.calls[n + 3][1]["labels"], real_tl(pic_r, 4).int().reshape(B, N, L))
        pic_r.add_(1)                                                    # an in-place change bumps the version
        attn(x, adain_regions=(pic_q, pic_r), adain_n_regions=R, **refs)
        assert calls == [4, 4, 4, 4]
        attn(x, adain_regions=(pic_q.clone(), pic_r), adain_n_regions=R, **refs)     # another tensor: another identity
        assert len(calls) == 6

        # malformed pairs
        for bad in (ql, (ql, None), (ql, rl, rl), (torch.zeros(B + 1, L, dtype=torch.int64), rl), (ql, rl[:, :2])):
            with pytest.raises(ValueError, match="adain_regions"):
                attn(x, adain_regions=bad, adain_n_regions=R, **refs)


def test_refusals_come_before_any_launch_and_other_layers_ignore_the_kwargs(shim, monkeypatch):
    import instantrestore_amd.attn_processors as ap
    from face_replace.models.attn_processors import AttnProcessor, FaceIDAttnProcessor, SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    attn, proc, x, refs = _shared_layer()
    B, L, N, R = 2, 16, 3, 2
    lab = (torch.zeros(B, L, dtype=torch.int64), torch.zeros(B, N, L, dtype=torch.int64))
    kw3 = dict(adain_regions=lab, adain_n_regions=R, adain_region_min_tokens=4)
    launched = lambda: [n for n in _names(shim) if n != "adain_stats"]

    class Table:                                                         # stands in for ops.RefKVTable
        shape = (B, N, L, 128)
        dtype = x.dtype
    with torch.no_grad():
        with pytest.raises(ValueError, match="adain_n_regions"):
            attn(x, adain_regions=lab, **refs)
        with pytest.raises(NotImplementedError, match="adain_weights"):
            attn(x, adain_weights=(torch.ones(B, L), None), **kw3, **refs)
        with pytest.raises(NotImplementedError, match="ref_lens"):
            attn(x, ref_lens=[torch.full((B, N), L, dtype=torch.int32)], ref_stats=[(torch.zeros(B, N, 2, 64),) * 2], **kw3, **refs)
        monkeypatch.setattr(ap, "_RefKVTable", Table)
        with pytest.raises(NotImplementedError, match="RefKVTable"):
            attn(x, ref_keys=[Table()], ref_values=[Table()], ref_stats=[(torch.zeros(B, N, 2, 64),) * 2], **kw3)
        assert launched() == []                                          # refused before any pass
        # the refusals the existing features pin stay: regions with a bias, masks with counts
        with pytest.raises(NotImplementedError, match="region_labels together"):
            attn(x, region_labels=lab, region_allow=torch.eye(R, dtype=torch.bool), ref_weights=torch.ones(B, N), **kw3, **refs)
        # without use_adain, on a non-shared layer and on the other processors the kwargs are accepted and ignored
        for layer, kw in ((_shared_layer(adain=False)[0], refs),
                          (Attention(query_dim=128, heads=2, dim_head=64, processor=SharedAttnProcessor(self_attn_idx=None, use_adain=True)), refs),
                          (Attention(query_dim=128, heads=2, dim_head=64, processor=AttnProcessor()), {}),       # (takes no references)
                          (Attention(query_dim=128, heads=2, dim_head=64, processor=FaceIDAttnProcessor(128)),
                           dict(refs, encoder_hidden_states=torch.ones(2, 1, 512)))):      # (a face embedding)
            n = len(shim.calls)
            assert torch.equal(layer(x, **kw3, **kw), layer(x, **kw))
            assert not {"token_stats_regions", "adain_affine_regions", "adain_apply_regions"} & set(_names(shim, n))


def test_overlay_exports_the_same_processors_with_the_three_kwargs():
    import face_replace.models.attn_processors as overlay
    import instantrestore_amd.attn_processors as ap
    assert overlay.SharedAttnProcessor is ap.SharedAttnProcessor
    for cls in (overlay.SharedAttnProcessor, overlay.AttnProcessor, overlay.FaceIDAttnProcessor):
        params = inspect.signature(cls.forward).parameters
        assert all(k in params and params[k].default is None for k in ("adain_regions", "adain_n_regions", "adain_region_min_tokens"))


def test_build_lists_the_new_source_and_the_resource_gate_names_its_kernels():
    import os
    repo = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    assert "adain_regions.hip" in open(os.path.join(repo, "instantrestore_amd", "csrc", "build.sh")).read()
    gate = open(os.path.join(repo, "tools", "check_resources.py")).read()
    assert "token_stats_regions" in gate and "adain_apply_regions" in gate
