"""Mask-aware AdaIN on the CPU-only box: the refusals of ``ir_token_stats_weighted`` / ``ir_adain_affine_from_stats`` (validation
happens before any launch; device pointers are never dereferenced), the ops' argument checks, the float64 oracle's tie to the
reference's own statistics lines, the weight sampling of ``attn_maps`` and the host logic of the processors, the harvest and the
cache (a CPU stand-in for ``ops``, as tests/test_ref_lens_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from adain_weighted_oracle import (affine_from_stats_np, subset_token_stats_np, weighted_adain_affine_np, weighted_token_stats_np)
from oracle import shared_attn_oracle as O

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def _host_ptr():
    buf = (C.c_char * 4096)()
    return buf, C.addressof(buf) + (64 - C.addressof(buf) % 64)        # a 64-byte aligned host address (never dereferenced)


def _stats_args(ptr, **over):
    a = dict(dtype=1, batch=2, heads=3, n_mats=5, len=600, x=ptr, x_sb=5 * 600 * 192, x_sn=600 * 192, x_sl=192, x_sh=64,
             weights=ptr, w_sb=5 * 600, w_sn=600, lens=ptr, ln_sb=5, mean=ptr, std=ptr, wsum=ptr, workspace=ptr, workspace_bytes=1 << 40)
    a.update(over)
    return [a[k] for k in ("dtype", "batch", "heads", "n_mats", "len", "x", "x_sb", "x_sn", "x_sl", "x_sh", "weights", "w_sb", "w_sn",
                           "lens", "ln_sb", "mean", "std", "wsum", "workspace", "workspace_bytes")] + [None]


def test_token_stats_weighted_refusals_name_the_argument_and_come_in_order():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    keep, ptr = _host_ptr()
    err = lambda: lib.ir_last_error_string().decode()
    call = lambda **over: lib.ir_token_stats_weighted(*_stats_args(ptr, **over))
    cases = [
        (dict(dtype=2), UNSUPPORTED, "dtype"),
        (dict(batch=0), INVALID, "batch"), (dict(heads=-1), INVALID, "heads"), (dict(n_mats=0), INVALID, "n_mats"), (dict(len=0), INVALID, "len"),
        (dict(x=None), INVALID, "x is NULL"), (dict(mean=None), INVALID, "mean is NULL"), (dict(std=None), INVALID, "std is NULL"),
        (dict(workspace=None), INVALID, "workspace is NULL"),
        (dict(x=ptr + 8), UNSUPPORTED, "x must be 16-byte aligned"), (dict(x_sl=196), UNSUPPORTED, "x stride"), (dict(x_sb=-192), UNSUPPORTED, "x stride"),
        (dict(w_sn=599), INVALID, "w_sn"), (dict(w_sb=-1), INVALID, "w_sb"), (dict(ln_sb=4), INVALID, "ln_sb"),
        (dict(weights=ptr + 2), UNSUPPORTED, "weights"), (dict(lens=ptr + 2), UNSUPPORTED, "lens"), (dict(mean=ptr + 2), UNSUPPORTED, "mean"),
        (dict(std=ptr + 2), UNSUPPORTED, "std"), (dict(wsum=ptr + 2), UNSUPPORTED, "wsum"),
        (dict(workspace_bytes=lib.ir_token_stats_weighted_workspace_bytes(2, 3, 5, 600) - 1), WORKSPACE, "workspace"),
    ]
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
    # strides of an absent weights / lens are not looked at
    assert call(weights=None, w_sn=0, w_sb=-5, workspace_bytes=0) == WORKSPACE
    assert call(lens=None, ln_sb=0, workspace_bytes=0) == WORKSPACE
    del keep


def test_workspace_bytes_grow_with_chunks_heads_and_matrices():
    from instantrestore_amd import _lib
    ws = _lib.lib().ir_token_stats_weighted_workspace_bytes
    one = ws(1, 1, 1, 1)
    assert one > 0 and ws(1, 1, 1, 256) == one and ws(1, 1, 1, 257) == 2 * one
    assert ws(2, 3, 5, 600) == 2 * 3 * 5 * 3 * one
    assert one >= (128 + 2) * 4                            # mean[64], M2[64], W, W2 per chunk
    assert ws(0, 1, 1, 1) == 0 and ws(1, 1, 1, 0) == 0


def test_adain_affine_from_stats_refusals():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    keep, ptr = _host_ptr()
    err = lambda: lib.ir_last_error_string().decode()
    ok = [2, 3, 4, ptr, ptr, ptr, ptr, 1e-5, ptr, ptr, None]
    for pos, word in ((0, "batch"), (1, "heads"), (2, "n_refs")):
        args = list(ok)
        args[pos] = 0
        assert lib.ir_adain_affine_from_stats(*args) == INVALID and word in err()
    for pos, word in ((3, "style_mean"), (4, "style_std"), (5, "content_mean"), (6, "content_std"), (8, "a"), (9, "b")):
        args = list(ok)
        args[pos] = None
        assert lib.ir_adain_affine_from_stats(*args) == INVALID and word in err(), err()
        args[pos] = ptr + 2
        assert lib.ir_adain_affine_from_stats(*args) == UNSUPPORTED and "4-byte" in err(), err()
    args = list(ok)
    args[0], args[3] = 0, ptr + 2
    assert lib.ir_adain_affine_from_stats(*args) == INVALID       # sizes before alignment
    del keep


# ---- ops --------------------------------------------------------------------------------------------------------------------------
def test_ops_have_no_cpu_path_and_check_their_arguments_before_any_launch(monkeypatch):
    from instantrestore_amd import ops
    x = torch.zeros(2, 3, 16, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_stats_weighted(x, heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_stats_weighted(x, heads=2, weights=torch.ones(2, 3, 16), lens=torch.ones(2, 3, dtype=torch.int32))
    st, ct = torch.zeros(2, 2, 64), torch.zeros(2, 3, 2, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.adain_affine((st, st), (ct, ct))
    # with the device check out of the way every shape / dtype error still comes before the library is touched
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: None)
    monkeypatch.setattr(ops._lib, "lib", lambda: pytest.fail("a launch was attempted"))
    bad = [
        (dict(weights=torch.ones(2, 3, 15)), ValueError, "weights"), (dict(weights=torch.ones(3, 3, 16)), ValueError, "weights"),
        (dict(weights=torch.ones(2, 16)), ValueError, "weights"), (dict(weights=torch.ones(2, 3, 16, dtype=torch.float64)), TypeError, "weights"),
        (dict(lens=torch.ones(2, 3, dtype=torch.int64)), TypeError, "lens"), (dict(lens=torch.ones(3, 2, dtype=torch.int32)), ValueError, "lens"),
    ]
    for kw, exc, word in bad:
        with pytest.raises(exc, match=word):
            ops.token_stats_weighted(x, heads=2, **kw)
    with pytest.raises(ValueError, match="expected"):
        ops.token_stats_weighted(x[0], heads=2)
    with pytest.raises(ValueError, match="content statistics"):
        ops.adain_affine((st, st), (ct[0], ct[0]))
    with pytest.raises(ValueError, match="style statistics"):
        ops.adain_affine((st[:1], st[:1]), (ct, ct))
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.adain_affine((st.double(), st.double()), (ct, ct))


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def test_oracle_with_a_mask_is_the_reference_statistics_of_the_kept_tokens():
    rng = np.random.default_rng(0)
    B, M, L, Cc = 2, 3, 37, 16
    x = rng.standard_normal((B, M, L, Cc)) + 0.3
    for rate in (0.1, 0.5, 0.9):
        keep = rng.random((B, M, L)) < rate
        keep[0, 0] = False                                   # no token
        keep[0, 1] = np.arange(L) == 11                      # one token
        mean, std, W = weighted_token_stats_np(x, keep.astype(np.float64))
        m2, s2 = subset_token_stats_np(x, keep)
        np.testing.assert_allclose(mean, m2, rtol=0, atol=1e-13)
        np.testing.assert_allclose(std, s2, rtol=1e-12, atol=1e-13)
        assert np.array_equal(W, keep.sum(-1))
        assert not mean[0, 0].any() and not std[0, 0].any()                       # W == 0: (0, 0)
        assert np.array_equal(mean[0, 1], x[0, 1, 11]) and not std[0, 1].any()    # one token: (x, 0)
    # counts are a prefix mask; counts with weights multiply; zero-weight tokens are selected away whatever their bytes
    lens = np.array([[0, 1, 37], [5, 40, -3]])
    pref = np.arange(L)[None, None] < np.clip(lens, 0, L)[:, :, None]
    a = weighted_token_stats_np(x, None, lens)
    b = subset_token_stats_np(x, pref)
    np.testing.assert_allclose(a[0], b[0], atol=1e-13)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-12, atol=1e-13)
    w = rng.random((B, M, L))
    bad = x.copy()
    bad[~pref] = np.nan
    bad[w < 0.2] = np.inf
    clean = weighted_token_stats_np(x, np.where(w < 0.2, 0, w), lens)
    dirty = weighted_token_stats_np(bad, np.where(w < 0.2, 0, w), lens)
    assert all(np.array_equal(c, d) for c, d in zip(clean, dirty)) and all(np.isfinite(c).all() for c in clean)
    # the full axis with unit weights is token_stats_np itself, and the affine is adain_affine_np
    mean, std, _ = weighted_token_stats_np(x)
    for m in range(M):
        mu, sd = O.token_stats_np(x[:, m])
        np.testing.assert_allclose(mean[:, m], mu[:, 0], atol=1e-13)
        np.testing.assert_allclose(std[:, m], sd[:, 0], rtol=1e-12)
    v = rng.standard_normal((B, L, Cc))
    x[1, 2] = 0.0                                            # a zero-filled reference: a = 0, b = the style mean
    a1, b1 = weighted_adain_affine_np(v, x)
    a0, b0 = O.adain_affine_np(v, x, 1)
    np.testing.assert_allclose(a1, a0, rtol=1e-12)
    np.testing.assert_allclose(b1, b0, rtol=1e-12, atol=1e-13)
    a2, _ = affine_from_stats_np((np.zeros((1, 4)), np.ones((1, 4))), (np.zeros((1, 2, 4)), np.zeros((1, 2, 4))))
    assert not a2.any()


# ---- attn_maps --------------------------------------------------------------------------------------------------------------------
def test_token_weights_sample_where_token_labels_sample():
    from instantrestore_amd import attn_maps
    g = torch.Generator().manual_seed(1)
    for shape in ((2, 64, 64), (2, 3, 48, 80), (1, 2, 7, 5)):
        pic = torch.rand(shape, generator=g) < 0.4
        for side in (1, 4, 16, 31):
            w = attn_maps.token_weights(pic, side)
            lab = attn_maps.token_labels(pic.to(torch.int32), side)
            assert w.dtype == torch.float32 and tuple(w.shape) == tuple(shape[:-2]) + (side * side,)
            assert torch.equal(w.reshape(shape[0], -1), lab.to(torch.float32))
        soft = torch.rand(shape, generator=g)
        w = attn_maps.token_weights(soft, 4)
        assert float(w.reshape(-1)[0]) == float(soft.reshape(-1, *shape[-2:])[0, shape[-2] // 8, shape[-1] // 8])   # the centre pixel, not a mean
    with pytest.raises(ValueError, match="token_weights"):
        attn_maps.token_weights(torch.ones(4, 4), 2)
    keep = torch.rand(2, 3, 16, generator=g) < 0.5
    w = attn_maps.weights_from_keep(keep)
    assert w.dtype == torch.float32 and torch.equal(w, keep.float())
    assert torch.equal(attn_maps.weights_from_keep(keep.view(2, 3, 4, 4)), w)
    with pytest.raises(ValueError, match="weights_from_keep"):
        attn_maps.weights_from_keep(keep[0, 0])


# ---- the processors' host logic (CPU stand-in) ------------------------------------------------------------------------------------
class _WeightedShim:
    """tests/oracle_ops.py plus float64 stand-ins of the two new ops and a call log"""

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

    def token_stats(self, x, *, heads):
        self.calls.append(("token_stats", None))
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

    def token_stats_weighted(self, x, *, heads, weights=None, lens=None, return_wsum=False):
        self.calls.append(("token_stats_weighted", dict(shape=tuple(x.shape), weights=None if weights is None else weights.clone(), lens=lens)))
        B, M, L, _ = x.shape
        mean, std, W = weighted_token_stats_np(x.double().numpy(), None if weights is None else weights.numpy(),
                                               None if lens is None else lens.numpy())
        f = lambda t: torch.from_numpy(t).float().reshape(B, M, heads, 64)
        return (f(mean), f(std), torch.from_numpy(W).float()) if return_wsum else (f(mean), f(std))

    def adain_affine(self, style, content, *, eps=1e-5):
        self.calls.append(("adain_affine", dict(style=style, content=content)))
        B, N, H, _ = content[0].shape
        g = lambda t, n: t.double().numpy().reshape(*((B, N) if n else (B,)), H * 64)
        a, b = affine_from_stats_np((g(style[0], 0), g(style[1], 0)), (g(content[0], 1), g(content[1], 1)), eps)
        f = lambda t: torch.from_numpy(t).float().reshape(B, N, H, 64)
        return f(a), f(b)

    def shared_attention(self, q, k_self, v_self, ref_k=None, ref_v=None, *, key_bias=None, **kw):
        self.calls.append(("shared_attention", dict(adain=kw.get("adain"), key_bias=key_bias)))
        return self._o.shared_attention(q, k_self, v_self, ref_k, ref_v, **kw)     # (the bias itself is not the subject here)


@pytest.fixture()
def shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    import instantrestore_amd.kv_harvest as kh
    s = _WeightedShim()
    monkeypatch.setattr(ap, "_ops", s)
    monkeypatch.setattr(kh, "_ops", s)
    ap._BIAS_ROWS.clear()
    ap._ADAIN_WEIGHTS.clear()
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


def test_processor_takes_the_weighted_branch_only_when_asked(shim, monkeypatch):
    import instantrestore_amd.attn_processors as ap
    attn, proc, x, refs = _shared_layer()
    B, L, N, H = 2, 16, 3, 2
    g = torch.Generator().manual_seed(5)
    self_w = torch.rand(B, L, generator=g) < 0.6
    ref_w = (torch.rand(B, N, L, generator=g) < 0.5).float()
    want = []
    real = ap._project_qkv
    monkeypatch.setattr(ap, "_project_qkv", lambda attn_, st, want_stats=False, bi=False: (want.append(want_stats), real(attn_, st, want_stats=want_stats, bi=bi))[1])
    rv = refs["ref_values"][0]
    full = (rv.view(B, N, L, H, 64).mean(2), rv.view(B, N, L, H, 64).std(2))
    with torch.no_grad():
        # default path untouched when the kwarg is absent
        plain = attn(x, **refs)
        assert _names(shim) == ["adain_stats", "shared_attention"]
        n = len(shim.calls)
        assert torch.equal(attn(x, adain_weights=None, **refs), plain) and _names(shim, n) == ["adain_stats", "shared_attention"]
        n = len(shim.calls)
        attn(x, ref_stats=[full], **refs)
        assert _names(shim, n) == ["adain_stats_cached", "shared_attention"] and want[-1] is True

        # no ref_stats: one weighted pass over the dense references, one over this layer's V, then the affine
        n = len(shim.calls)
        y = attn(x, adain_weights=(self_w, ref_w), **refs)
        assert _names(shim, n) == ["token_stats_weighted", "token_stats_weighted", "adain_affine", "shared_attention"]
        assert want[-1] is False                                         # the GEMM's statistics tail is off: its partials are unweighted
        content, style = shim.calls[n][1], shim.calls[n + 1][1]
        assert content["shape"] == (B, N, L, H * 64) and torch.equal(content["weights"], ref_w)
        assert style["shape"] == (B, 1, L, H * 64) and torch.equal(style["weights"], self_w.float().unsqueeze(1))
        assert shim.calls[n + 3][1]["adain"] is not None and not torch.equal(y, plain)
        # all-ones weights are the unweighted statistics
        ones = attn(x, adain_weights=(torch.ones(B, L), torch.ones(B, N, L)), **refs)
        torch.testing.assert_close(ones, plain, atol=1e-5, rtol=1e-5)
        # either element may be None
        n = len(shim.calls)
        attn(x, adain_weights=(None, ref_w), **refs)
        assert shim.calls[n + 1][1]["weights"] is None and torch.equal(shim.calls[n][1]["weights"], ref_w)
        n = len(shim.calls)
        attn(x, adain_weights=(self_w, None), **refs)
        assert shim.calls[n][1]["weights"] is None

        # ref_stats given: they ARE the content statistics (finished by the caller), only the style pass runs
        n = len(shim.calls)
        kept = shim.token_stats_weighted(rv, heads=H, weights=ref_w)
        shim.calls.pop()
        y2 = attn(x, adain_weights=(self_w, ref_w), ref_stats=[kept], **refs)
        assert _names(shim, n) == ["token_stats_weighted", "adain_affine", "shared_attention"] and want[-1] is False
        assert shim.calls[n][1]["shape"] == (B, 1, L, H * 64)
        assert shim.calls[n + 1][1]["content"][0] is kept[0] and shim.calls[n + 1][1]["content"][1] is kept[1]
        assert torch.equal(y2, y)

        class Finished:                                                  # the partials form: .finished() is consulted
            def finished(self):
                return kept
            def sync_to_current(self):
                pass
        assert torch.equal(attn(x, adain_weights=(self_w, ref_w), ref_stats=[Finished()], **refs), y)

        # with ref_lens the statistics are still required, and may now be kept-token statistics
        lens = torch.tensor([[16, 4, 5], [2, 16, 9]], dtype=torch.int32)
        with pytest.raises(ValueError, match="ref_stats"):
            attn(x, adain_weights=(self_w, ref_w), ref_lens=[lens], **refs)

        # works with ref_token_keep from the same mask: the bias and the affine both reach the attention
        n = len(shim.calls)
        attn(x, adain_weights=(self_w, ref_w), ref_token_keep=ref_w.bool(), **refs)
        last = shim.calls[-1][1]
        assert last["adain"] is not None and last["key_bias"] is not None

        # weight pictures are sampled at the layer's token centres, once per geometry
        pic_s, pic_r = torch.rand(B, 32, 32, generator=g), torch.rand(B, N, 32, 32, generator=g) < 0.5
        calls = []
        from instantrestore_amd import attn_maps
        real_tw = attn_maps.token_weights
        monkeypatch.setattr(attn_maps, "token_weights", lambda p, s: (calls.append(s), real_tw(p, s))[1])
        n = len(shim.calls)
        attn(x, adain_weights=(pic_s, pic_r), **refs)
        attn(x, adain_weights=(pic_s, pic_r), **refs)
        assert calls == [4, 4]                                           # the second call hit the cache
        assert torch.equal(shim.calls[n][1]["weights"], real_tw(pic_r, 4)) and torch.equal(shim.calls[n + 1][1]["weights"], real_tw(pic_s, 4).unsqueeze(1))
        pic_s.mul_(0.5)                                                  # an in-place change bumps the version
        attn(x, adain_weights=(pic_s, pic_r), **refs)
        assert calls == [4, 4, 4, 4]
        with pytest.raises(ValueError, match="adain_weights"):
            attn(x, adain_weights=self_w, **refs)
        with pytest.raises(ValueError, match="adain_weights"):
            attn(x, adain_weights=(torch.ones(B + 1, L), None), **refs)


def test_table_without_stats_raises_and_other_layers_ignore_the_kwarg(shim, monkeypatch):
    import instantrestore_amd.attn_processors as ap
    from face_replace.models.attn_processors import AttnProcessor, FaceIDAttnProcessor, SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    attn, proc, x, refs = _shared_layer()
    B, L, N = 2, 16, 3
    w = (torch.ones(B, L), torch.ones(B, N, L))

    class Table:                                                         # stands in for ops.RefKVTable
        shape = (B, N, L, 128)
        dtype = x.dtype
    monkeypatch.setattr(ap, "_RefKVTable", Table)
    with torch.no_grad():
        with pytest.raises(ValueError, match="ref_stats"):
            attn(x, adain_weights=w, ref_keys=[Table()], ref_values=[Table()])
        assert "token_stats_weighted" not in _names(shim)                # refused before any pass
        # without use_adain, on a non-shared layer and on the other processors the kwarg is accepted and ignored
        for layer, kw in ((_shared_layer(adain=False)[0], refs),
                          (Attention(query_dim=128, heads=2, dim_head=64, processor=SharedAttnProcessor(self_attn_idx=None, use_adain=True)), refs),
                          (Attention(query_dim=128, heads=2, dim_head=64, processor=AttnProcessor()), {}),       # (takes no references)
                          (Attention(query_dim=128, heads=2, dim_head=64, processor=FaceIDAttnProcessor(128)),
                           dict(refs, encoder_hidden_states=torch.ones(2, 1, 512)))):      # (a face embedding)
            n = len(shim.calls)
            assert torch.equal(layer(x, adain_weights=w, **kw), layer(x, **kw))
            assert "token_stats_weighted" not in _names(shim, n) and "adain_affine" not in _names(shim, n)


def test_overlay_exports_the_same_processor():
    import face_replace.models.attn_processors as overlay
    import instantrestore_amd.attn_processors as ap
    import inspect
    assert overlay.SharedAttnProcessor is ap.SharedAttnProcessor
    for cls in (overlay.SharedAttnProcessor, overlay.AttnProcessor, overlay.FaceIDAttnProcessor):
        assert "adain_weights" in inspect.signature(cls.forward).parameters


# ---- capture, harvest, cache ------------------------------------------------------------------------------------------------------
class _Unet(torch.nn.Module):
    def __init__(self, n_layers=2, heads=2):
        super().__init__()
        from face_replace.models.attn_processors import AttnProcessor
        from instantrestore_amd.attention import Attention
        self.layers = torch.nn.ModuleList([Attention(query_dim=64 * heads, heads=heads, dim_head=64, processor=AttnProcessor()) for _ in range(n_layers)])

    @property
    def attn_processors(self):
        return {f"up_blocks.{i}.attn1.processor": l.processor for i, l in enumerate(self.layers)}

    def forward(self, x, timestep=None, encoder_hidden_states=None):
        for l in self.layers:
            x = l(x)
        return x


def test_capture_layer_uses_the_weighted_call_and_the_harvest_restores_the_attribute(shim, monkeypatch):
    import instantrestore_amd.attn_processors as ap
    from instantrestore_amd import kv_harvest
    unet = _Unet()
    procs = list(unet.attn_processors.values())
    assert all(p.capture_stats_weights is None for p in procs)
    for p in procs:
        p.values = torch.zeros(1, 1, 1)          # the stand-in has no device: let the stash believe it is there
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ap.AttnProcessor, "_mark_ready", lambda self: None)
    B, N, L = 2, 3, 16
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B * N, L, 128, generator=g)
    w = torch.rand(B, N, L, generator=g) < 0.5
    want = []
    real = ap._project_qkv
    monkeypatch.setattr(ap, "_project_qkv", lambda attn_, st, want_stats=False, bi=False: (want.append(want_stats), real(attn_, st, want_stats=want_stats, bi=bi))[1])
    with torch.no_grad():
        keys, values, stats = kv_harvest.get_conditioning_keys_values(unet, x, None, None, N, [N] * B, with_stats=True, stats_weights=w)
    assert all(p.capture_stats_weights is None and p.capture_stats is False for p in procs)      # restored
    assert want == [False, False]                                        # never the GEMM-partials route
    assert _names(shim).count("token_stats_weighted") == 2 and "token_stats" not in _names(shim)
    call = [c for c in shim.calls if c[0] == "token_stats_weighted"][0][1]
    assert call["shape"] == (B * N, 1, L, 128) and torch.equal(call["weights"], w.float().reshape(B * N, 1, L))
    ref = subset_token_stats_np(values[0].double().numpy(), w.numpy())
    np.testing.assert_allclose(stats[0][0].reshape(B, N, 128).numpy(), ref[0], atol=1e-6)
    np.testing.assert_allclose(stats[0][1].reshape(B, N, 128).numpy(), ref[1], rtol=1e-5, atol=1e-6)
    # a call that raises restores too; stats_weights without with_stats is refused
    monkeypatch.setattr(unet, "forward", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom")))
    with pytest.raises(RuntimeError, match="boom"):
        kv_harvest.get_conditioning_keys_values(unet, x, None, None, N, [N] * B, with_stats=True, stats_weights=w)
    assert all(p.capture_stats_weights is None and p.capture_stats is False for p in procs)
    with pytest.raises(ValueError, match="with_stats"):
        kv_harvest.get_conditioning_keys_values(unet, x, None, None, N, [N] * B, stats_weights=w)
    # enable_ref_stats sets and clears it; a per-call value comes back to what enable_ref_stats had set
    kv_harvest.enable_ref_stats(unet, True, weights=w)
    assert all(p.capture_stats_weights is w and p.capture_stats for p in procs)
    kv_harvest.enable_ref_stats(unet, False)
    assert all(p.capture_stats_weights is None and not p.capture_stats for p in procs)


def test_cache_takes_new_statistics_after_a_compaction():
    from instantrestore_amd.kv_cache import ReferenceKVCache
    cache = ReferenceKVCache()
    g = torch.Generator().manual_seed(0)
    N, L, H = 2, 16, 2
    mk = lambda: [torch.randn(1, N, L, 64 * H, generator=g) for _ in range(2)]
    st = lambda: (torch.randn(1, N, H, 64, generator=g), torch.rand(1, N, H, 64, generator=g))
    cache.get_or_compute("a", lambda: (mk(), mk(), [st(), st()]))
    cache.get_or_compute("b", lambda: (mk(), mk()))
    new = [st(), None]
    cache.set_ref_stats("a", new)
    out = cache.assemble(["a"])
    assert torch.equal(out[2][0][0], new[0][0]) and torch.equal(out[2][0][1], new[0][1]) and out[2][1] is None
    new[0][0].zero_()
    assert out[2][0][0].abs().sum() > 0                                  # cloned
    cache.set_ref_stats("b", [st(), st()])                               # an entry cached without statistics gains them
    assert len(cache.assemble(["a", "b"])) == 3
    with pytest.raises(ValueError, match="layers"):
        cache.set_ref_stats("a", [st()])
    with pytest.raises(ValueError, match="layer 1"):
        cache.set_ref_stats("a", [st(), (torch.zeros(1, N, H, 32), torch.zeros(1, N, H, 32))])
    with pytest.raises(KeyError):
        cache.set_ref_stats("c", [st(), st()])
