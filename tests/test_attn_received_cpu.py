"""The key-side read-out (``ir_attn_received`` / ``ops.attn_received`` / ``SharedAttnProcessor.attention_received_weights``):
everything that can be checked without a GPU - the symbol and its validation, the wrapper's checks, the picture and keep-mask
helpers, the processor's host logic on the oracle-backed stand-in ``tests/oracle_ops_received.py``, that helper itself against a
brute-force loop, the kernel file's adherence to the shared read-out header, and the kernels' register report."""
import ctypes as C
import glob
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from test_attn_match_cpu import _args, _copy_into

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_bound_with_its_constants():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "ir_attn_received") and "ir_attn_received" in _lib.SYMBOLS
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION                      # a new function, no struct change
    header = open(os.path.join(REPO, "include", "instantrestore_hip.h")).read()
    for name, val in (("IR_RECEIVED_PER_HEAD", 0), ("IR_RECEIVED_HEAD_MEAN", 1), ("IR_RECEIVED_MAX_CHANNELS", 8)):
        assert re.search(r"#define %s %d\b" % (name, val), header), name
    assert (_lib.IR_RECEIVED_PER_HEAD, _lib.IR_RECEIVED_HEAD_MEAN, _lib.IR_RECEIVED_MAX_CHANNELS) == (0, 1, 8)
    assert re.search(r"int ir_attn_received\(const ir_shared_attn_args\* args, const float\* weights, int64_t w_sb, int64_t w_si, "
                     r"int32_t channels,\s*int32_t reduce, float\* recv, void\* stream\);", header)
    res, argtypes = _lib.SYMBOLS["ir_attn_received"]
    assert res is C.c_int and len(argtypes) == 8 and argtypes[2] is C.c_int64 and argtypes[3] is C.c_int64 and argtypes[4] is C.c_int32
    kernels = open(os.path.join(REPO, "instantrestore_amd", "csrc", "ir_kernels.h")).read()
    assert "ir_launch_attn_received" in kernels and "kReceivedMaxChannels = 8" in kernels


def test_validation_names_the_field_before_any_launch():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    off = lambda n: C.cast(C.c_void_p(ptr.value + n), C.c_void_p)

    def call(weights=ptr, sb=0, si=8, ch=2, red=0, recv=ptr, args=a):
        return lib.ir_attn_received(None if args is None else C.byref(args), weights, sb, si, ch, red, recv, None)

    assert call(args=None) == INVALID and b"args" in err()
    assert call(recv=None) == INVALID and b"recv" in err()
    a.lse = None
    assert call() == INVALID and b"lse" in err()
    a.lse = ptr
    for ch in (0, 9, -1):
        assert call(ch=ch, si=16) == UNSUPPORTED and b"channels" in err()
    for ch in (2, 8):
        assert call(weights=None, ch=ch, si=8) == INVALID and b"weights" in err() and b"channels" in err()
    assert call(ch=4, si=3) == INVALID and b"w_si" in err()
    assert call(si=-8) == INVALID and b"w_si" in err()
    assert call(weights=None, ch=1, si=-1) == INVALID and b"w_si" in err()
    assert call(sb=-1) == INVALID and b"w_sb" in err()
    assert call(weights=off(2)) == UNSUPPORTED and b"weights" in err()
    assert call(recv=off(2)) == UNSUPPORTED and b"recv" in err()
    assert call(recv=off(1)) == UNSUPPORTED and b"recv" in err()
    for bad in (-1, 2):
        assert call(red=bad) == UNSUPPORTED and b"reduce" in err()
    a.tuning = 13
    assert call() == UNSUPPORTED and b"tuning" in err() and b"ir_attn_received" in err()
    a.tuning = 0
    a.struct_size = 7
    assert call() == INVALID and b"ABI mismatch" in err()


def test_more_than_2_31_work_items_are_refused():
    """B * H * key groups beyond 2^31 - 4: refused by arithmetic on the sizes, before any launch"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    a.batch, a.heads, a.n_refs, a.len_ref = 1 << 15, 1 << 12, 64, 96 * 1024       # 2^27 (b, h) pairs, more than 16 groups each
    assert lib.ir_attn_received(C.byref(a), None, 0, 1, 1, 0, ptr, None) == UNSUPPORTED and b"grid too large" in lib.ir_last_error_string()


def test_bias_and_ragged_blocks_are_refused_like_the_other_readouts():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    bias = _copy_into(_lib.SharedAttnBiasArgs(), a)
    bias.key_bias = ptr
    assert lib.ir_attn_received(C.byref(bias), ptr, 0, 2, 2, 0, ptr, None) == UNSUPPORTED
    assert b"key_bias" in err() and b"ir_attn_received" in err() and b"ir_attn_transfer" in err()
    ragged = _copy_into(_lib.SharedAttnRaggedArgs(), a)
    ragged.ref_lens, ragged.rl_sb = ptr, 2
    assert lib.ir_attn_received(C.byref(ragged), None, 0, 1, 1, 1, ptr, None) == UNSUPPORTED
    assert b"ref_lens" in err() and b"ir_attn_received" in err() and b"ir_attn_transfer" in err()


# ---- ops ------------------------------------------------------------------------------------------------------------------
def test_ops_attn_received_has_no_cpu_path_and_checks_its_arguments():
    from instantrestore_amd import ops
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    lse = torch.zeros(1, 1, 8)
    w = torch.zeros(8, 2)
    with pytest.raises(ValueError, match="reduce"):
        ops.attn_received(q, q, None, lse, w, heads=1, scale=0.125, reduce="map")
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_received(q, q, None, lse, w, heads=1, scale=0.125)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_received(q, q, None, lse, heads=1, scale=0.125, reduce="head_mean")
    assert ops.RECEIVED_REDUCE == {"none": 0, "head_mean": 1}
    src = inspect.getsource(ops.attn_received)
    assert "_received_weights(weights, B, Lq, q.device)" in src
    assert ".contiguous()" not in src and ".contiguous()" not in inspect.getsource(ops._received_weights)     # the weights are never copied
    assert src.index("_received_weights(") < src.index("data_ptr()")                                           # validated before any pointer is taken


def test_weight_checks_and_strides():
    from instantrestore_amd import ops
    cpu = torch.device("cpu")
    chk = lambda t, B=2, L=24: ops._received_weights(t, B, L, cpu)
    base = torch.zeros(2, 24, 3)
    assert chk(base)[1:] == (72, 3, 3) and chk(base)[0] is base
    assert chk(base[0])[1:] == (0, 3, 3) and chk(base[:1])[1:] == (0, 3, 3)
    wide = torch.zeros(2, 24, 8)[..., :3]                                   # a row stride wider than C, passed through as it is
    got = chk(wide)
    assert got[0] is wide and got[1:] == (192, 8, 3)
    assert chk(torch.zeros(1, 24, 3).expand(2, 24, 3))[1:] == (0, 3, 3)    # an expanded batch axis is stride 0
    # one channel without a channel axis: (L,) and (B, L), any row stride
    one = torch.zeros(24)
    got = chk(one)
    assert got[1:] == (0, 1, 1) and got[0].data_ptr() == one.data_ptr() and tuple(got[0].shape) == (24, 1)
    assert chk(torch.zeros(2, 24))[1:] == (24, 1, 1) and chk(torch.zeros(1, 24))[1:] == (0, 1, 1)
    assert chk(torch.zeros(24, 4)[:, 1])[1:] == (0, 4, 1)                  # a column of a wider buffer
    assert chk(torch.zeros(2, 24, 4)[:, :, 2])[1:] == (96, 4, 1)
    for bad, word in ((base.double(), "fp32"), (base.to(torch.bfloat16), "fp32"), (torch.zeros(2, 2, 24, 3), "weights must be"),
                      (torch.zeros(3, 24, 3), "batch"), (torch.zeros(2, 23, 3), "rows"), (torch.zeros(3, 24), "batch"),
                      (torch.zeros(23), "rows"), (torch.zeros(2, 24, 9), "channels"), (torch.zeros(2, 24, 0), "channels"),
                      (torch.zeros(2, 3, 24).transpose(1, 2), "stride"), (np.zeros((24, 3), dtype=np.float32), "fp32")):
        with pytest.raises(ValueError, match=word):
            chk(bad)
    with pytest.raises(ValueError, match="is on"):
        ops._received_weights(base, 2, 24, torch.device("cuda", 0))
    # two axes that read as (L, C) and as (B, L) - a batch as large as the query axis - are refused, not guessed
    with pytest.raises(ValueError, match="reads as"):
        ops._received_weights(torch.zeros(4, 4), 4, 4, cpu)
    assert ops._received_weights(torch.zeros(4, 3), 4, 4, cpu)[1:] == (0, 3, 3)         # (L, C): only one reading
    assert ops._received_weights(torch.zeros(4, 4, 1), 4, 4, cpu)[1:] == (4, 1, 1)          # three axes say which


def test_ops_signature():
    from instantrestore_amd import ops
    sig = inspect.signature(ops.attn_received)
    names = list(sig.parameters)
    assert names == ["q", "k_self", "ref_k", "lse", "weights", "heads", "scale", "include_self", "reduce", "q_prescaled", "batch_invariant"]
    assert "key_bias" not in names and "ref_lens" not in names and "rows" not in names
    assert sig.parameters["weights"].default is None and sig.parameters["reduce"].default == "none"
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[5:])


# ---- pictures and the keep mask -------------------------------------------------------------------------------------------------
def test_received_maps_shapes_and_the_non_square_error():
    from instantrestore_amd.attn_maps import received_maps
    r = torch.arange(2 * 48 * 3, dtype=torch.float32).reshape(2, 48, 3)                  # self 16 + 2 references of 16
    m = received_maps(r, 16, 2, 16, True)
    assert m.shape == (2, 3, 4, 4, 3) and torch.equal(m[1, 2, 3, 1], r[1, 32 + 13]) and torch.equal(m[0, 0, 0, 0], r[0, 0])
    r4 = r[:, None].expand(2, 5, 48, 3)
    assert received_maps(r4, 16, 2, 16, True).shape == (2, 5, 3, 4, 4, 3)
    assert received_maps(r[:, :32], 7, 2, 16, False).shape == (2, 2, 4, 4, 3)            # the self length is not looked at without the self segment
    assert received_maps(r[:, :16], 16, 0, 0, True).shape == (2, 1, 4, 4, 3)
    for bad in ((r[:, :47], 15, 2, 16, True), (r[:, :40], 16, 2, 12, True)):
        with pytest.raises(ValueError, match="square"):
            received_maps(*bad)
    with pytest.raises(ValueError, match="different sides"):
        received_maps(torch.zeros(1, 16 + 2 * 4, 1), 16, 2, 4, True)
    with pytest.raises(ValueError, match="Lkv"):
        received_maps(r, 16, 3, 16, True)
    with pytest.raises(ValueError, match="empty"):
        received_maps(r, 16, 0, 16, False)


def test_keep_from_received_count_ties_and_reductions():
    from instantrestore_amd.attn_maps import keep_from_received
    B, N, Lr, Ls = 2, 3, 10, 4
    g = torch.Generator().manual_seed(0)
    recv = torch.rand(B, Ls + N * Lr, 1, generator=g)
    for frac in (0.05, 0.25, 0.3, 0.31, 0.5, 0.99, 1.0):
        keep = keep_from_received(recv, Ls, N, Lr, True, frac)
        want = min(Lr, max(1, math.ceil(frac * Lr - 1e-9)))
        assert keep.shape == (B, N, Lr) and keep.dtype == torch.bool
        assert bool((keep.sum(-1) == want).all()), frac                                   # the exact count per reference
        seg = recv[:, Ls:, 0].reshape(B, N, Lr)
        for b in range(B):
            for n in range(N):                                                            # every kept token received at least what every dropped one did
                if want < Lr:
                    assert float(seg[b, n][keep[b, n]].min()) >= float(seg[b, n][~keep[b, n]].max())
    assert bool(keep_from_received(recv, Ls, N, Lr, True, 1.0).all())
    assert keep_from_received(recv, Ls, N, Lr, True, 0.3)[0, 0].sum() == 3                 # 0.3 * 10 is 3, not 4 (the product rounds up in binary)
    # ties go to the lower token index
    tie = torch.tensor([1.0, 3.0, 3.0, 0.5, 3.0, 1.0, 1.0, 0.0]).reshape(1, 8, 1)
    assert keep_from_received(tie, 0, 1, 8, False, 0.25).tolist() == [[[False, True, True, False, False, False, False, False]]]
    assert keep_from_received(tie, 0, 1, 8, False, 0.5).tolist() == [[[True, True, True, False, True, False, False, False]]]
    assert keep_from_received(torch.zeros(1, 8, 1), 0, 2, 4, False, 0.5).tolist() == [[[True, True, False, False]] * 2]
    # several channels: channel 0 decides; heads: their mean decides
    two = torch.cat([tie, tie.flip(1)], dim=-1)
    assert torch.equal(keep_from_received(two, 0, 1, 8, False, 0.25), keep_from_received(tie, 0, 1, 8, False, 0.25))
    heads = torch.stack([tie, torch.zeros_like(tie)], dim=1)                               # (1, 2, 8, 1): the mean is tie / 2
    assert torch.equal(keep_from_received(heads, 0, 1, 8, False, 0.5), keep_from_received(tie, 0, 1, 8, False, 0.5))
    h2 = torch.zeros(1, 2, 8, 1)
    h2[0, 0, 1, 0], h2[0, 1, 6, 0] = 1.0, 4.0                                              # head 1 outweighs head 0 in the mean
    assert keep_from_received(h2, 0, 1, 8, False, 0.125)[0, 0].nonzero().flatten().tolist() == [6]
    # the self segment is skipped, not ranked
    withself = torch.cat([torch.full((1, 4, 1), 9.0), tie], dim=1)
    assert torch.equal(keep_from_received(withself, 4, 1, 8, True, 0.25), keep_from_received(tie, 0, 1, 8, False, 0.25))
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="keep_fraction"):
            keep_from_received(tie, 0, 1, 8, False, bad)
    with pytest.raises(ValueError, match="n_refs"):
        keep_from_received(tie, 8, 0, 0, True, 0.5)
    with pytest.raises(ValueError, match="Lkv"):
        keep_from_received(tie, 0, 1, 9, False, 0.5)


# ---- the oracle helper ----------------------------------------------------------------------------------------------------
def test_oracle_helper_against_a_brute_force_loop():
    import oracle_ops_received as R
    rng = np.random.default_rng(0)
    B, H, L, Lkv, Cn = 2, 3, 5, 7, 3
    p = rng.random((B, H, L, Lkv))
    for w in (rng.standard_normal((B, L, Cn)), rng.standard_normal((1, L, Cn)), rng.standard_normal((L, Cn)), rng.standard_normal((L,)),
              rng.standard_normal((B, L)), None):
        recv, recv_hm = R.received_np(p, w)
        wb = R.weights_np(w, B, L)
        Cw = wb.shape[-1]
        assert recv.shape == (B, H, Lkv, Cw) and recv_hm.shape == (B, Lkv, Cw)
        for b, h, j in np.ndindex(B, H, Lkv):
            acc = np.zeros(Cw)
            for i in range(L):
                acc += p[b, h, i, j] * wb[b, i]
            assert np.abs(recv[b, h, j] - acc).max() < 1e-12
        assert np.abs(recv_hm - recv.sum(axis=1) / H).max() < 1e-12
    assert np.abs(R.received_np(p)[0][..., 0] - p.sum(axis=2)).max() < 1e-12
    # the adjoint of the transfer: <w, P y> = <P^T w, y>
    import oracle_ops_transfer as T
    w, y = rng.standard_normal((B, L, 1)), rng.standard_normal((B, Lkv, 1))
    sums = T.transfer_np(p, y, [0, Lkv])[0]                                               # (B, H, L, 1, 1)
    lhs = np.einsum("bi,bhi->bh", w[..., 0], sums[..., 0, 0])
    rhs = np.einsum("bhj,bj->bh", R.received_np(p, w)[0][..., 0], y[..., 0])
    assert np.abs(lhs - rhs).max() < 1e-12


# ---- processor host logic on the stand-in -----------------------------------------------------------------------------------
@pytest.fixture()
def shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    import oracle_ops_received
    monkeypatch.setattr(ap, "_ops", oracle_ops_received)
    ap._BIAS_ROWS.clear()
    oracle_ops_received.CALLS.clear()
    return oracle_ops_received


def _layer(train_input=True):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    torch.manual_seed(3)
    B, H, L, N = 2, 2, 16, 3
    proc = SharedAttnProcessor(self_attn_idx=0, use_adain=True, train_input=train_input)
    attn = Attention(query_dim=H * 64, heads=H, dim_head=64, processor=proc)
    x = torch.randn(B, L, H * 64)
    rk, rv = torch.randn(B, N, L, H * 64), torch.randn(B, N, L, H * 64)
    run = lambda **kw: attn(x, ref_keys=[rk], ref_values=[rv], **kw)
    return proc, run, (B, H, L, N)


def test_processor_defaults_and_nothing_without_the_attribute(shim):
    from face_replace.models.attn_processors import SharedAttnProcessor
    p = SharedAttnProcessor()
    assert p.attention_received_weights is None and p.attention_received_reduce == "head_mean" and p.attention_received is None
    assert len(p.state_dict()) == 0
    assert list(inspect.signature(SharedAttnProcessor.__init__).parameters) == ["self", "self_attn_idx", "save_self_attentions", "use_adain", "train_input"]
    proc, run, _ = _layer()
    proc.attention_received_reduce = "none"                                   # the form alone switches nothing on
    with torch.no_grad():
        run()
    assert "attn_received" not in [c[0] for c in shim.CALLS] and proc.attention_received is None
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [False]


@pytest.mark.parametrize("train_input", [True, False])
def test_attribute_triggers_one_call_with_the_forwards_lse(shim, train_input):
    from instantrestore_amd.attn_maps import keep_from_received, received_maps
    proc, run, (B, H, L, N) = _layer(train_input)
    S = N + int(train_input)
    lkv = S * L
    with torch.no_grad():
        y_plain = run()
        shim.CALLS.clear()
        proc.attention_received_weights = "ones"
        y_ones = run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_received"]
    assert len(calls) == 1 and calls[0]["weights"] is None and calls[0]["reduce"] == "head_mean"      # "ones" goes down as no weights
    assert calls[0]["lse"] is shim.LAST_LSE[0] and shim.LAST_LSE[0] is not None                          # the LSE of the same forward
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [True]
    assert [c[0] for c in shim.CALLS].count("shared_attention") == 1 and "attn_probs" not in [c[0] for c in shim.CALLS]
    recv = proc.attention_received
    assert recv.shape == (B, lkv, 1) and recv.dtype == torch.float32
    assert float(recv.min()) > 0 and float((recv.sum(dim=(1, 2)) - L).abs().max()) < 1e-3              # every query token hands out 1
    assert received_maps(recv, L, N, L, train_input).shape == (B, S, 4, 4, 1)
    keep = keep_from_received(recv, L, N, L, train_input, 0.25)
    assert keep.shape == (B, N, L) and bool((keep.sum(-1) == 4).all())
    assert torch.equal(y_plain, y_ones)                                                                  # the layer output never depends on the option
    # a weight tensor goes through as it is; "none" gives the per-head shape
    shim.CALLS.clear()
    w = torch.rand(B, L, 3)
    proc.attention_received_weights, proc.attention_received_reduce = w, "none"
    with torch.no_grad():
        run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_received"]
    assert len(calls) == 1 and calls[0]["weights"] is w and calls[0]["reduce"] == "none"
    r2 = proc.attention_received
    assert r2.shape == (B, H, lkv, 3) and r2.dtype == torch.float32
    # beside the rows, match and transfer read-outs: one LSE serves all four
    shim.CALLS.clear()
    proc.attention_rows_index, proc.attention_match_index = torch.tensor([5, 0, 5]), "all"
    proc.attention_transfer_payload = torch.zeros(lkv, 2)
    with torch.no_grad():
        run()
    names = [c[0] for c in shim.CALLS]
    assert names.count("shared_attention") == 1 and all(names.count(n) == 1 for n in ("attn_rows", "attn_match", "attn_transfer", "attn_received"))
    proc.attention_received_weights = "every"
    shim.CALLS.clear()
    with torch.no_grad(), pytest.raises(ValueError, match="attention_received_weights"):
        run()
    assert not {"shared_attention", "attn_rows", "attn_match", "attn_transfer"} & {c[0] for c in shim.CALLS}   # refused before the attention and the other read-outs are launched


def test_a_layer_that_is_not_shared_ignores_the_attribute(shim):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    plain = SharedAttnProcessor(self_attn_idx=None)
    plain.attention_received_weights = "ones"
    with torch.no_grad():
        Attention(query_dim=64, heads=1, dim_head=64, processor=plain)(torch.randn(1, 4, 64))
    assert "attn_received" not in [c[0] for c in shim.CALLS] and plain.attention_received is None
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] in ([False], [])


def test_processor_raises_with_a_bias_or_counts(shim):
    proc, run, (B, H, L, N) = _layer()
    lkv = (N + 1) * L
    cases = {
        "mask": dict(attention_mask=torch.zeros(B, lkv)),
        "ref_weights": dict(ref_weights=torch.ones(B, N)),
        "ref_token_keep": dict(ref_token_keep=torch.ones(B, N, L, dtype=torch.bool)),
        "ref_lens": dict(ref_lens=[torch.full((B, N), L, dtype=torch.int32)], ref_stats=None),
    }
    for weights in ("ones", torch.zeros(L, 2)):
        proc.attention_received_weights = weights
        for name, kw in cases.items():
            shim.CALLS.clear()
            if name == "ref_lens":
                proc.use_adain = False           # (with use_adain the counts need ref_stats: an earlier, unrelated check)
            with torch.no_grad(), pytest.raises(NotImplementedError, match="attention_received_weights"):
                run(**kw)
            assert "shared_attention" not in [c[0] for c in shim.CALLS], name      # refused before anything is launched


# ---- the kernel file is built on the shared header -----------------------------------------------------------------------------
def test_kernel_takes_its_qk_block_from_the_readout_header():
    """attn_received.hip includes ir_readout.h, uses its pieces and defines none of them again; the probability expression and the
    key map stay in the header only (the rules of tests/test_readout_header_cpu.py for the other read-outs); the build lists the
    file in SRCS and on an MFMA-results-in-VGPRs line"""
    csrc = os.path.join(REPO, "instantrestore_amd", "csrc")
    text = open(os.path.join(csrc, "attn_received.hip")).read()
    assert re.search(r'#include\s+"ir_readout\.h"', text)
    for name in ("keymap", "key_segment", "load_q", "load_k", "scores", "prob"):
        assert re.search(r"\b%s\s*(<[^>]*>)?\(" % name, text), f"{name} is not used"
        assert not re.search(r"\b(int|void|float|hipError_t|f32x16|KeySeg<T>)\s+%s\s*\(" % name, text), f"{name} is defined again"
    assert "int keymap(" not in text
    assert not re.search(r"__builtin_fmaf\([^;]*scale_log2", text)
    assert "exp2" not in text.split('#include "ir_readout.h"')[1]                       # no exponential of its own
    assert "atomic" not in text.split('#include "ir_readout.h"')[1]
    build = open(os.path.join(csrc, "build.sh")).read()
    assert build.count("attn_received.hip") == 2                                        # SRCS and the MFMA-results-in-VGPRs line
    assert re.search(r'"\$s" == attn_received\.hip \]\] && extra\+=\(-mllvm -amdgpu-mfma-vgpr-form\)', build)


# ---- the build's register report -------------------------------------------------------------------------------------------
def test_kernels_report_no_spills_and_no_scratch():
    """every instantiation of attn_received_kernel in the remarks the build leaves behind: 0 spilled registers, 0 bytes of scratch
    (a wave at 4 or 8 channels holds 128 running sums per lane beside its operands; the head totals of the head-mean form live
    in LDS)"""
    paths = glob.glob(os.path.join(REPO, "instantrestore_amd", "csrc", "build", "attn_received.remarks")) + \
        glob.glob(os.path.join(REPO, "build", "attn_received.remarks"))
    assert paths, "attn_received.remarks is missing: run __graft_entry__.build()"
    text = open(paths[0], errors="replace").read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 16 and all("attn_received_kernel" in n for n in names), names   # 2 dtypes x 2 forms x 4 channel paddings
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", text)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    sgpr_spills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", text)]
    assert len(spills) == 16 and len(scratch) == 16
    assert not any(spills) and not any(scratch) and not any(sgpr_spills), (spills, scratch, sgpr_spills)
    assert "attn_received_kernel" in open(os.path.join(REPO, "tools", "check_resources.py")).read()


# ---- the example's switches ---------------------------------------------------------------------------------------------------
def test_example_refuses_prune_without_received(capsys):
    """--prune takes its tokens from the received attention: alone it is an argument error, not a switch that does nothing"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("synthetic_inference_prune", os.path.join(REPO, "examples", "synthetic_inference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit) as e:
        mod.main(["--prune", "0.5"])
    assert e.value.code == 2 and "--received" in capsys.readouterr().err
