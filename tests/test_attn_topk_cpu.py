"""The top-k read-out (``ir_attn_topk`` / ``ops.attn_topk`` / ``SharedAttnProcessor.attention_topk_index``): everything that can
be checked without a GPU - the symbol and its validation, the wrapper's checks, the ``attn_maps`` helpers, the processor's host
logic on the oracle-backed stand-in ``tests/oracle_ops_topk.py``, that helper itself against a stable sort and hand-made rows,
and the kernels' register report."""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_attn_match_cpu import _args, _copy_into

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
N_KERNELS = 36   # 2 element types x 3 row-block counts x 2 forms x 3 list capacities


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_bound_with_its_constant():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "ir_attn_topk") and "ir_attn_topk" in _lib.SYMBOLS
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION
    header = open(os.path.join(REPO, "include", "instantrestore_hip.h")).read()
    assert re.search(r"#define IR_TOPK_MAX 8\b", header) and _lib.IR_TOPK_MAX == 8
    assert re.search(r"#define IR_ABI_VERSION 10\b", header)
    assert re.search(r"int ir_attn_topk\(const ir_shared_attn_args\* args, const int32_t\* row_index, int32_t n_rows, int32_t k, int32_t reduce,\s*"
                     r"int32_t\* index, float\* prob, void\* stream\);", header)
    i32, vp = _lib.i32, _lib.vp
    assert _lib.SYMBOLS["ir_attn_topk"] == (C.c_int, [C.POINTER(_lib.SharedAttnArgs), vp, i32, i32, i32, vp, vp, vp])


def test_validation_names_the_reason_before_any_launch():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    off = lambda n: C.cast(C.c_void_p(ptr.value + n), C.c_void_p)
    call = lambda rows=ptr, n=4, k=4, red=0, index=ptr, prob=ptr, args=a: lib.ir_attn_topk(None if args is None else C.byref(args), rows, n, k, red, index,
                                                                                          prob, None)
    assert call(args=None) == INVALID and b"args" in err()
    assert call(rows=None) == INVALID and b"row_index" in err()
    assert call(index=None) == INVALID and b"index" in err()
    assert call(prob=None) == INVALID and b"prob" in err()
    a.lse = None
    assert call() == INVALID and b"lse" in err()
    a.lse = ptr
    assert call(rows=off(2)) == UNSUPPORTED and b"row_index" in err()
    assert call(index=off(2)) == UNSUPPORTED and b"index" in err() and b"row_index" not in err()
    assert call(prob=off(1)) == UNSUPPORTED and b"prob" in err()
    assert call(n=0) == INVALID and b"n_rows" in err()
    assert call(n=65) == INVALID and b"n_rows" in err() and b"len_q" in err()
    for bad in (0, -1, 9, 1 << 20):
        assert call(k=bad) == UNSUPPORTED and b"k " in err() and b"IR_TOPK_MAX" in err(), bad
    for bad in (-1, 2):
        assert call(red=bad) == UNSUPPORTED and b"reduce" in err()
    a.tuning = 13
    assert call() == UNSUPPORTED and b"tuning" in err() and b"ir_attn_topk" in err()
    a.tuning = 0
    a.struct_size = 7
    assert call() == INVALID and b"ABI mismatch" in err()


def test_more_work_items_than_attn_match_accepts_are_refused():
    """2^31 - 4 items at the most, as for ir_attn_match: a call of 3 * 2^30 items is refused by both, with the same reason, before
    any launch (the pointers are fake)"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    # 1 row group x 3 segments x 8 heads x B: B = 2^27 gives 3 * 2^30 items
    a.heads, a.batch = 8, 1 << 27
    a.q_sh = a.ks_sh = a.vs_sh = a.kr_sh = a.vr_sh = 64
    a.q_sl = a.ks_sl = a.vs_sl = a.kr_sl = a.vr_sl = 8 * 64
    a.q_sb = a.ks_sb = a.vs_sb = 64 * 8 * 64
    a.kr_sn = a.vr_sn = 64 * 8 * 64
    a.kr_sb = a.vr_sb = 2 * 64 * 8 * 64
    rc_match = lib.ir_attn_match(C.byref(a), ptr, 4, 0, ptr, ptr, None)
    msg_match = err()
    assert rc_match == UNSUPPORTED and b"grid too large" in msg_match
    assert lib.ir_attn_topk(C.byref(a), ptr, 4, 4, 0, ptr, ptr, None) == UNSUPPORTED and b"grid too large" in err()


def test_bias_and_ragged_blocks_are_refused_and_the_messages_name_the_entry_point():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    bias = _copy_into(_lib.SharedAttnBiasArgs(), a)
    bias.key_bias = ptr
    assert lib.ir_attn_topk(C.byref(bias), ptr, 4, 4, 0, ptr, ptr, None) == UNSUPPORTED
    assert b"key_bias" in err() and b"do not take a key bias" in err() and b"ir_attn_topk" in err()
    ragged = _copy_into(_lib.SharedAttnRaggedArgs(), a)
    ragged.ref_lens, ragged.rl_sb = ptr, 2
    assert lib.ir_attn_topk(C.byref(ragged), ptr, 4, 2, 1, ptr, ptr, None) == UNSUPPORTED
    assert b"ref_lens" in err() and b"walk the tails" in err() and b"ir_attn_topk" in err()
    for name in (b"ir_attn_match", b"ir_attn_transfer", b"ir_attn_received"):          # the shared messages keep their other names
        assert name in err()


# ---- ops ------------------------------------------------------------------------------------------------------------------
def test_ops_attn_topk_checks_k_first_and_has_no_cpu_path():
    from instantrestore_amd import ops
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    lse = torch.zeros(1, 1, 8)
    for bad in (0, 9, 2.5, -1, None, True):
        with pytest.raises(ValueError, match="k must be"):
            ops.attn_topk("not even a tensor", None, None, None, k=bad, heads=1, scale=0.125)       # before anything else is touched
    with pytest.raises(ValueError, match="reduce"):
        ops.attn_topk(q, q, None, lse, k=2, heads=1, scale=0.125, reduce="map")
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_topk(q, q, None, lse, k=2, heads=1, scale=0.125)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_topk(q, q, None, lse, torch.tensor([0]), k=8, heads=1, scale=0.125, reduce="head_mean")
    src = inspect.getsource(ops.attn_topk)
    assert "_row_index(rows, B, Lq, q.device)" in src and "_probs_args(" in src and "one_kernel=True" in src
    # (the one-kernel decision is _probs_args' argument: there the forward's A/B hook is switched off)
    assert re.search(r"if one_kernel:\n\s+args\.tuning = 0\n", inspect.getsource(ops._probs_args))


def test_ops_signature_has_no_bias_and_no_counts():
    from instantrestore_amd import ops
    sig = inspect.signature(ops.attn_topk)
    names = list(sig.parameters)
    assert names == ["q", "k_self", "ref_k", "lse", "rows", "k", "heads", "scale", "include_self", "reduce", "q_prescaled", "batch_invariant"]
    assert "key_bias" not in names and "ref_lens" not in names
    assert sig.parameters["rows"].default is None and sig.parameters["reduce"].default == "none"
    assert sig.parameters["k"].default is inspect.Parameter.empty
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[5:])


# ---- the oracle helper ----------------------------------------------------------------------------------------------------
def test_oracle_helper_against_a_stable_sort():
    import oracle_ops_topk as M
    rng = np.random.default_rng(0)
    B, H, R, Ls, N, Lr = 2, 3, 4, 5, 2, 7
    edges = M.segment_edges(Ls, N, Lr, True)
    p = rng.integers(0, 4, size=(B, H, R, edges[-1])).astype(np.float64) / 8           # few distinct values: ties everywhere
    for head_mean in (False, True):
        x = p.mean(axis=1) if head_mean else p
        lead = x.shape[:-1]
        for k in (1, 3, 6, 8):
            vals, keys = M.topk_np(p, edges, k, head_mean)
            assert vals.shape == lead + (3, k) and keys.shape == lead + (3, k) and vals.dtype == np.float64
            for pos in np.ndindex(*lead):
                for s, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                    seg = x[pos][a:b]
                    order = sorted(range(b - a), key=lambda j: (-seg[j], j))[:k]       # (value descending, key ascending)
                    n = len(order)
                    assert keys[pos + (s,)][:n].tolist() == order and np.array_equal(vals[pos + (s,)][:n], seg[order])
                    assert (keys[pos + (s,)][n:] == -1).all() and (vals[pos + (s,)][n:] == 0).all()
    # rank 0 is the match helper
    best, first, _ = M.match_np(p, edges, False)
    vals, keys = M.topk_np(p, edges, 2, False)
    assert np.array_equal(vals[..., 0], best) and np.array_equal(keys[..., 0], first)


def test_oracle_helper_on_hand_made_rows():
    import oracle_ops_topk as M
    row = np.array([0.1, 0.4, 0.4, 0.0,   0.3, 0.3,   0.2], dtype=np.float64).reshape(1, 1, 1, 7)
    vals, keys = M.topk_np(row, [0, 4, 6, 7], 3, False)
    assert keys[0, 0, 0].tolist() == [[1, 2, 0], [0, 1, -1], [0, -1, -1]]
    assert vals[0, 0, 0].tolist() == [[0.4, 0.4, 0.1], [0.3, 0.3, 0.0], [0.2, 0.0, 0.0]]
    two = np.concatenate([row, row[..., ::-1]], axis=1)                               # two heads: the mean ties in another way
    vals, keys = M.topk_np(two, [0, 7], 4, True)
    mean = two.mean(axis=1)[0, 0]
    assert keys[0, 0, 0].tolist() == sorted(range(7), key=lambda j: (-mean[j], j))[:4] and vals.shape == (1, 1, 1, 4)


# ---- attn_maps helpers ------------------------------------------------------------------------------------------------------
def test_topk_coordinates_keep_minus_one():
    from instantrestore_amd.attn_maps import match_coordinates, topk_coordinates
    index = np.array([[[[0, 5], [15, -1]]]], dtype=np.int32)                          # (B 1, R 1, S 2, k 2)
    y, x = topk_coordinates(index, 4)
    assert np.array_equal(y, [[[[0, 1], [3, -1]]]]) and np.array_equal(x, [[[[0, 1], [3, -1]]]])
    ty, tx = topk_coordinates(torch.from_numpy(index), 4)
    assert ty.dtype == torch.int64 and torch.equal(ty, torch.from_numpy(y)) and torch.equal(tx, torch.from_numpy(x))
    my, mx = match_coordinates(index[..., 0], 4)
    assert np.array_equal(my, y[..., 0]) and np.array_equal(mx, x[..., 0])          # rank 0: the match helper


def test_match_ambiguity_ends_and_its_k_error():
    from instantrestore_amd.attn_maps import match_ambiguity
    prob = np.array([[0.5, 0.5, 0.1], [0.8, 0.0, 0.0], [0.0, 0.0, 0.0], [0.4, 0.1, 0.1]], dtype=np.float32)
    want = np.array([1.0, 0.0, 0.0, 0.25], dtype=np.float32)
    got = match_ambiguity(prob)
    assert np.array_equal(got, want)
    tgot = match_ambiguity(torch.from_numpy(prob))
    assert torch.equal(tgot, torch.from_numpy(want)) and tgot.dtype == torch.float32
    for one in (prob[:, :1], torch.from_numpy(prob[:, :1])):
        with pytest.raises(ValueError, match="k >= 2"):
            match_ambiguity(one)


def test_topk_coverage_at_mass_zero_and_clamped():
    from instantrestore_amd.attn_maps import topk_coverage
    prob = np.array([[[0.25, 0.25], [0.0, 0.0], [0.5, 0.25], [0.125, 0.0]]], dtype=np.float32)   # (R 1, S 4, k 2)
    mass = np.array([[1.0, 0.0, 0.5, 0.5]], dtype=np.float32)
    want = np.array([[0.5, 0.0, 1.0, 0.25]], dtype=np.float32)                        # 0 at mass 0; 1.5 clamped to 1
    assert np.array_equal(topk_coverage(prob, mass), want)
    assert torch.equal(topk_coverage(torch.from_numpy(prob), torch.from_numpy(mass)), torch.from_numpy(want))
    with pytest.raises(ValueError, match="mass"):
        topk_coverage(prob, mass[:, :3])


def test_keep_from_topk_on_a_hand_made_index():
    from instantrestore_amd.attn_maps import keep_from_topk
    # (B 1, H 2, R 2, S 3 = self + 2 references, k 2), len_ref 6.  The self segment's entries (5, 4, ...) never count
    index = np.array([[[[[5, 4], [0, 3], [2, -1]],
                        [[5, 4], [0, 1], [-1, -1]]],
                       [[[5, 4], [5, 0], [2, 2]],
                        [[5, 4], [0, 0], [4, -1]]]]], dtype=np.int32)
    prob = np.array([[[[[.9, .9], [.5, .2], [.6, 0.]],
                       [[.9, .9], [.4, .3], [0., 0.]]],
                      [[[.9, .9], [.1, .7], [.3, .3]],
                       [[.9, .9], [.2, .2], [.05, 0.]]]]], dtype=np.float32)
    want = np.array([[[1, 1, 0, 1, 0, 1], [0, 0, 1, 0, 1, 0]]], dtype=bool)            # the union over rows, heads and ranks
    want_min = np.array([[[1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0]]], dtype=bool)        # prob >= 0.4 only
    for conv in (lambda x: x, torch.from_numpy):
        keep = keep_from_topk(conv(index), 2, 6, True)
        assert tuple(keep.shape) == (1, 2, 6) and np.array_equal(np.asarray(keep), want)
        assert np.array_equal(np.asarray(keep_from_topk(conv(index), 2, 6, True, min_prob=0.4, prob=conv(prob))), want_min)
        # one head alone, the head-mean shape (B, R, S, k)
        assert np.array_equal(np.asarray(keep_from_topk(conv(index[:, 0]), 2, 6, True)), [[[1, 1, 0, 1, 0, 0], [0, 0, 1, 0, 0, 0]]])
        # without a self segment the first segment is reference 0
        assert np.array_equal(np.asarray(keep_from_topk(conv(index[:, 0, :, 1:]), 2, 6, False)), [[[1, 1, 0, 1, 0, 0], [0, 0, 1, 0, 0, 0]]])
    assert keep_from_topk(torch.from_numpy(index), 2, 6, True).dtype == torch.bool
    with pytest.raises(ValueError, match="go together"):
        keep_from_topk(index, 2, 6, True, min_prob=0.5)
    with pytest.raises(ValueError, match="S = 2"):
        keep_from_topk(index, 2, 6, False)


# ---- processor host logic on the stand-in -----------------------------------------------------------------------------------
@pytest.fixture()
def shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    import oracle_ops_topk
    monkeypatch.setattr(ap, "_ops", oracle_ops_topk)
    ap._BIAS_ROWS.clear()
    oracle_ops_topk.CALLS.clear()
    return oracle_ops_topk


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
    assert p.attention_topk_index is None and p.attention_topk_k == 4 and p.attention_topk_reduce == "head_mean" and p.attention_topk is None
    assert len(p.state_dict()) == 0
    proc, run, _ = _layer()
    with torch.no_grad():
        run()
    assert "attn_topk" not in [c[0] for c in shim.CALLS] and proc.attention_topk is None
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [False]


@pytest.mark.parametrize("train_input", [True, False])
def test_attribute_triggers_one_call_with_the_forwards_lse(shim, train_input):
    proc, run, (B, H, L, N) = _layer(train_input)
    S = N + int(train_input)
    with torch.no_grad():
        y_plain = run()
        shim.CALLS.clear()
        proc.attention_topk_index = "all"
        y_all = run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_topk"]
    assert len(calls) == 1 and calls[0]["rows"] is None and calls[0]["reduce"] == "head_mean" and calls[0]["k"] == 4
    assert calls[0]["lse"] is shim.LAST_LSE[0] and shim.LAST_LSE[0] is not None          # the LSE of the same forward
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [True]
    assert [c[0] for c in shim.CALLS].count("shared_attention") == 1 and "attn_probs" not in [c[0] for c in shim.CALLS]
    index, prob = proc.attention_topk
    assert index.shape == (B, L, S, 4) and index.dtype == torch.int32 and prob.shape == (B, L, S, 4) and prob.dtype == torch.float32
    assert int(index.min()) >= 0 and int(index.max()) < L and bool((prob[..., :-1] >= prob[..., 1:]).all())
    assert torch.equal(y_plain, y_all)                                                    # the layer output never depends on the option
    # a row tensor goes through as it is; "none" gives the per-head shape; k follows the attribute
    shim.CALLS.clear()
    rows = torch.tensor([5, 0, 5])
    proc.attention_topk_index, proc.attention_topk_reduce, proc.attention_topk_k = rows, "none", 2
    with torch.no_grad():
        run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_topk"]
    assert len(calls) == 1 and calls[0]["rows"] is rows and calls[0]["reduce"] == "none" and calls[0]["k"] == 2
    i2, p2 = proc.attention_topk
    assert i2.shape == (B, H, 3, S, 2) and torch.equal(i2[:, :, 0], i2[:, :, 2]) and torch.equal(p2[:, :, 0], p2[:, :, 2])
    # beside the rows and the match read-outs: one forward call, one LSE, and rank 0 is the match
    shim.CALLS.clear()
    proc.attention_rows_index = rows
    proc.attention_match_index, proc.attention_match_reduce = rows, "none"
    with torch.no_grad():
        run()
    names = [c[0] for c in shim.CALLS]
    assert names.count("shared_attention") == 1 and names.count("attn_rows") == 1 and names.count("attn_match") == 1 and names.count("attn_topk") == 1
    lses = [c[1]["lse"] for c in shim.CALLS if c[0] in ("attn_match", "attn_topk")]
    assert all(x is shim.LAST_LSE[0] for x in lses)
    mi, mp = proc.attention_match
    ti, tp = proc.attention_topk
    assert torch.equal(ti[..., 0], mi) and torch.equal(tp[..., 0], mp)


def test_bad_attribute_values_raise(shim):
    proc, run, _ = _layer()
    proc.attention_topk_index = "every"
    with torch.no_grad(), pytest.raises(ValueError, match="attention_topk_index"):
        run()
    assert "shared_attention" not in [c[0] for c in shim.CALLS]                           # before anything is launched
    proc.attention_topk_index = "all"
    for bad in (0, 9, 2.5):
        proc.attention_topk_k = bad
        with torch.no_grad(), pytest.raises(ValueError, match="k must be"):
            run()
    proc.attention_topk_k, proc.attention_topk_reduce = 4, "map"
    with torch.no_grad(), pytest.raises(ValueError, match="reduce"):
        run()


def test_a_layer_that_is_not_shared_ignores_the_attribute(shim):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    plain = SharedAttnProcessor(self_attn_idx=None)
    plain.attention_topk_index = "all"
    with torch.no_grad():
        Attention(query_dim=64, heads=1, dim_head=64, processor=plain)(torch.randn(1, 4, 64))
    assert "attn_topk" not in [c[0] for c in shim.CALLS] and plain.attention_topk is None


def test_processor_raises_with_a_bias_or_counts(shim):
    proc, run, (B, H, L, N) = _layer()
    proc.attention_topk_index = "all"
    lkv = (N + 1) * L
    cases = {
        "mask": dict(attention_mask=torch.zeros(B, lkv)),
        "ref_weights": dict(ref_weights=torch.ones(B, N)),
        "ref_token_keep": dict(ref_token_keep=torch.ones(B, N, L, dtype=torch.bool)),
        "ref_lens": dict(ref_lens=[torch.full((B, N), L, dtype=torch.int32)], ref_stats=None),
    }
    for name, kw in cases.items():
        shim.CALLS.clear()
        if name == "ref_lens":
            proc.use_adain = False           # (with use_adain the counts need ref_stats: an earlier, unrelated check)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="attention_topk_index.*ir_attn_topk"):
            run(**kw)
        assert "shared_attention" not in [c[0] for c in shim.CALLS], name      # refused before anything is launched


def test_the_real_ops_is_passed_the_batch_invariant_keyword():
    """the processor hands the mode's keyword through, as it does for the match read-out, and only when the mode is on"""
    import processor_trace
    import instantrestore_amd.attn_processors as ap
    for mode in (True, False):
        case = dict(own=True, attrs=dict(batch_invariant=mode, attention_topk_index="all", attention_match_index="all",
                                         save_self_attentions=True))
        calls = {c[0]: c[2] for c in processor_trace.run_case(ap, case)["calls"]}
        for name in ("shared_attention", "attn_match", "attn_topk", "attn_probs"):
            assert calls[name].get("batch_invariant") is (True if mode else None), (mode, name)


# ---- the build's register report -------------------------------------------------------------------------------------------
def test_kernels_report_no_spills_and_no_scratch():
    """every instantiation of attn_topk_kernel in the remarks the build leaves behind: 0 spilled registers, 0 bytes of scratch
    (a wave of the head-mean form holds 192 fp32 sums and three sorted lists of up to 8 pairs per lane)"""
    paths = glob.glob(os.path.join(REPO, "instantrestore_amd", "csrc", "build", "attn_topk.remarks")) + \
        glob.glob(os.path.join(REPO, "build", "attn_topk.remarks"))
    assert paths, "attn_topk.remarks is missing: run __graft_entry__.build()"
    text = open(paths[0], errors="replace").read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == N_KERNELS and all("attn_topk_kernel" in n for n in names), names
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", text)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    sgpr_spills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", text)]
    assert len(spills) == N_KERNELS and len(scratch) == N_KERNELS
    assert not any(spills) and not any(scratch) and not any(sgpr_spills), (spills, scratch, sgpr_spills)
    assert "attn_topk_kernel" in open(os.path.join(REPO, "tools", "check_resources.py")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert re.search(r"= %d instantiations of `attn_topk_kernel`" % N_KERNELS, design)


def test_the_kernel_takes_its_qk_block_from_the_shared_header():
    text = open(os.path.join(REPO, "instantrestore_amd", "csrc", "attn_topk.hip")).read()
    assert re.search(r'#include\s+"ir_readout\.h"', text)
    assert "int keymap(" not in text and not re.search(r"__builtin_fmaf\([^;]*scale_log2", text)
    for name in ("keymap(", "key_segment<", "load_q<", "load_k(", "scores<", "prob(", "gather_rows<", "rows_ngroups(", "dispatch_rows("):
        assert name in text, name
    assert "__shared__" not in text and "__syncthreads" not in text and "atomic" not in text.split("#include")[1]
