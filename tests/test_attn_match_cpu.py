"""The best-match read-out (``ir_attn_match`` / ``ops.attn_match`` / ``SharedAttnProcessor.attention_match_index``): everything
that can be checked without a GPU - the symbol and its validation, the wrapper's checks, the coordinate helpers, the
processor's host logic on the oracle-backed stand-in ``tests/oracle_ops_match.py``, that helper itself against a brute-force
loop, and the kernels' register report."""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def _args(lib_mod):
    """a valid self + two-reference call on host pointers that are never dereferenced (validation precedes any launch)"""
    a = lib_mod.SharedAttnArgs()
    a.struct_size = C.sizeof(a)
    a.dtype, a.batch, a.heads, a.len_q, a.len_self, a.flags, a.scale = 1, 1, 1, 64, 64, 1, 0.125
    buf = (C.c_char * 65536)()
    ptr = C.cast(C.byref(buf, 64 - C.addressof(buf) % 64), C.c_void_p)
    a.q = a.k_self = a.v_self = a.lse = ptr
    a.q_sb = a.ks_sb = a.vs_sb = 64 * 64
    a.q_sl = a.ks_sl = a.vs_sl = 64
    a.q_sh = a.ks_sh = a.vs_sh = 64
    a.n_refs, a.len_ref = 2, 64
    a.k_ref = a.v_ref = ptr
    a.kr_sb = a.vr_sb = 2 * 64 * 64
    a.kr_sn = a.vr_sn = 64 * 64
    a.kr_sl = a.vr_sl = 64
    a.kr_sh = a.vr_sh = 64
    return a, ptr, buf


def test_symbol_is_exported_and_bound_with_its_constants():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "ir_attn_match") and "ir_attn_match" in _lib.SYMBOLS
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION
    header = open(os.path.join(REPO, "include", "instantrestore_hip.h")).read()
    for name, val in (("IR_MATCH_PER_HEAD", 0), ("IR_MATCH_HEAD_MEAN", 1)):
        assert re.search(r"#define %s %d\b" % (name, val), header), name
    assert (_lib.IR_MATCH_PER_HEAD, _lib.IR_MATCH_HEAD_MEAN) == (0, 1)
    assert re.search(r"int ir_attn_match\(const ir_shared_attn_args\* args, const int32_t\* row_index, int32_t n_rows, int32_t reduce, "
                     r"int32_t\* index, float\* prob,\s*void\* stream\);", header)


def test_validation_names_the_field_before_any_launch():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    off = lambda n: C.cast(C.c_void_p(ptr.value + n), C.c_void_p)
    call = lambda rows=ptr, n=4, red=0, index=ptr, prob=ptr, args=a: lib.ir_attn_match(None if args is None else C.byref(args), rows, n, red, index, prob, None)
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
    for bad in (-1, 2):
        assert call(red=bad) == UNSUPPORTED and b"reduce" in err()
    a.tuning = 13
    assert call() == UNSUPPORTED and b"tuning" in err()
    a.tuning = 0
    a.struct_size = 7
    assert call() == INVALID and b"ABI mismatch" in err()


def _copy_into(dst, src):
    for name, _ in type(src)._fields_:
        setattr(dst, name, getattr(src, name))
    dst.struct_size = C.sizeof(dst)
    return dst


def test_bias_and_ragged_blocks_are_refused_like_the_other_readouts():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    bias = _copy_into(_lib.SharedAttnBiasArgs(), a)
    bias.key_bias = ptr
    assert lib.ir_attn_match(C.byref(bias), ptr, 4, 0, ptr, ptr, None) == UNSUPPORTED and b"key_bias" in err()
    ragged = _copy_into(_lib.SharedAttnRaggedArgs(), a)
    ragged.ref_lens, ragged.rl_sb = ptr, 2
    assert lib.ir_attn_match(C.byref(ragged), ptr, 4, 1, ptr, ptr, None) == UNSUPPORTED and b"ref_lens" in err()


# ---- ops ------------------------------------------------------------------------------------------------------------------
def test_ops_attn_match_has_no_cpu_path_and_checks_its_arguments():
    from instantrestore_amd import ops
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    lse = torch.zeros(1, 1, 8)
    with pytest.raises(ValueError, match="reduce"):
        ops.attn_match(q, q, None, lse, heads=1, scale=0.125, reduce="map")
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_match(q, q, None, lse, heads=1, scale=0.125)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_match(q, q, None, lse, torch.tensor([0]), heads=1, scale=0.125, reduce="head_mean")
    assert ops.MATCH_REDUCE == {"none": 0, "head_mean": 1}
    # `rows` goes through _row_index, as in attn_rows: tests/test_attn_rows_cpu.py holds its checks; here that attn_match uses it
    src = inspect.getsource(ops.attn_match)
    assert "_row_index(rows, B, Lq, q.device)" in src
    for bad in ([-1, 2], [0, 8]):
        with pytest.raises(ValueError, match="indices"):
            ops._row_index(torch.tensor(bad), 1, 8, torch.device("cpu"))
    with pytest.raises(ValueError):
        ops._row_index(torch.zeros(9, dtype=torch.int64), 1, 8, torch.device("cpu"))


def test_ops_signature_has_no_bias_and_no_counts():
    from instantrestore_amd import ops
    sig = inspect.signature(ops.attn_match)
    names = list(sig.parameters)
    assert names == ["q", "k_self", "ref_k", "lse", "rows", "heads", "scale", "include_self", "reduce", "q_prescaled", "batch_invariant"]
    assert "key_bias" not in names and "ref_lens" not in names
    assert sig.parameters["rows"].default is None and sig.parameters["reduce"].default == "none"
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[5:])


# ---- coordinate helpers ---------------------------------------------------------------------------------------------------
def test_match_coordinates_and_field_on_hand_made_indices():
    from instantrestore_amd.attn_maps import match_coordinates, match_field
    side = 4
    index = np.array([[[0, 5, -1], [15, 3, 14]]], dtype=np.int32)          # (B = 1, R = 2, S = 3)
    y, x = match_coordinates(index, side)
    assert np.array_equal(y, [[[0, 1, -1], [3, 0, 3]]]) and np.array_equal(x, [[[0, 1, -1], [3, 3, 2]]])
    rows = np.array([1, 6])                                                 # tokens (0, 1) and (1, 2)
    dy, dx = match_field(index, rows, side)
    assert np.array_equal(dy, [[[0, 1, 0], [2, -1, 2]]]) and np.array_equal(dx, [[[-1, 0, 0], [1, 1, 0]]])
    # the same on torch tensors, with a (B, R) row list against a per-head (B, H, R, S) index
    ti = torch.from_numpy(index)[:, None].expand(1, 2, 2, 3)
    ty, tx = match_coordinates(ti, side)
    assert ty.dtype == torch.int64 and torch.equal(ty[0, 1], torch.from_numpy(y[0])) and torch.equal(tx[0, 0], torch.from_numpy(x[0]))
    tdy, tdx = match_field(ti, torch.tensor([[1, 6]]), side)
    assert tdy.shape == (1, 2, 2, 3) and torch.equal(tdy[0, 1], torch.from_numpy(dy[0])) and torch.equal(tdx[0, 0], torch.from_numpy(dx[0]))
    # every token ("all" / None): row r is token r; an out-of-range row (-1) has no displacement
    full = torch.arange(16, dtype=torch.int32).flip(0).reshape(1, 16, 1)
    ay, ax = match_field(full, None, side)
    assert torch.equal(ay[0, :, 0], 3 - 2 * (torch.arange(16) // 4)) and torch.equal(ax[0, :, 0], 3 - 2 * (torch.arange(16) % 4))
    by, bx = match_field(index, np.array([-1, 6]), side)
    assert np.array_equal(by[0, 0], [0, 0, 0]) and np.array_equal(bx[0, 0], [0, 0, 0]) and np.array_equal(by[0, 1], dy[0, 1])


# ---- the oracle helper ----------------------------------------------------------------------------------------------------
def test_oracle_helper_against_a_brute_force_loop():
    import oracle_ops_match as M
    rng = np.random.default_rng(0)
    B, H, R, Ls, N, Lr = 2, 3, 4, 5, 2, 7
    edges = M.segment_edges(Ls, N, Lr, True)
    assert edges == [0, 5, 12, 19] and M.segment_edges(Ls, N, Lr, False) == [0, 7, 14] and M.segment_edges(Ls, 0, 0, True) == [0, 5]
    p = rng.integers(0, 4, size=(B, H, R, edges[-1])).astype(np.float64) / 8           # few distinct values: ties everywhere
    for head_mean in (False, True):
        best, first, sets = M.match_np(p, edges, head_mean)
        x = p.mean(axis=1) if head_mean else p
        lead = x.shape[:-1]
        assert best.shape == lead + (3,) and first.shape == lead + (3,) and [s.shape for s in sets] == [lead + (5,), lead + (7,), lead + (7,)]
        for pos in np.ndindex(*lead):
            for s, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                m, where = -1.0, []
                for j in range(a, b):
                    v = x[pos + (j,)]
                    if v > m:
                        m, where = v, [j - a]
                    elif v == m:
                        where.append(j - a)
                assert best[pos + (s,)] == m and first[pos + (s,)] == where[0]
                assert np.flatnonzero(sets[s][pos]).tolist() == where
    g = M.gather_rows(rng.standard_normal((2, 1, 6, 3)), np.array([[5, 5], [0, 2]]))
    assert g.shape == (2, 1, 2, 3) and np.array_equal(g[0, 0, 0], g[0, 0, 1])


# ---- processor host logic on the stand-in -----------------------------------------------------------------------------------
@pytest.fixture()
def shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    import oracle_ops_match
    monkeypatch.setattr(ap, "_ops", oracle_ops_match)
    ap._BIAS_ROWS.clear()
    oracle_ops_match.CALLS.clear()
    return oracle_ops_match


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
    assert p.attention_match_index is None and p.attention_match_reduce == "head_mean" and p.attention_match is None
    assert len(p.state_dict()) == 0
    assert list(inspect.signature(SharedAttnProcessor.__init__).parameters) == ["self", "self_attn_idx", "save_self_attentions", "use_adain", "train_input"]
    proc, run, _ = _layer()
    with torch.no_grad():
        run()
    assert "attn_match" not in [c[0] for c in shim.CALLS] and proc.attention_match is None
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [False]


@pytest.mark.parametrize("train_input", [True, False])
def test_attribute_triggers_one_call_with_the_forwards_lse(shim, train_input):
    proc, run, (B, H, L, N) = _layer(train_input)
    S = N + int(train_input)
    with torch.no_grad():
        y_plain = run()
        shim.CALLS.clear()
        proc.attention_match_index = "all"
        y_all = run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_match"]
    assert len(calls) == 1 and calls[0]["rows"] is None and calls[0]["reduce"] == "head_mean"
    assert calls[0]["lse"] is shim.LAST_LSE[0] and shim.LAST_LSE[0] is not None          # the LSE of the same forward
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [True]
    assert [c[0] for c in shim.CALLS].count("shared_attention") == 1 and "attn_probs" not in [c[0] for c in shim.CALLS]
    index, prob = proc.attention_match
    assert index.shape == (B, L, S) and index.dtype == torch.int32 and prob.shape == (B, L, S) and prob.dtype == torch.float32
    assert int(index.min()) >= 0 and int(index.max()) < L and float(prob.min()) > 0 and float(prob.sum(-1).max()) <= 1.0
    assert torch.equal(y_plain, y_all)                                                    # the layer output never depends on the option
    # a row tensor goes through as it is; "none" gives the per-head shape
    shim.CALLS.clear()
    rows = torch.tensor([5, 0, 5])
    proc.attention_match_index, proc.attention_match_reduce = rows, "none"
    with torch.no_grad():
        run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_match"]
    assert len(calls) == 1 and calls[0]["rows"] is rows and calls[0]["reduce"] == "none"
    i2, p2 = proc.attention_match
    assert i2.shape == (B, H, 3, S) and torch.equal(i2[:, :, 0], i2[:, :, 2]) and torch.equal(p2[:, :, 0], p2[:, :, 2])
    # beside the rows read-out: one LSE serves both
    shim.CALLS.clear()
    proc.attention_rows_index = rows
    with torch.no_grad():
        run()
    names = [c[0] for c in shim.CALLS]
    assert names.count("shared_attention") == 1 and names.count("attn_rows") == 1 and names.count("attn_match") == 1
    proc.attention_match_index = "every"
    with torch.no_grad(), pytest.raises(ValueError, match="attention_match_index"):
        run()


def test_a_layer_that_is_not_shared_ignores_the_attribute(shim):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    plain = SharedAttnProcessor(self_attn_idx=None)
    plain.attention_match_index = "all"
    with torch.no_grad():
        Attention(query_dim=64, heads=1, dim_head=64, processor=plain)(torch.randn(1, 4, 64))
    assert "attn_match" not in [c[0] for c in shim.CALLS] and plain.attention_match is None


def test_processor_raises_with_a_bias_or_counts(shim):
    proc, run, (B, H, L, N) = _layer()
    proc.attention_match_index = "all"
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
        with torch.no_grad(), pytest.raises(NotImplementedError, match="attention_match_index"):
            run(**kw)
        assert "shared_attention" not in [c[0] for c in shim.CALLS], name      # refused before anything is launched


# ---- the build's register report -------------------------------------------------------------------------------------------
def test_kernels_report_no_spills_and_no_scratch():
    """every instantiation of attn_match_kernel in the remarks the build leaves behind: 0 spilled registers, 0 bytes of scratch
    (a wave of the head-mean form holds 192 fp32 sums per lane over its head walk)"""
    paths = glob.glob(os.path.join(REPO, "instantrestore_amd", "csrc", "build", "attn_match.remarks")) + \
        glob.glob(os.path.join(REPO, "build", "attn_match.remarks"))
    assert paths, "attn_match.remarks is missing: run __graft_entry__.build()"
    text = open(paths[0], errors="replace").read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 12 and all("attn_match_kernel" in n for n in names), names      # 2 dtypes x 3 row-block counts x 2 forms
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", text)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    sgpr_spills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", text)]
    assert len(spills) == 12 and len(scratch) == 12
    assert not any(spills) and not any(scratch) and not any(sgpr_spills), (spills, scratch, sgpr_spills)
    sys_path = os.path.join(REPO, "tools", "check_resources.py")
    assert "attn_match_kernel" in open(sys_path).read()
