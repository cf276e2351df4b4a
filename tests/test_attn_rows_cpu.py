"""Attention rows of chosen query tokens (``ir_attn_rows`` / ``ops.attn_rows`` / ``SharedAttnProcessor.attention_rows_index``):
everything that can be checked without a GPU - the symbol and its validation, the processor's host logic on the oracle-backed
stand-in ``tests/oracle_ops_rows.py``, the landmark helpers and the kernels' register report."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_symbol_is_exported_and_the_abi_is_unchanged():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "ir_attn_rows") and "ir_attn_rows" in _lib.SYMBOLS
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION
    assert C.sizeof(_lib.SharedAttnArgs) == 10 * 4 + 9 * 8 + 20 * 8 + 16 + 8 + 8 + 8
    header = open(os.path.join(REPO, "include", "instantrestore_hip.h")).read()
    for name, val in (("IR_ROWS_NONE", 0), ("IR_ROWS_HEAD_MEAN", 1), ("IR_ROWS_MAP", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), header), name
    assert (_lib.IR_ROWS_NONE, _lib.IR_ROWS_HEAD_MEAN, _lib.IR_ROWS_MAP) == (0, 1, 2)


def test_validation_names_the_field_before_any_launch():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    off = lambda n: C.cast(C.c_void_p(ptr.value + n), C.c_void_p)
    INVALID, UNSUPPORTED = -1, -2
    assert lib.ir_attn_rows(None, ptr, 4, 0, ptr, None) == INVALID and b"args" in err()
    assert lib.ir_attn_rows(C.byref(a), None, 4, 0, ptr, None) == INVALID and b"row_index" in err()
    assert lib.ir_attn_rows(C.byref(a), ptr, 4, 0, None, None) == INVALID and b"out" in err()
    a.lse = None
    assert lib.ir_attn_rows(C.byref(a), ptr, 4, 0, ptr, None) == INVALID and b"lse" in err()
    a.lse = ptr
    assert lib.ir_attn_rows(C.byref(a), ptr, 0, 0, ptr, None) == INVALID and b"n_rows" in err()
    assert lib.ir_attn_rows(C.byref(a), ptr, -3, 0, ptr, None) == INVALID and b"n_rows" in err()
    assert lib.ir_attn_rows(C.byref(a), ptr, 65, 0, ptr, None) == INVALID and b"n_rows" in err() and b"len_q" in err()
    for bad in (3, -1, 7):
        assert lib.ir_attn_rows(C.byref(a), ptr, 4, bad, ptr, None) == UNSUPPORTED and b"reduce" in err()
    assert lib.ir_attn_rows(C.byref(a), off(2), 4, 0, ptr, None) == UNSUPPORTED and b"row_index" in err()
    assert lib.ir_attn_rows(C.byref(a), ptr, 4, 1, off(8), None) == UNSUPPORTED and b"out" in err()
    a.tuning = 13
    assert lib.ir_attn_rows(C.byref(a), ptr, 4, 0, ptr, None) == UNSUPPORTED and b"tuning" in err()
    a.tuning = 0
    a.struct_size = 7
    assert lib.ir_attn_rows(C.byref(a), ptr, 4, 0, ptr, None) == INVALID and b"ABI mismatch" in err()


def test_ops_attn_rows_has_no_cpu_path_and_checks_reduce():
    from instantrestore_amd import ops
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    lse = torch.zeros(1, 1, 8)
    with pytest.raises(ValueError, match="reduce"):
        ops.attn_rows(q, q, None, lse, torch.tensor([0]), heads=1, scale=0.125, reduce="sum")
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_rows(q, q, None, lse, torch.tensor([0]), heads=1, scale=0.125)
    # the host-side check of a CPU index list (device lists are the kernel's business: zero rows)
    for bad in ([-1, 2], [0, 8]):
        with pytest.raises(ValueError, match="indices"):
            ops._row_index(torch.tensor(bad), 1, 8, torch.device("cpu"))
    with pytest.raises(ValueError):
        ops._row_index(torch.zeros(3, 2, dtype=torch.int64), 2, 8, torch.device("cpu"))      # 3 lists for a batch of 2
    with pytest.raises(ValueError):
        ops._row_index(torch.zeros(9, dtype=torch.int64), 1, 8, torch.device("cpu"))         # more rows than tokens
    with pytest.raises(ValueError):
        ops._row_index(torch.zeros(2), 1, 8, torch.device("cpu"))                            # not integers
    idx = ops._row_index(torch.tensor([3, 3, 1]), 2, 8, torch.device("cpu"))
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.tolist() == [[3, 3, 1], [3, 3, 1]]


# ---- processor host logic on the stand-in ---------------------------------------------------------------------------------
@pytest.fixture()
def shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    import oracle_ops_rows
    monkeypatch.setattr(ap, "_ops", oracle_ops_rows)
    oracle_ops_rows.CALLS.clear()
    return oracle_ops_rows


def _layer(train_input=True, save=False):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    torch.manual_seed(3)
    B, H, L, N = 2, 2, 16, 3
    proc = SharedAttnProcessor(self_attn_idx=0, save_self_attentions=save, use_adain=True, train_input=train_input)
    attn = Attention(query_dim=H * 64, heads=H, dim_head=64, processor=proc)
    x = torch.randn(B, L, H * 64)
    rk, rv = torch.randn(B, N, L, H * 64), torch.randn(B, N, L, H * 64)
    run = lambda: attn(x, ref_keys=[rk], ref_values=[rv])
    return proc, run, (B, H, L, N)


def test_processor_defaults_and_unchanged_calls_without_an_index(shim):
    from face_replace.models.attn_processors import SharedAttnProcessor
    p = SharedAttnProcessor()
    assert p.attention_rows_index is None and p.attention_rows_reduce == "head_mean" and p.attention_rows is None
    assert len(p.state_dict()) == 0
    proc, run, _ = _layer()
    with torch.no_grad():
        run()
    names = [c[0] for c in shim.CALLS]
    assert "attn_rows" not in names and "attn_probs" not in names
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [False]        # no LSE asked for
    assert proc.attention_rows is None


@pytest.mark.parametrize("train_input", [True, False])
def test_three_forms_broadcast_and_duplicates(shim, train_input):
    proc, run, (B, H, L, N) = _layer(train_input, save=True)
    lkv = (N + int(train_input)) * L
    idx = torch.tensor([5, 0, 5, 15, 5, 7])                        # (R,): one list for the batch, token 5 three times
    R = idx.numel()
    got = {}
    with torch.no_grad():
        for red in ("none", "head_mean", "map"):
            proc.attention_rows_index, proc.attention_rows_reduce = idx, red
            y = run()
            got[red] = proc.attention_rows
    P = proc.attention_probs
    assert P.shape == (B, H, L, lkv)
    assert got["none"].shape == (B, H, R, lkv) and got["head_mean"].shape == (B, R, lkv) and got["map"].shape == (B, lkv)
    assert got["head_mean"].dtype == torch.float32 and got["map"].dtype == torch.float32 and got["none"].dtype == P.dtype
    assert torch.equal(got["none"], P[:, :, idx])                                   # the gather, duplicates kept
    assert torch.equal(got["none"][:, :, 0], got["none"][:, :, 2]) and torch.equal(got["none"][:, :, 0], got["none"][:, :, 4])
    torch.testing.assert_close(got["head_mean"], P.double().mean(1)[:, idx].float(), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(got["map"], P.double().mean(1)[:, idx].sum(1).float(), rtol=1e-6, atol=1e-7)   # token 5 counted three times
    # a (B, R) index: one list per entry
    idx2 = torch.tensor([[1, 2, 3], [3, 3, 0]])
    proc.attention_rows_index, proc.attention_rows_reduce = idx2, "none"
    with torch.no_grad():
        run()
    for b in range(B):
        assert torch.equal(proc.attention_rows[b], proc.attention_probs[b][:, idx2[b]])
    assert y.shape == (B, L, H * 64)


def test_one_lse_serves_rows_and_dump_and_rows_alone_need_no_dump(shim):
    proc, run, (B, H, L, N) = _layer(save=True)
    proc.attention_rows_index = torch.tensor([2, 9])
    with torch.no_grad():
        y_both = run()
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [True]            # one attention call, one LSE
    names = [c[0] for c in shim.CALLS]
    assert names.count("shared_attention") == 1 and names.count("attn_rows") == 1 and names.count("attn_probs") == 1
    rows_both = proc.attention_rows
    shim.CALLS.clear()
    proc.save_self_attentions, proc.attention_probs = False, None
    with torch.no_grad():
        y_rows = run()
    names = [c[0] for c in shim.CALLS]
    assert names.count("attn_rows") == 1 and "attn_probs" not in names and proc.attention_probs is None
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [True]
    assert torch.equal(proc.attention_rows, rows_both) and rows_both.shape == (B, 2, (N + 1) * L)
    shim.CALLS.clear()
    proc.attention_rows_index = None
    with torch.no_grad():
        y_plain = run()
    assert torch.equal(y_plain, y_rows) and torch.equal(y_plain, y_both)           # the layer output never depends on the option
    # a layer that is not shared (no references handed over) ignores the index
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    plain = SharedAttnProcessor(self_attn_idx=None)
    plain.attention_rows_index = torch.tensor([0])
    shim.CALLS.clear()
    with torch.no_grad():
        Attention(query_dim=64, heads=1, dim_head=64, processor=plain)(torch.randn(1, 4, 64))
    assert "attn_rows" not in [c[0] for c in shim.CALLS] and plain.attention_rows is None


# ---- landmark helpers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [16, 32, 64])
def test_landmark_rows_and_picture_against_numpy(side):
    from instantrestore_amd.attn_maps import landmark_picture, landmark_rows
    rng = np.random.default_rng(side)
    step = 512 / side
    lm = rng.uniform(0, 512 - step, size=(68, 2))
    # half-way values: x * side / 512 = n + 0.5 exactly; np.round goes to the even neighbour
    lm[:6, 0] = (np.array([0, 1, 2, 3, 4, 5]) + 0.5) * step
    lm[:6, 1] = (np.array([5, 4, 3, 2, 1, 0]) + 0.5) * step
    want = np.round(lm * side / 512).astype(int)
    assert want[0, 0] == 0 and want[1, 0] == 2 and want[2, 0] == 2 and want[3, 0] == 4          # half to even
    want = want[:, 1] * side + want[:, 0]
    got = landmark_rows(lm, side)
    assert got.shape == (68,) and np.array_equal(got, want) and got.max() < side * side
    assert np.array_equal(landmark_rows(lm / 2, side, source=256), want)
    with pytest.raises(ValueError):
        landmark_rows(np.array([[10.0, 511.9]]), side)                # y rounds to `side`: past the last token row
    row = rng.standard_normal(5 * side * side).astype(np.float32)
    pic = landmark_picture(row, side)
    assert pic.shape == (side, 5 * side) and np.array_equal(pic, row.reshape(side, side * 5))
    assert np.array_equal(landmark_picture(torch.from_numpy(row), side), pic)
    with pytest.raises(ValueError):
        landmark_picture(row[:-1], side)


# ---- the build's register report -------------------------------------------------------------------------------------------
def test_kernels_report_no_spills_and_no_scratch():
    """every instantiation of attn_rows_kernel in the remarks the build leaves behind: 0 spilled VGPRs, 0 bytes of scratch
    (a wave of the summing forms holds up to 96 fp32 partial sums per lane over its head walk)"""
    paths = glob.glob(os.path.join(REPO, "instantrestore_amd", "csrc", "build", "attn_rows.remarks")) + \
        glob.glob(os.path.join(REPO, "build", "attn_rows.remarks"))
    assert paths, "attn_rows.remarks is missing: run __graft_entry__.build()"
    text = open(paths[0], errors="replace").read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 18 and all("attn_rows_kernel" in n for n in names), names      # 2 dtypes x 3 row-block counts x 3 forms
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", text)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    sgpr_spills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", text)]
    assert len(spills) == 18 and len(scratch) == 18
    assert not any(spills) and not any(scratch) and not any(sgpr_spills), (spills, scratch, sgpr_spills)
