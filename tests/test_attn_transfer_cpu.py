"""The payload read-out (``ir_attn_transfer`` / ``ops.attn_transfer`` / ``SharedAttnProcessor.attention_transfer_payload``):
everything that can be checked without a GPU - the symbol and its validation, the wrapper's checks, the payload and field
helpers, the processor's host logic on the oracle-backed stand-in ``tests/oracle_ops_transfer.py``, that helper itself against
a brute-force loop, and the kernels' register report."""
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


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_bound_with_its_constants():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "ir_attn_transfer") and "ir_attn_transfer" in _lib.SYMBOLS
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION                      # a new function, no struct change
    header = open(os.path.join(REPO, "include", "instantrestore_hip.h")).read()
    for name, val in (("IR_TRANSFER_PER_HEAD", 0), ("IR_TRANSFER_HEAD_MEAN", 1), ("IR_TRANSFER_MAX_CHANNELS", 8)):
        assert re.search(r"#define %s %d\b" % (name, val), header), name
    assert (_lib.IR_TRANSFER_PER_HEAD, _lib.IR_TRANSFER_HEAD_MEAN, _lib.IR_TRANSFER_MAX_CHANNELS) == (0, 1, 8)
    assert re.search(r"int ir_attn_transfer\(const ir_shared_attn_args\* args, const float\* payload, int64_t pay_sb, int64_t pay_sj, "
                     r"int32_t channels,\s*const int32_t\* row_index, int32_t n_rows, int32_t reduce, float\* sums, float\* mass, "
                     r"void\* stream\);", header)
    res, argtypes = _lib.SYMBOLS["ir_attn_transfer"]
    assert res is C.c_int and len(argtypes) == 11 and argtypes[2] is C.c_int64 and argtypes[3] is C.c_int64 and argtypes[4] is C.c_int32
    kernels = open(os.path.join(REPO, "instantrestore_amd", "csrc", "ir_kernels.h")).read()
    assert "ir_launch_attn_transfer" in kernels and "kTransferMaxChannels = 8" in kernels


def test_validation_names_the_field_before_any_launch():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    off = lambda n: C.cast(C.c_void_p(ptr.value + n), C.c_void_p)

    def call(payload=ptr, sb=0, sj=8, ch=2, rows=ptr, n=4, red=0, sums=ptr, mass=ptr, args=a):
        return lib.ir_attn_transfer(None if args is None else C.byref(args), payload, sb, sj, ch, rows, n, red, sums, mass, None)

    assert call(args=None) == INVALID and b"args" in err()
    assert call(payload=None) == INVALID and b"payload" in err()
    assert call(rows=None) == INVALID and b"row_index" in err()
    assert call(sums=None) == INVALID and b"sums" in err()
    a.lse = None
    assert call() == INVALID and b"lse" in err()
    a.lse = ptr
    for ch in (0, 9):
        assert call(ch=ch, sj=16) == UNSUPPORTED and b"channels" in err()
    assert call(ch=4, sj=3) == INVALID and b"pay_sj" in err()
    assert call(sb=-1) == INVALID and b"pay_sb" in err()
    assert call(payload=off(2)) == UNSUPPORTED and b"payload" in err()
    assert call(sums=off(2)) == UNSUPPORTED and b"sums" in err()
    assert call(mass=off(1)) == UNSUPPORTED and b"mass" in err()
    assert call(rows=off(2)) == UNSUPPORTED and b"row_index" in err()
    assert call(n=0) == INVALID and b"n_rows" in err()
    assert call(n=65) == INVALID and b"n_rows" in err() and b"len_q" in err()
    for bad in (-1, 2):
        assert call(red=bad) == UNSUPPORTED and b"reduce" in err()
    a.tuning = 13
    assert call() == UNSUPPORTED and b"tuning" in err() and b"ir_attn_transfer" in err()
    a.tuning = 0
    a.struct_size = 7
    assert call() == INVALID and b"ABI mismatch" in err()


def test_bias_and_ragged_blocks_are_refused_like_the_other_readouts():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    bias = _copy_into(_lib.SharedAttnBiasArgs(), a)
    bias.key_bias = ptr
    assert lib.ir_attn_transfer(C.byref(bias), ptr, 0, 2, 2, ptr, 4, 0, ptr, ptr, None) == UNSUPPORTED
    assert b"key_bias" in err() and b"ir_attn_transfer" in err() and b"ir_attn_match" in err()
    ragged = _copy_into(_lib.SharedAttnRaggedArgs(), a)
    ragged.ref_lens, ragged.rl_sb = ptr, 2
    assert lib.ir_attn_transfer(C.byref(ragged), ptr, 0, 2, 2, ptr, 4, 1, ptr, None, None) == UNSUPPORTED
    assert b"ref_lens" in err() and b"ir_attn_transfer" in err() and b"ir_attn_match" in err()


# ---- ops ------------------------------------------------------------------------------------------------------------------
def test_ops_attn_transfer_has_no_cpu_path_and_checks_its_arguments():
    from instantrestore_amd import ops
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    lse = torch.zeros(1, 1, 8)
    pay = torch.zeros(8, 2)
    with pytest.raises(ValueError, match="reduce"):
        ops.attn_transfer(q, q, None, lse, pay, heads=1, scale=0.125, reduce="map")
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_transfer(q, q, None, lse, pay, heads=1, scale=0.125)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_transfer(q, q, None, lse, pay, torch.tensor([0]), heads=1, scale=0.125, reduce="head_mean", normalize=True)
    assert ops.TRANSFER_REDUCE == {"none": 0, "head_mean": 1}
    src = inspect.getsource(ops.attn_transfer)
    assert "_row_index(rows, B, Lq, q.device)" in src and "_transfer_payload(payload, B, lkv, q.device)" in src
    assert ".contiguous()" not in src.split("_transfer_payload(payload")[1].split("idx =")[0]        # the payload is never copied


def test_payload_checks_and_strides():
    from instantrestore_amd import ops
    cpu = torch.device("cpu")
    chk = lambda t, B=2, lkv=24: ops._transfer_payload(t, B, lkv, cpu)
    base = torch.zeros(2, 24, 3)
    assert chk(base)[1:] == (72, 3, 3) and chk(base)[0] is base
    assert chk(base[0])[1:] == (0, 3, 3) and chk(base[:1])[1:] == (0, 3, 3)
    wide = torch.zeros(2, 24, 8)[..., :3]                                   # a row stride wider than C, passed through as it is
    got = chk(wide)
    assert got[0] is wide and got[1:] == (192, 8, 3)
    assert chk(torch.zeros(1, 24, 3).expand(2, 24, 3))[1:] == (0, 3, 3)    # an expanded batch axis is stride 0
    for bad, word in ((base.double(), "fp32"), (base.to(torch.bfloat16), "fp32"), (torch.zeros(24), "payload must be"),
                      (torch.zeros(2, 2, 24, 3), "payload must be"), (torch.zeros(3, 24, 3), "batch"), (torch.zeros(2, 23, 3), "keys"),
                      (torch.zeros(2, 24, 9), "channels"), (torch.zeros(2, 24, 0), "channels"),
                      (torch.zeros(2, 3, 24).transpose(1, 2), "stride"), (np.zeros((24, 3), dtype=np.float32), "fp32")):
        with pytest.raises(ValueError, match=word):
            chk(bad)
    with pytest.raises(ValueError, match="is on"):
        ops._transfer_payload(base, 2, 24, torch.device("cuda", 0))


def test_ops_signature():
    from instantrestore_amd import ops
    sig = inspect.signature(ops.attn_transfer)
    names = list(sig.parameters)
    assert names == ["q", "k_self", "ref_k", "lse", "payload", "rows", "heads", "scale", "include_self", "reduce", "normalize", "q_prescaled",
                     "batch_invariant"]
    assert "key_bias" not in names and "ref_lens" not in names
    assert sig.parameters["rows"].default is None and sig.parameters["reduce"].default == "none" and sig.parameters["normalize"].default is False
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[6:])


# ---- payload and field helpers ----------------------------------------------------------------------------------------------
def test_coordinate_payload_on_hand_made_shapes():
    from instantrestore_amd.attn_maps import coordinate_payload, match_coordinates
    p = coordinate_payload(16, 2, 4, True)
    assert p.shape == (1, 24, 2) and p.dtype == torch.float32
    assert p[0, :16].tolist() == [[float(i // 4), float(i % 4)] for i in range(16)]
    assert p[0, 16:20].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]] and torch.equal(p[0, 16:20], p[0, 20:24])
    y, x = match_coordinates(torch.arange(16), 4)                             # the convention of match_coordinates
    assert torch.equal(p[0, :16, 0].long(), y) and torch.equal(p[0, :16, 1].long(), x)
    assert coordinate_payload(16, 2, 4, False).shape == (1, 8, 2) and coordinate_payload(9, 0, 0, True).shape == (1, 9, 2)
    assert coordinate_payload(7, 1, 4, False).shape == (1, 4, 2)             # the self length is not looked at without the self segment
    for bad in ((15, 2, 4, True), (16, 2, 5, True), (16, 1, 2, False)):
        with pytest.raises(ValueError, match="square"):
            coordinate_payload(*bad)
    with pytest.raises(ValueError, match="empty"):
        coordinate_payload(16, 0, 4, False)


def test_image_payload_pools_by_area_onto_the_key_axis():
    from instantrestore_amd.attn_maps import image_payload
    B, N, Ci = 2, 3, 3
    g = torch.Generator().manual_seed(0)
    me = torch.rand(B, Ci, 8, 8, generator=g)
    refs = torch.rand(B, N, Ci, 8, 8, generator=g)
    p = image_payload(me, refs, 16, 4, True)                                  # a 4 x 4 self grid, 2 x 2 reference grids
    assert p.shape == (B, 16 + N * 4, Ci) and p.dtype == torch.float32 and p.is_contiguous()
    for b in range(B):
        for c in range(Ci):
            for t in range(16):
                ty, tx = divmod(t, 4)
                assert abs(float(p[b, t, c]) - float(me[b, c, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2].mean())) < 1e-6
            for n in range(N):
                for t in range(4):
                    ty, tx = divmod(t, 2)
                    assert abs(float(p[b, 16 + 4 * n + t, c]) - float(refs[b, n, c, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4].mean())) < 1e-6
    same = image_payload(me[:, :, ::2, ::2], refs, 16, 4, True)               # a picture already on the grid is taken as it is
    assert torch.equal(same[:, :16], me[:, :, ::2, ::2].flatten(2).transpose(1, 2))
    assert image_payload(None, refs, 16, 4, False).shape == (B, N * 4, Ci) and image_payload(me, None, 16, 4, True).shape == (B, 16, Ci)
    with pytest.raises(ValueError, match="square"):
        image_payload(me, refs, 15, 4, True)
    with pytest.raises(ValueError, match="self_image"):
        image_payload(None, refs, 16, 4, True)
    with pytest.raises(ValueError, match="disagree"):
        image_payload(me[:1], refs, 16, 4, True)


def test_soft_match_field_of_a_one_hot_distribution_is_match_field():
    from instantrestore_amd.attn_maps import coordinate_payload, match_coordinates, match_field, soft_match_field
    side = 4
    index = torch.tensor([[[0, 5, 9], [15, 3, 14]]], dtype=torch.int32)     # (B = 1, R = 2, S = 3)
    rows = torch.tensor([1, 6])
    coords = coordinate_payload(16, 0, 0, True)[0]                           # (16, 2)
    conf = torch.tensor([[[0.5, 0.25, 0.125], [1.0, 0.0, 0.75]]])
    sums = coords[index.long()] * conf[..., None]                            # a one-hot row of weight `conf` at key `index`
    pos, disp, c = soft_match_field(sums, conf, rows, side)
    y, x = match_coordinates(index, side)
    dy, dx = match_field(index, rows, side)
    live = conf > 0
    assert torch.equal(pos[..., 0][live], y[live].float()) and torch.equal(pos[..., 1][live], x[live].float())
    assert torch.equal(disp[..., 0][live], dy[live].float()) and torch.equal(disp[..., 1][live], dx[live].float())
    assert torch.equal(pos[0, 1, 1], torch.zeros(2)) and torch.equal(disp[0, 1, 1], torch.zeros(2)) and c is conf      # zero mass: zeros
    # per head (B, H, R, S, 2) with a (B, R) row list; an out-of-range row has no position and no displacement
    s4, m4 = sums[:, None].expand(1, 2, 2, 3, 2), conf[:, None].expand(1, 2, 2, 3)
    p4, d4, _ = soft_match_field(s4, m4, torch.tensor([[-1, 6]]), side)
    assert p4.shape == (1, 2, 2, 3, 2) and torch.equal(p4[0, 1, 1], pos[0, 1]) and torch.equal(d4[0, 0, 1], disp[0, 1])
    assert not bool(p4[:, :, 0].any()) and not bool(d4[:, :, 0].any())
    # every token (None / "all"): row r is token r; a soft row: the mean of two keys
    full = coords[None].clone() * 0.5                                        # (1, 16, 2): token r looks at key r with weight 0.5 ...
    full = (full + 0.5 * coords[None].flip(1))[:, :, None]                   # ... and at key 15 - r with weight 0.5: (1, 16, 1, 2)
    pa, da, _ = soft_match_field(full, torch.ones(1, 16, 1), "all", side)
    assert torch.equal(pa[0, :, 0], torch.full((16, 2), 1.5)) and torch.equal(da[0, :, 0], 1.5 - coords)


# ---- the oracle helper ----------------------------------------------------------------------------------------------------
def test_oracle_helper_against_a_brute_force_loop():
    import oracle_ops_transfer as T
    rng = np.random.default_rng(0)
    B, H, R, Ls, N, Lr, Cn = 2, 3, 4, 5, 2, 7, 3
    edges = T.segment_edges(Ls, N, Lr, True)
    p = rng.random((B, H, R, edges[-1]))
    for y in (rng.standard_normal((B, edges[-1], Cn)), rng.standard_normal((1, edges[-1], Cn)), rng.standard_normal((edges[-1], Cn))):
        sums, mass, sums_hm, mass_hm = T.transfer_np(p, y, edges)
        assert sums.shape == (B, H, R, 3, Cn) and mass.shape == (B, H, R, 3) and sums_hm.shape == (B, R, 3, Cn) and mass_hm.shape == (B, R, 3)
        yb = T.payload_np(y, B)
        for b, h, r in np.ndindex(B, H, R):
            for s, (a, e) in enumerate(zip(edges[:-1], edges[1:])):
                m, acc = 0.0, np.zeros(Cn)
                for j in range(a, e):
                    m += p[b, h, r, j]
                    acc += p[b, h, r, j] * yb[b, j]
                assert abs(mass[b, h, r, s] - m) < 1e-12 and np.abs(sums[b, h, r, s] - acc).max() < 1e-12
        assert np.abs(sums_hm - sums.sum(axis=1) / H).max() < 1e-12 and np.abs(mass_hm - mass.sum(axis=1) / H).max() < 1e-12
    assert np.abs(mass.sum(-1) - p.sum(-1)).max() < 1e-12


# ---- processor host logic on the stand-in -----------------------------------------------------------------------------------
@pytest.fixture()
def shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    import oracle_ops_transfer
    monkeypatch.setattr(ap, "_ops", oracle_ops_transfer)
    ap._BIAS_ROWS.clear()
    oracle_ops_transfer.CALLS.clear()
    return oracle_ops_transfer


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
    assert p.attention_transfer_payload is None and p.attention_transfer_index is None
    assert p.attention_transfer_reduce == "head_mean" and p.attention_transfer is None
    assert len(p.state_dict()) == 0
    assert list(inspect.signature(SharedAttnProcessor.__init__).parameters) == ["self", "self_attn_idx", "save_self_attentions", "use_adain", "train_input"]
    proc, run, _ = _layer()
    proc.attention_transfer_index = "all"                                     # the index alone switches nothing on
    with torch.no_grad():
        run()
    assert "attn_transfer" not in [c[0] for c in shim.CALLS] and proc.attention_transfer is None
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [False]


@pytest.mark.parametrize("train_input", [True, False])
def test_attribute_triggers_one_call_with_the_forwards_lse(shim, train_input):
    from instantrestore_amd.attn_maps import coordinate_payload, soft_match_field
    proc, run, (B, H, L, N) = _layer(train_input)
    S = N + int(train_input)
    payload = coordinate_payload(L, N, L, train_input)
    with torch.no_grad():
        y_plain = run()
        shim.CALLS.clear()
        proc.attention_transfer_payload = payload
        y_all = run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_transfer"]
    assert len(calls) == 1 and calls[0]["rows"] is None and calls[0]["reduce"] == "head_mean" and calls[0]["payload"] is payload
    assert calls[0]["lse"] is shim.LAST_LSE[0] and shim.LAST_LSE[0] is not None          # the LSE of the same forward
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [True]
    assert [c[0] for c in shim.CALLS].count("shared_attention") == 1 and "attn_probs" not in [c[0] for c in shim.CALLS]
    sums, mass = proc.attention_transfer
    assert sums.shape == (B, L, S, 2) and sums.dtype == torch.float32 and mass.shape == (B, L, S) and mass.dtype == torch.float32
    assert float(mass.min()) > 0 and float((mass.sum(-1) - 1).abs().max()) < 1e-5
    pos, disp, conf = soft_match_field(sums, mass, "all", 4)
    assert float(pos.min()) >= 0 and float(pos.max()) <= 3 and conf is mass            # an expectation stays on the grid
    assert torch.equal(y_plain, y_all)                                                    # the layer output never depends on the option
    # "all" is every row too; a row tensor goes through as it is; "none" gives the per-head shape
    shim.CALLS.clear()
    rows = torch.tensor([5, 0, 5])
    proc.attention_transfer_index, proc.attention_transfer_reduce = rows, "none"
    with torch.no_grad():
        run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_transfer"]
    assert len(calls) == 1 and calls[0]["rows"] is rows and calls[0]["reduce"] == "none"
    s2, m2 = proc.attention_transfer
    assert s2.shape == (B, H, 3, S, 2) and m2.shape == (B, H, 3, S) and torch.equal(s2[:, :, 0], s2[:, :, 2])
    proc.attention_transfer_index = "all"
    shim.CALLS.clear()
    with torch.no_grad():
        run()
    assert [c[1]["rows"] for c in shim.CALLS if c[0] == "attn_transfer"] == [None]
    # beside the rows and match read-outs: one LSE serves all three
    shim.CALLS.clear()
    proc.attention_rows_index, proc.attention_match_index = rows, "all"
    with torch.no_grad():
        run()
    names = [c[0] for c in shim.CALLS]
    assert names.count("shared_attention") == 1 and names.count("attn_rows") == 1 and names.count("attn_match") == 1 and names.count("attn_transfer") == 1
    proc.attention_transfer_index = "every"
    with torch.no_grad(), pytest.raises(ValueError, match="attention_transfer_index"):
        run()


def test_a_layer_that_is_not_shared_ignores_the_attribute(shim):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    plain = SharedAttnProcessor(self_attn_idx=None)
    plain.attention_transfer_payload = torch.zeros(4, 2)
    with torch.no_grad():
        Attention(query_dim=64, heads=1, dim_head=64, processor=plain)(torch.randn(1, 4, 64))
    assert "attn_transfer" not in [c[0] for c in shim.CALLS] and plain.attention_transfer is None
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] in ([False], [])


def test_processor_raises_with_a_bias_or_counts(shim):
    proc, run, (B, H, L, N) = _layer()
    lkv = (N + 1) * L
    proc.attention_transfer_payload = torch.zeros(lkv, 2)
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
        with torch.no_grad(), pytest.raises(NotImplementedError, match="attention_transfer_payload"):
            run(**kw)
        assert "shared_attention" not in [c[0] for c in shim.CALLS], name      # refused before anything is launched


# ---- the kernel file is built on the shared header -----------------------------------------------------------------------------
def test_kernel_takes_its_qk_block_from_the_readout_header():
    """attn_transfer.hip includes ir_readout.h, uses its pieces and defines none of them again; the probability expression stays in
    the header only (the rules of tests/test_readout_header_cpu.py for the other read-outs); the build lists the file twice"""
    csrc = os.path.join(REPO, "instantrestore_amd", "csrc")
    text = open(os.path.join(csrc, "attn_transfer.hip")).read()
    assert re.search(r'#include\s+"ir_readout\.h"', text)
    for name in ("keymap", "key_segment", "gather_rows", "load_q", "load_k", "scores", "prob", "rows_nq", "rows_ngroups", "dispatch_rows"):
        if name != "rows_nq":                                                  # (reached through dispatch_rows and rows_ngroups)
            assert re.search(r"\b%s\s*(<[^>]*>)?\(" % name, text), f"{name} is not used"
        assert not re.search(r"\b(int|void|float|hipError_t|f32x16|KeySeg<T>)\s+%s\s*\(" % name, text), f"{name} is defined again"
    assert not re.search(r"__builtin_fmaf\([^;]*scale_log2", text)
    build = open(os.path.join(csrc, "build.sh")).read()
    assert build.count("attn_transfer.hip") == 2                              # SRCS and the MFMA-results-in-VGPRs line
    assert re.search(r'"\$s" == attn_transfer\.hip \]\] && extra\+=\(-mllvm -amdgpu-mfma-vgpr-form\)', build)


# ---- the build's register report -------------------------------------------------------------------------------------------
def test_kernels_report_no_spills_and_no_scratch():
    """every instantiation of attn_transfer_kernel in the remarks the build leaves behind: 0 spilled registers, 0 bytes of scratch
    (a wave of the head-mean form holds 27 running sums, 27 head totals and 48 probabilities per lane beside its operands)"""
    paths = glob.glob(os.path.join(REPO, "instantrestore_amd", "csrc", "build", "attn_transfer.remarks")) + \
        glob.glob(os.path.join(REPO, "build", "attn_transfer.remarks"))
    assert paths, "attn_transfer.remarks is missing: run __graft_entry__.build()"
    text = open(paths[0], errors="replace").read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 36 and all("attn_transfer_kernel" in n for n in names), names   # 2 dtypes x 3 row-block counts x 2 forms x 3 channel paddings
    spills = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", text)]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    sgpr_spills = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", text)]
    assert len(spills) == 36 and len(scratch) == 36
    assert not any(spills) and not any(scratch) and not any(sgpr_spills), (spills, scratch, sgpr_spills)
    sys_path = os.path.join(REPO, "tools", "check_resources.py")
    assert "attn_transfer_kernel" in open(sys_path).read()
