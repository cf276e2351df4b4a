"""The additive key bias of the fused attention (``ir_shared_attn_bias_args`` / ``ops.shared_attention(key_bias=)`` /
``ops.key_bias``): everything that can be checked without a GPU - the third block's size rule and layout, the dispatch and
batch-invariant plan of a bias call, every refusal with its message, the arithmetic of the bias builder, the mask seam of
``attention.Attention`` and the processors' host logic."""
import ctypes as C
import math

import pytest
import torch

INVALID, UNSUPPORTED = -1, -2
IR_TUNE = {"default": 0, "exactmax": 7, "pipe32": 10, "presc": 11, "w64x4": 12, "w64x8": 13, "earlyqk": 14, "w128": 16, "postcheck": 18}


def _args(lib_mod, *, block="bias", bias=True, B=2, N=2, L=64, Lq=None, H=1, flags=1, valid=False, mass=False, adain=False, tuning=0,
          kb_sb=None, kb_sh=0):
    """a valid self + N-reference call on addresses that are never dereferenced (validation and planning precede any launch)"""
    a = {"short": lib_mod.SharedAttnArgs, "table": lib_mod.SharedAttnTableArgs, "bias": lib_mod.SharedAttnBiasArgs}[block]()
    a.struct_size = C.sizeof(a)
    c = 64 * H
    Lq = L if Lq is None else Lq
    a.dtype, a.batch, a.heads, a.len_q, a.len_self, a.flags, a.scale, a.tuning = 1, B, H, Lq, L, flags, 0.125, tuning
    a.q = a.k_self = a.v_self = a.out = 4096
    a.q_sb = a.o_sb = Lq * c
    a.ks_sb = a.vs_sb = L * c
    a.q_sl = a.ks_sl = a.vs_sl = a.o_sl = c
    a.q_sh = a.ks_sh = a.vs_sh = a.o_sh = 64
    a.n_refs, a.len_ref = N, (L if N else 0)
    if N:
        a.kr_sl = a.vr_sl = c
        a.kr_sh = a.vr_sh = 64
        a.k_ref = a.v_ref = 4096
        a.kr_sb = a.vr_sb = N * L * c
        a.kr_sn = a.vr_sn = L * c
    if valid:
        a.valid_refs = 4096
    if mass:
        a.seg_mass = 4096
    if adain:
        a.adain_a = a.adain_b = 4096
    if block == "bias" and bias:
        a.key_bias = 4100                      # a 4-byte quantity: no 16-byte alignment
        a.kb_sb = (1 + N) * L if kb_sb is None else kb_sb
        a.kb_sh = kb_sh
    return a


def _plan(lib_mod, a):
    p = lib_mod.SharedAttnPlan()
    p.struct_size = C.sizeof(p)
    rc = lib_mod.lib().ir_shared_attn_plan(C.byref(a), C.byref(p))
    return (rc,) + tuple(getattr(p, n) for n, _ in lib_mod.SharedAttnPlan._fields_[1:])


def test_abi_stays_10_three_block_sizes_are_taken_and_the_fields_lie_where_the_header_puts_them():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION
    old, tab, new = C.sizeof(_lib.SharedAttnArgs), C.sizeof(_lib.SharedAttnTableArgs), C.sizeof(_lib.SharedAttnBiasArgs)
    assert tab == old + 16 and new == tab + 24
    assert [f[0] for f in _lib.SharedAttnBiasArgs._fields_] == ["key_bias", "kb_sb", "kb_sh"]
    assert (_lib.SharedAttnBiasArgs.key_bias.offset, _lib.SharedAttnBiasArgs.kb_sb.offset, _lib.SharedAttnBiasArgs.kb_sh.offset) == (tab, tab + 8, tab + 16)
    assert _lib.SharedAttnBiasArgs.k_ref_table.offset == old and _lib.IR_KEY_BIAS_MASKED == -1.0e4
    for block in ("short", "table", "bias"):
        assert lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, block=block))) != b"", block
    a = _args(_lib)
    for bad in (7, old + 8, tab + 8, old - 8, new + 8, new - 8, tab + 16):
        a.struct_size = bad
        assert lib.ir_shared_attn_kernel_name(C.byref(a)) == b"" and b"ABI mismatch" in lib.ir_last_error_string(), bad
        assert lib.ir_shared_attn_fwd(C.byref(a), None) == INVALID
        assert lib.ir_shared_attn_workspace_bytes_for(C.byref(a)) == 0
        assert _plan(_lib, a)[0] == INVALID


def test_the_header_declares_the_block_as_the_binding_mirrors_it():
    import os
    from instantrestore_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "instantrestore_hip.h")).read()
    body = hdr[hdr.index("typedef struct ir_shared_attn_bias_args {"):hdr.index("} ir_shared_attn_bias_args;")]
    assert body.index("ir_shared_attn_table_args t;") < body.index("const float* key_bias;") < body.index("int64_t kb_sb, kb_sh;")
    assert "#define IR_KEY_BIAS_MASKED (-1.0e4f)" in hdr and "#define IR_ABI_VERSION 10" in hdr
    assert "key_bias given or not" in hdr                       # the batch-invariant contract lists it as a per-entry parameter
    assert issubclass(_lib.SharedAttnBiasArgs, _lib.SharedAttnTableArgs)


@pytest.mark.parametrize("len_q", [256, 1024, 4096])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescaledq"])
def test_a_bias_call_names_and_plans_the_32_row_kernel_and_a_null_bias_is_the_dense_call(len_q, presc):
    from instantrestore_amd import _lib
    lib = _lib.lib()
    for bi in (False, True):
        for mass, adain in ((False, False), (True, True)):
            flags = 1 | (2 if presc else 0) | (8 if bi else 0)
            kw = dict(B=8, N=4, L=len_q, H=5, flags=flags, mass=mass, adain=adain)
            name = lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, **kw)))
            assert name.startswith(b"shared_attn_fwd_pipe_kernel<4 waves") and b"key bias" in name, name
            assert (b"pre-scaled Q" in name) == presc and (b"early QK" in name) == (not presc), name
            dense = _args(_lib, block="short", **kw)
            null = _args(_lib, block="bias", bias=False, **kw)
            dname = lib.ir_shared_attn_kernel_name(C.byref(dense))
            assert lib.ir_shared_attn_kernel_name(C.byref(null)) == dname != b"" and b"key bias" not in dname
            assert lib.ir_shared_attn_workspace_bytes_for(C.byref(null)) == lib.ir_shared_attn_workspace_bytes_for(C.byref(dense))
            if len_q == 4096:
                assert b"pipe_kernel" not in dname, dname           # today's kernel without a bias
            if bi:
                pb, pn, pd = _plan(_lib, _args(_lib, **kw)), _plan(_lib, null), _plan(_lib, dense)
                assert pb[0] == 0 and pb[1] == (IR_TUNE["presc"] if presc else IR_TUNE["earlyqk"]) and pb[2] == 128, pb
                assert pb[3] == 5 * (len_q // 128)
                assert pn == pd and pd[0] == 0
                assert lib.ir_shared_attn_workspace_bytes_for(C.byref(_args(_lib, **kw))) == pb[-1]
                # the plan of a bias call does not read the batch size
                assert _plan(_lib, _args(_lib, **dict(kw, B=1)))[1:5] == pb[1:5]


def test_plain_attention_and_odd_lengths_take_a_bias_without_alignment_rules():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a = _args(_lib, N=0, L=77, Lq=128, H=5, kb_sb=77, kb_sh=0)               # cross attention over 77 text tokens
    assert b"key bias" in lib.ir_shared_attn_kernel_name(C.byref(a))
    a = _args(_lib, N=3, L=72, Lq=200, H=2, flags=0, kb_sb=1000, kb_sh=217)  # references only, ragged segments, strides of any size
    assert b"key bias" in lib.ir_shared_attn_kernel_name(C.byref(a))
    a.key_bias = 4098
    assert lib.ir_shared_attn_kernel_name(C.byref(a)) == b"" and b"4-byte aligned" in lib.ir_last_error_string()
    a = _args(_lib, kb_sb=-1)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == INVALID and b"kb_sb" in lib.ir_last_error_string()


def test_every_refusal_of_a_bias_call_names_its_reason():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.ir_last_error_string()
    a = _args(_lib, valid=True)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"valid_refs" in err() and b"key_bias" in err()
    assert lib.ir_shared_attn_kernel_name(C.byref(a)) == b""
    for name, tune in IR_TUNE.items():
        presc = name in ("w128", "postcheck")
        a = _args(_lib, tuning=tune, L=4096, flags=1 | (2 if presc else 0))
        if name in ("default", "presc", "earlyqk"):      # (named only: these addresses must never reach a launch)
            assert lib.ir_shared_attn_kernel_name(C.byref(a)).startswith(b"shared_attn_fwd_pipe_kernel"), name
        else:
            assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"key_bias" in err() and b"tuning" in err(), (name, err())
    # the read-out entry points: their exp(s - lse) would leave the bias out
    calls = {"ir_attn_probs": lambda a: lib.ir_attn_probs(C.byref(a), 4096, None),
             "ir_attn_probs_ex": lambda a: lib.ir_attn_probs_ex(C.byref(a), 4096, 0, None),
             "ir_attn_segment_mass": lambda a: lib.ir_attn_segment_mass(C.byref(a), 4096, None),
             "ir_attn_rows": lambda a: lib.ir_attn_rows(C.byref(a), 4096, 1, 0, 4096, None)}
    for what, call in calls.items():
        a = _args(_lib)
        a.lse = 4096
        assert call(a) == UNSUPPORTED and b"key_bias" in err() and b"do not take a key bias" in err(), (what, err())


def test_ops_reject_a_bias_of_the_wrong_kind_before_any_launch():
    from instantrestore_amd import ops
    q = torch.zeros(2, 8, 128, dtype=torch.bfloat16)
    r = torch.zeros(2, 2, 8, 128, dtype=torch.bfloat16)
    lkv = 8 + 2 * 8
    for bad, match in ((torch.zeros(2, lkv, dtype=torch.float16), "float32"), (torch.zeros(2, lkv + 1), "shape"),
                       (torch.zeros(2, 3, lkv), "shape"), (torch.zeros(lkv, 2).t(), "contiguous"), (torch.zeros(4, 1, lkv), "shape")):
        with pytest.raises(ValueError, match=match):
            ops._check_key_bias(bad, q, 2, lkv)
    ops._check_key_bias(torch.zeros(2, lkv), q, 2, lkv)
    ops._check_key_bias(torch.zeros(2, 2, lkv + 5)[:, :, :lkv], q, 2, lkv)         # rows of a wider buffer
    with pytest.raises(RuntimeError, match="CPU"):                                 # no CPU path, bias or not
        ops.shared_attention(q, q, q, r, r, heads=2, scale=0.125, key_bias=torch.zeros(2, lkv))
    import inspect
    for fn in (ops.shared_attention, ops.time_shared_attention, ops.shared_attention_kernel_name, ops.shared_attention_plan):
        assert "key_bias" in inspect.signature(fn).parameters, fn.__name__
    for fn in (ops.attn_probs, ops.attn_segment_mass, ops.attn_rows):
        assert "key_bias" not in inspect.signature(fn).parameters, fn.__name__
    plan = ops.shared_attention_plan(8, 4096, 5, len_self=4096, n_refs=4, len_ref=4096, q_prescaled=True, key_bias=True)
    assert plan["kernel"] == 11 and plan["rows_per_item"] == 128
    assert ops.shared_attention_plan(8, 4096, 5, len_self=4096, n_refs=4, len_ref=4096, q_prescaled=True)["rows_per_item"] == 512


def test_key_bias_builder_weights_masks_and_refill():
    from instantrestore_amd import ops
    B, Ls, N, Lr = 2, 5, 3, 4
    w = torch.tensor([[1.0, 0.25, 0.0], [4.0, 1.0, 2.0]])
    row = ops.key_bias(B, Ls, N, Lr, True, ref_weights=w)
    assert row.dtype == torch.float32 and tuple(row.shape) == (B, Ls + N * Lr)
    assert torch.equal(row[:, :Ls], torch.zeros(B, Ls))
    refs = row[:, Ls:].view(B, N, Lr)
    assert torch.equal(refs, torch.log(w).unsqueeze(-1).expand(B, N, Lr)) and refs[0, 2, 0] == float("-inf") and refs[0, 0, 0] == 0
    assert abs(float(refs[0, 1, 0]) - math.log(0.25)) < 1e-6
    # without the self segment the row starts at reference 0
    assert tuple(ops.key_bias(B, Ls, N, Lr, False, ref_weights=w).shape) == (B, N * Lr)
    assert ops.key_bias(B, Ls, N, Lr, False, ref_weights=w)[1, 0] == pytest.approx(math.log(4.0))
    # token masks
    keep = torch.ones(B, N, Lr, dtype=torch.bool)
    keep[1, 0, 2:] = False
    row = ops.key_bias(B, Ls, N, Lr, True, ref_weights=w, ref_token_keep=keep)
    refs = row[:, Ls:].view(B, N, Lr)
    assert refs[1, 0].tolist() == [pytest.approx(math.log(4.0))] * 2 + [float("-inf")] * 2
    # an additive mask of the extended length, (B, Lkv) or (B, 1, Lkv); it adds to the rest
    m = torch.zeros(B, 1, Ls + N * Lr)
    m[:, :, 1] = -10000.0
    row2 = ops.key_bias(B, Ls, N, Lr, True, ref_weights=w, ref_token_keep=keep, attention_mask=m)
    assert torch.equal(row2[:, 1], torch.full((B,), -10000.0)) and torch.equal(row2[:, 2:], row[:, 2:])
    assert torch.equal(ops.key_bias(B, Ls, N, Lr, True, attention_mask=m[:, 0]), m[:, 0])
    # out= refills in place
    addr = row2.data_ptr()
    again = ops.key_bias(B, Ls, N, Lr, True, ref_weights=torch.ones(B, N), out=row2)
    assert again is row2 and row2.data_ptr() == addr and torch.equal(row2, torch.zeros_like(row2))
    for kw, match in ((dict(ref_weights=torch.ones(B, N + 1)), "ref_weights"), (dict(ref_weights=-torch.ones(B, N)), ">= 0"),
                      (dict(ref_token_keep=torch.ones(B, N, Lr)), "bool"), (dict(ref_token_keep=torch.ones(B, N, Lr + 1, dtype=torch.bool)), "shape"),
                      (dict(attention_mask=torch.zeros(B, 1, Ls)), "extended"), (dict(attention_mask=torch.zeros(B, Ls + N * Lr, dtype=torch.bool)), "additive"),
                      (dict(attention_mask=torch.zeros(B, 3, Ls + N * Lr)), "extended"), (dict(out=torch.zeros(B, 3)), "out")):
        with pytest.raises(ValueError, match=match):
            ops.key_bias(B, Ls, N, Lr, True, **kw)
    with pytest.raises(ValueError, match="without references"):
        ops.key_bias(B, Ls, 0, 0, True, ref_weights=torch.ones(B, 0))


@pytest.mark.parametrize("side", [16, 32, 64])
def test_key_bias_builder_pools_a_keep_map_by_area(side):
    """an S x S keep map (S = 64) becomes the layer's side x side tokens: a token is kept when >= 0.5 of its area is"""
    from instantrestore_amd import ops
    S, B, N = 64, 1, 2
    g = torch.Generator().manual_seed(side)
    keep = torch.rand(B, N, S, S, generator=g) < 0.5
    keep[0, 0, : S // 2] = True                # a kept upper half, a dropped lower-right quadrant
    keep[0, 1, S // 2:, S // 2:] = False
    f = S // side
    want = keep.float().reshape(B, N, side, f, side, f).mean(dim=(3, 5)) >= 0.5
    row = ops.key_bias(B, 7, N, side * side, True, ref_token_keep=keep)
    got = row[:, 7:].view(B, N, side, side)
    assert torch.equal(got == 0, want) and torch.equal(got == float("-inf"), ~want)
    assert bool(want[0, 0, : side // 2].all()) and not bool(want[0, 1, side // 2:, side // 2:].any())
    assert torch.equal(row[:, :7], torch.zeros(B, 7))
    with pytest.raises(ValueError, match="square"):
        ops.key_bias(B, 7, N, side * side + 1, True, ref_token_keep=keep)


# ---- attention.Attention.prepare_attention_mask and the processors' host logic (CPU stand-ins, as tests/test_host_logic.py) ----
def test_prepare_attention_mask_shapes():
    from instantrestore_amd.attention import Attention
    attn = Attention(query_dim=128, heads=2, dim_head=64)
    assert attn.prepare_attention_mask(None, 77, 3) is None
    m = torch.zeros(3, 1, 77)
    m[1, 0, 50:] = -10000.0
    got = attn.prepare_attention_mask(m, 77, 3)
    assert tuple(got.shape) == (6, 1, 77) and torch.equal(got, m.repeat_interleave(2, dim=0))
    assert torch.equal(got[2], m[1]) and torch.equal(got[3], m[1])                     # heads of one entry are neighbours
    assert attn.prepare_attention_mask(got, 77, 3) is got                               # already batch * heads rows: as it is
    assert tuple(attn.prepare_attention_mask(m, 77, 3, out_dim=4).shape) == (3, 2, 1, 77)
    with pytest.raises(NotImplementedError, match="77"):
        attn.prepare_attention_mask(m, 80, 3)                                           # upstream pads here; not reproduced


class _BiasShim:
    """tests/oracle_ops.py with a ``shared_attention`` that takes ``key_bias`` (float64 helper oracle) and the real, plain-torch
    ``ops.key_bias``; every other entry point is the oracle stand-in's"""

    def __init__(self):
        import oracle_ops
        self._o = oracle_ops
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._o, name)

    def key_bias(self, *a, **kw):
        from instantrestore_amd import ops
        self.calls.append(("key_bias", a[1:4]))
        return ops.key_bias(*a, **kw)

    def shared_attention(self, q, k_self, v_self, ref_k=None, ref_v=None, *, key_bias=None, return_mass=False, **kw):
        if key_bias is None:
            return self._o.shared_attention(q, k_self, v_self, ref_k, ref_v, return_mass=return_mass, **kw)
        import numpy as np
        from key_bias_oracle import biased_attention_np
        assert key_bias.dtype == torch.float32 and not kw.get("return_lse") and kw.get("valid_refs") is None
        self.calls.append(("shared_attention", key_bias.clone()))
        f = lambda t: None if t is None else t.detach().double().numpy()
        rvn = f(ref_v)
        if kw.get("adain") is not None:
            a, b = (f(t).reshape(rvn.shape[0], rvn.shape[1], 1, -1) for t in kw["adain"])
            rvn = rvn * a + b
        inc = kw.get("include_self", True)
        segs = ([k_self.shape[1]] if inc else []) + ([ref_k.shape[2]] * ref_k.shape[1] if ref_k is not None else [])
        out, _, mass = biased_attention_np(f(q), f(k_self), f(v_self), f(ref_k), rvn, kw["heads"], kw["scale"], f(key_bias),
                                           train_input=inc, seg_lens=segs)
        out = torch.from_numpy(out).to(q.dtype)
        return (out, torch.from_numpy(mass).float()) if return_mass else out


@pytest.fixture()
def bias_shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    shim = _BiasShim()
    monkeypatch.setattr(ap, "_ops", shim)
    ap._BIAS_ROWS.clear()
    return shim


def _shared_layer(heads=2, L=16, N=3, adain=False):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    g = torch.Generator().manual_seed(3)
    proc = SharedAttnProcessor(self_attn_idx=0, use_adain=adain, train_input=True)
    attn = Attention(query_dim=64 * heads, heads=heads, dim_head=64, processor=proc)
    x = torch.randn(2, L, 64 * heads, generator=g)
    rk, rv = torch.randn(2, N, L, 64 * heads, generator=g), torch.randn(2, N, L, 64 * heads, generator=g)
    return attn, proc, x, {"ref_keys": [rk], "ref_values": [rv]}


def test_processor_masks_become_the_key_bias_and_wrong_masks_raise(bias_shim):
    attn, proc, x, refs = _shared_layer()
    B, L, N, H = 2, 16, 3, 2
    lkv = L + N * L
    mask = torch.zeros(B, 1, lkv)
    mask[0, 0, L: 2 * L] = -10000.0
    with torch.no_grad():
        plain = attn(x, **refs)
        y = attn(x, attention_mask=mask, **refs)
        passed = bias_shim.calls[-1][1]
        assert tuple(passed.shape) == (B, lkv) and torch.equal(passed, mask[:, 0])
        assert not torch.equal(y[0], plain[0]) and torch.allclose(y[1], plain[1], atol=1e-6)
        # (B, Lkv) and the head-repeated (B * H, 1, Lkv) form give the same result
        assert torch.equal(attn(x, attention_mask=mask[:, 0], **refs), y)
        rep = mask.repeat_interleave(H, dim=0)
        assert torch.equal(attn(x, attention_mask=rep, **refs), y)
        assert tuple(bias_shim.calls[-1][1].shape) == (B, H, lkv)                       # materialised rows: the head stride is passed
        assert tuple(_last_bias(bias_shim, attn, x, refs, mask.expand(B, 1, lkv)[:, None].expand(B, H, 1, lkv).reshape(B * H, 1, lkv)).shape) in ((B, H, lkv), (B, lkv))
        # masked equals removed: reference 0 of entry 0 masked = the call on the other two (entry 0)
        keep = {"ref_keys": [refs["ref_keys"][0][:, 1:]], "ref_values": [refs["ref_values"][0][:, 1:]]}
        torch.testing.assert_close(y[0], attn(x, **keep)[0], atol=1e-5, rtol=1e-5)
        with pytest.raises(ValueError, match=f"{L} keys.*{lkv} keys"):                   # a mask of the self length
            attn(x, attention_mask=torch.zeros(B, 1, L), **refs)
        with pytest.raises(NotImplementedError, match="per-query"):
            attn(x, attention_mask=torch.zeros(B, L, lkv), **refs)
        with pytest.raises(ValueError, match="additive"):
            attn(x, attention_mask=torch.zeros(B, 1, lkv, dtype=torch.bool), **refs)
        with pytest.raises(ValueError, match="rows"):
            attn(x, attention_mask=torch.zeros(3, 1, lkv), **refs)
        # the dump paths do not take a bias yet; the masses do
        proc.save_self_attentions = True
        with pytest.raises(NotImplementedError, match="follow-up"):
            attn(x, attention_mask=mask, **refs)
        proc.save_self_attentions = False
        proc.attention_rows_index = torch.tensor([0, 3])
        with pytest.raises(NotImplementedError, match="follow-up"):
            attn(x, ref_weights=torch.ones(B, N), **refs)
        proc.attention_rows_index = None
        proc.save_attention_mass = True
        attn(x, attention_mask=mask, **refs)
        m = proc.attention_mass
        assert tuple(m.shape) == (B, H, L, 1 + N) and float(m[0, :, :, 1].abs().max()) == 0.0 and float((m.sum(-1) - 1).abs().max()) < 1e-5


def _last_bias(shim, attn, x, refs, mask):
    attn(x, attention_mask=mask, **refs)
    return shim.calls[-1][1]


def test_processor_ref_weights_and_keep_maps(bias_shim):
    from face_replace.models.attn_processors import AttnProcessor, SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    attn, proc, x, refs = _shared_layer()
    B, L, N, H = 2, 16, 3, 2
    w = torch.tensor([[1.0, 0.0, 0.25], [2.0, 1.0, 1.0]])
    keep = torch.ones(B, N, 8, 8, dtype=torch.bool)
    keep[1, 2, :4] = False                                                             # the upper half of reference 2 of entry 1
    proc.save_attention_mass = True
    with torch.no_grad():
        attn(x, **refs)
        m0 = proc.attention_mass.double()
        y = attn(x, ref_weights=w, ref_token_keep=keep, **refs)
        m1 = proc.attention_mass.double()
        row = bias_shim.calls[-1][1]
        assert tuple(row.shape) == (B, L + N * L)
        assert torch.equal(row[0, L + L: L + 2 * L], torch.full((L,), float("-inf"))) and row[0, L + 2 * L] == pytest.approx(math.log(0.25))
        assert row[1, L + 2 * L: L + 2 * L + 8].tolist() == [float("-inf")] * 8 and row[1, L + 2 * L + 8] == 0    # 8 x 8 -> 4 x 4: two token rows dropped
        assert float(m1[0, :, :, 2].abs().max()) == 0.0
        ratio = (m1[0, :, :, 3] / m1[0, :, :, 0]) / (m0[0, :, :, 3] / m0[0, :, :, 0])
        assert float((ratio - 0.25).abs().max()) < 1e-4                                 # mass_n / mass_self scales by w_n
        # one row per geometry and kwargs identity: a second layer call with the same tensors builds nothing
        built = sum(1 for c in bias_shim.calls if c[0] == "key_bias")
        attn(x, ref_weights=w, ref_token_keep=keep, **refs)
        assert sum(1 for c in bias_shim.calls if c[0] == "key_bias") == built
        w[0, 1] = 1.0                                                                   # an in-place change is seen (tensor version)
        attn(x, ref_weights=w, ref_token_keep=keep, **refs)
        assert sum(1 for c in bias_shim.calls if c[0] == "key_bias") == built + 1 and float(proc.attention_mass[0, :, :, 2].abs().max()) > 0
        # with an attention mask on top: the two add
        mask = torch.zeros(B, 1, L + N * L)
        mask[:, :, :4] = -10000.0
        attn(x, attention_mask=mask, ref_weights=w, **refs)
        both = bias_shim.calls[-1][1]
        assert torch.equal(both[:, :4], torch.full((B, 4), -10000.0)) and both[0, L + 2 * L] == pytest.approx(math.log(0.25))
        # ignored where there are no references: a non-shared layer, AttnProcessor
        n = len(bias_shim.calls)
        plain = Attention(query_dim=128, heads=2, dim_head=64, processor=SharedAttnProcessor(self_attn_idx=None))
        a = plain(x, ref_weights=w, ref_token_keep=keep, **refs)
        assert torch.equal(a, plain(x)) and len(bias_shim.calls) == n
        cap = Attention(query_dim=128, heads=2, dim_head=64, processor=AttnProcessor())
        assert torch.equal(cap(x, ref_weights=w, ref_token_keep=keep), cap(x)) and len(bias_shim.calls) == n
        # a plain layer takes a mask over its own keys (cross attention: padded text)
        enc = torch.randn(B, 7, 128)
        tm = torch.zeros(B, 1, 7)
        tm[:, :, 5:] = -10000.0
        torch.testing.assert_close(plain(x, encoder_hidden_states=enc, attention_mask=tm), plain(x, encoder_hidden_states=enc[:, :5]), atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(cap(x, encoder_hidden_states=enc, attention_mask=tm), cap(x, encoder_hidden_states=enc[:, :5]), atol=1e-5, rtol=1e-5)


# ---- golden vectors of the imported reference with an attention_mask (tests/golden/make_golden_mask.py) ----
def _mask_golden():
    import json
    import os
    import sys
    import numpy as np
    here = os.path.dirname(os.path.abspath(__file__))
    if os.path.join(here, "golden") not in sys.path:
        sys.path.insert(0, os.path.join(here, "golden"))
    import mask_inputs as MI
    z = np.load(os.path.join(here, "golden", "attn_mask_golden.npz"))
    return MI, z, json.loads(bytes(z["manifest"]).decode())


def test_helper_oracle_matches_the_reference_with_an_attention_mask():
    """the float64 helper oracle, driven through the projections, against the reference's own AttnProcessor /
    SharedAttnProcessor(self_attn_idx=None) outputs with a mask: 2e-5, the bound of tests/test_oracle_golden.py (the reference ran in fp32)"""
    import numpy as np
    from key_bias_oracle import biased_attention_np
    MI, z, manifest = _mask_golden()
    assert [(m["kind"], m["H"]) for m in manifest] == [("cross", 5), ("self", 2)] and all(m["processors_agree"] for m in manifest)
    for m in manifest:
        d = MI.build(m)
        assert abs(MI.checksum(d) - m["checksum"]) <= 1e-6 * abs(m["checksum"]), "seeded inputs drifted: regenerate the fixture"
        assert m["mask_effect"] > 0.1                                        # the mask matters on these inputs
        f = lambda t: t.numpy().astype(np.float64)
        src = f(d["encoder"]) if "encoder" in d else f(d["hidden"])
        q, k, v = f(d["hidden"]) @ f(d["wq"]).T, src @ f(d["wk"]).T, src @ f(d["wv"]).T
        core, _ = biased_attention_np(q, k, v, None, None, m["H"], 64 ** -0.5, f(d["mask"])[:, 0])
        out = core @ f(d["wo"]).T + f(d["bo"])
        ref = z[f"{m['id']}/out"].astype(np.float64)
        assert ref.shape == out[0].shape and np.abs(out[0] - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())
        if m["kind"] == "cross":
            assert d["mask"].shape[-1] == 77 and int((d["mask"] == -10000.0).sum()) == 20 and ref.shape == (128, 320)
