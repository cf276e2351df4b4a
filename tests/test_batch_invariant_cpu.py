"""Batch-invariant mode (ABI v10), what a CPU-only box can hold: the plan and the kernel choices are pure functions of the
per-item parameters.

``ir_shared_attn_plan`` / ``ir_shared_attn_kernel_name`` run the parameter checks of a launch (pointers are copied, never read)
and report the kernel and the cut of every work item into K/V-range pieces; ``ir_linear_kernel_for_ex`` reports the GEMM a
selector resolves to.  Held to: with ``IR_FLAG_BATCH_INVARIANT`` neither changes with the batch size, the workspace, the
process state (``IR_ATTN_W128``, the tuning hook) or - for the kernel and the cut - whether masses are asked for; the flag
refuses a tuning value; the processors' attribute reaches every processor of a UNet."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 2, 3, 8, 9, 16, 32, 64)
# (Lq, heads, n_refs) of every shared layer class: cfg1gpu / cfg2 at 512 px (N = 4), cfg4 (N = 8), cfg5 at 1024 px (N = 4)
CLASSES = sorted({(256, 20, 4), (1024, 10, 4), (4096, 5, 4), (256, 20, 8), (1024, 10, 8), (4096, 5, 8),
                  (1024, 20, 4), (4096, 10, 4), (16384, 5, 4)})

_BUF = (C.c_char * 4096)()   # host memory for the pointer fields: 64-byte aligned, never dereferenced


def _args(B, H, L, N, *, inc=True, adain=True, presc=True, valid=False, mass=False, ws=None, tuning=0, flag=True):
    from instantrestore_amd import _lib
    ptr = C.cast(C.byref(_BUF, 64 - C.addressof(_BUF) % 64), C.c_void_p)
    a = _lib.SharedAttnArgs()
    a.struct_size = C.sizeof(a)
    a.dtype, a.batch, a.heads, a.len_q, a.scale = 1, B, H, L, 0.125
    a.flags = (_lib.IR_FLAG_INCLUDE_SELF if inc else 0) | (_lib.IR_FLAG_Q_PRESCALED if presc else 0) | \
              (_lib.IR_FLAG_BATCH_INVARIANT if flag else 0)
    a.tuning = tuning
    C_ = H * 64
    a.q = a.out = ptr
    a.q_sb = a.o_sb = L * C_
    a.q_sl = a.o_sl = C_
    a.q_sh = a.o_sh = 64
    if inc:
        a.len_self = L
        a.k_self = a.v_self = ptr
        a.ks_sb = a.vs_sb = L * C_
        a.ks_sl = a.vs_sl = C_
        a.ks_sh = a.vs_sh = 64
    if N > 0:
        a.n_refs, a.len_ref = N, L
        a.k_ref = a.v_ref = ptr
        a.kr_sb = a.vr_sb = N * L * C_
        a.kr_sn = a.vr_sn = L * C_
        a.kr_sl = a.vr_sl = C_
        a.kr_sh = a.vr_sh = 64
    if adain and N > 0:
        a.adain_a = a.adain_b = ptr
    if valid:
        a.valid_refs = ptr
    if mass:
        a.seg_mass = ptr
    if ws is not None and ws > 0:
        a.workspace, a.workspace_bytes = ptr, int(ws)
    return a


def _plan(a):
    from instantrestore_amd import _lib
    lib = _lib.lib()
    p = _lib.SharedAttnPlan()
    p.struct_size = C.sizeof(p)
    rc = lib.ir_shared_attn_plan(C.byref(a), C.byref(p))
    assert rc == 0, lib.ir_last_error_string()
    return p


def _pure(p):
    """the per-item part of a plan: what must not change with the batch"""
    return (p.kernel, p.rows_per_item, p.items_per_batch, p.pieces_per_item)


def _name(a):
    from instantrestore_amd import _lib
    return _lib.lib().ir_shared_attn_kernel_name(C.byref(a)).decode()


def test_abi_version_is_10():
    from instantrestore_amd import _lib
    assert _lib.lib().ir_abi_version() == 10 == _lib.ABI_VERSION


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: f"L{c[0]}H{c[1]}N{c[2]}")
def test_plan_and_name_do_not_depend_on_the_batch_or_the_workspace(cls):
    from instantrestore_amd import _lib
    lib = _lib.lib()
    L, H, N = cls
    for inc, adain, presc, valid, mass in itertools.product((True, False), (True, False), (True, False), (False, True), (False, True)):
        kw = dict(inc=inc, adain=adain, presc=presc, valid=valid, mass=mass)
        ref = _plan(_args(1, H, L, N, **kw))
        ref_name = _name(_args(1, H, L, N, **kw))
        assert ref.pieces_per_item >= 1 and ref.items_per_batch == H * -(-L // ref.rows_per_item), (kw, _pure(ref))
        assert "batch-invariant" in ref_name
        per_entry = ref.workspace_bytes
        for B in BATCHES:
            need = lib.ir_shared_attn_workspace_bytes_for(C.byref(_args(B, H, L, N, **kw)))
            for ws in (None, need, per_entry, need // 3, 1 << 20):
                a = _args(B, H, L, N, ws=ws, **kw)
                p = _plan(a)
                assert _pure(p) == _pure(ref), (B, ws, kw, _pure(p), _pure(ref))
                assert _name(a) == ref_name, (B, ws, kw)
                assert p.workspace_bytes == need
                if p.pieces_per_item == 1:
                    assert need == 0 and p.batch_per_launch == B        # whole items: no scratch, one launch
                else:
                    # several launches of the same per-item plan when the workspace holds fewer entries; none fits: 0
                    have = 0 if ws is None else ws
                    per = p.batch_per_launch
                    if have >= need:
                        assert per == B
                    else:
                        assert 0 <= per < B
                        if per > 0:
                            assert lib.ir_shared_attn_workspace_bytes_for(C.byref(_args(per, H, L, N, **kw))) <= have
                        if per + 1 <= B:
                            assert lib.ir_shared_attn_workspace_bytes_for(C.byref(_args(per + 1, H, L, N, **kw))) > have
        # the masses size the pieces' partials, never the kernel or the cut
        other = _plan(_args(4, H, L, N, **dict(kw, mass=not mass)))
        assert _pure(other) == _pure(ref)
        assert _name(_args(4, H, L, N, **dict(kw, mass=not mass))) == ref_name


def test_a_workspace_too_small_for_one_entry_is_refused_with_the_bytes_named():
    """one entry's pieces do not fit: the call fails (IR_ERR_WORKSPACE) and names what it needs - it never takes another plan"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a = _args(8, 5, 4096, 4, ws=4096)
    assert _plan(a).pieces_per_item > 1 and _plan(a).batch_per_launch == 0
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == -4
    msg = lib.ir_last_error_string().decode()
    assert "batch-invariant" in msg and str(lib.ir_shared_attn_workspace_bytes_for(C.byref(_args(1, 5, 4096, 4)))) in msg


def test_the_plan_fills_the_chip_with_one_entry_at_every_layer_class():
    """k per layer class: ONE batch entry's items times their pieces cover the 256 CUs wherever the K/V walk allows pieces of 8 tiles"""
    for L, H, N in CLASSES:
        p = _plan(_args(1, H, L, N))
        ntiles = (1 + N) * L // 64
        assert p.items_per_batch * p.pieces_per_item >= 256 or p.pieces_per_item == max(1, ntiles // 8), (L, H, N, _pure(p))
        assert ntiles // p.pieces_per_item >= 8 or p.pieces_per_item == 1


def test_plain_attention_runs_whole_items_without_scratch():
    """the K/V-capture layers' self-attention (n_refs = 0, a batch of identities x references) and the cross attention over 77 text
    tokens run whole items in the mode: no pieces, no per-call scratch, at any batch"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    for L, H in ((4096, 5), (1024, 10), (256, 20), (16384, 5), (77, 20)):
        for presc in (True, False):
            ref = _pure(_plan(_args(1, H, L, 0, presc=presc)))
            assert ref[3] == 1, (L, H, ref)
            for B in BATCHES + (4 * 8, 4 * 16):
                a = _args(B, H, L, 0, presc=presc)
                assert _pure(_plan(a)) == ref and lib.ir_shared_attn_workspace_bytes_for(C.byref(a)) == 0


def test_ops_plan_wrapper_needs_no_device():
    """ops.shared_attention_plan builds the arguments from sizes alone (host only) and agrees with the C query"""
    from instantrestore_amd import ops
    for L, H, N in CLASSES:
        p = ops.shared_attention_plan(8, L, H, len_self=L, n_refs=N, len_ref=L, adain=True, q_prescaled=True, valid_refs=True)
        c = _plan(_args(8, H, L, N, valid=True))
        assert (p["kernel"], p["rows_per_item"], p["items_per_batch"], p["pieces_per_item"]) == _pure(c)
        assert p["batch_per_launch"] == 8 and p["workspace_bytes"] == c.workspace_bytes
    assert ops.shared_attention_plan(32, 4096, 5, len_self=4096, q_prescaled=True)["workspace_bytes"] == 0


def test_flag_with_a_tuning_value_is_rejected():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    for tuning in (11, 13, 16):
        a = _args(2, 10, 1024, 4, tuning=tuning)
        assert lib.ir_shared_attn_fwd(C.byref(a), None) == -1
        assert b"tuning" in lib.ir_last_error_string()
        assert _name(a) == ""
        p = _lib.SharedAttnPlan()
        p.struct_size = C.sizeof(p)
        assert lib.ir_shared_attn_plan(C.byref(a), C.byref(p)) == -1
    # the plan query answers for the flag only (the default dispatch plans per launch), and checks its own struct
    p = _lib.SharedAttnPlan()
    p.struct_size = C.sizeof(p)
    assert lib.ir_shared_attn_plan(C.byref(_args(2, 10, 1024, 4, flag=False)), C.byref(p)) == -1
    p.struct_size = 3
    assert lib.ir_shared_attn_plan(C.byref(_args(2, 10, 1024, 4)), C.byref(p)) == -1


_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, {tests!r})
sys.path.insert(0, {repo!r})
import test_batch_invariant_cpu as T
out = []
for (L, H, N) in T.CLASSES:
    for kw in (dict(), dict(valid=True, mass=True), dict(presc=False)):
        for B in (1, 8, 32):
            a = T._args(B, H, L, N, **kw)
            out.append([L, H, N, sorted(kw), B, list(T._pure(T._plan(a))), T._name(a)])
print(json.dumps(out))
"""


def _child(env_extra):
    env = dict(os.environ)
    env.pop("IR_ATTN_W128", None)
    env.pop("IR_ATTN_VARIANT", None)
    env.update(env_extra)
    code = _CHILD.format(tests=os.path.join(REPO, "tests"), repo=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_process_state_does_not_reach_the_plan():
    """IR_ATTN_W128 (read once per process: fresh children), the tuning hook's environment value and the forced split of the
    32-row kernel change the default dispatch, not the batch-invariant plan"""
    base = _child({})
    assert _child({"IR_ATTN_W128": "1"}) == base
    assert _child({"IR_ATTN_W128": "0"}) == base
    assert _child({"IR_ATTN_VARIANT": "16", "IR_ATTN_FORCE_SPLIT": "4"}) == base


def _projection_shapes():
    """(N, K, bias) of every projection of the SD-Turbo topology (unet_host.SD_TURBO): fused q/k/v, q alone, the out projection
    (with bias), k/v of the cross attention from the text states, and the fused k/v of a self-attention"""
    from instantrestore_amd.unet_host import SD_TURBO
    shapes = set()
    for c in SD_TURBO["block_out_channels"]:
        shapes |= {(3 * c, c, False), (c, c, False), (c, c, True), (2 * c, SD_TURBO["cross_attention_dim"], False), (2 * c, c, False),
                   (c, SD_TURBO["cross_attention_dim"], False)}
    return sorted(shapes)


def test_gemm_selector_is_one_kernel_per_shape_for_every_batch():
    from instantrestore_amd import _lib, ops
    lib = _lib.lib()
    K2 = ops.LIN_KERNELS["128x128k2"]
    tokens = (64, 256, 1024, 4096, 16384)
    for n, k, bias in _projection_shapes():
        got = {lib.ir_linear_kernel_for_ex(L * B, n, k, int(bias), _lib.IR_LIN_BATCH_INVARIANT) for L in tokens for B in BATCHES}
        assert len(got) == 1, (n, k, bias, got)
        kern = got.pop()
        assert kern > 0 and kern != K2, (n, k, bias, kern)
        assert ops.linear_kernel_for(4096, n, k, bias, batch_invariant=True) == kern
        # IR_LIN_AUTO through the _ex query is the automatic choice itself (which does read M)
        assert lib.ir_linear_kernel_for_ex(4096, n, k, int(bias), ops.LIN_AUTO) == lib.ir_linear_kernel_for(4096, n, k, int(bias))
    # the default choice at the top layer's fused q/k/v still reads the row count (unchanged: 128x64 at one identity)
    assert lib.ir_linear_kernel_for(4096, 960, 320, 0) != lib.ir_linear_kernel_for(8 * 4096, 960, 320, 0)
    assert lib.ir_linear_kernel_for_ex(4096, 960, 320, 0, 99) == -1


def test_linear_stats_ex_validates_without_a_gpu():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    ptr = C.cast(C.byref(_BUF, 64 - C.addressof(_BUF) % 64), C.c_void_p)
    # no statistics buffer / an unknown selector are refused before any launch
    assert lib.ir_linear_fwd_stats_ex(1, 0, 256, 960, 320, ptr, 320, ptr, 320, None, ptr, 960, 0, 1.0, 640, 320, None, 0,
                                      _lib.IR_LIN_BATCH_INVARIANT, None) == -1
    assert lib.ir_linear_fwd_stats_ex(1, 0, 256, 960, 320, ptr, 320, ptr, 320, None, ptr, 960, 0, 1.0, 640, 320, ptr, 1 << 20,
                                      3, None) == -1


def _unets():
    from instantrestore_amd import attn_processors as ap
    from instantrestore_amd.unet_host import AttnTopologyUNet
    from types import SimpleNamespace
    cfg = SimpleNamespace(use_adain=True, train_input=True, condition_on_face_embeds=False)
    main, ref = AttnTopologyUNet(), AttnTopologyUNet()
    ap.register_attention_processor(main, cfg)
    ap.register_attention_processor_kv_unet(ref)
    return ap, main, ref


def test_set_batch_invariant_reaches_every_processor():
    ap, main, ref = _unets()
    for unet in (main, ref):
        procs = [p for p in unet.attn_processors.values() if isinstance(p, (ap.SharedAttnProcessor, ap.AttnProcessor))]
        assert procs and all(p.batch_invariant is False for p in procs)     # off by default: today's path
        assert ap.set_batch_invariant(unet) == len(procs)
        assert all(p.batch_invariant is True for p in procs)
        assert ap.set_batch_invariant(unet, enabled=False) == len(procs)
        assert all(p.batch_invariant is False for p in procs)
    # kinds: the reference UNet's capture layers are AttnProcessors, the main UNet's SharedAttnProcessors
    assert any(isinstance(p, ap.AttnProcessor) for p in ref.attn_processors.values())
    # the constructors keep the reference's signatures; no parameter or buffer appears
    p = ap.SharedAttnProcessor()
    p.batch_invariant = True
    assert len(p.state_dict()) == 0


def test_mode_refuses_the_vendor_gemm_fallback():
    """where ``_linear`` would take ``F.linear`` (a shape or tensor this library's GEMMs do not cover) the mode raises: the
    vendor GEMM picks its kernel from the row count"""
    import torch
    from instantrestore_amd import attn_processors as ap
    x, w = torch.randn(4, 96), torch.randn(48, 96)
    assert torch.equal(ap._linear(x, w, None), torch.nn.functional.linear(x, w))      # off: unchanged
    with pytest.raises(NotImplementedError, match="batch-invariant"):
        ap._linear(x, w, None, True)


def test_mode_refuses_the_module_call_fallbacks():
    """projections left to the module call (nn.Linear -> F.linear: autograd enabled, unfoldable modules) raise in the mode too"""
    import torch
    from instantrestore_amd import attn_processors as ap
    from instantrestore_amd.attention import Attention
    attn = Attention(query_dim=128, heads=2, dim_head=64, processor=ap.SharedAttnProcessor())
    tokens = torch.randn(1, 4, 128)
    assert torch.is_grad_enabled()
    assert ap._project_out(attn, tokens).shape == (1, 4, 128)          # off: the module call, as before
    with pytest.raises(NotImplementedError, match="batch-invariant"):
        ap._project_out(attn, tokens, True)
