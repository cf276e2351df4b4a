"""Per-reference token counts of the fused attention (``ir_shared_attn_ragged_args`` / ``ops.shared_attention(ref_lens=)`` /
``ops.compact_refs``): everything that can be checked without a GPU - the fourth block's size rule and layout, the dispatch and
batch-invariant plan of a counted call, every refusal with its message, the ops' validation, the processors' host logic, the cache's
counts, and the one oracle identity every GPU comparison of tests/test_gpu_ref_lens.py rests on: ``-inf`` on the keys behind a count
IS the attention over the references truncated to their counts."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

INVALID, UNSUPPORTED = -1, -2
IR_TUNE = {"default": 0, "exactmax": 7, "pipe32": 10, "presc": 11, "w64x4": 12, "w64x8": 13, "earlyqk": 14, "w128": 16, "postcheck": 18}
BLOCKS = ("short", "table", "bias", "ragged")


def _args(lib_mod, *, block="ragged", lens=True, B=2, N=2, L=64, Lq=None, H=1, flags=1, valid=False, mass=False, adain=False, tuning=0,
          bias=False, rl_sb=None, tables=False):
    """a valid self + N-reference call on addresses that are never dereferenced (validation and planning precede any launch)"""
    a = {"short": lib_mod.SharedAttnArgs, "table": lib_mod.SharedAttnTableArgs, "bias": lib_mod.SharedAttnBiasArgs,
         "ragged": lib_mod.SharedAttnRaggedArgs}[block]()
    a.struct_size = C.sizeof(a)
    c = 64 * H
    Lq = L if Lq is None else Lq
    inc = bool(flags & 1)
    a.dtype, a.batch, a.heads, a.len_q, a.len_self, a.flags, a.scale, a.tuning = 1, B, H, Lq, (L if inc else 0), flags, 0.125, tuning
    a.q = a.out = 4096
    a.q_sb = a.o_sb = Lq * c
    a.q_sl = a.o_sl = c
    a.q_sh = a.o_sh = 64
    if inc:
        a.k_self = a.v_self = 4096
        a.ks_sb = a.vs_sb = L * c
        a.ks_sl = a.vs_sl = c
        a.ks_sh = a.vs_sh = 64
    a.n_refs, a.len_ref = N, (L if N else 0)
    if N:
        a.kr_sl = a.vr_sl = c
        a.kr_sh = a.vr_sh = 64
        if tables:
            a.k_ref_table = a.v_ref_table = 4096
        else:
            a.k_ref = a.v_ref = 4096
            a.kr_sb = a.vr_sb = N * L * c
            a.kr_sn = a.vr_sn = L * c
    if valid:
        a.valid_refs = 4096
    if mass:
        a.seg_mass = 4096
    if adain:
        a.adain_a = a.adain_b = 4096
    if block == "ragged" and bias:
        a.key_bias = 4100
        a.kb_sb = (1 + N) * L
    if block == "ragged" and lens:
        a.ref_lens = 4100                      # a 4-byte quantity: no 16-byte alignment
        a.rl_sb = N if rl_sb is None else rl_sb
    return a


def _plan(lib_mod, a):
    p = lib_mod.SharedAttnPlan()
    p.struct_size = C.sizeof(p)
    rc = lib_mod.lib().ir_shared_attn_plan(C.byref(a), C.byref(p))
    return (rc,) + tuple(getattr(p, n) for n, _ in lib_mod.SharedAttnPlan._fields_[1:])


def test_abi_stays_10_four_block_sizes_are_taken_and_the_fields_lie_where_the_header_puts_them():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION
    old, tab, bia, new = (C.sizeof(t) for t in (_lib.SharedAttnArgs, _lib.SharedAttnTableArgs, _lib.SharedAttnBiasArgs, _lib.SharedAttnRaggedArgs))
    assert tab == old + 16 and bia == tab + 24 and new == bia + 16
    assert [f[0] for f in _lib.SharedAttnRaggedArgs._fields_] == ["ref_lens", "rl_sb"]
    assert (_lib.SharedAttnRaggedArgs.ref_lens.offset, _lib.SharedAttnRaggedArgs.rl_sb.offset) == (bia, bia + 8)
    assert _lib.SharedAttnRaggedArgs.key_bias.offset == tab and _lib.SharedAttnRaggedArgs.k_ref_table.offset == old
    # the sizes tests/test_key_bias_cpu.py pins as invalid stay invalid: the new size is none of them
    pinned = (7, old + 8, tab + 8, old - 8, bia + 8, bia - 8, tab + 16)
    assert new not in pinned
    for block in BLOCKS:
        assert lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, block=block))) != b"", block
    a = _args(_lib)
    for bad in pinned + (new + 8, new - 4, new + 16, 0):
        a.struct_size = bad
        assert lib.ir_shared_attn_kernel_name(C.byref(a)) == b"" and b"ABI mismatch" in lib.ir_last_error_string(), bad
        assert lib.ir_shared_attn_fwd(C.byref(a), None) == INVALID
        assert lib.ir_shared_attn_workspace_bytes_for(C.byref(a)) == 0
        assert _plan(_lib, a)[0] == INVALID


def test_the_header_declares_the_block_and_the_compaction_as_the_binding_mirrors_them():
    from instantrestore_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "instantrestore_hip.h")).read()
    body = hdr[hdr.index("typedef struct ir_shared_attn_ragged_args {"):hdr.index("} ir_shared_attn_ragged_args;")]
    assert body.index("ir_shared_attn_bias_args b;") < body.index("const int32_t* ref_lens;") < body.index("int64_t rl_sb;")
    assert "#define IR_ABI_VERSION 10" in hdr
    assert "ref_lens given or not" in hdr                       # the batch-invariant contract lists it as a per-entry parameter
    assert issubclass(_lib.SharedAttnRaggedArgs, _lib.SharedAttnBiasArgs)
    assert "int ir_compact_ref_tokens(" in hdr and "ir_compact_ref_tokens" in _lib.SYMBOLS
    decl = hdr[hdr.index("int ir_compact_ref_tokens("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == len(_lib.SYMBOLS["ir_compact_ref_tokens"][1]) == 29
    assert hasattr(_lib.lib(), "ir_compact_ref_tokens")


@pytest.mark.parametrize("len_q", [256, 1024, 4096])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescaledq"])
def test_a_counted_call_names_and_plans_the_32_row_kernel_and_null_counts_are_the_dense_call(len_q, presc):
    from instantrestore_amd import _lib
    lib = _lib.lib()
    for bi in (False, True):
        for mass, adain, tables in ((False, False, False), (True, True, False), (False, True, True)):
            flags = 1 | (2 if presc else 0) | (8 if bi else 0)
            kw = dict(B=8, N=4, L=len_q, H=5, flags=flags, mass=mass, adain=adain, tables=tables)
            name = lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, **kw)))
            assert name.startswith(b"shared_attn_fwd_pipe_kernel<4 waves") and b"ragged refs" in name, name
            assert (b"pre-scaled Q" in name) == presc and (b"early QK" in name) == (not presc), name
            dense = _args(_lib, block="table" if tables else "short", **kw)
            null = _args(_lib, block="ragged", lens=False, **kw)
            dname = lib.ir_shared_attn_kernel_name(C.byref(dense))
            assert lib.ir_shared_attn_kernel_name(C.byref(null)) == dname != b"" and b"ragged refs" not in dname
            assert lib.ir_shared_attn_workspace_bytes_for(C.byref(null)) == lib.ir_shared_attn_workspace_bytes_for(C.byref(dense))
            if len_q == 4096:
                assert b"pipe_kernel" not in dname, dname           # today's kernel without counts
            if bi:
                pr, pn, pd = _plan(_lib, _args(_lib, **kw)), _plan(_lib, null), _plan(_lib, dense)
                assert pr[0] == 0 and pr[1] == (IR_TUNE["presc"] if presc else IR_TUNE["earlyqk"]) and pr[2] == 128, pr
                assert pr[3] == 5 * (len_q // 128)
                assert pn == pd and pd[0] == 0
                assert lib.ir_shared_attn_workspace_bytes_for(C.byref(_args(_lib, **kw))) == pr[-1]
                # the pieces are planned for full references: capacity tiles, the rule of the uncounted 32-row plan
                want = max(1, min(-(-256 // pr[3]), 5 * (len_q // 64) // 8))
                assert pr[4] == want, (pr, want)
                # the plan of a counted call does not read the batch size
                assert _plan(_lib, _args(_lib, **dict(kw, B=1)))[1:5] == pr[1:5]
    # the tunings a counted call may name: the default and the two 32-row forms
    for tune, form in ((IR_TUNE["presc"], b"pre-scaled Q"), (IR_TUNE["earlyqk"], b"early QK")):
        if presc and tune == IR_TUNE["earlyqk"]:
            continue                                               # that form does not take a pre-scaled q
        name = lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, B=8, N=4, L=len_q, H=5, flags=1 | (2 if presc else 0), tuning=tune)))
        assert form in name and b"ragged refs" in name, name


def test_every_refusal_of_a_counted_call_names_its_reason():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.ir_last_error_string()
    a = _args(_lib, valid=True)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"valid_refs" in err() and b"absent" in err() and b"zero-filled" in err()
    assert lib.ir_shared_attn_kernel_name(C.byref(a)) == b"" and _plan(_lib, _args(_lib, valid=True, flags=9))[0] == UNSUPPORTED
    a = _args(_lib, bias=True)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"key_bias" in err() and b"follow-up" in err()
    assert lib.ir_shared_attn_workspace_bytes_for(C.byref(a)) == 0
    a = _args(_lib, N=0)
    a.ref_lens, a.rl_sb = 4100, 0
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"n_refs == 0" in err()
    for name, tune in IR_TUNE.items():
        presc = name in ("w128", "postcheck")
        a = _args(_lib, tuning=tune, L=4096, flags=1 | (2 if presc else 0))
        if name in ("default", "presc", "earlyqk"):      # (named only: these addresses must never reach a launch)
            assert lib.ir_shared_attn_kernel_name(C.byref(a)).startswith(b"shared_attn_fwd_pipe_kernel"), name
        else:
            assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"ref_lens" in err() and b"tuning" in err(), (name, err())
    a = _args(_lib)
    a.ref_lens = 4098
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"ref_lens must be 4-byte aligned" in err()
    a = _args(_lib, N=3, rl_sb=2)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == INVALID and b"rl_sb" in err()
    assert lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, N=3, rl_sb=7))) != b""        # rows of a wider buffer
    # the read-out entry points would walk the tails
    calls = {"ir_attn_probs": lambda a: lib.ir_attn_probs(C.byref(a), 4096, None),
             "ir_attn_probs_ex": lambda a: lib.ir_attn_probs_ex(C.byref(a), 4096, 0, None),
             "ir_attn_segment_mass": lambda a: lib.ir_attn_segment_mass(C.byref(a), 4096, None),
             "ir_attn_rows": lambda a: lib.ir_attn_rows(C.byref(a), 4096, 1, 0, 4096, None)}
    for what, call in calls.items():
        a = _args(_lib)
        a.lse = 4096
        assert call(a) == UNSUPPORTED and b"ref_lens" in err() and b"walk the tails" in err(), (what, err())
    # the compaction: aliasing, strides, sizes - before any launch
    cr = lambda **kw: lib.ir_compact_ref_tokens(*[kw.get(k, d) for k, d in (
        ("dtype", 1), ("B", 2), ("H", 2), ("N", 3), ("L", 40), ("k_in", 1 << 20), ("a", 15360), ("b", 5120), ("c", 128), ("d", 64),
        ("v_in", 2 << 20), ("e", 15360), ("f", 5120), ("g", 128), ("h", 64), ("keep", 4097), ("k_out", 3 << 20), ("i", 15360), ("j", 5120),
        ("k", 128), ("l", 64), ("v_out", 4 << 20), ("m", 15360), ("n", 5120), ("o", 128), ("p", 64), ("lens", 4100), ("rl_sb", 3), ("s", None))])
    # (each tensor spans 2 * 15360 * 2 = 61440 bytes; the defaults lie 1 MiB apart)
    assert cr(k_out=1 << 20) == INVALID and b"aliasing" in err()                       # the same base
    assert cr(v_out=2 << 20) == INVALID and b"aliasing" in err()
    assert cr(v_out=3 << 20) == INVALID and b"aliasing" in err()                       # the two outputs on each other
    assert cr(k_out=(1 << 20) + 2 * 5120) == INVALID and b"aliasing" in err()          # a view into the input, one reference further on
    assert cr(v_out=(2 << 20) - 256) == INVALID and b"aliasing" in err()               # one row in front of an input: the tail runs into it
    assert cr(k_out=(1 << 20) + 61440 - 16) == INVALID and b"aliasing" in err()        # the last 16 bytes of an input
    assert cr(v_out=(3 << 20) + 128) == INVALID and b"aliasing" in err()               # interleaved with the other output
    assert cr(rl_sb=2) == INVALID and b"rl_sb" in err()
    assert cr(lens=4098) == UNSUPPORTED and cr(k=100) == UNSUPPORTED and cr(dtype=2) == UNSUPPORTED and cr(L=0) == INVALID and cr(keep=None) == INVALID


def test_ops_reject_counts_of_the_wrong_kind_before_any_launch():
    from instantrestore_amd import ops
    q = torch.zeros(2, 8, 128, dtype=torch.bfloat16)
    r = torch.zeros(2, 3, 8, 128, dtype=torch.bfloat16)
    good = torch.zeros(2, 3, dtype=torch.int32)
    for bad, match in ((torch.zeros(2, 3, dtype=torch.int64), "int32"), (torch.zeros(2, 4, dtype=torch.int32), "shape"),
                       (torch.zeros(3, dtype=torch.int32), "shape"), (torch.zeros(3, 2, dtype=torch.int32).t(), "contiguous"), ([[1, 2, 3]] * 2, "int32")):
        with pytest.raises(ValueError, match=match):
            ops._check_ref_lens(bad, q, r)
    ops._check_ref_lens(good, q, r)
    ops._check_ref_lens(torch.zeros(2, 8, dtype=torch.int32)[:, :3], q, r)          # rows of a wider buffer
    with pytest.raises(ValueError, match="without references"):
        ops._check_ref_lens(good, q, None)
    with pytest.raises(ValueError, match="valid_refs"):
        ops._check_ref_lens(good, q, r, valid_refs=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="follow-up"):
        ops._check_ref_lens(good, q, r, key_bias=torch.zeros(2, 32))
    with pytest.raises(ValueError, match="int32"):                                 # _fill_args validates first, before any pointer is taken
        ops._fill_args(q, q, q, r, r, 2, 0.125, True, None, None, None, ref_lens=good.long())
    with pytest.raises(RuntimeError, match="CPU"):                                 # no CPU path, counts or not
        ops.shared_attention(q, q, q, r, r, heads=2, scale=0.125, ref_lens=good)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.compact_refs(r, r, torch.ones(2, 3, 8, dtype=torch.bool), heads=2)
    for fn in (ops.shared_attention, ops.time_shared_attention, ops.shared_attention_kernel_name, ops.shared_attention_plan):
        assert "ref_lens" in inspect.signature(fn).parameters, fn.__name__
    for fn in (ops.attn_probs, ops.attn_segment_mass, ops.attn_rows):
        assert "ref_lens" not in inspect.signature(fn).parameters, fn.__name__
    assert "absent" in ops.shared_attention.__doc__ and "valid_refs" in ops.shared_attention.__doc__
    plan = ops.shared_attention_plan(8, 4096, 5, len_self=4096, n_refs=4, len_ref=4096, q_prescaled=True, ref_lens=True)
    assert plan["kernel"] == 11 and plan["rows_per_item"] == 128
    assert ops.shared_attention_plan(8, 4096, 5, len_self=4096, n_refs=4, len_ref=4096, q_prescaled=True)["rows_per_item"] == 512
    # the keep map of compact_refs pools exactly as ops.key_bias pools ref_token_keep
    g = torch.Generator().manual_seed(5)
    keep = torch.rand(1, 2, 64, 64, generator=g) < 0.5
    for side in (16, 32, 64):
        row = ops.key_bias(1, 0, 2, side * side, False, ref_token_keep=keep)
        assert torch.equal(ops._pool_keep(keep, 1, 2, side * side), (row == 0).view(1, 2, side * side))
    with pytest.raises(ValueError, match="bool"):
        ops._pool_keep(torch.ones(1, 2, 16), 1, 2, 16)
    with pytest.raises(ValueError, match="shape"):
        ops._pool_keep(torch.ones(1, 2, 15, dtype=torch.bool), 1, 2, 16)


# ---- the oracle identity --------------------------------------------------------------------------------------------------------
def test_minus_inf_on_the_tails_is_the_attention_over_the_truncated_references():
    """``biased_attention_np`` on capacity-sized references with ``-inf`` on every key ``t >= c`` equals, to 1e-12, the plain oracle run
    per entry on references truncated to their counts (no AdaIN; counts include 0 and ``len_ref``).  The tails hold other data in the
    second run: they do not exist."""
    from key_bias_oracle import biased_attention_np
    from oracle.shared_attn_oracle import batch_to_head_dim_np, head_to_batch_dim_np
    B, H, Lq, Ls, N, cap = 2, 2, 24, 9, 3, 20
    counts = [[20, 0, 7], [1, 13, 20]]
    rng = np.random.default_rng(0)
    q, k, v = rng.standard_normal((B, Lq, H * 64)), rng.standard_normal((B, Ls, H * 64)), rng.standard_normal((B, Ls, H * 64))
    rk, rv = rng.standard_normal((B, N, cap, H * 64)), rng.standard_normal((B, N, cap, H * 64))
    for inc in (True, False):
        ls = Ls if inc else 0
        bias = np.zeros((B, ls + N * cap))
        for b in range(B):
            for n in range(N):
                bias[b, ls + n * cap + counts[b][n]: ls + (n + 1) * cap] = -np.inf
        out, lse, mass = biased_attention_np(q, k, v, rk, rv, H, 0.125, bias, train_input=inc, seg_lens=([Ls] if inc else []) + [cap] * N)
        rk2, rv2 = rk.copy(), rv.copy()
        for b in range(B):
            for n in range(N):
                rk2[b, n, counts[b][n]:] = 1e3 * rng.standard_normal((cap - counts[b][n], H * 64))
                rv2[b, n, counts[b][n]:] = 1e3
        out2, lse2, mass2 = biased_attention_np(q, k, v, rk2, rv2, H, 0.125, bias, train_input=inc, seg_lens=([Ls] if inc else []) + [cap] * N)
        assert np.array_equal(out, out2) and np.array_equal(lse, lse2) and np.array_equal(mass, mass2)
        for b in range(B):
            ek = np.concatenate(([k[b]] if inc else []) + [rk[b, n, :counts[b][n]] for n in range(N)])
            ev = np.concatenate(([v[b]] if inc else []) + [rv[b, n, :counts[b][n]] for n in range(N)])
            qh, kh, vh = (head_to_batch_dim_np(t[None], H) for t in (q[b], ek, ev))
            s = np.matmul(qh, kh.transpose(0, 2, 1)) * 0.125
            m = s.max(-1, keepdims=True)
            e = np.exp(s - m)
            p = e / e.sum(-1, keepdims=True)
            ref = batch_to_head_dim_np(np.matmul(p, vh), H)[0]
            assert np.abs(out[b] - ref).max() <= 1e-12
            assert np.abs(lse[b] - (m + np.log(e.sum(-1, keepdims=True)))[..., 0]).max() <= 1e-12
            edges = np.cumsum([0] + ([Ls] if inc else []) + counts[b])
            for sgm in range(len(edges) - 1):
                assert np.abs(mass[b, :, :, sgm] - p[..., edges[sgm]:edges[sgm + 1]].sum(-1)).max() <= 1e-12
            assert np.all(mass[b, :, :, (1 if inc else 0) + counts[b].index(0)] == 0.0) if 0 in counts[b] else True


# ---- the processors' host logic (CPU stand-in, as tests/test_key_bias_cpu.py) -----------------------------------------------------
class _CountShim:
    """tests/oracle_ops.py with a ``shared_attention`` that takes ``ref_lens``: the float64 helper oracle with ``-inf`` behind the counts"""

    def __init__(self):
        import oracle_ops
        self._o = oracle_ops
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._o, name)

    def key_bias(self, *a, **kw):
        from instantrestore_amd import ops
        return ops.key_bias(*a, **kw)

    def adain_stats_cached(self, v_self, content_mean, content_std, *, heads, eps=1e-5):
        B, L, _ = v_self.shape
        v = v_self.double().view(B, L, heads, 64)
        a = (v.std(dim=1) + eps).unsqueeze(1) / (content_std.double() + eps)
        b = v.mean(dim=1).unsqueeze(1) - content_mean.double() * a
        return a.float().contiguous(), b.float().contiguous()

    def shared_attention(self, q, k_self, v_self, ref_k=None, ref_v=None, *, ref_lens=None, return_mass=False, key_bias=None, **kw):
        self.calls.append(("shared_attention", None if ref_lens is None else ref_lens.clone(), kw.get("adain"), ref_v))
        if ref_lens is None:
            assert key_bias is None
            return self._o.shared_attention(q, k_self, v_self, ref_k, ref_v, return_mass=return_mass, **kw)
        from key_bias_oracle import biased_attention_np
        assert ref_lens.dtype == torch.int32 and tuple(ref_lens.shape) == tuple(ref_k.shape[:2]) and key_bias is None
        assert not kw.get("return_lse") and kw.get("valid_refs") is None
        f = lambda t: None if t is None else t.detach().double().numpy()
        rvn = f(ref_v)
        if kw.get("adain") is not None:
            a, b = (f(t).reshape(rvn.shape[0], rvn.shape[1], 1, -1) for t in kw["adain"])
            rvn = rvn * a + b
        inc = kw.get("include_self", True)
        B, N, cap = ref_k.shape[:3]
        ls = k_self.shape[1] if inc else 0
        bias = np.zeros((B, ls + N * cap))
        for b in range(B):
            for n in range(N):
                bias[b, ls + n * cap + min(max(int(ref_lens[b, n]), 0), cap): ls + (n + 1) * cap] = -np.inf
        out, _, mass = biased_attention_np(f(q), f(k_self), f(v_self), f(ref_k), rvn, kw["heads"], kw["scale"], bias,
                                           train_input=inc, seg_lens=([ls] if inc else []) + [cap] * N)
        out = torch.from_numpy(out).to(q.dtype)
        return (out, torch.from_numpy(mass).float()) if return_mass else out


@pytest.fixture()
def count_shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    shim = _CountShim()
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


def test_processor_hands_the_counts_to_the_shared_layer_only_and_forbidden_combinations_raise(count_shim):
    from face_replace.models.attn_processors import AttnProcessor, SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    attn, proc, x, refs = _shared_layer()
    B, L, N, H = 2, 16, 3, 2
    lens = torch.tensor([[16, 0, 5], [1, 16, 9]], dtype=torch.int32)
    with torch.no_grad():
        plain = attn(x, **refs)
        assert count_shim.calls[-1][1] is None
        y = attn(x, ref_lens=[lens], **refs)
        assert torch.equal(count_shim.calls[-1][1], lens)
        assert not torch.equal(y, plain)
        assert torch.equal(attn(x, ref_lens=[None], **refs), plain) and torch.equal(attn(x, ref_lens=None, **refs), plain)
        full = attn(x, ref_lens=[torch.full((B, N), L, dtype=torch.int32)], **refs)
        torch.testing.assert_close(full, plain, atol=1e-6, rtol=1e-6)
        # counted equals truncated: what lies behind a count does not exist
        junk = {"ref_keys": [refs["ref_keys"][0].clone()], "ref_values": [refs["ref_values"][0].clone()]}
        for b in range(B):
            for n in range(N):
                junk["ref_keys"][0][b, n, int(lens[b, n]):] = 1e4
                junk["ref_values"][0][b, n, int(lens[b, n]):] = -3e4     # (finite: the float64 stand-in multiplies by an exact 0)
        assert torch.equal(attn(x, ref_lens=[lens], **junk), y)
        # the masses honour the counts
        proc.save_attention_mass = True
        attn(x, ref_lens=[lens], **refs)
        m = proc.attention_mass
        assert tuple(m.shape) == (B, H, L, 1 + N) and float(m[0, :, :, 2].abs().max()) == 0.0 and float((m.sum(-1) - 1).abs().max()) < 1e-5
        proc.save_attention_mass = False
        # forbidden combinations, each with its reason
        with pytest.raises(ValueError, match="zero-filled"):
            attn(x, ref_lens=[lens], ref_valid=torch.tensor([3, 2], dtype=torch.int32), **refs)
        with pytest.raises(NotImplementedError, match="follow-up"):
            attn(x, ref_lens=[lens], attention_mask=torch.zeros(B, 1, L + N * L), **refs)
        with pytest.raises(NotImplementedError, match="key bias"):
            attn(x, ref_lens=[lens], ref_weights=torch.ones(B, N), **refs)
        with pytest.raises(NotImplementedError, match="key bias"):
            attn(x, ref_lens=[lens], ref_token_keep=torch.ones(B, N, L, dtype=torch.bool), **refs)
        proc.save_self_attentions = True
        with pytest.raises(NotImplementedError, match="tails"):
            attn(x, ref_lens=[lens], **refs)
        proc.save_self_attentions = False
        proc.attention_rows_index = torch.tensor([0, 3])
        with pytest.raises(NotImplementedError, match="tails"):
            attn(x, ref_lens=[lens], **refs)
        proc.attention_rows_index = None
        # ref_token_keep alone keeps running the bias path
        n = len(count_shim.calls)
        with pytest.raises(AssertionError):          # (the stand-in takes no bias: reaching it with one shows the path)
            attn(x, ref_token_keep=torch.ones(B, N, L, dtype=torch.bool) & (torch.arange(L) < 8), **refs)
        assert len(count_shim.calls) == n + 1 and count_shim.calls[-1][1] is None
        # ignored where there are no references: a non-shared layer, AttnProcessor
        n = len(count_shim.calls)
        nonshared = Attention(query_dim=128, heads=2, dim_head=64, processor=SharedAttnProcessor(self_attn_idx=None))
        assert torch.equal(nonshared(x, ref_lens=[lens], **refs), nonshared(x)) and all(c[1] is None for c in count_shim.calls[n:])
        cap = Attention(query_dim=128, heads=2, dim_head=64, processor=AttnProcessor())
        assert torch.equal(cap(x, ref_lens=[lens]), cap(x))


def test_processor_with_adain_needs_the_statistics_of_the_full_reference(count_shim):
    attn, proc, x, refs = _shared_layer(adain=True)
    lens = torch.tensor([[16, 0, 5], [1, 16, 9]], dtype=torch.int32)
    rv = refs["ref_values"][0]
    H = 2
    v5 = rv.view(2, 3, 16, H, 64)
    stats = (v5.mean(dim=2), v5.std(dim=2))                       # content statistics over every token of the full reference
    with torch.no_grad():
        with pytest.raises(ValueError, match="ref_stats"):
            attn(x, ref_lens=[lens], **refs)
        y = attn(x, ref_lens=[lens], ref_stats=[stats], **refs)
        assert torch.isfinite(y).all() and torch.equal(count_shim.calls[-1][1], lens)
        # the affine is the one the uncounted call gets from the same statistics
        attn(x, ref_stats=[stats], **refs)
        (_, l0, a0, v0), (_, l1, a1, v1) = count_shim.calls[-2], count_shim.calls[-1]
        assert l1 is None and torch.equal(a0[0], a1[0]) and torch.equal(a0[1], a1[1]) and v0 is v1


def test_cache_tables_carry_per_layer_counts():
    from instantrestore_amd.kv_cache import ReferenceKVCache
    cache = ReferenceKVCache()
    mk = lambda n, seed: ([torch.full((1, n, 8, 64), float(seed)), torch.full((1, n, 4, 64), float(seed))],
                          [torch.full((1, n, 8, 64), float(-seed)), torch.full((1, n, 4, 64), float(-seed))])
    cache.get_or_compute("a", lambda: mk(3, 1))
    cache.get_or_compute("b", lambda: mk(2, 2))
    cache.get_or_compute("c", lambda: mk(3, 3))
    cache.set_ref_lens("a", [[8, 0, 5], None])
    cache.set_ref_lens("c", [torch.tensor([1, 2, 3], dtype=torch.int32), [4, 0, 2]])
    for bad in ([[9, 0, 0], None], [[1, 2], None], [[1, 2, 3]]):
        with pytest.raises(ValueError, match="set_ref_lens"):
            cache.set_ref_lens("a", bad)
    tables = cache.assemble_tables(["a", "b"])
    assert len(tables) == 4                                        # the return value keeps its form: the counts ride on the key list
    keys = tables[0]
    assert [t.dtype for t in keys.ref_lens] == [torch.int32] * 2 and [tuple(t.shape) for t in keys.ref_lens] == [(2, 3)] * 2
    assert keys.ref_lens[0].tolist() == [[8, 0, 5], [8, 8, 0]]     # own counts; the capacity for an identity without; 0 for a missing slot
    assert keys.ref_lens[1].tolist() == [[4, 4, 4], [4, 4, 0]]
    # the counts are views into the set's one pointer block (addresses, valid counts, token counts): one upload fills them all
    lo, hi = keys.buf.data_ptr(), keys.buf.data_ptr() + keys.buf.numel() * 8
    assert all(lo <= t.data_ptr() and t.data_ptr() + t.numel() * 4 <= hi and t.is_contiguous() for t in keys.ref_lens)
    assert keys.buf.numel() == 2 * 2 * 2 * 3 + 1 + (2 * 2 * 3) // 2 and keys.valid_all.tolist() == [3, 2]
    with pytest.raises(ValueError, match="key list"):              # a copy of the list has lost the block: refused, not skipped
        cache.refill_tables((list(keys),) + tuple(tables[1:]), ["a", "b"])
    cache.set_ref_lens("b", [[7, 6], [1, 0]])                      # counts set after assembling reach the device with the next refill
    assert keys.ref_lens[0].tolist() == [[8, 0, 5], [8, 8, 0]]
    cache.refill_tables(tables, ["a", "b"])
    assert keys.ref_lens[0].tolist() == [[8, 0, 5], [7, 6, 0]] and keys.ref_lens[1].tolist() == [[4, 4, 4], [1, 0, 0]]
    cache.set_ref_lens("b", None)
    cache.refill_tables(tables, ["a", "b"])
    addr = [t.data_ptr() for t in keys.ref_lens]
    cache.refill_tables(tables, ["c", "a"])
    assert [t.data_ptr() for t in keys.ref_lens] == addr           # in place: a captured step follows
    assert keys.ref_lens[0].tolist() == [[1, 2, 3], [8, 0, 5]] and keys.ref_lens[1].tolist() == [[4, 0, 2], [4, 4, 4]]
    cache.set_ref_lens("a", None)
    cache.refill_tables(tables, ["a", "b"])
    assert keys.ref_lens[0].tolist() == [[8, 8, 8], [8, 8, 0]]
    cache.invalidate("c")
    cache.get_or_compute("c", lambda: mk(3, 3))
    assert cache.assemble_tables(["c"])[0].ref_lens[0].tolist() == [[8, 8, 8]]   # a recomputed entry is full again
