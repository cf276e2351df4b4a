"""Region-restricted attention (``ir_shared_attn_region_args`` / ``ops.shared_attention(q_allow=, key_region=)`` /
``ops.region_masks`` / ``attn_maps.token_labels`` / the processors' ``region_labels``): everything that can be checked without a GPU -
the fifth block's size rule and layout, the dispatch and batch-invariant plan of a region call, every refusal with its message, the
arithmetic of the mask builder and of the label sampling, the processors' cache and raises, and the float64 oracle itself."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

INVALID, UNSUPPORTED = -1, -2
IR_TUNE = {"default": 0, "exactmax": 7, "pipe32": 10, "presc": 11, "w64x4": 12, "w64x8": 13, "earlyqk": 14, "w128": 16, "postcheck": 18}
BLOCKS = ("short", "table", "bias", "ragged", "region")


def _args(lib_mod, *, block="region", regions=True, B=2, N=2, L=64, Lq=None, H=1, flags=1, valid=False, mass=False, adain=False, tuning=0,
          bias=False, lens=False, tables=False, qa_sb=None, kg_sb=None):
    """a valid self + N-reference call on addresses that are never dereferenced (validation and planning precede any launch)"""
    a = {"short": lib_mod.SharedAttnArgs, "table": lib_mod.SharedAttnTableArgs, "bias": lib_mod.SharedAttnBiasArgs,
         "ragged": lib_mod.SharedAttnRaggedArgs, "region": lib_mod.SharedAttnRegionArgs}[block]()
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
    lkv = (L if inc else 0) + N * L
    if bias:
        a.key_bias = 4100
        a.kb_sb = lkv
    if lens:
        a.ref_lens = 4100
        a.rl_sb = N
    if block == "region" and regions:
        a.q_allow = 4100                       # 4-byte quantities: no 16-byte alignment
        a.key_region = 4104
        a.qa_sb = Lq if qa_sb is None else qa_sb
        a.kg_sb = lkv if kg_sb is None else kg_sb
    return a


def _plan(lib_mod, a):
    p = lib_mod.SharedAttnPlan()
    p.struct_size = C.sizeof(p)
    rc = lib_mod.lib().ir_shared_attn_plan(C.byref(a), C.byref(p))
    return (rc,) + tuple(getattr(p, n) for n, _ in lib_mod.SharedAttnPlan._fields_[1:])


def test_abi_stays_10_five_block_sizes_are_taken_and_the_fields_lie_where_the_header_puts_them():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION
    old, tab, bia, rag, new = (C.sizeof(t) for t in (_lib.SharedAttnArgs, _lib.SharedAttnTableArgs, _lib.SharedAttnBiasArgs,
                                                     _lib.SharedAttnRaggedArgs, _lib.SharedAttnRegionArgs))
    assert tab == old + 16 and bia == tab + 24 and rag == bia + 16 and new == rag + 32 == old + 88
    R = _lib.SharedAttnRegionArgs
    assert [f[0] for f in R._fields_] == ["q_allow", "qa_sb", "key_region", "kg_sb"]
    assert (R.q_allow.offset, R.qa_sb.offset, R.key_region.offset, R.kg_sb.offset) == (rag, rag + 8, rag + 16, rag + 24)
    assert R.ref_lens.offset == bia and R.key_bias.offset == tab and R.k_ref_table.offset == old and _lib.IR_REGION_MAX == 32
    # every size tests/test_key_bias_cpu.py and tests/test_ref_lens_cpu.py pin as invalid stays invalid: the new size is none of them
    pinned = (7, old + 8, tab + 8, old - 8, bia + 8, bia - 8, tab + 16, rag + 8, rag - 4, rag + 16, 0)
    assert new not in pinned and {p - old for p in pinned if p > old} == {8, 24, 32, 48, 64, 72, 52}
    for block in BLOCKS:
        assert lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, block=block))) != b"", block
    a = _args(_lib)
    for bad in pinned + (new + 8, new - 8, new - 4, new + 16, new + 32):
        a.struct_size = bad
        assert lib.ir_shared_attn_kernel_name(C.byref(a)) == b"" and b"ABI mismatch" in lib.ir_last_error_string(), bad
        assert lib.ir_shared_attn_fwd(C.byref(a), None) == INVALID
        assert lib.ir_shared_attn_workspace_bytes_for(C.byref(a)) == 0
        assert _plan(_lib, a)[0] == INVALID


def test_the_header_declares_the_block_as_the_binding_mirrors_it():
    from instantrestore_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "instantrestore_hip.h")).read()
    body = hdr[hdr.index("typedef struct ir_shared_attn_region_args {"):hdr.index("} ir_shared_attn_region_args;")]
    assert body.index("ir_shared_attn_ragged_args r;") < body.index("const uint32_t* q_allow;") < body.index("int64_t qa_sb;") \
        < body.index("const int32_t* key_region;") < body.index("int64_t kg_sb;")
    assert "#define IR_REGION_MAX 32" in hdr and "#define IR_ABI_VERSION 10" in hdr
    assert "regions together with a bias" in hdr and "follow-up" in hdr      # the combinations left for later are named
    assert issubclass(_lib.SharedAttnRegionArgs, _lib.SharedAttnRaggedArgs)
    assert "SharedAttnRegionArgs" not in _lib.SYMBOLS and len([s for s in _lib.SYMBOLS if "region" in s]) == 0   # no new entry point


@pytest.mark.parametrize("len_q", [256, 1024, 4096])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescaledq"])
def test_a_region_call_names_and_plans_the_32_row_kernel_and_null_arrays_are_the_shorter_call(len_q, presc):
    from instantrestore_amd import _lib
    lib = _lib.lib()
    for bi in (False, True):
        for mass, adain in ((False, False), (True, True)):
            flags = 1 | (2 if presc else 0) | (8 if bi else 0)
            kw = dict(B=8, N=4, L=len_q, H=5, flags=flags, mass=mass, adain=adain)
            name = lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, **kw)))
            assert name.startswith(b"shared_attn_fwd_pipe_kernel<4 waves") and b"regions" in name and b"key bias" not in name, name
            assert (b"pre-scaled Q" in name) == presc and (b"early QK" in name) == (not presc), name
            dense = _args(_lib, block="short", **kw)
            null = _args(_lib, block="region", regions=False, **kw)
            dname = lib.ir_shared_attn_kernel_name(C.byref(dense))
            assert lib.ir_shared_attn_kernel_name(C.byref(null)) == dname != b"" and b"regions" not in dname
            assert lib.ir_shared_attn_workspace_bytes_for(C.byref(null)) == lib.ir_shared_attn_workspace_bytes_for(C.byref(dense))
            # a region block whose own arrays are NULL is the call of the block it extends: a bias call, a counted call
            for other, word in (("bias", b"key bias"), ("lens", b"ragged refs")):
                inner = lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, block="region", regions=False, **dict(kw, **{other: True}))))
                assert word in inner and b"regions" not in inner, inner
            if len_q == 4096:
                assert b"pipe_kernel" not in dname, dname           # today's kernel without regions
            if bi:
                pr, pn, pd = _plan(_lib, _args(_lib, **kw)), _plan(_lib, null), _plan(_lib, dense)
                pbias = _plan(_lib, _args(_lib, block="bias", bias=True, **kw))
                assert pr[0] == 0 and pr[1] == (IR_TUNE["presc"] if presc else IR_TUNE["earlyqk"]) and pr[2] == 128, pr
                assert pr[3] == 5 * (len_q // 128)
                assert pr == pbias                                   # the cut of the bias form: the same per-item parameters
                assert pn == pd and pd[0] == 0
                assert lib.ir_shared_attn_workspace_bytes_for(C.byref(_args(_lib, **kw))) == pr[-1]
                assert _plan(_lib, _args(_lib, **dict(kw, B=1)))[1:5] == pr[1:5]     # the plan does not read the batch size


def test_plain_attention_odd_lengths_tables_and_strides():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.ir_last_error_string()
    a = _args(_lib, N=0, L=77, Lq=128, H=5)                              # n_refs = 0
    assert b"regions" in lib.ir_shared_attn_kernel_name(C.byref(a))
    a = _args(_lib, N=3, L=72, Lq=200, H=2, flags=0, qa_sb=1000, kg_sb=217)  # references only, ragged segments, wider rows
    assert b"regions" in lib.ir_shared_attn_kernel_name(C.byref(a))
    assert b"regions" in lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, tables=True)))
    for field in ("q_allow", "key_region"):
        a = _args(_lib)
        setattr(a, field, 4098)
        assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"4-byte aligned" in err(), field
    a = _args(_lib, L=64, Lq=128, qa_sb=127)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == INVALID and b"qa_sb" in err() and b"len_q" in err()
    a = _args(_lib, N=2, L=64, kg_sb=3 * 64 - 1)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == INVALID and b"kg_sb" in err() and b"Lkv" in err()
    assert lib.ir_shared_attn_kernel_name(C.byref(_args(_lib, N=2, L=64, kg_sb=3 * 64))) != b""
    for only in ("q_allow", "key_region"):                               # exactly one NULL
        a = _args(_lib)
        setattr(a, "key_region" if only == "q_allow" else "q_allow", None)
        assert lib.ir_shared_attn_fwd(C.byref(a), None) == INVALID and b"both" in err(), only
        assert lib.ir_shared_attn_kernel_name(C.byref(a)) == b"" and _plan(_lib, a)[0] == INVALID


def test_every_refusal_of_a_region_call_names_its_reason():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.ir_last_error_string()
    a = _args(_lib, bias=True)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"key_bias" in err() and b"follow-up" in err() and b"q_allow" in err()
    a = _args(_lib, lens=True)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"ref_lens" in err() and b"follow-up" in err() and b"q_allow" in err()
    a = _args(_lib, valid=True)
    assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"valid_refs" in err() and b"q_allow" in err()
    assert lib.ir_shared_attn_kernel_name(C.byref(a)) == b"" and lib.ir_shared_attn_workspace_bytes_for(C.byref(a)) == 0
    for name, tune in IR_TUNE.items():
        presc = name in ("w128", "postcheck")
        a = _args(_lib, tuning=tune, L=4096, flags=1 | (2 if presc else 0))
        if name in ("default", "presc", "earlyqk"):      # (named only: these addresses must never reach a launch)
            got = lib.ir_shared_attn_kernel_name(C.byref(a))
            assert got.startswith(b"shared_attn_fwd_pipe_kernel") and b"regions" in got, name
            assert (b"pre-scaled Q" in got) == (name == "presc")
        else:
            assert lib.ir_shared_attn_fwd(C.byref(a), None) == UNSUPPORTED and b"REGION" in err() and b"tuning" in err(), (name, err())
    # every read-out entry point: their exp(s - lse) would count the pairs the forward left out
    p = 4096
    calls = {"ir_attn_probs": lambda a: lib.ir_attn_probs(C.byref(a), p, None),
             "ir_attn_probs_ex": lambda a: lib.ir_attn_probs_ex(C.byref(a), p, 0, None),
             "ir_attn_segment_mass": lambda a: lib.ir_attn_segment_mass(C.byref(a), p, None),
             "ir_attn_rows": lambda a: lib.ir_attn_rows(C.byref(a), p, 1, 0, p, None),
             "ir_attn_match": lambda a: lib.ir_attn_match(C.byref(a), p, 1, 0, p, p, None),
             "ir_attn_topk": lambda a: lib.ir_attn_topk(C.byref(a), p, 1, 2, 0, p, p, None),
             "ir_attn_transfer": lambda a: lib.ir_attn_transfer(C.byref(a), p, 3 * 64, 1, 1, p, 1, 0, p, p, None),
             "ir_attn_received": lambda a: lib.ir_attn_received(C.byref(a), None, 0, 0, 1, 0, p, None),
             "ir_attn_key_match": lambda a: lib.ir_attn_key_match(C.byref(a), 0, p, p, None)}
    for what, call in calls.items():
        a = _args(_lib)
        a.lse = p
        assert call(a) == UNSUPPORTED and b"q_allow" in err() and b"do not take regions" in err(), (what, err())


def test_ops_reject_regions_of_the_wrong_kind_before_any_launch():
    from instantrestore_amd import ops
    q = torch.zeros(2, 8, 128, dtype=torch.bfloat16)
    r = torch.zeros(2, 2, 8, 128, dtype=torch.bfloat16)
    lkv = 8 + 2 * 8
    qa, kr = torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, lkv, dtype=torch.int32)
    ops._check_regions(qa, kr, q, lkv)
    ops._check_regions(qa.view(torch.uint32), kr, q, lkv)                               # uint32 storage of the words
    ops._check_regions(torch.zeros(2, 12, dtype=torch.int32)[:, :8], torch.zeros(2, lkv + 3, dtype=torch.int32)[:, :lkv], q, lkv)   # rows of wider buffers
    for bad_qa, bad_kr, match in ((None, kr, "together"), (qa, None, "together"), (qa.long(), kr, "q_allow must be"), (qa.float(), kr, "q_allow must be"),
                                  (qa, kr.long(), "key_region must be"), (qa, kr.view(torch.uint32), "key_region must be"),
                                  (torch.zeros(2, 9, dtype=torch.int32), kr, r"\(B, Lq\)"), (qa, torch.zeros(2, lkv + 1, dtype=torch.int32), r"\(B, Lkv\)"),
                                  (torch.zeros(3, 8, dtype=torch.int32), kr, r"\(B, Lq\)"), (torch.zeros(8, 2, dtype=torch.int32).t(), kr, "contiguous"),
                                  (qa, torch.zeros(lkv, 2, dtype=torch.int32).t(), "contiguous")):
        with pytest.raises(ValueError, match=match):
            ops._check_regions(bad_qa, bad_kr, q, lkv)
    with pytest.raises(ValueError, match="key_bias.*follow-up"):
        ops._check_regions(qa, kr, q, lkv, key_bias=torch.zeros(2, lkv))
    with pytest.raises(ValueError, match="ref_lens.*follow-up"):
        ops._check_regions(qa, kr, q, lkv, ref_lens=torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CPU"):                                      # no CPU path, regions or not
        ops.shared_attention(q, q, q, r, r, heads=2, scale=0.125, q_allow=qa, key_region=kr)
    for fn in (ops.shared_attention, ops.time_shared_attention, ops.shared_attention_kernel_name):
        assert {"q_allow", "key_region"} <= set(inspect.signature(fn).parameters), fn.__name__
    assert "regions" in inspect.signature(ops.shared_attention_plan).parameters
    for fn in (ops.attn_probs, ops.attn_segment_mass, ops.attn_rows, ops.attn_match, ops.attn_topk, ops.attn_transfer, ops.attn_received, ops.attn_key_match):
        assert "q_allow" not in inspect.signature(fn).parameters, fn.__name__
    plan = ops.shared_attention_plan(8, 4096, 5, len_self=4096, n_refs=4, len_ref=4096, q_prescaled=True, regions=True)
    assert plan["kernel"] == 11 and plan["rows_per_item"] == 128
    assert plan == ops.shared_attention_plan(8, 4096, 5, len_self=4096, n_refs=4, len_ref=4096, q_prescaled=True, key_bias=True)
    assert ops.shared_attention_plan(8, 4096, 5, len_self=4096, n_refs=4, len_ref=4096, q_prescaled=True)["rows_per_item"] == 512


# ---- ops.region_masks against a plain-Python restatement ----
def _masks_py(q_labels, key_labels, allow, self_len, self_free):
    """the rule, one pair at a time"""
    allow = [[bool(x) for x in row] for row in allow] if isinstance(allow[0], (list, tuple)) else \
        [[bool((int(w) >> d) & 1) for d in range(len(allow))] for w in allow]
    C_ = len(allow)
    free = self_free and self_len > 0
    qa, kr = [], []
    for row in q_labels:
        out = []
        for c in row:
            w = 0
            if 0 <= c < C_:
                for d in range(C_):
                    if allow[c][d]:
                        w |= 1 << d
            if free:
                w |= 1 << 31
            out.append(w)
        qa.append(out)
    for row in key_labels:
        kr.append([31 if (free and j < self_len) else (d if 0 <= d < C_ else -1) for j, d in enumerate(row)])
    return qa, kr


@pytest.mark.parametrize("self_free", [True, False], ids=["selffree", "selfruled"])
@pytest.mark.parametrize("form", ["matrix", "bitmasks"])
def test_region_masks_against_a_plain_python_restatement(self_free, form):
    from instantrestore_amd import ops
    from region_oracle import allowed_np
    g = torch.Generator().manual_seed(11 + 2 * self_free + (form == "matrix"))
    B, Lq, Ls, Lr, N, C_ = 2, 9, 9, 7, 2, 5
    ql = torch.randint(-2, C_ + 2, (B, Lq), generator=g)                  # out-of-range labels on both sides
    kl = torch.randint(-2, C_ + 2, (B, Ls + N * Lr), generator=g)
    m = torch.rand(C_, C_, generator=g) < 0.5
    m[3] = False                                                          # a class that may attend nothing
    allow = m if form == "matrix" else torch.tensor([sum(1 << d for d in range(C_) if m[c, d]) for c in range(C_)])
    qa, kr = ops.region_masks(ql, kl, allow, self_len=Ls, self_free=self_free)
    assert qa.dtype == torch.int32 and kr.dtype == torch.int32 and tuple(qa.shape) == (B, Lq) and tuple(kr.shape) == (B, Ls + N * Lr)
    assert qa.is_contiguous() and kr.is_contiguous()
    want_qa, want_kr = _masks_py(ql.tolist(), kl.tolist(), m.tolist() if form == "matrix" else allow.tolist(), Ls, self_free)
    assert (qa.to(torch.int64) & 0xFFFFFFFF).tolist() == want_qa and kr.tolist() == want_kr
    # what the pair means, pair by pair: allowed iff the classes say so (or the key is a self key under self_free)
    al = allowed_np(qa.numpy(), kr.numpy())[:, 0]
    for b in range(B):
        for i in range(Lq):
            for j in range(Ls + N * Lr):
                c, d = int(ql[b, i]), int(kl[b, j])
                want = (self_free and j < Ls) or (0 <= c < C_ and 0 <= d < C_ and bool(m[c, d]))
                assert bool(al[b, i, j]) == want, (b, i, j, c, d)
    # integer dtypes of any width; self_len = 0 means there is nothing to free
    qa2, kr2 = ops.region_masks(ql.to(torch.int16), kl.to(torch.uint8 if int(kl.min()) >= 0 else torch.int8), allow, self_len=Ls, self_free=self_free)
    assert torch.equal(qa2, qa) and torch.equal(kr2, kr)
    qa0, kr0 = ops.region_masks(ql, kl, allow, self_len=0, self_free=self_free)
    assert int((qa0.to(torch.int64) >> 31 & 1).sum()) == 0 and int((kr0 == 31).sum()) == 0


def test_region_masks_limits_and_bad_inputs():
    from instantrestore_amd import ops
    ql, kl = torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 6, dtype=torch.int64)
    full = torch.ones(32, 32, dtype=torch.bool)
    qa, kr = ops.region_masks(ql, kl, full, self_len=0)                   # 32 classes fit without the self rule: every bit, sign bit included
    assert qa.tolist() == [[-1] * 4] and kr.tolist() == [[0] * 6]
    ops.region_masks(ql, kl, full, self_len=2, self_free=False)
    with pytest.raises(ValueError, match="self_free takes region 31"):
        ops.region_masks(ql, kl, full, self_len=2)
    ops.region_masks(ql, kl, full[:31, :31], self_len=2)
    # a bitmask rule drops the bits of classes that do not exist
    qa, _ = ops.region_masks(ql, kl, torch.tensor([0xFF, 1, 1]), self_len=0)
    assert qa.tolist() == [[7] * 4]
    for kw, match in ((dict(allow=torch.ones(3, 4, dtype=torch.bool)), "bool matrix"), (dict(allow=torch.ones(3, 3)), "bool matrix"),
                      (dict(allow=torch.ones(3)), "bitmasks"), (dict(allow=torch.ones(33, 33, dtype=torch.bool)), "classes"),
                      (dict(allow=full[:2, :2], self_len=7), "self_len"), (dict(allow=full[:2, :2], q_labels=torch.zeros(1, 4)), "integer"),
                      (dict(allow=full[:2, :2], key_labels=torch.zeros(2, 6, dtype=torch.int64)), "batch")):
        args = dict(q_labels=ql, key_labels=kl, self_len=0)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.region_masks(args.pop("q_labels"), args.pop("key_labels"), args.pop("allow"), **args)


# ---- attn_maps.token_labels ----
@pytest.mark.parametrize("hpx,wpx,side", [(8, 8, 8), (16, 16, 4), (64, 48, 8), (10, 7, 4), (3, 5, 8), (512, 512, 16)])
def test_token_labels_samples_the_pixel_at_every_token_centre(hpx, wpx, side):
    from instantrestore_amd import attn_maps
    g = torch.Generator().manual_seed(hpx * 100 + wpx + side)
    img = torch.randint(0, 19, (2, hpx, wpx), generator=g, dtype=torch.int32)
    got = attn_maps.token_labels(img, side)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, side * side)
    for b in range(2):
        for ty in range(side):
            for tx in range(side):
                py, px = ((2 * ty + 1) * hpx) // (2 * side), ((2 * tx + 1) * wpx) // (2 * side)
                assert 0 <= py < hpx and 0 <= px < wpx
                assert int(got[b, ty * side + tx]) == int(img[b, py, px]), (b, ty, tx)
    if hpx == side and wpx == side:
        assert torch.equal(got, img.reshape(2, -1))                       # the picture itself
    if hpx % side == 0:
        k = hpx // side
        assert all(((2 * ty + 1) * hpx) // (2 * side) == ty * k + k // 2 for ty in range(side))
    refs = torch.stack([img, img.flip(1)], dim=1)                          # (B, N, Hpx, Wpx): the references laid end to end
    both = attn_maps.token_labels(refs, side)
    assert tuple(both.shape) == (2, 2 * side * side) and torch.equal(both[:, :side * side], got)
    assert torch.equal(both[:, side * side:], attn_maps.token_labels(img.flip(1), side))


def test_token_labels_rejects_what_is_no_label_picture():
    from instantrestore_amd import attn_maps
    for bad in (torch.zeros(2, 8, 8), torch.zeros(8, 8, dtype=torch.int64), torch.zeros(2, 8, 8, dtype=torch.bool), torch.zeros(1, 2, 3, 8, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="label_image"):
            attn_maps.token_labels(bad, 4)
    with pytest.raises(ValueError, match=">= 1"):
        attn_maps.token_labels(torch.zeros(2, 8, 8, dtype=torch.int64), 0)


# ---- the float64 oracle itself ----
def _oracle_inputs(seed, B=2, H=2, Lq=11, Ls=11, N=2, Lr=7):
    g = np.random.default_rng(seed)
    c = 64 * H
    return (g.standard_normal((B, Lq, c)), g.standard_normal((B, Ls, c)), g.standard_normal((B, Ls, c)),
            g.standard_normal((B, N, Lr, c)), g.standard_normal((B, N, Lr, c)))


@pytest.mark.parametrize("train_input", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("use_adain", [False, True], ids=["plain", "adain"])
def test_oracle_with_everything_allowed_is_the_unbiased_oracle(train_input, use_adain):
    from key_bias_oracle import biased_attention_np
    from region_oracle import masked_attention_np, region_attention_np
    q, ks, vs, rk, rv = _oracle_inputs(1)
    H, segs = 2, ([11] if train_input else []) + [7, 7]
    lkv = sum(segs)
    want = biased_attention_np(q, ks, vs, rk, rv, H, 0.125, None, use_adain=use_adain, train_input=train_input, seg_lens=segs)
    for got in (masked_attention_np(q, ks, vs, rk, rv, H, 0.125, None, use_adain=use_adain, train_input=train_input, seg_lens=segs),
                masked_attention_np(q, ks, vs, rk, rv, H, 0.125, np.ones((2, 1, 11, lkv), dtype=bool), use_adain=use_adain, train_input=train_input, seg_lens=segs),
                region_attention_np(q, ks, vs, rk, rv, H, 0.125, np.full((2, 11), -1, dtype=np.int32), np.arange(2 * lkv, dtype=np.int32).reshape(2, lkv) % 32,
                                    use_adain=use_adain, train_input=train_input, seg_lens=segs)):
        for a, b in zip(got, want):
            assert np.array_equal(a, b)


def test_oracle_with_one_word_for_all_rows_is_the_key_bias_oracle_with_minus_inf():
    from key_bias_oracle import biased_attention_np
    from region_oracle import allowed_np, region_attention_np
    q, ks, vs, rk, rv = _oracle_inputs(2)
    H, segs, lkv = 2, [11, 7, 7], 25
    g = np.random.default_rng(5)
    kr = g.integers(-1, 6, size=(2, lkv)).astype(np.int32)
    kr[0, 3] = 32                                                          # nobody's, both ways
    word = np.array([0b001011, 0], dtype=np.int64)                         # entry 1: nothing at all - every row dead
    qa = np.repeat(word[:, None], 11, axis=1).astype(np.int32)
    bias = np.where(allowed_np(qa, kr)[:, 0, 0], 0.0, -np.inf)             # (B, Lkv): the same mask with no query axis
    assert bias[0, 3] == -np.inf and np.isfinite(bias[0]).any() and not np.isfinite(bias[1]).any()
    got = region_attention_np(q, ks, vs, rk, rv, H, 0.125, qa, kr, seg_lens=segs)
    want = biased_attention_np(q, ks, vs, rk, rv, H, 0.125, bias, seg_lens=segs)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    out, lse, mass = got
    assert np.all(out[1] == 0) and np.all(lse[1] == -np.inf) and np.all(mass[1] == 0)      # the dead-row rule
    assert np.isfinite(out).all() and np.isfinite(mass).all() and np.allclose(mass[0].sum(-1), 1)


def test_oracle_rows_differ_and_uint32_storage_means_the_same_bits():
    from region_oracle import allowed_np, region_attention_np
    q, ks, vs, rk, rv = _oracle_inputs(3)
    kr = (np.arange(25) % 3).astype(np.int32)[None].repeat(2, axis=0)
    kr[:, :11] = 31
    qa = np.zeros((2, 11), dtype=np.int64)
    qa[:, ::2], qa[:, 1::2] = (1 << 31) | 1, 0b110
    as_i32 = qa.astype(np.uint32).view(np.int32)
    assert (as_i32 < 0).any() and np.array_equal(allowed_np(as_i32, kr), allowed_np(qa.astype(np.uint32), kr))
    out, lse, mass = region_attention_np(q, ks, vs, rk, rv, 2, 0.125, as_i32, kr, seg_lens=[11, 7, 7])
    assert np.all(mass[:, :, 1::2, 0] == 0) and np.all(mass[:, :, ::2, 0] > 0)     # odd rows may not see their own picture
    # a row's result is the plain softmax over its allowed keys
    al = allowed_np(as_i32, kr)[0, 0, 1]
    ek = np.concatenate([ks[0], rk[0, 0], rk[0, 1]])[:, :64]
    ev = np.concatenate([vs[0], rv[0, 0], rv[0, 1]])[:, :64]
    s = (ek[al] @ q[0, 1, :64]) * 0.125
    p = np.exp(s - s.max())
    assert np.allclose(out[0, 1, :64], (p / p.sum()) @ ev[al], atol=1e-12) and np.isclose(lse[0, 0, 1], s.max() + np.log(p.sum()))


# ---- the processors (CPU stand-ins, as tests/test_key_bias_cpu.py) ----
class _RegionShim:
    """tests/oracle_ops.py with a ``shared_attention`` that takes ``q_allow`` / ``key_region`` (the float64 region oracle) and the real,
    plain-torch ``ops.region_masks``; every other entry point is the oracle stand-in's"""

    def __init__(self):
        import oracle_ops
        self._o = oracle_ops
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._o, name)

    def region_masks(self, *a, **kw):
        from instantrestore_amd import ops
        self.calls.append(("region_masks", tuple(a[1].shape), kw))
        return ops.region_masks(*a, **kw)

    def key_bias(self, *a, **kw):
        from instantrestore_amd import ops
        return ops.key_bias(*a, **kw)

    def shared_attention(self, q, k_self, v_self, ref_k=None, ref_v=None, *, q_allow=None, key_region=None, return_mass=False, key_bias=None,
                         ref_lens=None, **kw):
        self.calls.append(("shared_attention", q_allow, key_region, kw.get("valid_refs")))
        if q_allow is None:
            assert key_region is None and key_bias is None and ref_lens is None
            return self._o.shared_attention(q, k_self, v_self, ref_k, ref_v, return_mass=return_mass, **kw)
        from region_oracle import region_attention_np
        assert q_allow.dtype == torch.int32 and key_region.dtype == torch.int32 and key_bias is None and ref_lens is None
        assert not kw.get("return_lse")
        f = lambda t: None if t is None else t.detach().double().numpy()
        rvn = f(ref_v)
        if kw.get("adain") is not None:
            a, b = (f(t).reshape(rvn.shape[0], rvn.shape[1], 1, -1) for t in kw["adain"])
            rvn = rvn * a + b
        inc = kw.get("include_self", True)
        segs = ([k_self.shape[1]] if inc else []) + [ref_k.shape[2]] * ref_k.shape[1]
        out, _, mass = region_attention_np(f(q), f(k_self), f(v_self), f(ref_k), rvn, kw["heads"], kw["scale"], q_allow.numpy(), key_region.numpy(),
                                           train_input=inc, seg_lens=segs)
        out = torch.from_numpy(out).to(q.dtype)
        return (out, torch.from_numpy(mass).float()) if return_mass else out


@pytest.fixture()
def region_shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    shim = _RegionShim()
    monkeypatch.setattr(ap, "_ops", shim)
    ap._BIAS_ROWS.clear()
    ap._REGION_PAIRS.clear()
    return shim


def _shared_layer(heads=2, L=16, N=3, adain=False, train_input=True):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    g = torch.Generator().manual_seed(3)
    proc = SharedAttnProcessor(self_attn_idx=0, use_adain=adain, train_input=train_input)
    attn = Attention(query_dim=64 * heads, heads=heads, dim_head=64, processor=proc)
    x = torch.randn(2, L, 64 * heads, generator=g)
    rk, rv = torch.randn(2, N, L, 64 * heads, generator=g), torch.randn(2, N, L, 64 * heads, generator=g)
    return attn, proc, x, {"ref_keys": [rk], "ref_values": [rv]}


def _label_pictures(B=2, N=3, px=8):
    """three classes in vertical bands; reference 1 is class 2 everywhere, and class 2 is a class nobody may attend"""
    band = (torch.arange(px) * 2 // px).view(1, 1, px).expand(B, px, px).contiguous()          # classes 0 | 1 by column
    refs = band[:, None].expand(B, N, px, px).contiguous()
    refs[:, 1] = 2
    allow = torch.eye(3, dtype=torch.bool)
    allow[2, 2] = False
    return band, refs, allow


def test_processor_builds_the_pair_once_per_geometry_and_the_masses_follow_the_rule(region_shim):
    from instantrestore_amd import attn_maps, ops
    attn, proc, x, refs = _shared_layer()
    B, L, N, H, side = 2, 16, 3, 2, 4
    qpic, rpic, allow = _label_pictures()
    proc.save_attention_mass = True
    with torch.no_grad():
        plain = attn(x, **refs)
        m_plain = proc.attention_mass.clone()
        y = attn(x, region_labels=(qpic, rpic), region_allow=allow, **refs)
        _, qa, kr, _ = region_shim.calls[-1]
        # what reached the kernel is ops.region_masks of the pictures sampled at the token centres, self keys = the query labels, self free
        ql = attn_maps.token_labels(qpic, side)
        want = ops.region_masks(ql, torch.cat([ql, attn_maps.token_labels(rpic, side)], dim=1), allow, self_len=L, self_free=True)
        assert torch.equal(qa, want[0]) and torch.equal(kr, want[1]) and tuple(qa.shape) == (B, L) and tuple(kr.shape) == (B, L + N * L)
        m = proc.attention_mass
        assert tuple(m.shape) == (B, H, L, 1 + N)
        assert float(m[:, :, :, 2].abs().max()) == 0.0                    # reference 1: labels no query class may attend - mass exactly 0
        assert float(m_plain[:, :, :, 2].min()) > 0 and float((m.sum(-1) - 1).abs().max()) < 1e-5
        assert float(m[:, :, :, 0].min()) > 0 and float(m[:, :, :, 1].min()) > 0 and not torch.equal(y, plain)
        # cached by tensor identity and version: the same kwargs build nothing, an in-place change is seen, new tensors build
        built = lambda: sum(1 for c in region_shim.calls if c[0] == "region_masks")
        n0 = built()
        assert n0 == 1
        assert torch.equal(attn(x, region_labels=(qpic, rpic), region_allow=allow, **refs), y) and built() == n0
        assert region_shim.calls[-1][1] is qa                             # the very tensors: a captured call keeps reading them
        rpic[:, 1] = 1
        attn(x, region_labels=(qpic, rpic), region_allow=allow, **refs)
        assert built() == n0 + 1 and float(proc.attention_mass[:, :, :, 2].max()) > 0      # its class-1 rows see reference 1 now
        allow[0, 0] = False
        attn(x, region_labels=(qpic, rpic), region_allow=allow, **refs)
        assert built() == n0 + 2
        attn(x, region_labels=(qpic.clone(), rpic), region_allow=allow, **refs)
        assert built() == n0 + 3
        # per-token labels of another square grid are sampled like a picture; of this layer's grid they are taken as they are
        tok_q, tok_r = attn_maps.token_labels(qpic, side), attn_maps.token_labels(rpic, side).view(B, N, L)
        y_tok = attn(x, region_labels=(tok_q, tok_r), region_allow=allow, **refs)
        assert torch.equal(y_tok, attn(x, region_labels=(qpic, rpic), region_allow=allow, **refs))
        # bounded
        import instantrestore_amd.attn_processors as ap
        for _ in range(2 * ap._REGION_PAIRS_MAX):
            attn(x, region_labels=(qpic.clone(), rpic), region_allow=allow, **refs)
        assert len(ap._REGION_PAIRS) <= ap._REGION_PAIRS_MAX
        # a rule that allows nothing leaves every token its own picture (self free)
        none = torch.zeros(3, 3, dtype=torch.bool)
        attn(x, region_labels=(qpic, rpic), region_allow=none, **refs)
        assert float((proc.attention_mass[:, :, :, 0] - 1).abs().max()) < 1e-6 and region_shim.calls[-2][2]["self_free"] is True


def test_processor_without_the_self_segment_and_with_adain(region_shim):
    attn, proc, x, refs = _shared_layer(train_input=False, adain=True)
    qpic, rpic, allow = _label_pictures()
    proc.save_attention_mass = True
    with torch.no_grad():
        attn(x, region_labels=(qpic, rpic), region_allow=allow, **refs)
    _, qa, kr, _ = region_shim.calls[-1]
    assert tuple(kr.shape) == (2, 3 * 16) and int((kr == 31).sum()) == 0 and int((qa.to(torch.int64) >> 31 & 1).sum()) == 0
    m = proc.attention_mass
    assert tuple(m.shape) == (2, 2, 16, 3) and float(m[:, :, :, 1].abs().max()) == 0.0 and float((m.sum(-1) - 1).abs().max()) < 1e-5


def test_processor_refuses_the_combinations_that_are_not_built_before_anything_is_launched(region_shim, monkeypatch):
    import instantrestore_amd.attn_processors as ap
    attn, proc, x, refs = _shared_layer()
    B, L, N = 2, 16, 3
    qpic, rpic, allow = _label_pictures()
    rg = dict(region_labels=(qpic, rpic), region_allow=allow)
    launched = []
    real = ap._project_qkv
    monkeypatch.setattr(ap, "_project_qkv", lambda *a, **kw: (launched.append(1), real(*a, **kw))[1])
    with torch.no_grad():
        for kw in (dict(attention_mask=torch.zeros(B, 1, L + N * L)), dict(ref_weights=torch.ones(B, N)),
                   dict(ref_token_keep=torch.ones(B, N, L, dtype=torch.bool))):
            with pytest.raises(NotImplementedError, match="key bias.*follow-up"):
                attn(x, **rg, **kw, **refs)
        with pytest.raises(NotImplementedError, match="ref_lens.*follow-up"):
            attn(x, ref_lens=[torch.full((B, N), L, dtype=torch.int32)], **rg, **refs)
        with pytest.raises(ValueError, match="region_allow"):
            attn(x, region_labels=(qpic, rpic), **refs)
        for name, value in (("save_self_attentions", True), ("attention_rows_index", torch.tensor([0, 3])), ("attention_match_index", "all"),
                            ("attention_topk_index", "all"), ("attention_transfer_payload", torch.zeros(L + N * L, 2)),
                            ("attention_received_weights", "ones"), ("attention_key_match_reduce", "head_mean")):
            old = getattr(proc, name)
            setattr(proc, name, value)
            with pytest.raises(NotImplementedError, match=f"{name}.*do not take regions"):
                attn(x, **rg, **refs)
            setattr(proc, name, old)
        assert launched == [] and not any(c[0] == "shared_attention" for c in region_shim.calls)
        # the per-query attention mask stays refused, and says where to go
        with pytest.raises(NotImplementedError, match="per-query.*region_labels"):
            attn(x, attention_mask=torch.zeros(B, L, L + N * L), **refs)
        # ref_valid goes through: ops drops the promise on a dense call
        attn(x, ref_valid=torch.tensor([3, 2], dtype=torch.int32), **rg, **refs)
        assert region_shim.calls[-1][3] is not None and region_shim.calls[-1][1] is not None
        with pytest.raises(ValueError, match="pair"):
            attn(x, region_labels=qpic, region_allow=allow, **refs)
        with pytest.raises(ValueError, match="batch of 2"):
            attn(x, region_labels=(qpic[:1], rpic), region_allow=allow, **refs)


def test_layers_without_references_accept_and_ignore_the_kwargs(region_shim):
    from face_replace.models.attn_processors import AttnProcessor, FaceIDAttnProcessor, SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    _, _, x, refs = _shared_layer()
    qpic, rpic, allow = _label_pictures()
    rg = dict(region_labels=(qpic, rpic), region_allow=allow)
    with torch.no_grad():
        plain = Attention(query_dim=128, heads=2, dim_head=64, processor=SharedAttnProcessor(self_attn_idx=None))
        assert torch.equal(plain(x, **rg, **refs), plain(x))
        cap = Attention(query_dim=128, heads=2, dim_head=64, processor=AttnProcessor())
        assert torch.equal(cap(x, **rg), cap(x))
        for proc in (AttnProcessor, FaceIDAttnProcessor, SharedAttnProcessor):
            assert {"region_labels", "region_allow"} <= set(inspect.signature(proc.forward).parameters), proc.__name__
    assert not any(c[0] == "region_masks" for c in region_shim.calls)
    assert all(c[1] is None for c in region_shim.calls if c[0] == "shared_attention")
