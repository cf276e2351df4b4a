"""The column maximum (``ir_attn_key_match`` / ``ops.attn_key_match`` / ``SharedAttnProcessor.attention_key_match_reduce``):
everything that can be checked without a GPU - the symbol and its validation in the stated order, the wrapper's checks, the
mutual-check and keep-mask helpers against the NumPy restatement ``tests/oracle_ops_key_match.py`` on planted cases, the
processor's host logic on that oracle-backed stand-in, the kernel file's adherence to the shared read-out header, and the
kernels' register report."""
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
SIBLINGS = (b"ir_attn_probs[_ex]", b"ir_attn_segment_mass", b"ir_attn_rows", b"ir_attn_match", b"ir_attn_transfer", b"ir_attn_received",
            b"ir_attn_topk")


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_bound():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "ir_attn_key_match") and "ir_attn_key_match" in _lib.SYMBOLS
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION                      # a new function, no struct change
    header = open(os.path.join(REPO, "include", "instantrestore_hip.h")).read()
    assert re.search(r"int ir_attn_key_match\(const ir_shared_attn_args\* args, int32_t reduce,\s*int32_t\* index, float\* prob, void\* stream\);",
                     header)
    res, argtypes = _lib.SYMBOLS["ir_attn_key_match"]
    assert res is C.c_int and len(argtypes) == 5 and argtypes[1] is C.c_int32
    kernels = open(os.path.join(REPO, "instantrestore_amd", "csrc", "ir_kernels.h")).read()
    assert "ir_launch_attn_key_match" in kernels and "kKeyMatchMaxItems" in kernels
    # the header says why this call, unlike its siblings, has no order to state
    doc = header[header.index("ir_attn_key_match (opt-in)"):header.index("int ir_attn_key_match(")]
    assert "TOTAL" in doc and "LOWEST" in doc and "does not" in doc and "attention_probs.max(dim=-2)" in doc


def test_validation_in_the_stated_order_before_any_launch():
    """NULL index / prob / lse (INVALID_ARG) come before another reduce and a misaligned index / prob (UNSUPPORTED); the host
    pointers are never dereferenced, so a launch would have faulted"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    off = lambda n: C.cast(C.c_void_p(ptr.value + n), C.c_void_p)

    def call(red=0, index=ptr, prob=ptr, args=a):
        return lib.ir_attn_key_match(None if args is None else C.byref(args), red, index, prob, None)

    assert call(args=None) == INVALID and b"args" in err()
    assert call(index=None) == INVALID and b"index" in err()
    assert call(prob=None) == INVALID and b"prob" in err()
    assert call(index=None, prob=None) == INVALID and b"index" in err()             # index first
    a.lse = None
    assert call() == INVALID and b"lse" in err()
    assert call(prob=None) == INVALID and b"prob" in err()                           # prob before lse
    assert call(red=7) == INVALID and b"lse" in err()                                # every NULL before the form
    a.lse = ptr
    for bad in (-1, 2, 7):
        assert call(red=bad) == UNSUPPORTED and b"reduce" in err()
    assert call(red=2, index=off(2)) == UNSUPPORTED and b"reduce" in err()           # the form before the alignments
    assert call(red=2, index=None) == INVALID and b"index" in err()                  # a NULL before the form
    for n in (1, 2, 3):
        assert call(index=off(n)) == UNSUPPORTED and b"index" in err()
        assert call(prob=off(n)) == UNSUPPORTED and b"prob" in err()
    assert call(index=off(2), prob=off(2)) == UNSUPPORTED and b"index" in err()
    a.tuning = 13
    assert call() == UNSUPPORTED and b"tuning" in err() and b"ir_attn_key_match" in err()
    assert call(index=None) == UNSUPPORTED and b"tuning" in err()                    # the args block is checked first
    a.tuning = 0
    a.struct_size = 7
    assert call() == INVALID and b"ABI mismatch" in err()


def test_more_than_2_31_work_items_are_refused():
    """B * H * key groups beyond 2^31 - 4: refused by arithmetic on the sizes, before any launch"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    a.batch, a.heads, a.n_refs, a.len_ref = 1 << 15, 1 << 12, 64, 96 * 1024       # 2^27 (b, h) pairs, more than 16 groups each
    assert lib.ir_attn_key_match(C.byref(a), 0, ptr, ptr, None) == UNSUPPORTED and b"grid too large" in lib.ir_last_error_string()


def test_bias_and_ragged_blocks_are_refused_with_the_familys_messages():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a, ptr, _buf = _args(_lib)
    err = lambda: lib.ir_last_error_string()
    bias = _copy_into(_lib.SharedAttnBiasArgs(), a)
    bias.key_bias = ptr
    assert lib.ir_attn_key_match(C.byref(bias), 0, ptr, ptr, None) == UNSUPPORTED
    msg = err()
    assert b"key_bias" in msg and b"ir_attn_key_match" in msg and all(s in msg for s in SIBLINGS), msg
    assert b"do not take a key bias yet" in msg and b"the forward's seg_mass by-product does" in msg
    ragged = _copy_into(_lib.SharedAttnRaggedArgs(), a)
    ragged.ref_lens, ragged.rl_sb = ptr, 2
    assert lib.ir_attn_key_match(C.byref(ragged), 1, ptr, ptr, None) == UNSUPPORTED
    msg = err()
    assert b"ref_lens" in msg and b"ir_attn_key_match" in msg and all(s in msg for s in SIBLINGS), msg
    assert b"do not take per-reference counts yet" in msg and b"walk the tails behind the counts" in msg
    # the siblings' refusals name the new entry point as well: one message for the family
    assert lib.ir_attn_received(C.byref(bias), None, 0, 1, 1, 0, ptr, None) == UNSUPPORTED and b"ir_attn_key_match" in err()


# ---- ops ------------------------------------------------------------------------------------------------------------------
def test_ops_attn_key_match_has_no_cpu_path_and_checks_its_arguments():
    from instantrestore_amd import ops
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    lse = torch.zeros(1, 1, 8)
    for bad in ("map", "mean", None):
        with pytest.raises(ValueError, match="reduce"):
            ops.attn_key_match(q, q, None, lse, heads=1, scale=0.125, reduce=bad)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_key_match(q, q, None, lse, heads=1, scale=0.125)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.attn_key_match(q, q, None, lse, heads=1, scale=0.125, reduce="head_mean")
    src = inspect.getsource(ops.attn_key_match)
    assert "_probs_args(" in src and "MATCH_REDUCE[reduce]" in src and "one_kernel=True" in src
    # (the one-kernel decision is _probs_args' argument: there the forward's A/B hook is switched off)
    assert re.search(r"if one_kernel:\n\s+args\.tuning = 0\n", inspect.getsource(ops._probs_args))
    assert src.index("_check_reduce(reduce, MATCH_REDUCE)") < src.index("_probs_args(")                  # the form is checked before anything else


def test_ops_signature():
    from instantrestore_amd import ops
    sig = inspect.signature(ops.attn_key_match)
    names = list(sig.parameters)
    assert names == ["q", "k_self", "ref_k", "lse", "heads", "scale", "include_self", "reduce", "q_prescaled", "batch_invariant"]
    assert sig.parameters["reduce"].default == "none" and sig.parameters["include_self"].default is True
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[4:])


# ---- the NumPy restatement itself ------------------------------------------------------------------------------------------
def test_oracle_helper_against_a_brute_force_loop():
    import oracle_ops_key_match as K
    rng = np.random.default_rng(0)
    B, H, L, Lkv = 2, 3, 7, 9
    for p in (rng.random((B, H, L, Lkv)), rng.integers(0, 3, (B, H, L, Lkv)).astype(np.float32)):      # the second one is full of ties
        for hm in (False, True):
            best, first = K.key_match_np(p, hm)
            x = p.mean(axis=1) if hm else p
            assert best.shape == x.shape[:-2] + (Lkv,) and first.shape == best.shape
            for lead in np.ndindex(*best.shape):
                col = x[lead[:-1] + (slice(None), lead[-1])]
                bi, bv = 0, col[0]
                for i in range(1, L):
                    if col[i] > bv:
                        bi, bv = i, col[i]
                assert best[lead] == bv and first[lead] == bi
    assert K.key_match_np(np.zeros((1, 1, 5, 4)), False)[1].tolist() == [[[0, 0, 0, 0]]]              # a column of zeros: row 0


# ---- the mutual check ---------------------------------------------------------------------------------------------------------
def _planted(L=6, Ls=6, N=2, Lr=5, inc=True):
    import oracle_ops_key_match as K
    edges = K.segment_edges(Ls, N, Lr, inc)
    return K, edges, edges[-1]


def test_mutual_matches_on_planted_cases_against_the_oracle():
    from instantrestore_amd.attn_maps import mutual_matches
    K, edges, lkv = _planted()
    L, Ls, N, Lr = 6, 6, 2, 5
    # one to one: row r looks at key r of every segment and key r of every segment is looked at by row r
    x = np.full((1, L, lkv), 0.01)
    for r in range(5):
        for a in edges[:-1]:
            x[0, r, a + r] = 0.5
    x[0, 5, edges[0] + 5] = 0.5                                         # the self segment has a sixth key; the references do not
    mi = K.match_of_matrix_np(x, edges)
    ki = K.key_match_of_matrix_np(x)[1]
    got = mutual_matches(torch.from_numpy(mi), torch.from_numpy(ki), Ls, N, Lr, True)
    want = K.mutual_np(mi, ki, edges)
    assert got.dtype == torch.bool and tuple(got.shape) == mi.shape and np.array_equal(got.numpy(), want)
    assert bool(got[0, :5].all()) and got[0, 5].tolist() == [True, False, False]      # row 5 has no partner in the 5-key references

    # many to one: rows 1, 2, 3 all look hardest at key 2 of reference 0; only the strongest of them, row 3, survives there
    y = np.full((1, L, lkv), 0.01)
    for r, v in ((1, 0.3), (2, 0.2), (3, 0.6)):
        y[0, r, edges[1] + 2] = v
    mi = K.match_of_matrix_np(y, edges)
    ki = K.key_match_of_matrix_np(y)[1]
    got = mutual_matches(torch.from_numpy(mi), torch.from_numpy(ki), Ls, N, Lr, True)
    assert np.array_equal(got.numpy(), K.mutual_np(mi, ki, edges))
    assert got[0, 1:4, 1].tolist() == [False, False, True]              # (the other rows hold a flat 0.01 everywhere: not the planted case)
    # a tie between rows goes to the lower one (the rule of ir_attn_key_match), and the check follows it
    y[0, 1, edges[1] + 2] = 0.6
    ki = K.key_match_of_matrix_np(y)[1]
    got = mutual_matches(torch.from_numpy(mi), torch.from_numpy(ki), Ls, N, Lr, True)
    assert got[0, 1:4, 1].tolist() == [True, False, False]


def test_mutual_matches_minus_one_rows_subsets_heads_and_errors():
    from instantrestore_amd.attn_maps import mutual_matches
    K, edges, lkv = _planted()
    L, Ls, N, Lr, B, H = 6, 6, 2, 5, 2, 3
    rng = np.random.default_rng(3)
    p = rng.random((B, H, L, lkv))
    for x in (p, p.mean(axis=1)):                                                          # per head (B, H, ..) and head mean (B, ..)
        mi = K.match_of_matrix_np(x, edges)
        ki = K.key_match_of_matrix_np(x)[1]
        want = K.mutual_np(mi, ki, edges)
        got = mutual_matches(torch.from_numpy(mi).int(), torch.from_numpy(ki).int(), Ls, N, Lr, True)
        assert np.array_equal(got.numpy(), want) and want.any() and not want.all()
        assert np.array_equal(mutual_matches(torch.from_numpy(mi), torch.from_numpy(ki), Ls, N, Lr, True, rows="all").numpy(), want)
        # -1 entries are false, whatever the key axis says about column col0 - 1 or col0
        bad = mi.copy()
        bad[..., 2, :] = -1
        gb = mutual_matches(torch.from_numpy(bad), torch.from_numpy(ki), Ls, N, Lr, True)
        assert not gb[..., 2, :].any() and np.array_equal(gb.numpy(), K.mutual_np(bad, ki, edges))
        # rows=: a subset in any order with a duplicate, one list for the batch and one per entry
        for rows in (np.array([4, 0, 4, 3]), np.array([[5, 1, 1, 0], [2, 2, 3, 4]])):
            sub = np.stack([np.take(mi[b], rows if rows.ndim == 1 else rows[b], axis=-2) for b in range(B)])
            gs = mutual_matches(torch.from_numpy(sub), torch.from_numpy(ki), Ls, N, Lr, True, rows=torch.from_numpy(rows))
            assert np.array_equal(gs.numpy(), K.mutual_np(sub, ki, edges, rows))
            for b in range(B):
                rb = rows if rows.ndim == 1 else rows[b]
                assert np.array_equal(gs.numpy()[b], np.take(want[b], rb, axis=-2))          # the subset of the full answer
    # without the self segment the columns start at reference 0
    e2 = K.segment_edges(Ls, N, Lr, False)
    x = p[..., Ls:].mean(axis=1)
    mi, ki = K.match_of_matrix_np(x, e2), K.key_match_of_matrix_np(x)[1]
    assert np.array_equal(mutual_matches(torch.from_numpy(mi), torch.from_numpy(ki), Ls, N, Lr, False).numpy(), K.mutual_np(mi, ki, e2))
    mi_t, ki_t = torch.from_numpy(mi), torch.from_numpy(ki)
    with pytest.raises(ValueError, match="match_index"):
        mutual_matches(mi_t, ki_t, Ls, N, Lr, True)                                        # S does not fit
    with pytest.raises(ValueError, match="key_index"):
        mutual_matches(mi_t, ki_t[:, :-1], Ls, N, Lr, False)
    with pytest.raises(ValueError, match="key_index"):
        mutual_matches(mi_t[:, None], ki_t, Ls, N, Lr, False)                              # per head against head mean
    with pytest.raises(ValueError, match="rows"):
        mutual_matches(mi_t, ki_t, Ls, N, Lr, False, rows=torch.arange(3))
    with pytest.raises(ValueError, match="empty"):
        mutual_matches(mi_t, ki_t, Ls, 0, Lr, False)


def test_mutual_match_field_is_match_field_through_the_mask():
    from instantrestore_amd.attn_maps import match_field, mutual_match_field, mutual_matches
    import oracle_ops_key_match as K
    L = Ls = Lr = 16
    N, side = 2, 4
    edges = K.segment_edges(Ls, N, Lr, True)
    x = np.random.default_rng(5).random((2, L, edges[-1]))
    mi, ki = torch.from_numpy(K.match_of_matrix_np(x, edges)), torch.from_numpy(K.key_match_of_matrix_np(x)[1])
    for rows in (None, "all", torch.tensor([3, 3, 15, 0])):
        sub = mi if rows is None or isinstance(rows, str) else mi[:, rows]
        dy, dx, mask = mutual_match_field(sub, ki, rows, side, Ls, N, Lr, True)
        fy, fx = match_field(sub, rows, side)
        want = mutual_matches(sub, ki, Ls, N, Lr, True, rows=None if rows is None or isinstance(rows, str) else rows)
        assert torch.equal(mask, want) and mask.any() and not mask.all()
        assert torch.equal(dy[mask], fy[mask]) and torch.equal(dx[mask], fx[mask])
        assert not dy[~mask].any() and not dx[~mask].any()                                 # marked as match_field marks an invalid entry: 0


# ---- the keep mask ---------------------------------------------------------------------------------------------------------------
def test_keep_from_key_match_thresholds_fractions_and_reductions():
    from instantrestore_amd.attn_maps import keep_from_key_match, keep_from_received
    B, N, Lr, Ls = 2, 3, 10, 4
    g = torch.Generator().manual_seed(0)
    prob = torch.rand(B, Ls + N * Lr, generator=g)
    seg = prob[:, Ls:].reshape(B, N, Lr)
    for thr in (0.0, 0.25, 0.5, 0.99, 2.0):
        keep = keep_from_key_match(prob, Ls, N, Lr, True, min_prob=thr)
        assert keep.shape == (B, N, Lr) and keep.dtype == torch.bool and torch.equal(keep, seg >= thr)
    assert bool(keep_from_key_match(prob, Ls, N, Lr, True, min_prob=0.0).all()) and not bool(keep_from_key_match(prob, Ls, N, Lr, True, min_prob=2.0).any())
    edge = torch.tensor([[0.5, 0.25, 0.75, 0.5]])
    assert keep_from_key_match(edge, 0, 1, 4, False, min_prob=0.5).tolist() == [[[True, False, True, True]]]      # >=, not >
    for frac in (0.05, 0.25, 0.3, 0.31, 0.5, 0.99, 1.0):
        keep = keep_from_key_match(prob, Ls, N, Lr, True, keep_fraction=frac)
        want = min(Lr, max(1, math.ceil(frac * Lr - 1e-9)))
        assert bool((keep.sum(-1) == want).all()), frac
        assert torch.equal(keep, keep_from_received(prob[..., None], Ls, N, Lr, True, frac))         # the count and the order of the sum rule
    tie = torch.tensor([1.0, 3.0, 3.0, 0.5, 3.0, 1.0, 1.0, 0.0]).reshape(1, 8)
    assert keep_from_key_match(tie, 0, 1, 8, False, keep_fraction=0.25).tolist() == [[[False, True, True, False, False, False, False, False]]]
    # per head: reduced by a MAXIMUM over the heads - the token one head looks at strongly stays, where a mean would drop it
    h2 = torch.zeros(1, 2, 8)
    h2[0, 0, 1], h2[0, 1, 6], h2[0, 0, 6], h2[0, 1, 1] = 0.9, 0.5, 0.5, 0.0
    assert keep_from_key_match(h2, 0, 1, 8, False, keep_fraction=0.125)[0, 0].nonzero().flatten().tolist() == [1]
    assert keep_from_key_match(h2, 0, 1, 8, False, min_prob=0.6)[0, 0].nonzero().flatten().tolist() == [1]
    assert torch.equal(keep_from_key_match(h2, 0, 1, 8, False, min_prob=0.4), keep_from_key_match(h2.amax(1), 0, 1, 8, False, min_prob=0.4))
    # the self segment is skipped
    withself = torch.cat([torch.full((1, 4), 9.0), tie], dim=1)
    assert torch.equal(keep_from_key_match(withself, 4, 1, 8, True, keep_fraction=0.25), keep_from_key_match(tie, 0, 1, 8, False, keep_fraction=0.25))
    with pytest.raises(ValueError, match="exactly one"):
        keep_from_key_match(tie, 0, 1, 8, False)
    with pytest.raises(ValueError, match="exactly one"):
        keep_from_key_match(tie, 0, 1, 8, False, min_prob=0.1, keep_fraction=0.5)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="keep_fraction"):
            keep_from_key_match(tie, 0, 1, 8, False, keep_fraction=bad)
    with pytest.raises(ValueError, match="n_refs"):
        keep_from_key_match(tie, 8, 0, 0, True, min_prob=0.5)
    with pytest.raises(ValueError, match="Lkv"):
        keep_from_key_match(tie, 0, 1, 9, False, min_prob=0.5)


# ---- processor host logic on the stand-in -----------------------------------------------------------------------------------
@pytest.fixture()
def shim(monkeypatch):
    import instantrestore_amd.attn_processors as ap
    import oracle_ops_key_match
    monkeypatch.setattr(ap, "_ops", oracle_ops_key_match)
    ap._BIAS_ROWS.clear()
    oracle_ops_key_match.CALLS.clear()
    return oracle_ops_key_match


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
    assert p.attention_key_match_reduce is None and p.attention_key_match is None
    assert len(p.state_dict()) == 0
    proc, run, _ = _layer()
    with torch.no_grad():
        run()
    assert "attn_key_match" not in [c[0] for c in shim.CALLS] and proc.attention_key_match is None
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [False]


@pytest.mark.parametrize("train_input", [True, False])
def test_attribute_triggers_one_call_with_the_forwards_lse(shim, train_input):
    from instantrestore_amd.attn_maps import keep_from_key_match, mutual_matches
    proc, run, (B, H, L, N) = _layer(train_input)
    S = N + int(train_input)
    lkv = S * L
    with torch.no_grad():
        y_plain = run()
        shim.CALLS.clear()
        proc.attention_key_match_reduce = "head_mean"
        y_on = run()
    calls = [c[1] for c in shim.CALLS if c[0] == "attn_key_match"]
    assert len(calls) == 1 and calls[0]["reduce"] == "head_mean"
    assert calls[0]["lse"] is shim.LAST_LSE[0] and shim.LAST_LSE[0] is not None                          # the LSE of the same forward
    assert [c[1] for c in shim.CALLS if c[0] == "return_lse"] == [True]
    assert [c[0] for c in shim.CALLS].count("shared_attention") == 1 and "attn_probs" not in [c[0] for c in shim.CALLS]
    index, prob = proc.attention_key_match
    assert index.shape == (B, lkv) and index.dtype == torch.int32 and prob.shape == (B, lkv) and prob.dtype == torch.float32
    assert int(index.min()) >= 0 and int(index.max()) < L and float(prob.min()) > 0
    assert torch.equal(y_plain, y_on)                                                                    # the layer output never depends on the option
    assert keep_from_key_match(prob, L, N, L, train_input, keep_fraction=0.25).sum(-1).tolist() == [[4] * N] * B
    # "none" gives the per-head shape; beside the match read-out one LSE serves both and the two go through the mutual check
    shim.CALLS.clear()
    proc.attention_key_match_reduce, proc.attention_match_index, proc.attention_match_reduce = "none", "all", "none"
    with torch.no_grad():
        run()
    names = [c[0] for c in shim.CALLS]
    assert names.count("shared_attention") == 1 and names.count("attn_match") == 1 and names.count("attn_key_match") == 1
    i2, p2 = proc.attention_key_match
    assert i2.shape == (B, H, lkv) and p2.shape == (B, H, lkv)
    mutual = mutual_matches(proc.attention_match[0], i2, L, N, L, train_input)
    want = shim.mutual_np(proc.attention_match[0].numpy(), i2.numpy(), shim.segment_edges(L, N, L, train_input))
    assert mutual.shape == (B, H, L, S) and np.array_equal(mutual.numpy(), want) and want.any()
    proc.attention_key_match_reduce = "mean"
    shim.CALLS.clear()
    with torch.no_grad(), pytest.raises(ValueError, match="attention_key_match_reduce"):
        run()
    assert not {"shared_attention", "attn_match", "attn_key_match"} & {c[0] for c in shim.CALLS}       # refused before anything is launched


def test_a_layer_that_is_not_shared_ignores_the_attribute(shim):
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    plain = SharedAttnProcessor(self_attn_idx=None)
    plain.attention_key_match_reduce = "head_mean"
    with torch.no_grad():
        Attention(query_dim=64, heads=1, dim_head=64, processor=plain)(torch.randn(1, 4, 64))
    assert "attn_key_match" not in [c[0] for c in shim.CALLS] and plain.attention_key_match is None
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
    for form in ("head_mean", "none"):
        proc.attention_key_match_reduce = form
        for name, kw in cases.items():
            shim.CALLS.clear()
            if name == "ref_lens":
                proc.use_adain = False           # (with use_adain the counts need ref_stats: an earlier, unrelated check)
            with torch.no_grad(), pytest.raises(NotImplementedError, match="attention_key_match_reduce"):
                run(**kw)
            assert "shared_attention" not in [c[0] for c in shim.CALLS], name      # refused before anything is launched


# ---- the kernel file is built on the shared header -----------------------------------------------------------------------------
def test_kernel_takes_its_qk_block_from_the_readout_header():
    """attn_key_match.hip includes ir_readout.h, uses its pieces and defines none of them again; no exponential, no atomics, no
    LDS and no inline assembly of its own; the build lists the file in SRCS and on an MFMA-results-in-VGPRs line"""
    csrc = os.path.join(REPO, "instantrestore_amd", "csrc")
    text = open(os.path.join(csrc, "attn_key_match.hip")).read()
    assert re.search(r'#include\s+"ir_readout\.h"', text)
    body = text.split('#include "ir_readout.h"')[1]
    for name in ("keymap", "key_segment", "load_q", "load_k", "scores", "prob"):
        assert re.search(r"\b%s\s*(<[^>]*>)?\(" % name, body), f"{name} is not used"
        assert not re.search(r"\b(int|void|float|hipError_t|f32x16|KeySeg<T>)\s+%s\s*\(" % name, body), f"{name} is defined again"
    assert not re.search(r"__builtin_fmaf\([^;]*scale_log2", body)
    assert "exp2" not in body and "atomic" not in body and "__shared__" not in body and "asm" not in body and "__syncthreads" not in body
    assert "__shfl_xor" in body
    build = open(os.path.join(csrc, "build.sh")).read()
    assert build.count("attn_key_match.hip") == 2                                       # SRCS and the MFMA-results-in-VGPRs line
    assert re.search(r'"\$s" == attn_key_match\.hip \]\] && extra\+=\(-mllvm -amdgpu-mfma-vgpr-form\)', build)


def test_kernels_report_no_spills_no_scratch_and_no_lds():
    paths = glob.glob(os.path.join(REPO, "instantrestore_amd", "csrc", "build", "attn_key_match.remarks")) + \
        glob.glob(os.path.join(REPO, "build", "attn_key_match.remarks"))
    assert paths, "attn_key_match.remarks is missing: run __graft_entry__.build()"
    text = open(paths[0], errors="replace").read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 4 and all("attn_key_match_kernel" in n for n in names), names    # 2 dtypes x 2 forms
    for what in (r"VGPRs Spill: (\d+)", r"SGPRs Spill: (\d+)", r"ScratchSize \[bytes/lane\]: (\d+)", r"LDS Size \[bytes/block\]: (\d+)"):
        vals = [int(x) for x in re.findall(what, text)]
        assert len(vals) == 4 and not any(vals), (what, vals)
    assert "attn_key_match_kernel" in open(os.path.join(REPO, "tools", "check_resources.py")).read()
