"""Batch-invariant mode (ABI v10) on the MI355X: an identity's bytes do not depend on the rest of its batch.

Every comparison is ``torch.equal``.  Item ``j`` is computed alone, first and last in batches of 2, 3 and 8 whose other entries
hold different random data and different ``valid_refs`` counts, and inside B = 32 at the 32x32-token class (where the default
dispatch switches kernels); the outputs must be the same bytes, and the same with or without the LSE / masses asked for, under
hipGraph replay and on a side stream.  The GEMMs, the statistics merges, the dump paths and the processors are held to the same,
and the mode to the oracle bounds of the default dispatch."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LOG2E = 1.4426950408889634
SCALE = 0.125
# cfg 2's three shared layer classes (three layers each, same shapes): (Lq, heads); N = 4 references of Lq tokens
CLASSES = [(4096, 5), (1024, 10), (256, 20)]
N = 4


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from instantrestore_amd import ops as _ops
    return _ops


def _identity(g, L, H, dtype, valid):
    """one identity's tensors (B = 1): q, k_self, v_self, ref_k, ref_v with references n >= valid zero-filled"""
    C = H * 64
    q, ks, vs = (torch.randn(1, L, C, generator=g) for _ in range(3))
    rk, rv = torch.randn(1, N, L, C, generator=g), torch.randn(1, N, L, C, generator=g)
    rk[:, valid:] = 0
    rv[:, valid:] = 0
    return [t.to("cuda", dtype) for t in (q, ks, vs, rk, rv)]


def _batch(items):
    return [torch.cat([it[i] for it in items]) for i in range(5)]


def _run(ops, t, valid, *, inc, fold, presc, lse=True, mass=True):
    q, ks, vs, rk, rv = t
    H = q.shape[-1] // 64
    if presc:
        q = (q.float() * (SCALE * LOG2E)).to(q.dtype)
    aff = ops.adain_stats(vs, rv, heads=H) if fold else None
    v = valid if valid is None or isinstance(valid, torch.Tensor) else torch.tensor(valid, dtype=torch.int32, device="cuda")
    res = ops.shared_attention(q, ks, vs, rk, rv, heads=H, scale=SCALE, include_self=inc, adain=aff, q_prescaled=presc,
                               valid_refs=v, return_lse=lse, return_mass=mass, batch_invariant=True)
    return res if isinstance(res, tuple) else (res,)


def _same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y), f"{what}: max |diff| {(x.float() - y.float()).abs().max().item():.3e}"


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: f"L{c[0]}")
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_attention_item_alone_first_last_and_in_batches(ops, cls, dtype):
    L, H = cls
    g = torch.Generator().manual_seed(L + H + (dtype == torch.float16))
    j_valid = 3
    item = _identity(g, L, H, dtype, j_valid)
    others = [_identity(g, L, H, dtype, v) for v in (4, 1, 2, 0, 4, 3, 1)]
    ovalid = [4, 1, 2, 0, 4, 3, 1]
    for inc in (True, False):
        for fold in (True, False):
            for presc in (True, False):
                kw = dict(inc=inc, fold=fold, presc=presc)
                for use_valid in (True, False):
                    alone = _run(ops, item, [j_valid] if use_valid else None, **kw)
                    for B in (2, 3, 8):
                        for pos in (0, B - 1):
                            its = others[:B - 1]
                            vals = ovalid[:B - 1]
                            its = its[:pos] + [item] + its[pos:]
                            vals = vals[:pos] + [j_valid] + vals[pos:]
                            got = _run(ops, _batch(its), vals if use_valid else None, **kw)
                            _same([x[pos:pos + 1] for x in got], alone, f"L{L} {dtype} {kw} valid={use_valid} B={B} pos={pos}")
                # the output does not change with what else is asked for
                out_only = _run(ops, item, [j_valid], lse=False, mass=False, **kw)
                lse_only = _run(ops, item, [j_valid], lse=True, mass=False, **kw)
                full = _run(ops, item, [j_valid], **kw)
                _same(out_only, full[:1], f"L{L} {kw} out without / with lse + masses")
                _same(lse_only, full[:2], f"L{L} {kw} out + lse without / with masses")


def test_attention_across_the_kernel_switch_at_b32(ops):
    """cfg 2's 32x32-token class: the default dispatch runs the 32-row kernel at B = 1...9 and the 128-row kernel at B = 32"""
    L, H = 1024, 10
    g = torch.Generator().manual_seed(32)
    items = [_identity(g, L, H, torch.bfloat16, 1 + i % 4) for i in range(32)]
    valid = [1 + i % 4 for i in range(32)]
    for fold in (True, False):
        full = _run(ops, _batch(items), valid, inc=True, fold=fold, presc=True)
        for j in (0, 5, 31):
            alone = _run(ops, items[j], [valid[j]], inc=True, fold=fold, presc=True)
            _same([x[j:j + 1] for x in full], alone, f"B=32 item {j} fold={fold}")


def test_graph_replay_and_side_stream_match_eager(ops):
    from instantrestore_amd.kv_harvest import capture_step
    L, H = 4096, 5
    g = torch.Generator().manual_seed(7)
    t = _batch([_identity(g, L, H, torch.bfloat16, v) for v in (4, 2, 3)])
    valid = torch.tensor([4, 2, 3], dtype=torch.int32, device="cuda")     # (no host-to-device copy inside the capture)
    eager = _run(ops, t, valid, inc=True, fold=True, presc=True)
    step = capture_step(lambda: _run(ops, t, valid, inc=True, fold=True, presc=True))
    for _ in range(2):
        res = step.replay()
        torch.cuda.synchronize()
        _same(res, eager, "graph replay")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = _run(ops, t, valid, inc=True, fold=True, presc=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same(res, eager, "side stream")


@pytest.mark.parametrize("total", [64, 61])
def test_sharded_identities_match_one_call(ops, total):
    """the 32x32 class: ``total`` identities split by ``shard_sizes(total, 8)`` give the bytes of the same identities in one call"""
    from instantrestore_amd.sharding import shard_sizes
    L, H = 1024, 10
    g = torch.Generator().manual_seed(total)
    items = [_identity(g, L, H, torch.bfloat16, 1 + i % 4) for i in range(total)]
    valid = [1 + i % 4 for i in range(total)]
    full = _run(ops, _batch(items), valid, inc=True, fold=True, presc=True)
    b0 = 0
    for n in shard_sizes(total, 8):
        part = _run(ops, _batch(items[b0:b0 + n]), valid[b0:b0 + n], inc=True, fold=True, presc=True)
        _same(part, [x[b0:b0 + n] for x in full], f"shard [{b0}, {b0 + n}) of {total}")
        b0 += n


def _projection_shapes():
    """(L, N, K, bias) of the projections: fused q/k/v and the out projection of each layer class, and the cross attention's fused
    k/v from the 77 text states (K = cross_attention_dim = 1024, M = 77 * B: ragged row tiles)"""
    return ([(L, 3 * 64 * H, 64 * H, False) for L, H in CLASSES] + [(L, 64 * H, 64 * H, True) for L, H in CLASSES]
            + [(77, 2 * 64 * H, 1024, False) for _, H in CLASSES])


def test_gemm_rows_do_not_depend_on_the_row_count(ops):
    g = torch.Generator().manual_seed(11)
    for L, n, k, bias in _projection_shapes():
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to("cuda", torch.bfloat16)
        b = torch.randn(n, generator=g).to("cuda", torch.bfloat16) if bias else None
        xs = torch.randn(16, L, k, generator=g).to("cuda")             # fp32 activations (autocast's LayerNorm output)
        for x_f32 in (True, False):
            x_all = xs if x_f32 else xs.to(torch.bfloat16)
            qkv = not bias and k != 1024
            for sc in ((0, 1.0), (n // 3, SCALE * LOG2E)) if qkv else ((0, 1.0),):
                kw = dict(scale_cols=sc[0], col_scale=sc[1], batch_invariant=True)
                ref = ops.linear(x_all[:1], w, b, **kw)
                for B in (4, 8, 16):
                    y = ops.linear(x_all[:B], w, b, **kw)
                    assert torch.equal(y[:1], ref), (L, n, k, bias, x_f32, sc, B)
                    assert torch.equal(y[B - 1:B], ops.linear(x_all[B - 1:B], w, b, **kw)), (L, n, k, B, "last row block")
            if qkv:   # the statistics tail of the V third: partials per 64-row block, merged per set
                c = n // 3
                ref_y, ref_st = ops.linear(x_all[:1], w, None, stats=(2 * c, c), batch_invariant=True)
                for B in (4, 16):
                    y, st = ops.linear(x_all[:B], w, None, stats=(2 * c, c), batch_invariant=True)
                    assert torch.equal(y[:1], ref_y)
                    per = L // st.rows
                    assert torch.equal(st.ws[:per], ref_st.ws), (L, n, B, "statistics partials")
                    m, sd = ops.token_stats_from_partials(st, B, L)
                    m1, sd1 = ops.token_stats_from_partials(ref_st, 1, L)
                    assert torch.equal(m[:1], m1) and torch.equal(sd[:1], sd1)


def test_capture_layer_gemm_at_b_times_n_rows(ops):
    """the K/V-capture layer's q/k/v projection runs over B * N token sets: an identity's references keep their bytes"""
    g = torch.Generator().manual_seed(12)
    L, H = 4096, 5
    C = 64 * H
    w = (torch.randn(3 * C, C, generator=g) / C ** 0.5).to("cuda", torch.bfloat16)
    x = torch.randn(8 * N, L, C, generator=g).to("cuda")
    ref = ops.linear(x[:N], w, None, batch_invariant=True)
    y = ops.linear(x, w, None, batch_invariant=True)
    assert torch.equal(y[:N], ref) and torch.equal(y[-N:], ops.linear(x[-N:], w, None, batch_invariant=True))


def test_adain_affine_from_partials_per_item(ops):
    g = torch.Generator().manual_seed(13)
    L, H = 1024, 10
    C = 64 * H
    w = (torch.randn(3 * C, C, generator=g) / C ** 0.5).to("cuda", torch.bfloat16)
    xs = torch.randn(8, L, C, generator=g).to("cuda")
    xr = torch.randn(8 * N, L, C, generator=g).to("cuda")
    valid = torch.tensor([3, 4, 1, 2, 4, 0, 2, 3], dtype=torch.int32, device="cuda")

    def affine(b0, nb):
        _, st = ops.linear(xs[b0:b0 + nb], w, None, stats=(2 * C, C), batch_invariant=True)
        _, ct = ops.linear(xr[b0 * N:(b0 + nb) * N], w, None, stats=(2 * C, C), batch_invariant=True)
        return ops.adain_affine_from_partials(st, nb, L, N, L, content=ct, valid=valid[b0:b0 + nb].contiguous())

    a8, b8 = affine(0, 8)
    for j in (0, 7):
        a1, b1 = affine(j, 1)
        assert torch.equal(a8[j:j + 1], a1) and torch.equal(b8[j:j + 1], b1), j
    # the one-pass statistics entry points as well
    v = torch.randn(8, L, C, generator=g).to("cuda", torch.bfloat16)
    rv = torch.randn(8, N, L, C, generator=g).to("cuda", torch.bfloat16)
    a8, b8 = ops.adain_stats(v, rv, heads=H)
    a1, b1 = ops.adain_stats(v[7:], rv[7:], heads=H)
    assert torch.equal(a8[7:], a1) and torch.equal(b8[7:], b1)


@pytest.mark.parametrize("nb", [3, 32])
def test_probabilities_and_second_pass_masses_per_item(ops, nb):
    """B = 32 at the 32x32-token class: the dump kernel's cut of the key axis reads the batch (1024 keys per chunk at B = 32, 256 at
    B = 1) - every probability is still its own exp(s - lse), the same bytes"""
    for L, H in CLASSES[1:] if nb == 3 else CLASSES[1:2]:
        g = torch.Generator().manual_seed(L + nb)
        items = [_identity(g, L, H, torch.bfloat16, 1 + i % 4) for i in range(nb)]
        t = _batch(items)
        for presc in (True, False):
            q = (t[0].float() * (SCALE * LOG2E)).to(t[0].dtype) if presc else t[0]
            sc = 0.6931471805599453 if presc else SCALE
            _, lse = ops.shared_attention(q, t[1], t[2], t[3], t[4], heads=H, scale=SCALE, q_prescaled=presc, return_lse=True,
                                          batch_invariant=True)
            probs = ops.attn_probs(q, t[1], t[3], lse, heads=H, scale=sc, batch_invariant=True)
            mass = ops.attn_segment_mass(q, t[1], t[3], lse, heads=H, scale=sc, batch_invariant=True)
            j = slice(2, 3)     # entry 2 alone
            _, lse1 = ops.shared_attention(q[j], t[1][j], t[2][j], t[3][j], t[4][j], heads=H, scale=SCALE, q_prescaled=presc,
                                           return_lse=True, batch_invariant=True)
            assert torch.equal(lse[j], lse1)
            assert torch.equal(probs[j], ops.attn_probs(q[j], t[1][j], t[3][j], lse1, heads=H, scale=sc, batch_invariant=True))
            assert torch.equal(mass[j], ops.attn_segment_mass(q[j], t[1][j], t[3][j], lse1, heads=H, scale=sc, batch_invariant=True))
            del probs, mass


def _layer(L, C, H, shared, seed):
    from instantrestore_amd import attn_processors as ap
    from instantrestore_amd.attention import Attention
    g = torch.Generator().manual_seed(seed)
    proc = ap.SharedAttnProcessor(self_attn_idx=0, use_adain=True, train_input=True) if shared else ap.AttnProcessor()
    attn = Attention(query_dim=C, heads=H, dim_head=64, processor=proc)
    with torch.no_grad():
        for lin in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0]):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) / C ** 0.5)
    proc.batch_invariant = True
    return attn.to("cuda")


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: f"L{c[0]}")
def test_processors_item_alone_and_in_a_batch(ops, cls):
    """each layer class's AttnProcessor (K/V capture) and SharedAttnProcessor under bf16 autocast with fp32 hidden states, as
    the bench feeds them: output, attention_mass and attention_probs of an identity alone and inside B = 3"""
    L, H = cls
    C = 64 * H
    g = torch.Generator().manual_seed(100 + L)
    kv, main = _layer(L, C, H, False, L), _layer(L, C, H, True, L + 1)
    main.processor.save_attention_mass = True
    main.processor.save_self_attentions = L <= 1024     # the (B, H, L, Lkv) dump of the top layer is 1.3 GB per identity
    h_ref = torch.randn(3 * N, L, C, generator=g).to("cuda")
    h_main = torch.randn(3, L, C, generator=g).to("cuda")

    def step(b0, nb):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            cap = kv(h_ref[b0 * N:(b0 + nb) * N])
            rk = kv.processor.keys.reshape(nb, N, L, C)
            rv = kv.processor.values.reshape(nb, N, L, C)
            out = main(h_main[b0:b0 + nb], ref_keys=[rk], ref_values=[rv])
        res = [cap, out, main.processor.attention_mass]
        if main.processor.save_self_attentions:
            res.append(main.processor.attention_probs)
        return res

    full = step(0, 3)
    for j in (0, 2):
        one = step(j, 1)
        _same([full[0][j * N:(j + 1) * N]] + [x[j:j + 1] for x in full[1:]], one, f"processors L{L} item {j}")


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: f"L{c[0]}")
def test_mode_holds_the_oracle_bounds(ops, cls):
    from oracle import shared_attn_oracle as O
    from parity_bounds import check_parity
    L, H = cls
    g = torch.Generator().manual_seed(200 + L)
    f = lambda x: x.float().cpu()
    # first, middle and last 128 query rows: different work items (and K/V-range pieces) of every kernel the mode picks
    blocks = [slice(0, 128), slice(L // 2 - 64, L // 2 + 64), slice(L - 128, L)]
    for dtype in (torch.bfloat16, torch.float16):
        valid = [4, 2]     # entry 1: references 2, 3 zero-filled and closed analytically (valid_refs)
        t = _batch([_identity(g, L, H, dtype, v) for v in valid])
        for inc in (True, False):
            for fold in (True, False):
                for use_valid in (False, True):
                    for presc in (False, True):
                        out = _run(ops, t, valid if use_valid else None, inc=inc, fold=fold, presc=presc, lse=False, mass=False)[0]
                        for rows in blocks:
                            ref = O.shared_attention_port(f(t[0][:, rows]), f(t[1]), f(t[2]), f(t[3]), f(t[4]), H, SCALE,
                                                          use_adain=fold, train_input=inc)
                            # pre-scaled Q: one more rounding of Q (the bounds' factor for it, as for tuning 11)
                            check_parity(out[:, rows], ref, dtype, f"batch-invariant L{L} {dtype} inc={inc} fold={fold} "
                                         f"valid={use_valid} presc={presc} rows {rows.start}", factor=2.0 if presc else 1.0)


def test_workspace_for_three_of_eight_entries_runs_three_launches_of_the_same_plan(ops):
    """a caller workspace that holds the pieces of 3 of the 8 entries: the library runs the batch as launches of 3, 3 and 2 entries
    (every pointer moved by the launch's first entry: q / k / v, AdaIN affine, out - also as fp32 - LSE, masses, valid counts), and
    the bytes are those of the one-launch call"""
    import ctypes as C
    from instantrestore_amd import _lib
    lib = _lib.lib()
    L, H = 4096, 5
    g = torch.Generator().manual_seed(21)
    valid = [4, 1, 3, 2, 4, 0, 2, 3]
    t = _batch([_identity(g, L, H, torch.bfloat16, v) for v in valid])
    q = (t[0].float() * (SCALE * LOG2E)).to(t[0].dtype)
    vt = torch.tensor(valid, dtype=torch.int32, device="cuda")
    aff = ops.adain_stats(t[2], t[4], heads=H)
    for out_dtype in (torch.bfloat16, torch.float32):
        want = ops.shared_attention(q, t[1], t[2], t[3], t[4], heads=H, scale=SCALE, adain=aff, q_prescaled=True, valid_refs=vt,
                                    return_lse=True, return_mass=True, out_dtype=out_dtype, batch_invariant=True)
        out = torch.empty_like(want[0])
        lse = torch.empty_like(want[1])
        mass = torch.empty_like(want[2])
        a = ops._fill_args(q, t[1], t[2], t[3], t[4], H, SCALE, True, aff, out, lse, True, True, vt, True)
        a.seg_mass = mass.data_ptr()
        a3 = ops._fill_args(q[:3], t[1][:3], t[2][:3], t[3][:3], t[4][:3], H, SCALE, True, aff, out[:3], lse[:3], True, True, vt[:3], True)
        a3.seg_mass = mass.data_ptr()
        need3 = int(lib.ir_shared_attn_workspace_bytes_for(C.byref(a3)))
        assert 0 < need3 < int(lib.ir_shared_attn_workspace_bytes_for(C.byref(a)))
        ws = torch.empty(need3 // 4 + 1, dtype=torch.float32, device="cuda")
        a.workspace, a.workspace_bytes = ws.data_ptr(), need3
        plan = _lib.SharedAttnPlan()
        plan.struct_size = C.sizeof(plan)
        _lib.check(lib.ir_shared_attn_plan(C.byref(a), C.byref(plan)), "ir_shared_attn_plan")
        assert plan.batch_per_launch == 3 and plan.pieces_per_item > 1
        _lib.check(lib.ir_shared_attn_fwd(C.byref(a), ops._stream()), "ir_shared_attn_fwd")
        torch.cuda.synchronize()
        _same((out, lse, mass), want, f"three launches, out {out_dtype}")
