"""Reference K/V through pointer tables on the MI355X (``ir_shared_attn_table_args`` / ``ops.RefKVTable``).

Every test compares a table call with the dense call on ``torch.stack`` of the same entries - same tuning, same flags, same
workspace - with ``torch.equal`` on ``out``, ``lse`` and ``seg_mass``: the arithmetic is the same, so the bytes are.  The dense
path is held to the oracle by the rest of the suite; one case per dtype goes through the oracle here as well.  The entries are
slices of one pool, handed out in shuffled order with gaps of different sizes, so that no table address is an affine function of
``(b, n)``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOG2E = 1.4426950408889634
SCALE = 0.125
TUNE_DEFAULT, TUNE_PRESCALE_Q, TUNE_W64X8, TUNE_EARLYQK, TUNE_W128 = 0, 11, 13, 14, 16      # IR_TUNE_* of the public header
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from instantrestore_amd import ops as _ops
    return _ops


def _pool_grid(g, B, N, L, Cc, dtype, *, thirds=False, scale=1.0, shift=0.0):
    """``B x N`` entries of ``(L, Cc)`` cut from ONE pool in shuffled order with gaps: two grids (K and V).  ``thirds``: every
    entry pair is the K and the V third of one ``(L, 3 Cc)`` buffer (row stride ``3 Cc``), as harvested views are."""
    n = B * N
    gaps = [8 * (1 + (5 * i) % 7) for i in range(2 * n + 1)]            # multiples of 16 bytes, all different neighbours
    order = torch.randperm(n, generator=g).tolist()
    if thirds:
        size = L * 3 * Cc
        pool = torch.randn(sum(gaps[:n + 1]) + n * size, generator=g).to("cuda", dtype)
        gk, gv, off = [None] * n, [None] * n, gaps[0]
        for slot, i in enumerate(order):
            buf = pool[off: off + size].view(L, 3 * Cc)
            gk[i], gv[i] = buf[:, Cc:2 * Cc], buf[:, 2 * Cc:]
            off += size + gaps[slot + 1]
    else:
        size = L * Cc
        pool = (torch.randn(sum(gaps) + 2 * n * size, generator=g) * scale + shift).to("cuda", dtype)
        cut, off = [], gaps[0]
        for slot in range(2 * n):
            cut.append(pool[off: off + size].view(L, Cc))
            off += size + gaps[slot + 1]
        gk, gv = [None] * n, [None] * n
        for slot, i in enumerate(order):                                # K and V entries interleaved through the pool
            gk[i], gv[i] = cut[2 * slot + (i & 1)], cut[2 * slot + 1 - (i & 1)]
    assert pool.data_ptr() % 16 == 0
    grid = lambda flat: [[flat[b * N + j] for j in range(N)] for b in range(B)]
    return grid(gk), grid(gv)


def _stack(grid):
    return torch.stack([torch.stack(row) for row in grid])


def _qkv(g, B, Lq, Cc, dtype, presc):
    q, ks, vs = (torch.randn(B, Lq, Cc, generator=g) for _ in range(3))
    if presc:
        q = q * (SCALE * LOG2E)
    return [t.to("cuda", dtype) for t in (q, ks, vs * 0.9 + 0.2)]


def _same(a, b, what):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x.float()).all(), f"{what}: non-finite result {i}"
        assert torch.equal(x, y), f"{what}: result {i} differs, max |diff| {(x.float() - y.float()).abs().max().item():.3e}"


def _dense_and_table(ops, variant, q, ks, vs, gk, gv, *, H, inc, fold, presc, valid=None, mass=False, bi=False, dense=None):
    """the dense call on the stacked entries and the table call on the entries themselves, under one tuning value"""
    dk, dv = dense if dense is not None else (_stack(gk), _stack(gv))
    counts = None if valid is None else valid.tolist()
    tk, tv = ops.RefKVTable.from_tensors(gk, counts), ops.RefKVTable.from_tensors(gv, counts)
    aff = ops.adain_stats(vs, dv, heads=H) if fold else None
    kw = dict(heads=H, scale=SCALE, include_self=inc, adain=aff, q_prescaled=presc, valid_refs=valid, return_mass=mass,
              batch_invariant=bi)
    prev = ops.set_attn_variant(variant)
    try:
        want = ops.shared_attention(q, ks, vs, dk, dv, return_lse=True, **kw)
        got = ops.shared_attention(q, ks, vs, tk, tv, return_lse=True, **kw)
        assert ops.shared_attention_kernel_name(q, ks, vs, tk, tv, **kw) == ops.shared_attention_kernel_name(q, ks, vs, dk, dv, **kw) != ""
    finally:
        ops.set_attn_variant(prev)
    return want, got, (dk, dv)


# (id, tuning, (B, H, Lq, N, Lr), pre-scaled Q, forms of the call: (valid_refs, seg_mass))
FAMILIES = [
    ("pipe32_default", TUNE_DEFAULT, (2, 2, 200, 3, 72), False, [(False, False)]),
    ("pipe32_earlyqk", TUNE_EARLYQK, (2, 2, 200, 3, 72), False, [(False, False)]),
    ("pipe32_prescale_q", TUNE_PRESCALE_Q, (2, 2, 200, 3, 72), True, [(False, False)]),
    ("w64x8", TUNE_W64X8, (2, 2, 512, 2, 128), False, [(False, False)]),
    ("w64x8_ragged", TUNE_W64X8, (2, 2, 512, 2, 72), False, [(False, False)]),
    ("w128", TUNE_W128, (2, 2, 512, 2, 128), True, [(False, False), (False, True), (True, False)]),     # plain, then both FORMS
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_table_call_equals_dense_call_in_every_kernel_family(ops, family, dtype):
    name, tuning, (B, H, Lq, N, Lr), presc, forms = family
    Cc = H * 64
    g = torch.Generator().manual_seed(len(name) * 31 + (dtype == torch.float16))
    q, ks, vs = _qkv(g, B, Lq, Cc, dtype, presc)
    gk, gv = _pool_grid(g, B, N, Lr, Cc, dtype, scale=1.3, shift=-0.2)
    for use_valid, mass in forms:
        valid = None
        if use_valid:          # the promise of valid_refs: the references behind the count are all-zero
            valid = torch.tensor([N, N - 1], dtype=torch.int32, device="cuda")
            gk[1][N - 1].zero_()
            gv[1][N - 1].zero_()
        for inc in (True, False):
            for fold in (True, False):
                want, got, (dk, dv) = _dense_and_table(ops, tuning, q, ks, vs, gk, gv, H=H, inc=inc, fold=fold, presc=presc, valid=valid, mass=mass)
                _same(got, want, f"{name} {dtype} inc={inc} fold={fold} valid={use_valid} mass={mass}")
                if name == "pipe32_default" and inc and fold:      # one case per dtype against the oracle
                    from oracle.shared_attn_oracle import shared_attention_np
                    from parity_bounds import check_parity
                    f = lambda t: t.float().cpu().numpy().astype(np.float64)
                    ref = shared_attention_np(f(q), f(ks), f(vs), f(dk), f(dv), H, SCALE, True, True)
                    check_parity(got[0], ref, dtype, f"table call vs oracle {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_entries_that_are_thirds_of_fused_buffers(ops, dtype):
    """entries with a row stride of 3 C: the K and V thirds of ``(L, 3C)`` projection outputs, as harvested views are"""
    B, H, Lq, N, Lr = 2, 2, 200, 3, 72
    g = torch.Generator().manual_seed(11)
    q, ks, vs = _qkv(g, B, Lq, H * 64, dtype, False)
    gk, gv = _pool_grid(g, B, N, Lr, H * 64, dtype, thirds=True)
    assert gk[0][0].stride(0) == 3 * H * 64
    for fold in (True, False):
        want, got, _ = _dense_and_table(ops, TUNE_DEFAULT, q, ks, vs, gk, gv, H=H, inc=True, fold=fold, presc=False)
        _same(got, want, f"thirds {dtype} fold={fold}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_pieces_that_start_inside_a_later_reference(ops, dtype):
    """batch-invariant mode cuts every item into K/V-range pieces: a piece that starts inside reference 1 or 2 takes its base
    address from the table like the first.  B = 3 and B = 5 also run on a workspace sized for ONE entry: the partials are laid out
    in chunks of eight items and an entry has two, so that workspace carries four entries - B = 3 still fits one launch, B = 5
    goes through batch_slice, whose second launch starts at table row 4"""
    from instantrestore_amd import _lib
    H, Lq, N, Lr = 2, 128, 3, 512
    shape = dict(len_self=Lq, n_refs=N, len_ref=Lr, dtype=dtype)
    assert ops.shared_attention_plan(1, Lq, H, adain=True, **shape)["pieces_per_item"] > 1
    one = ops.shared_attention_plan(1, Lq, H, **shape)["workspace_bytes"]
    g = torch.Generator().manual_seed(3)
    for B in (1, 3, 5):
        q, ks, vs = _qkv(g, B, Lq, H * 64, dtype, False)
        gk, gv = _pool_grid(g, B, N, Lr, H * 64, dtype)
        got = {}
        for fold in (True, False):
            want, got[fold], (dk, dv) = _dense_and_table(ops, TUNE_DEFAULT, q, ks, vs, gk, gv, H=H, inc=True, fold=fold, presc=False,
                                                         mass=True, bi=True)
            _same(got[fold], want, f"batch-invariant B={B} {dtype} fold={fold}")
        if B == 1:
            continue
        info = ops.shared_attention_plan(B, Lq, H, workspace_bytes=one, **shape)
        assert info["workspace_bytes"] >= one and info["batch_per_launch"] == min(B, 4)
        ws = torch.empty(one // 4, dtype=torch.float32, device="cuda")
        tk, tv = ops.RefKVTable.from_tensors(gk), ops.RefKVTable.from_tensors(gv)
        outs = []
        for rk, rv in ((dk, dv), (tk, tv)):
            out = torch.empty_like(q)
            lse = torch.empty(B, H, Lq, dtype=torch.float32, device="cuda")
            a = ops._fill_args(q, ks, vs, rk, rv, H, SCALE, True, None, out, lse, batch_invariant=True)
            a.workspace, a.workspace_bytes = ws.data_ptr(), one
            _lib.check(_lib.lib().ir_shared_attn_fwd(C.byref(a), ops._stream()), "ir_shared_attn_fwd")
            outs.append((out, lse))
        _same(outs[1], outs[0], f"one-entry workspace, B={B} {dtype}: table vs dense")
        _same(outs[1], got[False][:2], f"one-entry workspace, B={B} {dtype}: vs the launch with a whole-batch workspace")


@pytest.mark.parametrize("case", [(TUNE_DEFAULT, 200, 72, False), (TUNE_W64X8, 512, 128, False), (TUNE_W128, 512, 128, True)],
                         ids=["pipe32", "w64x8", "w128_forms"])
def test_valid_refs_never_reads_the_unused_entries(ops, case):
    """B 3, N 3, valid [3, 1, 0]: the unused table slots point at a NaN-filled (allocated, readable) buffer - a kernel that read
    one would carry the NaN into its row sums.  Equal to the dense call on zero-filled references with the same counts."""
    tuning, Lq, Lr, presc = case
    B, H, N, dtype = 3, 2, 3, torch.bfloat16
    Cc = H * 64
    counts = [3, 1, 0]
    g = torch.Generator().manual_seed(5)
    q, ks, vs = _qkv(g, B, Lq, Cc, dtype, presc)
    gk, gv = _pool_grid(g, B, N, Lr, Cc, dtype)
    poison = torch.full((Lr, Cc), float("nan"), dtype=dtype, device="cuda")
    dk, dv = _stack(gk), _stack(gv)
    for b, c in enumerate(counts):
        dk[b, c:] = 0
        dv[b, c:] = 0
        for n in range(c, N):
            gk[b][n] = gv[b][n] = poison
    valid = torch.tensor(counts, dtype=torch.int32, device="cuda")
    for mass in (False, True):
        for fold in (True, False):
            want, got, _ = _dense_and_table(ops, tuning, q, ks, vs, gk, gv, H=H, inc=True, fold=fold, presc=presc, valid=valid, mass=mass,
                                            dense=(dk, dv))
            _same(got, want, f"valid_refs with poisoned slots, tuning {tuning} fold={fold} mass={mass}")


def test_graph_replay_follows_fill(ops):
    """one table call captured on a side stream; ``fill_`` points the table at other identities' entries; the replay equals the
    eager dense call on those entries (the kernel reads the table when it runs)"""
    B, H, Lq, N, Lr, dtype = 2, 2, 200, 3, 72, torch.bfloat16
    g = torch.Generator().manual_seed(9)
    q, ks, vs = _qkv(g, B, Lq, H * 64, dtype, False)
    gk0, gv0 = _pool_grid(g, B, N, Lr, H * 64, dtype)
    gk1, gv1 = _pool_grid(g, B, N, Lr, H * 64, dtype, scale=0.7, shift=0.1)
    tk, tv = ops.RefKVTable.from_tensors(gk0), ops.RefKVTable.from_tensors(gv0)
    call = lambda rk, rv: ops.shared_attention(q, ks, vs, rk, rv, heads=H, scale=SCALE, include_self=True, return_lse=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(tk, tv)                                     # warm-up: the stream's workspace exists before the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = call(tk, tv)
    graph.replay()
    torch.cuda.synchronize()
    _same(res, call(_stack(gk0), _stack(gv0)), "replay on the captured entries")
    addr = tk.ptrs.data_ptr()
    tk.fill_(gk1)
    tv.fill_(gv1)
    assert tk.ptrs.data_ptr() == addr
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = call(_stack(gk1), _stack(gv1))
    _same(res, want, "replay after fill_")
    assert not torch.equal(res[0], call(_stack(gk0), _stack(gv0))[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_probability_readouts_take_a_key_table(ops, dtype):
    B, H, Lq, N, Lr = 2, 2, 128, 2, 72
    g = torch.Generator().manual_seed(13)
    q, ks, vs = _qkv(g, B, Lq, H * 64, dtype, False)
    gk, gv = _pool_grid(g, B, N, Lr, H * 64, dtype)
    dk, dv = _stack(gk), _stack(gv)
    tk = ops.RefKVTable.from_tensors(gk)
    _, lse = ops.shared_attention(q, ks, vs, dk, dv, heads=H, scale=SCALE, include_self=True, return_lse=True)
    kw = dict(heads=H, scale=SCALE, include_self=True)
    for kernel in ("auto", "generic"):
        _same(ops.attn_probs(q, ks, tk, lse, kernel=kernel, **kw), ops.attn_probs(q, ks, dk, lse, kernel=kernel, **kw), f"attn_probs {kernel}")
    _same(ops.attn_segment_mass(q, ks, tk, lse, **kw), ops.attn_segment_mass(q, ks, dk, lse, **kw), "attn_segment_mass")
    rows = torch.tensor([[0, 5, 127], [64, 3, 3]])
    for reduce in ("none", "map", "head_mean"):
        _same(ops.attn_rows(q, ks, tk, lse, rows, reduce=reduce, **kw), ops.attn_rows(q, ks, dk, lse, rows, reduce=reduce, **kw), f"attn_rows {reduce}")


def _cached_identity(ops, g, n_refs, L, Cc, H, dtype):
    keys = [torch.randn(1, n_refs, L, Cc, generator=g).to("cuda", dtype)]
    values = [(torch.randn(1, n_refs, L, Cc, generator=g) * 1.2 + 0.3).to("cuda", dtype)]
    return keys, values, [ops.token_stats(values[0], heads=H)]


def test_cache_tables_through_the_processor(ops):
    """``assemble_tables`` against ``assemble`` through ``SharedAttnProcessor`` (AdaIN on): bit-equal outputs, no K/V-sized
    allocation, identities with different reference counts in one batch, and a table that outlives its cache entries"""
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    from instantrestore_amd.kv_cache import ReferenceKVCache
    Cc, H, L, N, dtype = 128, 2, 256, 2, torch.bfloat16
    torch.manual_seed(21)
    attn = Attention(query_dim=Cc, heads=H, dim_head=64, processor=SharedAttnProcessor(self_attn_idx=0, use_adain=True, train_input=True)).eval().cuda()
    g = torch.Generator().manual_seed(22)
    cache = ReferenceKVCache()
    for name, n in (("a", N), ("b", N), ("one", 1)):
        cache.get_or_compute(name, lambda n=n: _cached_identity(ops, g, n, L, Cc, H, dtype))
    x = torch.randn(2, L, Cc, generator=g).cuda()

    def run(keys, values, stats, valid=None):
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
            return attn(x, ref_keys=keys, ref_values=values, ref_stats=stats, ref_valid=valid)

    torch.cuda.synchronize()
    kv_bytes = 2 * 2 * N * L * Cc * 2                         # keys and values of two identities
    m0 = torch.cuda.memory_allocated()
    dense = cache.assemble(["a", "b"])
    m1 = torch.cuda.memory_allocated()
    tables = cache.assemble_tables(["a", "b"])
    m2 = torch.cuda.memory_allocated()
    assert m1 - m0 >= kv_bytes, (m1 - m0, kv_bytes)
    assert m2 - m1 < (1 << 20), m2 - m1
    assert tables[3] is None
    want = run(*dense)
    _same(run(*tables), want, "assemble_tables vs assemble")
    # use_adain without statistics: an error that says what to do, never a dense copy behind the caller's back
    with pytest.raises(ValueError, match="ref_stats"):
        run(tables[0], tables[1], None)
    # 1 and 2 references in one batch against the dense zero-filled batch with ref_valid
    keys, values, stats, valid = cache.assemble_tables(["one", "b"])
    assert valid.tolist() == [1, 2]
    e1, eb = cache._store["one"], cache._store["b"]
    pad = lambda t: torch.cat([t, torch.zeros_like(t)], dim=1)
    dk, dv = [torch.cat([pad(e1[0][0]), eb[0][0]])], [torch.cat([pad(e1[1][0]), eb[1][0]])]
    ds = [(torch.cat([pad(e1[2][0][0]), eb[2][0][0]]), torch.cat([pad(e1[2][0][1]), eb[2][0][1]]))]
    _same(run(keys, values, stats, valid), run(dk, dv, ds, valid.clone()), "ragged batch vs zero-filled dense batch")
    # refill in place, then drop the cache: the tables keep their entries alive
    cache.refill_tables(tables, ["b", "a"])
    want_ba = run(*cache.assemble(["b", "a"]))
    cache.invalidate()
    assert len(cache) == 0
    junk = torch.full((8 * N * L * Cc,), float("nan"), dtype=dtype, device="cuda")      # what a freed entry would be reused for
    _same(run(*tables), want_ba, "tables after refill_tables and cache.invalidate()")
    del junk


def test_example_kv_tables_switch():
    """examples/synthetic_inference.py --kv-tables: the cached frame served through pointer tables reproduces the first frame
    (the example asserts it byte for byte)"""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "synthetic_inference.py")
    spec = importlib.util.spec_from_file_location("synthetic_inference_tables", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--identities", "2", "--refs", "3", "--px", "256", "--small", "--kv-tables", "--dtype", "bf16"])
    assert out.shape == (2, 256, 256, 3)
