"""Reference K/V through pointer tables (``ir_shared_attn_table_args`` / ``ops.RefKVTable`` / ``ReferenceKVCache.assemble_tables``):
everything that can be checked without a GPU - the block's size rule, the rules of a table call, that the dispatch and the
batch-invariant plan never look at the tables, and the host side of the table classes on CPU tensors."""
import ctypes as C
import itertools

import pytest
import torch

INVALID = -1
CFG2_CLASSES = [(8, 4, 4096, 5), (8, 4, 1024, 10), (8, 4, 256, 20)]     # (B, N, L, heads) of cfg 2's three shared layer classes
CFG4_TOP = (8, 8, 4096, 5)                                              # cfg 4: eight references


def _args(lib_mod, *, table, B=2, N=2, L=64, H=1, flags=1, valid=False, mass=False, adain=False):
    """a valid self + N-reference call on addresses that are never dereferenced (validation and planning precede any launch)"""
    a = lib_mod.SharedAttnTableArgs() if table else lib_mod.SharedAttnArgs()
    a.struct_size = C.sizeof(a)
    c = 64 * H
    a.dtype, a.batch, a.heads, a.len_q, a.len_self, a.flags, a.scale = 1, B, H, L, L, flags, 0.125
    a.q = a.k_self = a.v_self = a.out = 4096
    a.q_sb = a.ks_sb = a.vs_sb = a.o_sb = L * c
    a.q_sl = a.ks_sl = a.vs_sl = a.o_sl = c
    a.q_sh = a.ks_sh = a.vs_sh = a.o_sh = 64
    a.n_refs, a.len_ref = N, L
    a.kr_sl = a.vr_sl = c
    a.kr_sh = a.vr_sh = 64
    if table:
        a.k_ref_table, a.v_ref_table = 8192, 8192 + 8 * B * N
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
    return a


def test_abi_version_stays_10_and_both_block_sizes_are_taken():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    assert lib.ir_abi_version() == 10 == _lib.ABI_VERSION
    old, new = C.sizeof(_lib.SharedAttnArgs), C.sizeof(_lib.SharedAttnTableArgs)
    assert new == old + 16 and _lib.SharedAttnTableArgs.k_ref_table.offset == old and _lib.SharedAttnTableArgs.v_ref_table.offset == old + 8
    assert [f[0] for f in _lib.SharedAttnTableArgs._fields_] == ["k_ref_table", "v_ref_table"]
    dense = _args(_lib, table=False)
    assert lib.ir_shared_attn_kernel_name(C.byref(dense)) != b""                      # the block that ends behind seg_mass
    tab = _args(_lib, table=True)
    assert lib.ir_shared_attn_kernel_name(C.byref(tab)) != b""                        # ... and the one with the two table fields
    long_dense = _args(_lib, table=True)                                                # the long block with both tables NULL: a dense call
    long_dense.k_ref_table = long_dense.v_ref_table = None
    long_dense.k_ref = long_dense.v_ref = 4096
    long_dense.kr_sb = long_dense.vr_sb = 2 * 64 * 64
    long_dense.kr_sn = long_dense.vr_sn = 64 * 64
    assert lib.ir_shared_attn_kernel_name(C.byref(long_dense)) == lib.ir_shared_attn_kernel_name(C.byref(dense)) != b""
    for bad in (7, old + 8, new + 8, old - 8):
        tab.struct_size = bad
        assert lib.ir_shared_attn_kernel_name(C.byref(tab)) == b"" and b"ABI mismatch" in lib.ir_last_error_string()
        assert lib.ir_shared_attn_fwd(C.byref(tab), None) == INVALID


def test_the_rules_of_a_table_call_are_checked_before_any_launch():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.ir_last_error_string()
    calls = [lambda a: lib.ir_shared_attn_fwd(C.byref(a), None),
             lambda a: lib.ir_attn_segment_mass(C.byref(a), 4096, None),
             lambda a: lib.ir_attn_rows(C.byref(a), 4096, 1, 0, 4096, None)]
    for call in calls:
        a = _args(_lib, table=True)
        a.lse = 4096
        a.v_ref_table = None                                          # one table without the other
        assert call(a) == INVALID and b"both" in err() and b"v_ref_table" in err()
        a = _args(_lib, table=True)
        a.k_ref_table = None
        assert call(a) == INVALID and b"both" in err()
        a = _args(_lib, table=True)
        a.k_ref = 4096                                                # a table together with k_ref
        assert call(a) == INVALID and b"k_ref and v_ref must be NULL" in err()
        a = _args(_lib, table=True)
        a.n_refs = 0                                                  # a table without references
        assert call(a) == INVALID and b"n_refs > 0" in err()
        for field in ("kr_sb", "kr_sn", "vr_sb", "vr_sn"):            # the tables hold every base address
            a = _args(_lib, table=True)
            setattr(a, field, 64)
            assert call(a) == INVALID and b"must be 0" in err() and field.encode() in err()


def _plan(lib_mod, a):
    p = lib_mod.SharedAttnPlan()
    p.struct_size = C.sizeof(p)
    rc = lib_mod.lib().ir_shared_attn_plan(C.byref(a), C.byref(p))
    return (rc,) + tuple(getattr(p, n) for n, _ in lib_mod.SharedAttnPlan._fields_[1:])


@pytest.mark.parametrize("shape", CFG2_CLASSES + [CFG4_TOP], ids=lambda s: "B%d_N%d_L%d_H%d" % s)
def test_dispatch_and_plan_do_not_look_at_the_tables(shape):
    """host only: the same kernel name, batch-invariant plan and workspace size for table and dense arguments"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    B, N, L, H = shape
    seen = set()
    for presc, valid, mass, bi, adain in itertools.product((False, True), repeat=5):
        flags = 1 | (2 if presc else 0) | (8 if bi else 0)
        kw = dict(B=B, N=N, L=L, H=H, flags=flags, valid=valid, mass=mass, adain=adain)
        dense, tab = _args(_lib, table=False, **kw), _args(_lib, table=True, **kw)
        name = lib.ir_shared_attn_kernel_name(C.byref(dense))
        assert name != b"" and lib.ir_shared_attn_kernel_name(C.byref(tab)) == name, kw
        assert lib.ir_shared_attn_workspace_bytes_for(C.byref(tab)) == lib.ir_shared_attn_workspace_bytes_for(C.byref(dense))
        seen.add(name)
        if bi:
            pd, pt = _plan(_lib, dense), _plan(_lib, tab)
            assert pd[0] == 0 and pt == pd, (kw, pd, pt)
            assert lib.ir_shared_attn_workspace_bytes_for(C.byref(tab)) == pd[-1]
        else:
            assert _plan(_lib, tab)[0] == _plan(_lib, dense)[0] == INVALID          # the plan is the batch-invariant mode's
    if L == 4096:      # the top layer's pre-scaled call stays on the 128-row kernel: its plain instantiation takes tables
        assert any(b"w128" in n and b"segment masses" not in n and b"zero suffix" not in n and b"forms" not in n for n in seen)


def _pool_entries(n, L=8, Cc=64, dtype=torch.bfloat16, gap=3):
    pool = torch.zeros(n * (L * Cc + gap * 8) + 64, dtype=dtype)
    off = (-pool.data_ptr() // pool.element_size()) % 8                # first 16-byte aligned element
    return pool, [pool[off + i * (L * Cc + gap * 8): off + i * (L * Cc + gap * 8) + L * Cc].view(L, Cc) for i in range(n)]


def test_ref_kv_table_from_tensors_on_cpu_tensors():
    from instantrestore_amd.ops import RefKVTable
    pool, e = _pool_entries(6)
    grid = [[e[4], e[1], e[3]], [e[0], e[5], e[2]]]
    t = RefKVTable.from_tensors(grid)
    assert t.ptrs.dtype == torch.int64 and tuple(t.ptrs.shape) == (2, 3) and t.ptrs.is_contiguous()
    assert tuple(t.shape) == (2, 3, 8, 64) and t.dtype == torch.bfloat16 and t.device == pool.device and t.row_stride == 64 and t.dim() == 4
    for b in range(2):
        for n in range(3):
            assert int(t.ptrs[b, n]) == grid[b][n].data_ptr()
    assert len(t.tensors) == 6 and all(any(x is y for y in t.tensors) for r in grid for x in r)      # the table keeps its entries alive
    # fill_ rewrites ptrs in place
    addr = t.ptrs.data_ptr()
    t.fill_([[e[0], e[1], e[2]], [e[3], e[4], e[5]]])
    assert t.ptrs.data_ptr() == addr and int(t.ptrs[1, 0]) == e[3].data_ptr()
    with pytest.raises(ValueError, match="match"):
        t.fill_([[e[0], e[1]], [e[3], e[4]]])
    # a misaligned entry
    flat = pool.view(-1)
    off = (-pool.data_ptr() // 2) % 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        RefKVTable.from_tensors([[e[0], flat[off + 4: off + 4 + 512].view(8, 64)]])
    # mixed dtype, length, row stride
    with pytest.raises(ValueError, match="dtype"):
        RefKVTable.from_tensors([[e[0], torch.zeros(8, 64, dtype=torch.float16)]])
    with pytest.raises(ValueError, match="shapes"):
        RefKVTable.from_tensors([[e[0], torch.zeros(16, 64, dtype=torch.bfloat16)]])
    wide = torch.zeros(8, 192, dtype=torch.bfloat16)
    third = wide[:, 64:128]
    if third.data_ptr() % 16 == 0:
        with pytest.raises(ValueError, match="row strides"):
            RefKVTable.from_tensors([[e[0], third]])
        assert RefKVTable.from_tensors([[wide[:, :64], third]]).row_stride == 192        # thirds of one fused buffer: a table of their own
    # None only where a valid count excludes the slot
    with pytest.raises(ValueError, match="None"):
        RefKVTable.from_tensors([[e[0], None]])
    with pytest.raises(ValueError, match="None"):
        RefKVTable.from_tensors([[e[0], None], [None, e[1]]], valid=[1, 1])
    ok = RefKVTable.from_tensors([[e[0], None], [None, None]], valid=[1, 0])
    assert int(ok.ptrs[0, 1]) == e[0].data_ptr() and int(ok.ptrs[1, 0]) == e[0].data_ptr()          # readable addresses, never used


def test_table_calls_have_no_cpu_path_and_never_densify():
    from instantrestore_amd import ops
    _pool, e = _pool_entries(2)
    t = ops.RefKVTable.from_tensors([[e[0], e[1]]])
    q = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.shared_attention(q, q, q, t, t, heads=1, scale=0.125)
    with pytest.raises(TypeError, match="both"):
        ops.shared_attention(q, q, q, t, torch.zeros(1, 2, 8, 64, dtype=torch.bfloat16), heads=1, scale=0.125)
    with pytest.raises(TypeError, match="cached content statistics"):
        ops.adain_stats(q, t, heads=1)


def _identity(n, seed, layers=3, H=2, L=8):
    g = torch.Generator().manual_seed(seed)
    keys = [torch.randn(1, n, L, H * 64, generator=g).to(torch.bfloat16) for _ in range(layers)]
    values = [torch.randn(1, n, L, H * 64, generator=g).to(torch.bfloat16) for _ in range(layers)]
    stats = [(torch.randn(1, n, H, 64, generator=g), torch.rand(1, n, H, 64, generator=g) + 0.5) for _ in range(layers)]
    return keys, values, stats


def test_assemble_tables_on_cpu_entries():
    from instantrestore_amd.kv_cache import ReferenceKVCache
    from instantrestore_amd.ops import RefKVTable
    cache = ReferenceKVCache()
    for name, n, seed in (("a", 2, 0), ("b", 1, 1), ("c", 2, 2)):
        cache.get_or_compute(name, lambda n=n, seed=seed: _identity(n, seed))
    keys, values, stats, valid = cache.assemble_tables(["b", "a"])
    assert list(cache._store) == ["c", "b", "a"]                                   # touched as assemble() touches it
    dk, dv, ds = cache.assemble(["a", "c"])
    assert list(cache._store) == ["b", "a", "c"]
    assert len(keys) == len(values) == 3 and all(isinstance(t, RefKVTable) for t in list(keys) + list(values))
    assert valid.dtype == torch.int32 and valid.tolist() == [1, 2]
    eb, ea = cache._store["b"], cache._store["a"]
    for side, tabs in ((0, keys), (1, values)):
        for l, t in enumerate(tabs):
            assert tuple(t.shape) == (2, 2, 8, 128) and t.dtype == torch.bfloat16 and t.row_stride == 128
            assert t.ptrs.tolist() == [[eb[side][l][0, 0].data_ptr(), eb[side][l][0, 0].data_ptr()],      # unused slot: reference 0
                                       [ea[side][l][0, 0].data_ptr(), ea[side][l][0, 1].data_ptr()]]
            assert any(x is eb[side][l] for x in t.tensors) and any(x is ea[side][l] for x in t.tensors)
    # all 18 (here 6) pointer arrays in one buffer
    base = keys[0].ptrs.data_ptr()
    assert [t.ptrs.data_ptr() - base for t in list(keys) + list(values)] == [32 * i for i in range(6)]
    for l, (mean, std) in enumerate(stats):
        assert tuple(mean.shape) == tuple(std.shape) == (2, 2, 2, 64) and mean.dtype == torch.float32
        assert torch.equal(mean[0, 0], eb[2][l][0][0, 0]) and torch.equal(std[1], ea[2][l][1][0])
        assert mean[0, 1].abs().max() == 0 and std[0, 1].abs().max() == 0           # (0, 0): what the harvest writes for a zero-filled reference
    # equal counts: no valid tensor - the call is the dense call's
    k2, v2, s2, valid2 = cache.assemble_tables(["a", "c"])
    assert valid2 is None and torch.equal(s2[1][0], ds[1][0])
    assert k2[2].ptrs.tolist() == [[ea[0][2][0, n].data_ptr() for n in range(2)], [cache._store["c"][0][2][0, n].data_ptr() for n in range(2)]]
    # refill in place
    addr = [t.ptrs.data_ptr() for t in keys], stats[0][0].data_ptr(), valid.data_ptr()
    cache.refill_tables((keys, values, stats, valid), ["c", "b"])
    assert ([t.ptrs.data_ptr() for t in keys], stats[0][0].data_ptr(), valid.data_ptr()) == addr
    assert valid.tolist() == [2, 1] and values[1].ptrs[1].tolist() == [eb[1][1][0, 0].data_ptr()] * 2
    assert torch.equal(stats[2][1][0], cache._store["c"][2][2][1][0]) and stats[2][1][1, 1].abs().max() == 0
    with pytest.raises(ValueError, match="without valid"):
        cache.refill_tables((k2, v2, s2, valid2), ["a", "b"])
    with pytest.raises(KeyError):
        cache.assemble_tables(["a", "nobody"])
    # a table outlives its cache entries
    held = keys[0].tensors
    cache.invalidate()
    assert len(cache) == 0 and keys[0].ptrs[0, 0] == held[0][0, 0].data_ptr()
