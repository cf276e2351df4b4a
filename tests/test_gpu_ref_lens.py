"""Per-reference token counts of the fused attention on the GPU (``ir_shared_attn_ragged_args``, ``ops.shared_attention(ref_lens=)``,
``ops.compact_refs``): the RAGGED forms of the software-pipelined 32-row kernel against the float64 helper oracle
(``key_bias_oracle.biased_attention_np`` with ``-inf`` on every key behind a count - tests/test_ref_lens_cpu.py shows that this IS the
attention over the truncated references) on identical 16-bit-rounded inputs, held to ``parity_bounds.check_parity`` with its default
factors; every element of the LSE and of the masses to tests/lse_bounds.py (fp32 accuracy at the row's own scale), the bounds
tests/test_gpu_key_bias.py holds the same kernel family to.

What can go wrong and is looked at: the item's tile count and where a K/V-range piece starts (inside a later reference, nowhere at
all), the descriptor that must end at the count (NaN behind it), the step over an absent reference in both streams of the pipeline
(prefetch and softmax / fold), the cumulative masses across absent references, rows without any key, table slots that must not be
dereferenced, and that full counts leave the bytes of the uncounted form.

The shapes are the smallest at which the walk can go wrong: capacity 200 (four tiles, the last ragged) with counts that are full, 0,
one key past a tile, a single key, a whole tile, and ragged.  fp32 output: the same kernel stores the same numbers before their
rounding, so it is held to the same bounds and must round to the 16-bit output bit for bit.

Measured on an MI355X over the file's 143 ``check_parity`` comparisons (N(0, 1) inputs, the seeds below), err / regression bound:
75 in bf16 median 0.55, largest 0.87; 68 in fp16 median 0.47, largest 0.59 (both largest: Lq 128, no self block, no fold, pre-scaled Q)."""
import numpy as np
import pytest
import torch

from key_bias_oracle import biased_attention_np
from lse_bounds import check_lse, check_mass, pack_keys, row_scale
from parity_bounds import check_parity

pytestmark = pytest.mark.gpu

SCALE = 0.125
QC = SCALE * 1.4426950408889634
NEG = float("-inf")
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["f16", "bf16"]
COUNTS = [[200, 0, 65], [1, 64, 137]]      # full, absent, one key past a tile / a single key, a whole tile, ragged
TUNE_PRESC, TUNE_EARLYQK = 11, 14


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


def _np64(t):
    return None if t is None else t.float().cpu().numpy().astype(np.float64)


def _tail_bias(B, ls, cap, counts):
    """(B, Lkv) float64: -inf on every key t >= c of every reference"""
    N = len(counts[0])
    bias = np.zeros((B, ls + N * cap))
    for b in range(B):
        for n in range(N):
            bias[b, ls + n * cap + min(max(counts[b][n], 0), cap): ls + (n + 1) * cap] = NEG
    return bias


class Case:
    """inputs of one call (CPU, rounded to the 16-bit type), its counts, what the call needs on the device, and the oracle"""

    def __init__(self, B, H, Lq, Ls, N, cap, counts, dtype, presc, inc=True, adain=False, seed=0):
        self.B, self.H, self.Lq, self.Ls, self.N, self.cap, self.counts = B, H, Lq, Ls, N, cap, counts
        self.dtype, self.presc, self.inc, self.adain = dtype, presc, inc, adain
        Cc = H * 64
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s, sc=1.0, sh=0.0: (torch.randn(*s, generator=g) * sc + sh)
        q, k, v = rnd(B, Lq, Cc), rnd(B, Ls, Cc), rnd(B, Ls, Cc)
        rk, rv = rnd(B, N, cap, Cc), rnd(B, N, cap, Cc, sc=1.4, sh=-0.2)
        self.q = (q * QC if presc else q).to(dtype)
        self.q_true = _np64(self.q) / QC if presc else _np64(self.q)
        self.k, self.v, self.rk, self.rv = k.to(dtype), v.to(dtype), rk.to(dtype), rv.to(dtype)
        self.seg_lens = ([Ls] if inc else []) + [cap] * N
        self.lens = torch.tensor(counts, dtype=torch.int32)
        self._dev = self._ref = self._scales = None

    def dev(self):
        if self._dev is None:
            self._dev = tuple(t.cuda() for t in (self.q, self.k, self.v, self.rk, self.rv))
        return self._dev

    def run(self, ops, lens="own", rk=None, rv=None, aff="own", **kw):
        q, k, v, drk, drv = self.dev()
        rk, rv = drk if rk is None else rk, drv if rv is None else rv
        if isinstance(aff, str):     # the affine of the capacity tensors (they hold real data)
            aff = ops.adain_stats(v, drv, heads=self.H) if self.adain else None
        if isinstance(lens, str):
            lens = self.lens.cuda()
        return ops.shared_attention(q, k, v, rk, rv, heads=self.H, scale=SCALE, include_self=self.inc, adain=aff,
                                    q_prescaled=self.presc, ref_lens=lens, **kw)

    def oracle(self):
        """out, lse, mass - computed once per case and left unchanged"""
        if self._ref is None:
            bias = _tail_bias(self.B, self.Ls if self.inc else 0, self.cap, self.counts)
            self._ref = biased_attention_np(self.q_true, _np64(self.k), _np64(self.v), _np64(self.rk), _np64(self.rv), self.H, SCALE, bias,
                                            use_adain=self.adain, train_input=self.inc, seg_lens=self.seg_lens)
        return self._ref

    def scales(self):
        """tests/lse_bounds.py::row_scale of every (b, h, row) of the oracle's call, once per case"""
        if self._scales is None:
            bias = _tail_bias(self.B, self.Ls if self.inc else 0, self.cap, self.counts)
            self._scales = row_scale(self.q_true, pack_keys(self.k, self.rk, self.inc), SCALE, self.oracle()[1], bias=bias)
        return self._scales


def _check(case, got, what, ref=None, bias=None):
    """out, lse [, mass] of a call against the oracle (``ref`` with the ``bias`` it was computed with, or the case's own): the
    output to parity_bounds, every element of the LSE and of the masses to lse_bounds"""
    ro, rl, rm = case.oracle() if ref is None else ref
    err = check_parity(got[0], ro, case.dtype, what)
    live = np.isfinite(rl)
    if ref is None:
        sc = case.scales()
    else:
        sc = row_scale(case.q_true, pack_keys(case.k, case.rk, case.inc), SCALE, rl, bias=bias)
    check_lse(got[1], rl, sc, what)              # every element; -inf exactly on the rows without a key
    if len(got) > 2:
        m = got[2].cpu().numpy().astype(np.float64)
        assert np.isfinite(m).all(), what
        lives = live[..., None] & np.ones_like(m, dtype=bool)
        check_mass(m, rm, sc, what)
        assert np.abs(m.sum(-1)[live] - 1.0).max(initial=0.0) <= 1e-5, f"{what}: the masses of a row sum to 1"
        assert np.all(m[~lives] == 0.0), f"{what}: a row without keys has no mass"
        off = 1 if case.inc else 0
        for b in range(case.B):
            for n in range(case.N):
                if case.counts[b][n] <= 0:
                    assert np.all(m[b, :, :, off + n] == 0.0), f"{what}: the absent reference {n} of entry {b} carries exactly no mass"
    return err


_CASES = {}


def _small(dtype, presc, lq, inc, adain):
    key = (dtype, presc, lq, inc, adain)
    if key not in _CASES:
        _CASES[key] = Case(2, 2, lq, 72, 3, 200, COUNTS, dtype, presc, inc=inc, adain=adain, seed=1)
    return _CASES[key]


@pytest.mark.parametrize("lq", [128, 200])
@pytest.mark.parametrize("inc", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("adain", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_oracle_parity(ops, dtype, presc, adain, inc, lq):
    case = _small(dtype, presc, lq, inc, adain)
    what = f"counts Lq{lq} {'self' if inc else 'noself'} {'fold' if adain else 'plain'} {'prescq' if presc else 'plainq'}"
    got = case.run(ops, return_lse=True, return_mass=True)
    name = ops.shared_attention_kernel_name(*case.dev(), heads=case.H, scale=SCALE, include_self=inc, q_prescaled=presc, ref_lens=case.lens.cuda())
    assert "ragged refs" in name and "pipe_kernel" in name, name
    _check(case, got, what)
    # without the by-products: the same bytes (the MASS instantiation is a second one)
    assert torch.equal(case.run(ops), got[0])
    # fp32 out: the same numbers before their rounding
    o32 = case.run(ops, return_lse=True, out_dtype=torch.float32)
    assert o32[0].dtype == torch.float32 and torch.equal(o32[0].to(dtype), got[0]) and torch.equal(o32[1], got[1])
    check_parity(o32[0], case.oracle()[0], dtype, what + " fp32 out")


@pytest.mark.parametrize("adain", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_tails_do_not_exist(ops, dtype, presc, adain):
    """every row t >= c of K and V (the whole of a count-0 reference too) NaN, then random: the same bytes, and finite"""
    case = _small(dtype, presc, 200, True, adain)
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H) if adain else None        # the caller's affine: an input as before
    g = torch.Generator().manual_seed(2)
    outs = []
    for fill in ("nan", "random"):
        pk, pv = rk.clone(), rv.clone()
        for b in range(case.B):
            for n in range(case.N):
                c = case.counts[b][n]
                junk = torch.full((case.cap - c, case.H * 64), float("nan")) if fill == "nan" else 30 * torch.randn(case.cap - c, case.H * 64, generator=g)
                pk[b, n, c:] = junk.to(dtype).cuda()
                pv[b, n, c:] = junk.flip(0).to(dtype).cuda()
        outs.append(case.run(ops, rk=pk, rv=pv, aff=aff, return_lse=True, return_mass=True))
    for x, y in zip(*outs):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    for x, y in zip(outs[0], case.run(ops, return_lse=True, return_mass=True)):
        assert torch.equal(x, y)                                         # ... the bytes of the call on the clean tensors
    _check(case, outs[0], "poisoned tails")


FULL_SHAPES = [(2, 2, 200, 72, 3, 200), (9, 2, 1024, 1024, 4, 1024)]      # the small shape; a grid whose last round the default plan cuts


@pytest.mark.parametrize("form", ["presc_flag", "presc_tuning", "earlyqk"])
@pytest.mark.parametrize("adain", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("shape", FULL_SHAPES, ids=["small", "split"])
def test_full_counts_are_the_dense_call_bit_for_bit(ops, shape, adain, form):
    """ref_lens = len_ref everywhere: out, lse and masses ``torch.equal`` to the call without counts pinned to the same form by
    ``tuning`` (also counts above the capacity: they are clamped)"""
    B, H, Lq, Ls, N, cap = shape
    presc = form == "presc_flag"
    case = Case(B, H, Lq, Ls, N, cap, [[cap] * N] * B, torch.bfloat16, presc, adain=adain, seed=3)
    prev = ops.set_attn_variant(TUNE_EARLYQK if form == "earlyqk" else TUNE_PRESC)
    try:
        dense = case.run(ops, lens=None, return_lse=True, return_mass=True)
        dname = ops.shared_attention_kernel_name(*case.dev(), heads=H, scale=SCALE, q_prescaled=presc)
        full = case.run(ops, return_lse=True, return_mass=True)
        over = case.run(ops, lens=torch.full((B, N), cap + 77, dtype=torch.int32, device="cuda"), return_lse=True, return_mass=True)
        name = ops.shared_attention_kernel_name(*case.dev(), heads=H, scale=SCALE, q_prescaled=presc, ref_lens=case.lens.cuda())
    finally:
        ops.set_attn_variant(prev)
    assert "pipe_kernel" in dname and "ragged" not in dname and name.startswith(dname[:-1]) and "ragged refs" in name, (dname, name)
    for x, y, z in zip(dense, full, over):
        assert torch.equal(x, y) and torch.equal(x, z)
    if form != "presc_tuning":       # under the default dispatch the counted call is the same form (without the flag: the early-QK one)
        for x, y in zip(full, case.run(ops, return_lse=True, return_mass=True)):
            assert torch.equal(x, y)


# ---- K/V-range pieces ---------------------------------------------------------------------------------------------------------
# N 4, capacity 256, len_self 128: 18 capacity tiles -> the batch-invariant plan cuts every item in 2 pieces (16 tiles without the
# self block: 2 as well).  Pieces are cut over the tiles that EXIST: [nt * p / 2, nt * (p + 1) / 2).
PIECE_COUNTS_NOSELF = [[0, 0, 0, 5],        # 1 tile: piece 0 is empty, piece 1 starts (and ends) inside reference 3
                       [256, 0, 100, 64],   # 7 tiles: piece 1 starts at tile 3 of reference 0
                       [64, 0, 200, 256],   # 9 tiles: piece 1 starts at tile 3 of reference 2, behind an absent one
                       [0, 0, 0, 0]]        # no key at all: both pieces empty
PIECE_COUNTS_SELF = [[0, 0, 0, 0],          # the self block alone: one tile per piece
                     [1, 0, 256, 0],        # 7 tiles: piece 1 starts at tile 0 of reference 2, behind an absent one
                     [256, 256, 256, 256],  # full
                     [0, 65, 0, 129]]       # 7 tiles: absent references between, before and behind


@pytest.mark.parametrize("adain", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("inc", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_pieces_that_are_empty_or_start_inside_a_later_reference(ops, dtype, presc, inc, adain):
    B, H, Lq, Ls, N, cap = 4, 2, 128, 128, 4, 256
    plan = ops.shared_attention_plan(B, Lq, H, len_self=Ls, n_refs=N, len_ref=cap, dtype=dtype, include_self=inc, adain=adain,
                                     q_prescaled=presc, return_mass=True, ref_lens=True)
    assert plan["pieces_per_item"] == 2 and plan["rows_per_item"] == 128, plan
    case = Case(B, H, Lq, Ls, N, cap, PIECE_COUNTS_SELF if inc else PIECE_COUNTS_NOSELF, dtype, presc, inc=inc, adain=adain, seed=4)
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=H) if adain else None
    lens = case.lens.cuda()

    def run(idx):
        i = torch.tensor(idx, device="cuda")
        a = None if aff is None else (aff[0][i].contiguous(), aff[1][i].contiguous())
        return ops.shared_attention(q[i], k[i], v[i], rk[i], rv[i], heads=H, scale=SCALE, include_self=inc, adain=a, q_prescaled=presc,
                                    ref_lens=lens[i].contiguous(), return_lse=True, return_mass=True, batch_invariant=True)
    whole = run([0, 1, 2, 3])
    _check(case, whole, f"pieces {'self' if inc else 'noself'}")
    rev = run([3, 2, 1, 0])
    for b in range(B):
        alone = run([b])
        for x, y, z in zip(alone, whole, rev):
            assert torch.equal(x[0], y[b]) and torch.equal(x[0], z[B - 1 - b]), f"entry {b} depends on its batch"
    # the default dispatch, with the plan of its own, meets the same oracle
    _check(case, case.run(ops, aff=aff, return_lse=True, return_mass=True), "whole items")


@pytest.mark.parametrize("adain", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_an_entry_without_any_key(ops, dtype, presc, adain):
    """no self block and every count of entry 1 at 0: zeros, lse = -inf, masses 0, no NaN - and entry 0 does not notice"""
    case = Case(2, 2, 200, 72, 3, 200, [COUNTS[0], [0, 0, 0]], dtype, presc, inc=False, adain=adain, seed=5)
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H) if adain else None
    for bi in (False, True):
        out, lse, mass = case.run(ops, aff=aff, return_lse=True, return_mass=True, batch_invariant=bi)
        assert torch.isfinite(out).all() and not torch.isnan(lse).any() and not torch.isnan(mass).any()
        assert out[1].abs().max() == 0 and bool(torch.isneginf(lse[1]).all()) and mass[1].abs().max() == 0
        assert bool(torch.isfinite(lse[0]).all())
        _check(case, (out, lse, mass), f"entry without keys (batch_invariant={bi})")
        o32 = case.run(ops, aff=aff, out_dtype=torch.float32, batch_invariant=bi)
        assert o32[1].abs().max() == 0 and torch.equal(o32.to(dtype), out)
    a0 = None if aff is None else (aff[0][:1].contiguous(), aff[1][:1].contiguous())
    alone = ops.shared_attention(q[:1], k[:1], v[:1], rk[:1], rv[:1], heads=case.H, scale=SCALE, include_self=False, adain=a0, q_prescaled=presc,
                                 ref_lens=case.lens[:1].cuda(), return_lse=True, return_mass=True, batch_invariant=True)
    for x, y in zip(alone, (out, lse, mass)):
        assert torch.equal(x[0], y[0])


# ---- pointer tables -----------------------------------------------------------------------------------------------------------
def _pool_tables(ops, case, null_absent):
    """every reference cut from one pool in shuffled order; an absent reference's slot holds the address 0"""
    q, k, v, rk, rv = case.dev()
    B, N, cap, Cc = case.B, case.N, case.cap, case.H * 64
    perm = torch.randperm(B * N, generator=torch.Generator().manual_seed(6)).tolist()
    pool_k = torch.empty(B * N, cap, Cc, dtype=case.dtype, device="cuda")
    pool_v = torch.empty(B * N, cap, Cc, dtype=case.dtype, device="cuda")
    grid_k, grid_v = [[None] * N for _ in range(B)], [[None] * N for _ in range(B)]
    for slot, i in enumerate(perm):
        b, n = divmod(i, N)
        pool_k[slot].copy_(rk[b, n])
        pool_v[slot].copy_(rv[b, n])
        grid_k[b][n], grid_v[b][n] = pool_k[slot], pool_v[slot]
    tk, tv = ops.RefKVTable.from_tensors(grid_k), ops.RefKVTable.from_tensors(grid_v)
    if null_absent:
        for b in range(B):
            for n in range(N):
                if case.counts[b][n] == 0:
                    tk.ptrs[b, n] = 0
                    tv.ptrs[b, n] = 0
    return tk, tv


@pytest.mark.parametrize("adain", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
def test_table_call_gives_the_dense_bytes_and_never_reads_an_absent_slot(ops, presc, adain):
    case = _small(torch.bfloat16, presc, 200, True, adain)
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H) if adain else None
    tk, tv = _pool_tables(ops, case, null_absent=True)
    assert int(tk.ptrs[0, 1]) == 0 and int((tk.ptrs == 0).sum()) == 1
    for bi in (False, True):
        dense = case.run(ops, aff=aff, return_lse=True, return_mass=True, batch_invariant=bi)
        table = case.run(ops, rk=tk, rv=tv, aff=aff, return_lse=True, return_mass=True, batch_invariant=bi)
        for x, y in zip(table, dense):
            assert torch.equal(x, y)
    _check(case, table, "tables")
    with pytest.raises(ValueError, match="valid_refs"):
        case.run(ops, rk=tk, rv=tv, aff=aff, valid_refs=torch.tensor([3, 3], dtype=torch.int32, device="cuda"))


def test_a_captured_call_follows_an_in_place_change_of_the_counts(ops):
    case = _small(torch.bfloat16, True, 200, True, True)
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H)
    tk, tv = _pool_tables(ops, case, null_absent=False)
    lens = torch.full((case.B, case.N), case.cap, dtype=torch.int32, device="cuda")
    call = lambda rl: case.run(ops, lens=rl, rk=tk, rv=tv, aff=aff, return_lse=True, return_mass=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(lens)                                       # warm-up: the stream's workspace exists before the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = call(lens)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(res, case.run(ops, lens=None, aff=aff, return_lse=True, return_mass=True)):
        assert torch.equal(x, y)                         # full counts: the dense call
    addr = lens.data_ptr()
    lens.copy_(case.lens)
    assert lens.data_ptr() == addr
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(res, call(lens.clone())):
        assert torch.equal(x, y)
    _check(case, res, "replay after the counts changed")


# ---- compaction ---------------------------------------------------------------------------------------------------------------
def _gather(rk, keep):
    """torch reference of the compaction: kept rows to the front, in order"""
    B, N = keep.shape[:2]
    out = torch.zeros_like(rk)
    lens = torch.zeros(B, N, dtype=torch.int32)
    for b in range(B):
        for n in range(N):
            rows = rk[b, n][keep[b, n]]
            out[b, n, : rows.shape[0]] = rows
            lens[b, n] = rows.shape[0]
    return out, lens


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(2, 2, 3, 200), (1, 5, 2, 1024), (2, 9, 2, 257)], ids=["L200", "H5L1024", "H9L257"])
def test_compaction_is_a_stable_gather_that_leaves_the_tail_alone(ops, shape, dtype):
    B, H, N, L = shape
    g = torch.Generator().manual_seed(7)
    # row t of K holds t in its first element: order and identity of every moved row are visible
    rk, rv = torch.randn(B, N, L, H * 64, generator=g).to(dtype), torch.randn(B, N, L, H * 64, generator=g).to(dtype)
    rk[..., 0] = (torch.arange(L) % 251).to(dtype)
    keep = torch.rand(B, N, L, generator=g) < 0.4
    keep[0, 0] = True                                    # everything kept
    keep[0, 1] = False                                   # nothing kept
    keep[-1, -1] = False
    keep[-1, -1, L - 1] = True                           # the last row alone
    wk, wl = _gather(rk, keep)
    wv, _ = _gather(rv, keep)
    sent = torch.full_like(rk, 7.0)
    ok, ov, ol = sent.clone().cuda(), (sent * 2).cuda(), torch.full((B, N), -1, dtype=torch.int32, device="cuda")
    res = ops.compact_refs(rk.cuda(), rv.cuda(), keep.cuda(), heads=H, out=(ok, ov, ol))
    assert res[0] is ok and res[1] is ov and res[2] is ol
    assert torch.equal(ol.cpu(), wl)
    for b in range(B):
        for n in range(N):
            c = int(wl[b, n])
            assert torch.equal(ok[b, n, :c].cpu(), wk[b, n, :c]) and torch.equal(ov[b, n, :c].cpu(), wv[b, n, :c]), (b, n)
            assert bool((ok[b, n, c:] == 7.0).all()) and bool((ov[b, n, c:] == 14.0).all()), "rows behind the count are not written"
    k2, v2, l2 = ops.compact_refs(rk.cuda(), rv.cuda(), keep.cuda(), heads=H)          # fresh buffers; deterministic
    assert torch.equal(l2, ol) and all(torch.equal(k2[b, n, :int(wl[b, n])], ok[b, n, :int(wl[b, n])]) for b in range(B) for n in range(N))
    # strided inputs (the K third of a fused projection) and rows of a wider counts buffer
    fused = torch.zeros(B, N, L, 3 * H * 64, dtype=dtype)
    fused[..., H * 64: 2 * H * 64] = rk
    fused = fused.cuda()
    wide = torch.full((B, N + 3), -1, dtype=torch.int32, device="cuda")
    k3, _, l3 = ops.compact_refs(fused[..., H * 64: 2 * H * 64], rv.cuda(), keep.cuda(), heads=H, out=(torch.empty_like(ok), torch.empty_like(ov), wide[:, :N]))
    assert torch.equal(l3.cpu(), wl) and bool((wide[:, N:] == -1).all())
    assert all(torch.equal(k3[b, n, :int(wl[b, n])], ok[b, n, :int(wl[b, n])]) for b in range(B) for n in range(N))
    with pytest.raises(Exception, match="aliasing"):
        ops.compact_refs(ok, ov, keep.cuda(), heads=H, out=(ok, ov, ol))
    # ... and an output that overlaps an input at another offset: a view into the same allocation, eight rows further on
    big = torch.zeros(B, N, L + 8, H * 64, dtype=dtype, device="cuda")
    with pytest.raises(Exception, match="aliasing"):
        ops.compact_refs(big[:, :, :L], rv.cuda(), keep.cuda(), heads=H, out=(big[:, :, 8:], ov, ol))


def test_compaction_pools_a_keep_map_like_the_key_bias(ops):
    B, N, side, H = 1, 2, 16, 2
    g = torch.Generator().manual_seed(8)
    keep = torch.rand(B, N, 64, 64, generator=g) < 0.5
    keep[0, 0, :32] = True
    rk, rv = torch.randn(B, N, side * side, H * 64, generator=g).bfloat16().cuda(), torch.randn(B, N, side * side, H * 64, generator=g).bfloat16().cuda()
    row = ops.key_bias(B, 0, N, side * side, False, ref_token_keep=keep)
    tok = (row == 0).view(B, N, side * side)
    _, _, lens = ops.compact_refs(rk, rv, keep.cuda(), heads=H)
    k2, _, lens2 = ops.compact_refs(rk, rv, tok.cuda(), heads=H)
    assert torch.equal(lens, lens2) and torch.equal(lens.cpu(), tok.sum(-1).to(torch.int32))
    k1, _, _ = ops.compact_refs(rk, rv, keep.cuda(), heads=H)
    assert all(torch.equal(k1[0, n, :int(lens[0, n])], k2[0, n, :int(lens[0, n])]) for n in range(N))


@pytest.mark.parametrize("adain", [False, True], ids=["plain", "fold"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_compacted_call_and_bias_call_meet_the_same_oracle(ops, dtype, presc, adain):
    """end to end: compact under a scattered mask, attend with the counts and the affine of the UNCOMPACTED references - against the
    oracle with the mask as a -inf bias; today's way (the bias call with the same mask) is held to the same oracle"""
    case = Case(2, 2, 200, 72, 3, 200, [[200] * 3] * 2, dtype, presc, adain=adain, seed=9)
    g = torch.Generator().manual_seed(10)
    keep = torch.rand(case.B, case.N, case.cap, generator=g) < 0.5
    keep[0, 1] = False                                   # a wholly dropped reference
    keep[1, 2, 70:] = False
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H) if adain else None
    bias = ops.key_bias(case.B, case.Ls, case.N, case.cap, True, ref_token_keep=keep)
    ref = biased_attention_np(case.q_true, _np64(case.k), _np64(case.v), _np64(case.rk), _np64(case.rv), case.H, SCALE, bias.numpy().astype(np.float64),
                              use_adain=adain, train_input=True, seg_lens=case.seg_lens)
    ck, cv, lens = ops.compact_refs(rk, rv, keep.cuda(), heads=case.H)
    assert torch.equal(lens.cpu(), keep.sum(-1).to(torch.int32))
    case.counts = lens.cpu().tolist()                    # (what _check reads for the absent references)
    got = case.run(ops, lens=lens, rk=ck, rv=cv, aff=aff, return_lse=True, return_mass=True)
    _check(case, got, "compacted", ref=ref, bias=bias.numpy().astype(np.float64))
    biased = ops.shared_attention(q, k, v, rk, rv, heads=case.H, scale=SCALE, include_self=True, adain=aff, q_prescaled=presc,
                                  key_bias=bias.cuda(), return_lse=True, return_mass=True)
    _check(case, biased, "bias call with the same mask", ref=ref, bias=bias.numpy().astype(np.float64))


# ---- processor ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adain", [False, True], ids=["plain", "adain"])
def test_shared_processor_with_counts_and_full_reference_statistics(ops, adain):
    """a shared layer with ref_lens (and, with AdaIN, the content statistics of the full references as ref_stats) against the helper
    oracle driven through the same projections; two runs give the same bytes"""
    from face_replace.models.attn_processors import AttnProcessor, SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    B, L, N, H, dtype = 2, 256, 3, 2, torch.bfloat16
    C = 64 * H
    g = torch.Generator().manual_seed(21)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype).float()
    d = dict(wq=r(C, C, sc=C ** -0.5), wk=r(C, C, sc=C ** -0.5), wv=r(C, C, sc=C ** -0.5), wo=r(C, C, sc=C ** -0.5), bo=r(C, sc=0.1))
    hidden, rk, rv = r(B, L, C), r(B, N, L, C), r(B, N, L, C, sc=1.3)
    counts = [[256, 0, 65], [1, 64, 137]]
    lens = torch.tensor(counts, dtype=torch.int32).cuda()
    proc = SharedAttnProcessor(self_attn_idx=0, use_adain=adain, train_input=True)
    proc.save_attention_mass = True
    def host(p):
        a = Attention(query_dim=C, heads=H, dim_head=64)
        with torch.no_grad():
            a.to_q.weight.copy_(d["wq"]); a.to_k.weight.copy_(d["wk"]); a.to_v.weight.copy_(d["wv"])
            a.to_out[0].weight.copy_(d["wo"]); a.to_out[0].bias.copy_(d["bo"])
        a = a.cuda()
        a.set_processor(p)
        return a
    attn = host(proc)
    drk, drv = rk.to(dtype).cuda(), rv.to(dtype).cuda()
    kwargs = dict(ref_keys=[drk], ref_values=[drv], ref_lens=[lens])
    if adain:
        kwargs["ref_stats"] = [ops.token_stats(drv, heads=H)]
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        if adain:
            with pytest.raises(ValueError, match="ref_stats"):
                attn(hidden.cuda(), ref_keys=[drk], ref_values=[drv], ref_lens=[lens])
        out = attn(hidden.cuda(), **kwargs)
        mass = proc.attention_mass.clone()
        again = attn(hidden.cuda(), **kwargs)
        assert torch.equal(out, again) and torch.equal(mass, proc.attention_mass)
        cap = host(AttnProcessor())
        assert torch.equal(cap(hidden.cuda(), ref_lens=[lens]), cap(hidden.cuda()))
    f = lambda t: t.numpy().astype(np.float64)
    rnd = lambda a: torch.from_numpy(a).to(dtype).double().numpy()
    q, k, v = (rnd(f(hidden) @ f(d[n]).T) for n in ("wq", "wk", "wv"))
    bias = _tail_bias(B, L, L, counts)
    core, _, rmass = biased_attention_np(q, k, v, f(rk), f(rv), H, 0.125, bias, use_adain=adain, train_input=True, seg_lens=[L] * (N + 1))
    ref = core @ f(d["wo"]).T + f(d["bo"])
    check_parity(out, ref, dtype, "shared layer with ref_lens", factor=2.0)    # two more 16-bit GEMM roundings (core, out), as tests/test_gpu_key_bias.py
    gm = mass.double().cpu().numpy()
    assert np.all(gm[0, :, :, 2] == 0.0) and np.abs(gm.sum(-1) - 1).max() <= 1e-5 and np.abs(gm - rmass).max() <= 4e-3
