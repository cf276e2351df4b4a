"""Region-restricted attention on the GPU (``ir_shared_attn_region_args``, ``ops.shared_attention(q_allow=, key_region=)``): the REGION
forms of the software-pipelined 32-row kernel against the float64 oracle (``region_oracle``) on identical 16-bit-rounded inputs.

``out`` is held to ``parity_bounds.check_parity`` with its default factors (the stated tolerance and the calibrated regression bound,
as tests/test_gpu_key_bias.py applies them); every element of the LSE and of the by-product masses to tests/lse_bounds.py's constants
(class "fp32", KAPPA_MASS) at the row's own scale - ``max(1, |lse_ref|, T_row)`` with T_row taken over the ALLOWED keys that carry
weight, which is ``lse_bounds.row_scale``'s definition with a mask that has a query axis.  Rows without an allowed key: ``lse = -inf``
exactly, ``out`` and the masses exact zeros; no NaN or Inf anywhere.

What can go wrong and is looked at - everything the key-bias form decides per wave because its mask has no query axis: rows of one
32-row block that meet their first allowed key in different tiles (the adoption of the first live tile's max, per row), rows whose
allowed keys all lie in the first tile, a tile masked for every row, rows and whole entries that may attend nothing beside live ones,
keys that are nobody's (regions -1 and 32), and huge scores on never-allowed keys (they must not move a reference); the lane -> key
map of the region fetch, ragged tiles (the next segment's regions, or region 0 past the end, behind a segment's last key), padding
rows past len_q, K/V-range pieces that start mid-segment and pieces that are empty for some rows only, and the AdaIN fold across
segments that are masked for some rows only.

Measured on an MI355X (inputs N(0, 1), the seeds below; err / regression bound over the 265 bf16 and 258 fp16 comparisons held to the
default factors): bf16 median 0.53, largest 0.77 (B2H2Lq32N3Lr64s, empty_rows, pre-scaled Q); fp16 median 0.43, largest 0.66.  LSE:
largest 1.23 x 2^-23 x row scale over 543 comparisons (bound 16); masses: 1.44 over 306 (bound 8)."""
import numpy as np
import pytest
import torch

from key_bias_oracle import biased_attention_np
from lse_bounds import P_FLOOR, check_lse, check_mass
from parity_bounds import check_parity, stated_bound
from region_oracle import allowed_np, masked_attention_np

pytestmark = pytest.mark.gpu

SCALE = 0.125
QC = SCALE * 1.4426950408889634
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["f16", "bf16"]
KVB = 64            # keys per K/V tile of the kernel's walk


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


def _np64(t):
    return None if t is None else t.float().cpu().numpy().astype(np.float64)


class Case:
    """inputs of one call (CPU, rounded to the 16-bit type) and what the call needs on the device"""

    def __init__(self, shape, dtype, presc, seed=0, lkv_self=None, poison=None):
        B, H, Lq, N, Lr, inc, adain = shape
        self.shape, self.dtype, self.presc = shape, dtype, presc
        Ls = Lq if lkv_self is None else lkv_self
        self.Ls, Cc = Ls, H * 64
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s, sc=1.0, sh=0.0: (torch.randn(*s, generator=g) * sc + sh)
        q, k = rnd(B, Lq, Cc), rnd(B, Ls, Cc)           # N(0, 1) activations: what parity_bounds' regression bound is calibrated on
        rk = rnd(B, N, Lr, Cc) if N else None
        v = rnd(B, Ls, Cc)
        rv = rnd(B, N, Lr, Cc, sc=1.4, sh=-0.2) if N else None
        self.inc, self.adain, self.N, self.Lr, self.H, self.B, self.Lq = inc, adain, N, Lr, H, B, Lq
        self.seg_lens = ([Ls] if inc else []) + [Lr] * N
        self.lkv = sum(self.seg_lens)
        if poison is not None:      # (B, Lkv) bool over the packed key axis: those K rows are 1e4 everywhere
            off = Ls if inc else 0
            if inc:
                k[poison[:, :Ls]] = 1.0e4
            if N:
                rk.view(B, N * Lr, Cc)[poison[:, off:]] = 1.0e4
        self.q = (q * QC if presc else q).to(dtype)                 # pre-scaled: Q * scale * log2(e), rounded once
        self.q_true = _np64(self.q) / QC if presc else _np64(self.q)
        self.k, self.v = k.to(dtype), v.to(dtype)
        self.rk, self.rv = (rk.to(dtype), rv.to(dtype)) if N else (None, None)
        self._dev = None

    def tiles(self):
        """(first key, one past the last key) of every 64-key tile of the walk over the packed key axis"""
        out, off = [], 0
        for n in self.seg_lens:
            out += [(off + t, min(off + t + KVB, off + n)) for t in range(0, n, KVB)]
            off += n
        return out

    def dev(self):
        if self._dev is None:
            d = lambda t: None if t is None else t.cuda()
            self._dev = tuple(map(d, (self.q, self.k, self.v, self.rk, self.rv)))
        return self._dev

    def run(self, ops, qa, kr, tables=False, **kw):
        q, k, v, rk, rv = self.dev()
        aff = ops.adain_stats(v, rv, heads=self.H) if self.adain else None
        if tables:
            rk, rv = (ops.RefKVTable.from_tensors([[t[b, n] for n in range(self.N)] for b in range(self.B)]) for t in (rk, rv))
        dv = lambda t: t if t is None or t.is_cuda else t.cuda()
        return ops.shared_attention(q, k, v, rk, rv, heads=self.H, scale=SCALE, include_self=self.inc, adain=aff,
                                    q_prescaled=self.presc, q_allow=dv(qa), key_region=dv(kr), **kw)

    def allowed(self, qa, kr):
        return allowed_np(qa.cpu().numpy(), kr.cpu().numpy())

    def oracle(self, qa, kr):
        return masked_attention_np(self.q_true, _np64(self.k), _np64(self.v), _np64(self.rk), _np64(self.rv), self.H, SCALE,
                                   None if qa is None else self.allowed(qa, kr), use_adain=self.adain, train_input=self.inc, seg_lens=self.seg_lens)

    def row_scale(self, allowed, lse_ref):
        """tests/lse_bounds.py::row_scale with a mask that has a query axis: max(1, |lse_ref|, T_row), T_row over the allowed keys
        with p_ref >= 2^-30 of scale * sum_d |q_d k_jd|"""
        B, H, Lq = lse_ref.shape
        keys = np.concatenate(([_np64(self.k)] if self.inc else []) + ([_np64(self.rk).reshape(B, self.N * self.Lr, -1)] if self.N else []), axis=1)
        qh = self.q_true.reshape(B, Lq, H, 64).transpose(0, 2, 1, 3)
        kh = keys.reshape(B, self.lkv, H, 64).transpose(0, 2, 3, 1)
        s, t = np.matmul(qh, kh) * SCALE, np.matmul(np.abs(qh), np.abs(kh)) * SCALE
        alive = np.isfinite(lse_ref)[..., None]
        ok = np.broadcast_to(np.ones((B, 1, Lq, self.lkv), dtype=bool) if allowed is None else allowed, s.shape)
        counts = ok & alive & (np.where(ok, s, -np.inf) - np.where(alive, lse_ref[..., None], 0.0) >= np.log(P_FLOOR))
        t_row = np.where(counts, t, 0.0).max(-1)
        return np.maximum(1.0, np.maximum(t_row, np.where(alive[..., 0], np.abs(lse_ref), 0.0)))


def _check(case, got, ref, what, allowed):
    """out to parity_bounds; every element of the LSE and (when returned) of the masses to lse_bounds; dead rows exact; nothing
    non-finite but the -inf of a dead row's LSE"""
    out, lse = got[0], got[1]
    ro, rl, rm = ref
    assert torch.isfinite(out).all() and not torch.isnan(lse).any() and not torch.isposinf(lse).any(), what
    check_parity(out, ro, case.dtype, what)
    sc = case.row_scale(allowed, rl)
    check_lse(lse, rl, sc, what)
    dead = ~np.isfinite(rl)                                             # (B, H, Lq)
    o = out.float().cpu().numpy().reshape(case.B, case.Lq, case.H, 64).transpose(0, 2, 1, 3)
    assert np.all(o[dead] == 0.0), f"{what}: a row without an allowed key has exact zeros"
    if len(got) > 2:
        mass = got[2]
        assert torch.isfinite(mass).all(), what
        check_mass(mass, rm, sc, what)
        m = mass.cpu().numpy().astype(np.float64)
        assert np.all(m[dead] == 0.0) and np.abs(m[~dead].sum(-1) - 1.0).max(initial=0.0) <= 1e-5, what
    return dead


# B, H, Lq, N, Lr, include_self, adain, [self length when it is not Lq]
SHAPES = [
    (2, 2, 32, 3, 64, True, False),
    (2, 2, 48, 1, 40, True, True),        # padding rows of the 32-row block, ragged tiles
    (2, 2, 160, 3, 72, False, False),     # references only: a ragged tail reads the next segment's regions (the last one: region 0 past the end)
    (2, 2, 160, 3, 200, True, True),      # two 128-row blocks, four tiles per reference, the last one ragged
    (2, 2, 48, 0, 0, True, False, 200),   # plain attention over 200 keys
    (2, 2, 32, 1, 200, False, True),
]


def _sid(s):
    return "B%dH%dLq%dN%dLr%d%s%s" % (s[0], s[1], s[2], s[3], s[4], "s" if s[5] else "n", "a" if s[6] else "") + ("Ls%d" % s[7] if len(s) > 7 else "")


def _case(shape, dtype, presc, seed=0, **kw):
    return Case(shape[:7], dtype, presc, seed, lkv_self=shape[7] if len(shape) > 7 else None, **kw)


PATTERNS = ["random", "late_start", "early_only", "masked_tile", "empty_rows", "empty_entry", "nobodys_keys", "poisoned_keys"]


def _random(case, g):
    """4 classes, own class only, self free - through ops.region_masks (plain torch, on the CPU here)"""
    from instantrestore_amd import ops
    ql = torch.randint(0, 4, (case.B, case.Lq), generator=g)
    kl = torch.randint(0, 4, (case.B, case.lkv), generator=g)
    return ops.region_masks(ql, kl, torch.eye(4, dtype=torch.bool), self_len=case.Ls if case.inc else 0, self_free=True)


def _pattern(name, case, seed=1):
    """-> q_allow (B, Lq) int32, key_region (B, Lkv) int32, poison (B, Lkv) bool or None"""
    g = torch.Generator().manual_seed(seed)
    B, Lq, lkv = case.B, case.Lq, case.lkv
    tiles = case.tiles()
    rows = torch.arange(Lq)
    if name == "random":
        return _random(case, g) + (None,)
    kr = torch.randint(0, 4, (B, lkv), generator=g, dtype=torch.int32)
    qa = torch.randint(1, 16, (B, Lq), generator=g, dtype=torch.int32)            # a non-empty subset of regions 0 .. 3 per row
    if name == "late_start":     # a quarter of the rows of every 32-row block meet their first allowed key in the LAST tile of the walk
        a, e = tiles[-1]
        kr[:, a:e:2] = 5
        qa[:, rows % 4 == 1] = 1 << 5
        return qa, kr, None
    if name == "early_only":     # rows whose only allowed keys lie in the FIRST tile: every later tile is masked for them
        a, e = tiles[0]
        kr[:, a:e:3] = 6
        qa[:, rows % 4 == 2] = 1 << 6
        return qa, kr, None
    if name == "masked_tile":    # a whole tile of keys that every row is forbidden
        a, e = tiles[len(tiles) // 2]
        kr[:, a:e] = 7
        return qa, kr, None
    if name == "empty_rows":     # rows that may attend nothing, next to live rows
        qa, kr = _random(case, g)
        qa[:, rows % 3 == 0] = 0
        return qa, kr, None
    if name == "empty_entry":    # one batch entry wholly empty
        qa, kr = _random(case, g)
        qa[1] = 0
        return qa, kr, None
    if name == "nobodys_keys":   # regions -1 and 32 belong to nobody, whatever the row's word says
        pick = torch.rand(B, lkv, generator=g) < 0.3
        kr[pick] = torch.where(torch.rand(int(pick.sum()), generator=g) < 0.5, -1, 32).to(torch.int32)
        qa[:, rows % 5 == 0] = -1                     # every bit set: still not theirs
        return qa, kr, None
    if name == "poisoned_keys":  # K rows of 1e4 on keys masked for everybody: a huge never-allowed score must not move a reference
        pick = torch.rand(B, lkv, generator=g) < 0.2
        pick[:, tiles[0][0]] = True                   # the very first key of the walk among them
        kr[pick] = 9
        return qa, kr, pick
    raise KeyError(name)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_oracle_parity(ops, shape, dtype, presc, pattern):
    probe = _case(shape, dtype, presc)
    qa, kr, poison = _pattern(pattern, probe)
    case = probe if poison is None else _case(shape, dtype, presc, poison=poison)
    allowed = case.allowed(qa, kr)
    ref = case.oracle(qa, kr)
    what = f"{_sid(shape)} {pattern}"
    # the instantiation without the by-product and the one with it
    _check(case, case.run(ops, qa, kr, return_lse=True), ref, what, allowed)
    dead = _check(case, case.run(ops, qa, kr, return_lse=True, return_mass=True), ref, what + " (masses)", allowed)
    if pattern == "random":          # a condition on the INPUTS (the seeds are fixed so that it holds): at most a quarter of the rows empty
        assert dead.mean() <= 0.25, dead.mean()
    if pattern in ("empty_rows", "empty_entry"):
        assert dead.any() and not dead.all()
    if pattern == "late_start":      # the rows in question do start in the last tile only, beside rows that start in the first
        a, e = case.tiles()[-1]
        first = allowed[:, 0].argmax(-1)
        assert (first[:, 1::4] >= a).all() and (first[:, 0::4] < case.tiles()[0][1]).all() and not dead.any()


@pytest.mark.parametrize("pattern", ["random", "late_start", "empty_rows"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=_sid)
def test_pointer_tables_give_the_dense_bytes(ops, shape, dtype, pattern):
    case = _case(shape, dtype, True, seed=2)
    qa, kr, _ = _pattern(pattern, case, seed=3)
    kw = dict(return_lse=True, return_mass=True)
    for x, y in zip(case.run(ops, qa, kr, tables=True, **kw), case.run(ops, qa, kr, **kw)):
        assert torch.equal(x, y)


SPLIT = (2, 2, 160, 3, 200, True, True, 328)      # 6 + 3 * 4 = 18 tiles: the batch-invariant plan cuts every item into 2 pieces
SPLIT_PATTERNS = ["random", "late_start", "early_only", "masked_tile", "empty_rows", "poisoned_keys"]


@pytest.fixture(scope="module")
def split_refs():
    """one oracle per (pattern, dtype, presc) of the split shape, shared by the tests that need it"""
    cache = {}

    def get(pattern, dtype, presc):
        key = (pattern, dtype, presc)
        if key not in cache:
            probe = _case(SPLIT, dtype, presc, seed=4)
            qa, kr, poison = _pattern(pattern, probe, seed=5)
            case = probe if poison is None else _case(SPLIT, dtype, presc, seed=4, poison=poison)
            cache[key] = (case, qa, kr, case.allowed(qa, kr), case.oracle(qa, kr))
        return cache[key]
    return get


@pytest.mark.parametrize("pattern", SPLIT_PATTERNS)
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_kv_range_pieces_and_whole_items(ops, split_refs, dtype, presc, pattern):
    """the fixed plan of the batch-invariant mode cuts this shape's items into pieces (read from the plan, asserted): a row may be
    empty in one piece and live in the other; the same call through the default dispatch runs whole items"""
    case, qa, kr, allowed, ref = split_refs(pattern, dtype, presc)
    plan = ops.shared_attention_plan(case.B, case.Lq, case.H, len_self=case.Ls, n_refs=case.N, len_ref=case.Lr, dtype=dtype, adain=True,
                                     q_prescaled=presc, return_mass=True, regions=True)
    assert plan["pieces_per_item"] == 2 and plan["rows_per_item"] == 128 and plan["workspace_bytes"] > 0, plan
    cut = case.run(ops, qa, kr, return_lse=True, return_mass=True, batch_invariant=True)
    whole = case.run(ops, qa, kr, return_lse=True, return_mass=True)
    _check(case, cut, ref, f"split {pattern}", allowed)
    _check(case, whole, ref, f"whole items {pattern}", allowed)
    _check(case, case.run(ops, qa, kr, return_lse=True, batch_invariant=True), ref, f"split {pattern}, no masses", allowed)


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES[:5], ids=_sid)
def test_a_rule_that_allows_everything_is_the_plain_call(ops, shape, dtype, presc):
    """every key in a region, every row every bit: the plain call's result, within the project's stated tolerance of each other and
    each within its bounds of the oracle without a mask"""
    case = _case(shape, dtype, presc, seed=6)
    g = torch.Generator().manual_seed(7)
    kr = torch.randint(0, 32, (case.B, case.lkv), generator=g, dtype=torch.int32)
    qa = torch.full((case.B, case.Lq), -1, dtype=torch.int32)
    ref = case.oracle(None, None)
    got = case.run(ops, qa, kr, return_lse=True, return_mass=True)
    _check(case, got, ref, "everything allowed", None)
    plain = case.run(ops, None, None, return_lse=True, return_mass=True)
    err = float((got[0].float() - plain[0].float()).abs().max())
    assert err <= stated_bound(dtype, float(np.abs(ref[0]).max())), err
    sc = case.row_scale(None, ref[1])
    check_lse(plain[1], ref[1], sc, "plain call")


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES[:5], ids=_sid)
def test_one_word_for_all_rows_is_the_key_bias_call(ops, shape, dtype, presc):
    """the same q_allow in every row is a mask without a query axis: the key_bias call with -inf on the excluded keys"""
    case = _case(shape, dtype, presc, seed=8)
    g = torch.Generator().manual_seed(9)
    kr = torch.randint(-1, 6, (case.B, case.lkv), generator=g, dtype=torch.int32)
    qa = torch.full((case.B, case.Lq), 0b010110, dtype=torch.int32)
    allowed = case.allowed(qa, kr)
    bias = torch.from_numpy(np.where(allowed[:, 0, 0], 0.0, -np.inf)).float()
    ref = case.oracle(qa, kr)
    rb = biased_attention_np(case.q_true, _np64(case.k), _np64(case.v), _np64(case.rk), _np64(case.rv), case.H, SCALE, bias.numpy().astype(np.float64),
                             use_adain=case.adain, train_input=case.inc, seg_lens=case.seg_lens)
    for a, b in zip(ref, rb):
        assert np.array_equal(a, b)                                   # the two oracles agree to the bit
    got = case.run(ops, qa, kr, return_lse=True, return_mass=True)
    _check(case, got, ref, "one word for all rows", allowed)
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H) if case.adain else None
    biased = ops.shared_attention(q, k, v, rk, rv, heads=case.H, scale=SCALE, include_self=case.inc, adain=aff, q_prescaled=presc,
                                  key_bias=bias.cuda(), return_lse=True, return_mass=True)
    err = float((got[0].float() - biased[0].float()).abs().max())
    assert err <= stated_bound(dtype, float(np.abs(ref[0]).max())), err
    _check(case, biased, ref, "the key_bias call", allowed)


@pytest.mark.parametrize("bi", [False, True], ids=["default", "batch_invariant"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
def test_two_runs_a_replayed_graph_and_an_in_place_update(ops, split_refs, presc, bi):
    """bit for bit: the same call twice; one stream against the replay of its capture; and after q_allow and key_region are refilled
    in place, the replay against a fresh call (both arrays are read when the kernel runs)"""
    case, qa, kr, _, _ = split_refs("random", torch.bfloat16, presc)
    qa2, kr2, _ = _pattern("late_start", case, seed=11)
    dqa, dkr = qa.cuda(), kr.cuda()
    call = lambda a, r: case.run(ops, a, r, return_lse=True, return_mass=True, batch_invariant=bi)
    first, second = call(dqa, dkr), call(dqa, dkr)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(dqa, dkr)                                  # warm-up: the stream's workspace exists before the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = call(dqa, dkr)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(res, first):
        assert torch.equal(x, y)
    addr = dqa.data_ptr(), dkr.data_ptr()
    dqa.copy_(qa2.cuda())
    dkr.copy_(kr2.cuda())
    assert (dqa.data_ptr(), dkr.data_ptr()) == addr
    graph.replay()
    torch.cuda.synchronize()
    fresh = call(qa2.cuda(), kr2.cuda())
    for x, y in zip(res, fresh):
        assert torch.equal(x, y)
    assert not torch.equal(fresh[0], first[0])
    _check(case, res, case.oracle(qa2, kr2), "replay after the refill", case.allowed(qa2, kr2))


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
def test_batch_invariance(ops, presc):
    """entry b's bytes with its regions are the same alone and inside a batch of 3, at either position"""
    shape = (3,) + SPLIT[1:]
    case = _case(shape, torch.bfloat16, presc, seed=12)
    qa, kr, _ = _pattern("late_start", case, seed=13)
    qa[1, ::7] = 0                                      # entry 1 has rows that may attend nothing
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H)
    dqa, dkr = qa.cuda(), kr.cuda()

    def run(idx):
        i = torch.tensor(idx, device="cuda")
        return ops.shared_attention(q[i], k[i], v[i], rk[i], rv[i], heads=case.H, scale=SCALE, include_self=True,
                                    adain=(aff[0][i].contiguous(), aff[1][i].contiguous()), q_prescaled=presc, q_allow=dqa[i].contiguous(),
                                    key_region=dkr[i].contiguous(), return_lse=True, return_mass=True, batch_invariant=True)
    whole, swapped = run([0, 1, 2]), run([2, 0, 1])
    for b in range(3):
        alone = run([b])
        for x, y, z in zip(alone, whole, swapped):
            assert torch.equal(x[0], y[b]) and torch.equal(x[0], z[(b + 1) % 3])
    _check(case, whole, case.oracle(qa, kr), "batch-invariant", case.allowed(qa, kr))


@pytest.mark.parametrize("bi", [False, True], ids=["default", "batch_invariant"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_a_lost_pair_moves_its_own_row_only(ops, split_refs, dtype, presc, bi):
    """one allowed bit of one row flipped to forbidden: that row's output moves (all heads), every other row of every entry keeps its
    bytes - the mask has a query axis, and no row's state leaks into its neighbours of the 32-row block"""
    case, qa, kr, _, _ = split_refs("masked_tile", dtype, presc)
    b, row = 1, 37
    word = int(qa[b, row])
    region = next(r for r in range(4) if (word >> r) & 1 and int((kr[b] == r).sum()) > 0)
    flipped = qa.clone()
    flipped[b, row] = word & ~(1 << region)
    kw = dict(return_lse=True, return_mass=True, batch_invariant=bi)
    base, lost = case.run(ops, qa, kr, **kw), case.run(ops, flipped, kr, **kw)
    others = torch.ones(case.B, case.Lq, dtype=torch.bool)
    others[b, row] = False
    assert torch.equal(base[0][others], lost[0][others]) and not torch.equal(base[0][b, row], lost[0][b, row])
    for x, y in zip(base[1:], lost[1:]):                 # lse (B, H, Lq), mass (B, H, Lq, S)
        xo, yo = x.transpose(1, 2), y.transpose(1, 2)
        assert torch.equal(xo[others.cuda()], yo[others.cuda()]) and not torch.equal(xo[b, row], yo[b, row])
    assert bool((lost[1][b, :, row] < base[1][b, :, row]).all())        # keys were taken away: every head's LSE falls


def test_a_region_call_runs_the_32_row_kernel_at_4096_rows_and_says_so(ops):
    case = Case((1, 1, 4096, 1, 64, True, False), torch.bfloat16, True, seed=14, lkv_self=64)
    q, k, v, rk, rv = case.dev()
    qa, kr, _ = _pattern("random", case, seed=15)
    kw = dict(heads=1, scale=SCALE, include_self=True, q_prescaled=True)
    name = ops.shared_attention_kernel_name(q, k, v, rk, rv, q_allow=qa.cuda(), key_region=kr.cuda(), **kw)
    assert name.startswith("shared_attn_fwd_pipe_kernel") and "regions" in name and "key bias" not in name, name
    assert "regions" not in ops.shared_attention_kernel_name(q, k, v, rk, rv, **kw)
    _check(case, case.run(ops, qa, kr, return_lse=True), case.oracle(qa, kr), "Lq 4096", case.allowed(qa, kr))
    valid = torch.tensor([0], dtype=torch.int32, device="cuda")
    rk0, rv0 = torch.zeros_like(rk), torch.zeros_like(rv)
    a = ops.shared_attention(q, k, v, rk0, rv0, valid_refs=valid, q_allow=qa.cuda(), key_region=kr.cuda(), **kw)     # dense: the promise is dropped
    assert torch.equal(a, ops.shared_attention(q, k, v, rk0, rv0, q_allow=qa.cuda(), key_region=kr.cuda(), **kw))
    tk, tv = (ops.RefKVTable.from_tensors([[t[0, 0]]]) for t in (rk0, rv0))
    with pytest.raises(ValueError, match="valid_refs"):
        ops.shared_attention(q, k, v, tk, tv, valid_refs=valid, q_allow=qa.cuda(), key_region=kr.cuda(), **kw)


# ---- the processor route on the synthetic UNet topology ------------------------------------------------------------------------
class _Recorder:
    """``ops`` with a ``shared_attention`` that runs the real one and keeps what a shared layer passed and got"""

    def __init__(self, ops):
        self._o, self.calls = ops, []

    def __getattr__(self, name):
        return getattr(self._o, name)

    def shared_attention(self, *a, **kw):
        res = self._o.shared_attention(*a, **kw)
        if kw.get("q_allow") is not None:
            self.calls.append((a, kw, res))
        return res


def test_processors_take_region_labels_through_the_unet_host(ops, monkeypatch):
    """reference UNet -> harvest -> main UNet with region_labels / region_allow in cross_attention_kwargs: label pictures at the
    latent's resolution, sampled by every shared layer at its own token centres.  Reference 1 carries a class no query class may
    attend: its mass is exactly 0 in every shared layer; and every shared layer's output is the ops call on the pair that
    ops.region_masks builds from attn_maps.token_labels"""
    from types import SimpleNamespace
    from face_replace.models.attn_processors import SharedAttnProcessor, register_attention_processor, register_attention_processor_kv_unet
    from instantrestore_amd import attn_maps, attn_processors as ap
    from instantrestore_amd.kv_harvest import get_conditioning_keys_values
    from instantrestore_amd.unet_host import AttnTopologyUNet
    import __graft_entry__ as ge
    cfg = SimpleNamespace(use_adain=True, train_input=True, condition_on_face_embeds=False)
    kv_unet, unet = AttnTopologyUNet(seed=5).to("cuda"), AttnTopologyUNet(seed=6).to("cuda")
    ge.register_attention_processor_kv_unet_default(kv_unet, cfg)
    register_attention_processor_kv_unet(kv_unet)
    register_attention_processor(unet, cfg)
    rec = _Recorder(ops)
    monkeypatch.setattr(ap, "_ops", rec)
    ap._REGION_PAIRS.clear()
    B, N, S = 2, 3, 32                                            # 32 x 32 latent: token axes of 64 / 256 / 1024 in the decoder
    g = torch.Generator().manual_seed(16)
    text = torch.randn(1, 77, 1024, generator=g).cuda()
    x = torch.randn(B, 4, S, S, generator=g).cuda()
    refs_in = torch.randn(B * N, 4, S, S, generator=g).cuda()
    coarse = torch.randint(0, 3, (B, 1 + N, 4, 4), generator=g).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)    # a coarse grid of classes 0 .. 2
    q_pic, r_pic = coarse[:, 0].contiguous().cuda(), coarse[:, 1:].contiguous().cuda()
    r_pic[:, 1] = 3                                                # class 3: allowed to nobody
    allow = torch.eye(4, dtype=torch.bool)
    allow[3, 3] = False
    shared = [p for p in unet.attn_processors.values() if isinstance(p, SharedAttnProcessor) and p.self_attn_idx is not None]
    assert len(shared) == 9
    for p in shared:
        p.save_attention_mass = True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        keys, vals, stats = get_conditioning_keys_values(kv_unet, refs_in, None, text.repeat(B * N, 1, 1), N, [N] * B, with_stats=True)
        kw = {"ref_keys": keys, "ref_values": vals, "ref_stats": stats}
        plain = unet(x, None, encoder_hidden_states=text.repeat(B, 1, 1), cross_attention_kwargs=kw).sample
        assert rec.calls == []
        out = unet(x, None, encoder_hidden_states=text.repeat(B, 1, 1),
                   cross_attention_kwargs=dict(kw, region_labels=(q_pic, r_pic), region_allow=allow.cuda())).sample
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not torch.equal(out, plain)
    assert len(rec.calls) == 9 and len({id(c[1]["q_allow"]) for c in rec.calls}) == 3          # nine layers, three geometries, three pairs
    for p in shared:
        m = p.attention_mass
        assert tuple(m.shape[:1]) == (B,) and m.shape[-1] == 1 + N and torch.isfinite(m).all()
        assert float(m[..., 2].abs().max()) == 0.0                 # reference 1: exactly no mass
        assert float(m[..., 0].min()) > 0.0 and float((m.sum(-1) - 1).abs().max()) < 1e-5
    for a, kw_call, res in rec.calls:
        length = a[0].shape[1]
        side = int(round(length ** 0.5))
        ql = attn_maps.token_labels(q_pic, side)
        qa, kr = ops.region_masks(ql, torch.cat([ql, attn_maps.token_labels(r_pic, side)], dim=1), allow.cuda(), self_len=length, self_free=True)
        assert torch.equal(kw_call["q_allow"], qa) and torch.equal(kw_call["key_region"], kr)
        again = ops.shared_attention(*a, **dict(kw_call, q_allow=qa, key_region=kr))
        for u, w in zip(res, again):
            assert torch.equal(u, w)


def test_example_regions_switch(capsys):
    """examples/synthetic_inference.py --regions: the top shared layer's masses with and without the rule, per identity"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "synthetic_inference.py")
    spec = importlib.util.spec_from_file_location("synthetic_inference_regions", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--identities", "2", "--refs", "3", "--px", "256", "--small", "--regions", "--dtype", "bf16"])
    text = capsys.readouterr().out
    assert out.shape == (2, 256, 256, 3)
    assert text.count("16 classes, own class only, self free:") == 2 and text.count("unrestricted") == 2, text
