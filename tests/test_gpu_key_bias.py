"""The additive key bias of the fused attention on the GPU (``ir_shared_attn_bias_args``, ``ops.shared_attention(key_bias=)``): the
BIAS forms of the software-pipelined 32-row kernel against the float64 helper oracle (``key_bias_oracle``) on identical 16-bit-rounded
inputs, held to ``parity_bounds.check_parity`` with its default factors (a CPU model of the kernels' arithmetic - 16-bit
probabilities, one output rounding - on rows carried by 1 to 1280 unmasked keys stays at <= 0.70 of the regression bound: masks do
not justify a wider one); the LSE and the by-product masses, every element, to tests/lse_bounds.py (fp32 accuracy at the row's own
scale, |bias| included; -inf exactly on the rows without an unmasked key).

What can go wrong and is looked at: the lane -> key map of the bias fetch, ragged tiles (the next segment's bias behind a
segment's last key), K/V-range pieces that start mid-segment, masked keys that must not take part in the row max, wholly masked
leading tiles (a kernel that keeps a start-value reference returns zeros or NaN when every live score lies far below it), wholly
masked (b, h) (zeros, lse = -inf, zero masses - never NaN), the AdaIN fold across masked segments, and that nothing outside a
bias row is used.

Measured on an MI355X (inputs N(0, 1), the seeds below, err / regression bound over the 118 bf16 and 106 fp16 comparisons held to the
default factors): bf16 median 0.51, largest 0.73; fp16 median 0.43, largest 0.65.  The bias forms let their reference follow every
growth of a row's max; with the lazy reference of their unbiased twins two bf16 cases (scatter on B1H2Lq200N3Lr72n, soft on
B3H2Lq96N0Lr0s) sat at 1.01 and 1.06 of the regression bound - the key that carries a row then has a probability that is not exactly 1
and takes a rounding of its own (the same keys through the unbiased kernels: 0.79 lazy, 0.53 exact)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from key_bias_oracle import MASKED, biased_attention_np
from lse_bounds import check_lse, check_mass, pack_keys, row_scale
from parity_bounds import check_parity

pytestmark = pytest.mark.gpu

SCALE = 0.125
QC = SCALE * 1.4426950408889634
NEG = float("-inf")
DTYPES = [torch.float16, torch.bfloat16]
DT_IDS = ["f16", "bf16"]


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

    def __init__(self, shape, dtype, presc, seed=0, lkv_self=None, far=None):
        B, H, Lq, N, Lr, inc, adain = shape
        self.shape, self.dtype, self.presc = shape, dtype, presc
        Ls = Lq if lkv_self is None else lkv_self
        self.Ls, Cc = Ls, H * 64
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s, sc=1.0, sh=0.0: (torch.randn(*s, generator=g) * sc + sh)
        if far is None:
            q, k = rnd(B, Lq, Cc), rnd(B, Ls, Cc)       # N(0, 1) activations: what parity_bounds' regression bound is calibrated on
            rk = rnd(B, N, Lr, Cc) if N else None
        else:     # every score below -110 natural units: q = 4 sigma + noise, k = -4 sigma + noise
            sig = torch.where(torch.rand(Cc, generator=g) < 0.5, -1.0, 1.0)
            q, k = 4 * sig + 0.1 * rnd(B, Lq, Cc), -4 * sig + 0.1 * rnd(B, Ls, Cc)
            rk = -4 * sig + 0.1 * rnd(B, N, Lr, Cc)
        v = rnd(B, Ls, Cc)
        rv = rnd(B, N, Lr, Cc, sc=1.4, sh=-0.2) if N else None
        self.q = (q * QC if presc else q).to(dtype)                 # pre-scaled: Q * scale * log2(e), rounded once
        self.q_true = _np64(self.q) / QC if presc else _np64(self.q)
        self.k, self.v = k.to(dtype), v.to(dtype)
        self.rk, self.rv = (rk.to(dtype), rv.to(dtype)) if N else (None, None)
        self.inc, self.adain, self.N, self.Lr, self.H, self.B, self.Lq = inc, adain, N, Lr, H, B, Lq
        self.seg_lens = ([Ls] if inc else []) + [Lr] * N
        self.lkv = sum(self.seg_lens)
        self._dev = None

    def dev(self):
        if self._dev is None:
            d = lambda t: None if t is None else t.cuda()
            self._dev = tuple(map(d, (self.q, self.k, self.v, self.rk, self.rv)))
        return self._dev

    def run(self, ops, bias, **kw):
        q, k, v, rk, rv = self.dev()
        aff = ops.adain_stats(v, rv, heads=self.H) if self.adain else None
        if bias is not None and not bias.is_cuda:
            bias = bias.cuda()
        return ops.shared_attention(q, k, v, rk, rv, heads=self.H, scale=SCALE, include_self=self.inc, adain=aff,
                                    q_prescaled=self.presc, key_bias=bias, **kw)

    def oracle(self, bias, mass=False):
        kb = None if bias is None else bias.detach().cpu().numpy().astype(np.float64)
        return biased_attention_np(self.q_true, _np64(self.k), _np64(self.v), _np64(self.rk), _np64(self.rv), self.H, SCALE, kb,
                                   use_adain=self.adain, train_input=self.inc, seg_lens=self.seg_lens if mass else None)


def _scales(case, bias, lse_ref):
    """tests/lse_bounds.py::row_scale of every (b, h, row) of a call: |bias| counts where a biased key carries weight"""
    kb = None if bias is None else bias.detach().cpu().numpy().astype(np.float64)
    return row_scale(case.q_true, pack_keys(case.k, case.rk, case.inc), SCALE, lse_ref, bias=kb)


def _check(case, got, ref, what, bias, lse=True):
    """out to parity_bounds; every element of the LSE to lse_bounds (-inf exactly on the rows without an unmasked key).  Returns
    the row scales"""
    out, glse = got[0], got[1]
    check_parity(out, ref[0], case.dtype, what)
    if lse:
        sc = _scales(case, bias, ref[1])
        check_lse(glse, ref[1], sc, what)
        return sc


# B, H, Lq, N, Lr, include_self, adain
SMALL = [
    (2, 2, 64, 4, 64, True, False),
    (2, 1, 40, 2, 56, True, True),        # ragged tiles, partial query block
    (1, 2, 200, 3, 72, False, False),     # the next segment's bias must not leak into a ragged tail
    (1, 5, 256, 4, 256, True, True),
    (2, 2, 33, 1, 1, True, False),
    (3, 2, 96, 0, 0, True, False),        # plain
    (1, 5, 128, 0, 0, True, False),       # with 77 keys: cross attention
]


def _sid(s):
    return "B%dH%dLq%dN%dLr%d%s%s" % (s[0], s[1], s[2], s[3], s[4], "s" if s[5] else "n", "a" if s[6] else "")


def _case(shape, dtype, presc, seed=0, **kw):
    lkv_self = 77 if shape == SMALL[6] else None
    return Case(shape, dtype, presc, seed, lkv_self=lkv_self, **kw)


PATTERNS = ["soft", "soft_per_head", "ref_consts", "scatter", "trailing"]


def _pattern(name, case, seed=1, masked_value=NEG):
    g = torch.Generator().manual_seed(seed)
    B, H, lkv = case.B, case.H, case.lkv
    if name == "soft":
        return torch.rand(B, lkv, generator=g) * 6 - 3
    if name == "soft_per_head":
        return torch.rand(B, H, lkv, generator=g) * 6 - 3
    if name == "ref_consts":          # log{0.25, 1, 4} per reference, one reference at -inf (the self segment keeps 0)
        row = torch.zeros(B, lkv)
        off = case.Ls if case.inc else 0
        consts = [math.log(0.25), 0.0, math.log(4.0)]
        for n in range(case.N):
            val = NEG if n == (1 if case.N > 1 else 0) and (case.inc or case.N > 1) else consts[n % 3]
            row[:, off + n * case.Lr: off + (n + 1) * case.Lr] = val
        if case.N == 0:
            row[:, lkv // 2:] = math.log(0.25)
        return row
    if name == "scatter":             # 30 % of the keys masked (key 0 of every row stays)
        row = torch.zeros(B, lkv)
        m = torch.rand(B, lkv, generator=g) < 0.3
        m[:, 0] = False
        row[m] = masked_value
        return row
    if name == "trailing":            # diffusers' padded-text mask: the last quarter (at least one key) at -10000
        row = torch.zeros(B, 1, lkv)
        row[:, :, lkv - max(1, lkv // 4):] = -10000.0
        return row[:, 0] if lkv > 1 else torch.zeros(B, lkv)
    raise KeyError(name)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SMALL, ids=_sid)
def test_oracle_parity(ops, shape, dtype, presc, pattern):
    case = _case(shape, dtype, presc)
    bias = _pattern(pattern, case)
    got = case.run(ops, bias, return_lse=True)
    _check(case, got, case.oracle(bias), f"{_sid(shape)} {pattern}", bias)
    if pattern == "scatter":          # -inf and IR_KEY_BIAS_MASKED are the same mask: identical bytes
        got2 = case.run(ops, _pattern(pattern, case, masked_value=MASKED), return_lse=True)
        assert torch.equal(got[0], got2[0]) and torch.equal(got[1], got2[1])


BIG = (9, 2, 1024, 4, 1024, True, True)       # the remainder split


@pytest.fixture(scope="module")
def big(ops):
    """one oracle for the split shape, shared by the tests that need it (bf16, pre-scaled Q, a soft bias with reference 2 masked)"""
    case = Case(BIG, torch.bfloat16, True, seed=3)
    bias = _pattern("soft", case, seed=4)
    bias[:, case.Ls + 2 * case.Lr: case.Ls + 3 * case.Lr] = NEG
    outs, lses = [], []
    for b in range(case.B):           # entry by entry: the float64 score matrix of the whole batch is 750 MB
        sl = lambda t: None if t is None else t[b:b + 1]
        o, l = biased_attention_np(case.q_true[b:b + 1], _np64(sl(case.k)), _np64(sl(case.v)), _np64(sl(case.rk)), _np64(sl(case.rv)),
                                   case.H, SCALE, bias[b:b + 1].numpy().astype(np.float64), use_adain=True, train_input=True)
        outs.append(o)
        lses.append(l)
    return case, bias, (np.concatenate(outs), np.concatenate(lses))


def test_remainder_split_and_whole_items_agree(ops, big):
    case, bias, ref = big
    a = case.run(ops, bias, return_lse=True)
    b = case.run(ops, bias, return_lse=True, split=False)
    _check(case, a, ref, "split", bias)
    _check(case, b, ref, "whole items", bias)
    check_parity(a[0], b[0], case.dtype, "split vs whole items", factor=2.0)


def test_fully_masked_entry_in_the_split_shape(ops, big):
    case, bias, _ = big
    base = case.run(ops, bias, return_lse=True, return_mass=True)
    dead = bias.clone()
    dead[1] = NEG
    out, lse, mass = case.run(ops, dead, return_lse=True, return_mass=True)
    assert torch.isfinite(out).all() and not torch.isnan(lse).any() and not torch.isnan(mass).any()
    assert out[1].abs().max() == 0 and bool(torch.isneginf(lse[1]).all()) and mass[1].abs().max() == 0
    keep = [0] + list(range(2, case.B))
    for x, y in zip((out, lse, mass), base):
        assert torch.equal(x[keep], y[keep])


def test_a_bias_call_runs_the_32_row_kernel_at_4096_rows(ops):
    shape = (1, 1, 4096, 1, 4096, True, False)
    case = Case(shape, torch.bfloat16, True, seed=5)
    bias = _pattern("scatter", case, seed=6)
    q, k, v, rk, rv = case.dev()
    kw = dict(heads=1, scale=SCALE, include_self=True, q_prescaled=True)
    with_bias = ops.shared_attention_kernel_name(q, k, v, rk, rv, key_bias=bias.cuda(), **kw)
    without = ops.shared_attention_kernel_name(q, k, v, rk, rv, **kw)
    assert with_bias.startswith("shared_attn_fwd_pipe_kernel") and "key bias" in with_bias, with_bias
    assert "pipe_kernel" not in without and "key bias" not in without, without
    _check(case, case.run(ops, bias, return_lse=True), case.oracle(bias), "Lq 4096", bias)


LEAD = [(2, 2, 64, 4, 64, True, False), (2, 2, 64, 4, 64, True, True), (1, 2, 40, 3, 72, True, True)]


@pytest.mark.parametrize("far", [None, True], ids=["ordinary", "far_below_start"])
@pytest.mark.parametrize("masked_value", [NEG, -10000.0], ids=["neginf", "m10000"])
@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", LEAD, ids=_sid)
def test_leading_masked_tiles(ops, shape, dtype, presc, masked_value, far):
    """the self segment and reference 0 wholly masked: (i) ordinary scores behind them, (ii) every live score below -110 natural
    units - a kernel that keeps its start-value reference returns zeros or NaN there; the oracle is unaffected"""
    case = Case(shape, dtype, presc, seed=7, far=far)
    bias = torch.zeros(case.B, case.lkv)
    bias[:, : case.Ls + case.Lr] = masked_value
    out, lse, mass = case.run(ops, bias, return_lse=True, return_mass=True)
    ro, rl, rm = case.oracle(bias, mass=True)
    if far:
        assert rl.max() < -110.0
    sc = _check(case, (out, lse), (ro, rl), f"{_sid(shape)} leading masked", bias)
    m = mass.cpu().numpy().astype(np.float64)
    assert np.all(m[..., :2] == 0.0), "masked segments carry exactly no mass"
    assert np.abs(m.sum(-1) - 1.0).max() <= 1e-5
    check_mass(m, rm, sc, f"{_sid(shape)} leading masked")


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("adain", [False, True], ids=["plain", "adain"])
def test_fully_masked_entry(ops, dtype, presc, adain):
    case = Case((3, 2, 72, 2, 40, True, adain), dtype, presc, seed=8)
    bias = _pattern("soft", case, seed=9)
    base = case.run(ops, bias, return_lse=True, return_mass=True)
    bias[1] = NEG
    out, lse, mass = case.run(ops, bias, return_lse=True, return_mass=True)
    assert torch.isfinite(out).all() and not torch.isnan(lse).any() and not torch.isnan(mass).any()
    assert out[1].abs().max() == 0 and bool(torch.isneginf(lse[1]).all()) and mass[1].abs().max() == 0
    for x, y in zip((out, lse, mass), base):
        assert torch.equal(x[[0, 2]], y[[0, 2]])
    _check(case, (out, lse), case.oracle(bias), "fully masked entry", bias)


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SMALL[:4], ids=_sid)
def test_zero_bias_is_neutral_and_a_null_bias_is_the_short_call(ops, shape, dtype, presc):
    case = _case(shape, dtype, presc, seed=10)
    ref = case.oracle(None)
    _check(case, case.run(ops, torch.zeros(case.B, case.lkv), return_lse=True), ref, "all-zero bias vs the oracle without bias", None)
    short = case.run(ops, None, return_lse=True)
    # the long block with key_bias = NULL: the bytes of the short block's call
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H) if case.adain else None
    out, lse = torch.empty_like(short[0]), torch.empty_like(short[1])
    args = ops._fill_args(q, k, v, rk, rv, case.H, SCALE, case.inc, aff, out, lse, True, presc, None, False,
                          torch.zeros(case.B, case.lkv, device="cuda"))
    assert args.struct_size == C.sizeof(ops._lib.SharedAttnBiasArgs)
    args.key_bias = None
    ops._lib.check(ops._lib.lib().ir_shared_attn_fwd(C.byref(args), ops._stream()), "ir_shared_attn_fwd")
    torch.cuda.synchronize()
    assert torch.equal(out, short[0]) and torch.equal(lse, short[1])


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
def test_ref_weights_scale_the_mass_ratio(ops, presc):
    case = Case((2, 2, 96, 3, 72, True, True), torch.bfloat16, presc, seed=11)
    w = torch.tensor([[0.25, 1.0, 4.0], [2.0, 0.5, 1.0]])
    bias = ops.key_bias(case.B, case.Ls, case.N, case.Lr, True, ref_weights=w.cuda(), device="cuda")
    _, m0 = case.run(ops, None, return_mass=True)
    _, m1 = case.run(ops, bias, return_mass=True)
    m0, m1 = m0.double().cpu(), m1.double().cpu()
    for n in range(case.N):
        r0, r1 = m0[..., 1 + n] / m0[..., 0], m1[..., 1 + n] / m1[..., 0]
        ok = (m0[..., 1 + n] > 1e-3) & (m0[..., 0] > 1e-3) & (m1[..., 1 + n] > 1e-3) & (m1[..., 0] > 1e-3)
        assert ok.any()
        rel = (r1 / (r0 * w[:, n].double().view(-1, 1, 1)) - 1.0).abs()[ok]
        assert rel.max() <= 1e-3, (n, float(rel.max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_masked_equals_removed(ops, dtype):
    case = Case((2, 2, 96, 4, 72, True, False), dtype, False, seed=12)
    bias = torch.zeros(case.B, case.lkv)
    bias[:, case.Ls + 2 * case.Lr: case.Ls + 3 * case.Lr] = NEG
    masked = case.run(ops, bias)
    q, k, v, rk, rv = case.dev()
    keep = [0, 1, 3]
    removed = ops.shared_attention(q, k, v, rk[:, keep].contiguous(), rv[:, keep].contiguous(), heads=case.H, scale=SCALE, include_self=True)
    check_parity(masked, removed, dtype, "masked vs removed", factor=2.0)


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
@pytest.mark.parametrize("shape", [SMALL[1], SMALL[2], SMALL[6]], ids=_sid)
def test_poisoned_padding_and_strides(ops, shape, presc):
    """bias rows are slices of a wider buffer whose gaps, and whose 64 floats behind the last row, hold NaN: nothing outside a
    row is used (kb_sb != Lkv, kb_sh != Lkv)"""
    case = _case(shape, torch.bfloat16, presc, seed=13)
    bias = _pattern("soft_per_head", case, seed=14)
    gap = 5
    flat = torch.full((case.B * case.H * (case.lkv + gap) + 64,), float("nan"))
    rows = flat[: case.B * case.H * (case.lkv + gap)].view(case.B, case.H, case.lkv + gap)[:, :, : case.lkv]
    rows.copy_(bias)
    dev = flat.cuda()
    drows = dev[: case.B * case.H * (case.lkv + gap)].view(case.B, case.H, case.lkv + gap)[:, :, : case.lkv]
    assert drows.stride() == (case.H * (case.lkv + gap), case.lkv + gap, 1)
    got = case.run(ops, drows, return_lse=True)
    _check(case, got, case.oracle(bias), "poisoned padding", bias)
    dense = case.run(ops, bias, return_lse=True)
    assert torch.equal(got[0], dense[0]) and torch.equal(got[1], dense[1])
    # a (B, Lkv) row with a batch stride of its own
    wide = torch.full((case.B, case.lkv + 11), float("nan"), device="cuda")
    wide[:, : case.lkv] = bias[:, 0].cuda()
    a = case.run(ops, wide[:, : case.lkv])
    assert torch.equal(a, case.run(ops, bias[:, 0].contiguous()))


def test_table_call_gives_the_dense_bytes(ops):
    case = Case((2, 2, 96, 3, 72, True, False), torch.bfloat16, True, seed=15)
    bias = _pattern("ref_consts", case).cuda()
    q, k, v, rk, rv = case.dev()
    tk = ops.RefKVTable.from_tensors([[rk[b, n] for n in range(case.N)] for b in range(case.B)])
    tv = ops.RefKVTable.from_tensors([[rv[b, n] for n in range(case.N)] for b in range(case.B)])
    kw = dict(heads=case.H, scale=SCALE, include_self=True, q_prescaled=True, key_bias=bias, return_lse=True, return_mass=True)
    for x, y in zip(ops.shared_attention(q, k, v, tk, tv, **kw), ops.shared_attention(q, k, v, rk, rv, **kw)):
        assert torch.equal(x, y)
    valid = torch.tensor([3, 2], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="valid_refs"):
        ops.shared_attention(q, k, v, tk, tv, valid_refs=valid, **kw)
    # dense + valid_refs: the promise is dropped and the zeros are walked - the numbers of the call without it
    rk0, rv0 = rk.clone(), rv.clone()
    ops.zero_invalid_refs(rk0, rv0, valid, heads=case.H)
    for x, y in zip(ops.shared_attention(q, k, v, rk0, rv0, valid_refs=valid, **kw), ops.shared_attention(q, k, v, rk0, rv0, **kw)):
        assert torch.equal(x, y)


def test_a_captured_call_follows_an_in_place_refill(ops):
    case = Case((2, 2, 96, 3, 72, True, True), torch.bfloat16, True, seed=16)
    w0, w1 = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]), torch.tensor([[1.0, 0.0, 0.25], [4.0, 1.0, 0.0]])
    bias = ops.key_bias(case.B, case.Ls, case.N, case.Lr, True, ref_weights=w0, device="cuda")
    call = lambda kb: case.run(ops, kb, return_lse=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(bias)                                       # warm-up: the stream's workspace exists before the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = call(bias)
    graph.replay()
    torch.cuda.synchronize()
    eager = call(bias.clone())
    assert torch.equal(res[0], eager[0]) and torch.equal(res[1], eager[1])
    addr = bias.data_ptr()
    ops.key_bias(case.B, case.Ls, case.N, case.Lr, True, ref_weights=w1, out=bias)
    assert bias.data_ptr() == addr
    graph.replay()
    torch.cuda.synchronize()
    eager = call(bias.clone())
    assert torch.equal(res[0], eager[0]) and torch.equal(res[1], eager[1])
    _check(case, res, case.oracle(bias), "replay after the refill", bias)


@pytest.mark.parametrize("presc", [False, True], ids=["plainq", "prescq"])
def test_batch_invariance(ops, presc):
    """entry b's bytes with its bias are the same at B = 1 and inside B = 3, at either position"""
    case = Case((3, 2, 256, 4, 256, True, True), torch.bfloat16, presc, seed=17)
    bias = _pattern("soft_per_head", case, seed=18)
    bias[1, :, case.Ls: case.Ls + case.Lr] = NEG
    q, k, v, rk, rv = case.dev()
    aff = ops.adain_stats(v, rv, heads=case.H)

    def run(idx):
        i = torch.tensor(idx, device="cuda")
        return ops.shared_attention(q[i], k[i], v[i], rk[i], rv[i], heads=case.H, scale=SCALE, include_self=True,
                                    adain=(aff[0][i].contiguous(), aff[1][i].contiguous()), q_prescaled=presc, key_bias=bias.cuda()[i].contiguous(),
                                    return_lse=True, return_mass=True, batch_invariant=True)
    whole, swapped = run([0, 1, 2]), run([2, 0, 1])
    for b in range(3):
        alone = run([b])
        for x, y, z in zip(alone, whole, swapped):
            assert torch.equal(x[0], y[b]) and torch.equal(x[0], z[(b + 1) % 3])
    _check(case, whole[:2], case.oracle(bias), "batch-invariant", bias)


# ---- processors ---------------------------------------------------------------------------------------------------------------
def _mask_golden():
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    if os.path.join(here, "golden") not in sys.path:
        sys.path.insert(0, os.path.join(here, "golden"))
    import f1_inputs as FI
    import mask_inputs as MI
    z = np.load(os.path.join(here, "golden", "attn_mask_golden.npz"))
    return FI, MI, z, json.loads(bytes(z["manifest"]).decode())


def _host(C, H, cross, d, proc):
    from instantrestore_amd.attention import Attention
    attn = Attention(query_dim=C, cross_attention_dim=cross, heads=H, dim_head=64)
    with torch.no_grad():
        attn.to_q.weight.copy_(d["wq"]); attn.to_k.weight.copy_(d["wk"]); attn.to_v.weight.copy_(d["wv"])
        attn.to_out[0].weight.copy_(d["wo"]); attn.to_out[0].bias.copy_(d["bo"])
    attn = attn.cuda()
    attn.set_processor(proc)
    return attn


@pytest.mark.parametrize("which", ["AttnProcessor", "SharedAttnProcessor"])
@pytest.mark.parametrize("case_id", ["mx320h5", "ms96h2"])
def test_processors_against_the_reference_with_an_attention_mask(ops, case_id, which):
    """the imported reference's outputs with an attention_mask (tests/golden/make_golden_mask.py), through our processors under
    autocast; the tolerance of tests/test_golden_r4.py: max(2 TOL max(1, |ref|), the reference's own 16-bit deviation)"""
    from face_replace.models.attn_processors import AttnProcessor, SharedAttnProcessor
    FI, MI, z, manifest = _mask_golden()
    m = next(x for x in manifest if x["id"] == case_id)
    d = MI.build(m)
    assert abs(MI.checksum(d) - m["checksum"]) <= 1e-6 * abs(m["checksum"])
    dtype = FI.TORCH_DT[m["lowp"]]
    proc = AttnProcessor() if which == "AttnProcessor" else SharedAttnProcessor(self_attn_idx=None)
    attn = _host(m["C"], m["H"], FI.CROSS if m["kind"] == "cross" else None, d, proc)
    enc = d["encoder"].cuda() if "encoder" in d else None
    outs = []
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        for mask in (d["mask"], d["mask"].repeat_interleave(m["H"], dim=0), d["mask"][:, 0]):     # (B, 1, Lkv), (B * H, 1, Lkv), (B, Lkv)
            outs.append(attn(d["hidden"].cuda(), encoder_hidden_states=enc, attention_mask=mask.cuda()))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    ref = z[f"{case_id}/out"].astype(np.float64)
    got = outs[0][0].float().cpu().numpy()
    err, ref_err = np.abs(got - ref).max(), np.abs(z[f"{case_id}/out_lowp"] - ref).max()
    assert err <= max(2 * {"f16": 1e-3, "bf16": 8e-3}[m["lowp"]] * max(1.0, np.abs(ref).max()), ref_err), (err, ref_err)


@pytest.mark.parametrize("adain", [False, True], ids=["plain", "adain"])
def test_shared_processor_with_ref_weights_and_keep_maps(ops, adain):
    """a shared layer with ref_weights / ref_token_keep in cross_attention_kwargs against the helper oracle driven through the same
    projections (the 16-bit q / k / v the layer computed); AttnProcessor takes the kwargs and ignores them"""
    from face_replace.models.attn_processors import AttnProcessor, SharedAttnProcessor
    from oracle import shared_attn_oracle as O
    B, L, N, H, dtype = 2, 256, 3, 2, torch.bfloat16
    C = 64 * H
    g = torch.Generator().manual_seed(21)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype).float()
    d = dict(wq=r(C, C, sc=C ** -0.5), wk=r(C, C, sc=C ** -0.5), wv=r(C, C, sc=C ** -0.5), wo=r(C, C, sc=C ** -0.5), bo=r(C, sc=0.1))
    hidden, rk, rv = r(B, L, C), r(B, N, L, C), r(B, N, L, C, sc=1.3)
    w = torch.tensor([[1.0, 0.0, 0.25], [4.0, 1.0, 1.0]])
    keep = torch.ones(B, N, 64, 64, dtype=torch.bool)
    keep[1, 0, 32:] = False                                                  # the lower half of reference 0 of entry 1
    proc = SharedAttnProcessor(self_attn_idx=0, use_adain=adain, train_input=True)
    proc.save_attention_mass = True
    attn = _host(C, H, None, d, proc)
    kwargs = dict(ref_keys=[rk.to(dtype).cuda()], ref_values=[rv.to(dtype).cuda()], ref_weights=w.cuda(), ref_token_keep=keep.cuda())
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        out = attn(hidden.cuda(), **kwargs)
        mass = proc.attention_mass
        cap = _host(C, H, None, d, AttnProcessor())
        assert torch.equal(cap(hidden.cuda(), ref_weights=w.cuda(), ref_token_keep=keep.cuda()), cap(hidden.cuda()))
    # the oracle on the layer's own 16-bit q / k / v
    f = lambda t: t.numpy().astype(np.float64)
    rnd = lambda a: torch.from_numpy(a).to(dtype).double().numpy()
    q, k, v = (rnd(f(hidden) @ f(d[n]).T) for n in ("wq", "wk", "wv"))
    bias = ops.key_bias(B, L, N, L, True, ref_weights=w, ref_token_keep=keep).numpy()
    core, _, rmass = biased_attention_np(q, k, v, f(rk), f(rv), H, 0.125, bias, use_adain=adain, train_input=True, seg_lens=[L] * (N + 1))
    ref = core @ f(d["wo"]).T + f(d["bo"])
    check_parity(out, ref, dtype, "shared layer with ref_weights / ref_token_keep", factor=2.0)    # two more 16-bit GEMM roundings (core, out)
    gm = mass.double().cpu().numpy()
    assert np.all(gm[0, :, :, 2] == 0.0) and np.abs(gm.sum(-1) - 1).max() <= 1e-5 and np.abs(gm - rmass).max() <= 4e-3
