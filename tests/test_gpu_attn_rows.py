"""``ir_attn_rows`` on the GPU: the probability rows of chosen query tokens and their head-mean / row-sum reductions.

What is held to what (u = unit roundoff of the 16-bit output format: 2^-8 bf16, 2^-11 fp16):
  1. form "none" is the dump's rows BIT FOR BIT (``torch.equal`` with ``attn_probs(...)[:, :, idx]``): the same expression on the
     same fp32 MFMA result, like the dump kernels among themselves (tests/test_gpu_probs.py);
  2. form "head_mean" against form "none": ``|hm - mean_h float(P0)| <= u * mean_h float(P0) * (1 + 1e-3) + 1e-7`` per element - the
     one rounding that separates the two (the 1e-7 covers fp16 subnormals and the fp32 sum over <= 20 heads);
  3. form "map" against form "head_mean": ``|map - sum_r hm| <= R * 2^-23 * sum_r hm``, the fp32 summation bound;
  4. all forms against the float64 oracle: ``TOL[dtype]`` of tests/test_gpu_probs.py (1e-3 fp16 / 8e-3 bf16) for forms 0 and 1,
     ``R * TOL`` for form 2 - the project's stated bound for probabilities (the LSE of the fused forward limits it);
  5. all forms against the float64 oracle element by element under the relative fp32 bound of tests/prob_bounds.py (reference B).
Each test prints the maxima it saw before it asserts (``pytest -s``; tools/gpu_attn_rows_ab.py records them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import prob_bounds as PB
from oracle import shared_attn_oracle as O

pytestmark = pytest.mark.gpu

TOL = {torch.float16: 1e-3, torch.bfloat16: 8e-3}
UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
FORMS = ("none", "head_mean", "map")

CASES = [
    # B, H, Lq, Ls, N, Lr, include_self        (the lists of tests/test_gpu_probs.py)
    (2, 2, 72, 72, 3, 40, True),       # ragged 64-key steps, partial row block
    (2, 2, 72, 72, 3, 40, False),
    (1, 3, 256, 256, 4, 256, True),    # the 16x16-token class, thin
    (1, 2, 300, 304, 2, 136, True),    # rows not a multiple of 32, key tails of 8 / 48 keys
    (1, 1, 520, 520, 1, 1032, False),  # more than one 256-row workgroup, a reference longer than the query axis
    (2, 1, 64, 64, 8, 64, True),       # eight references
    (1, 2, 96, 96, 0, 0, True),        # no references: plain self attention
    (1, 1, 1024, 1024, 4, 1024, True), # the 32x32-token class, one head: key chunks cut the segments
]
ODD_CASES = [
    (2, 2, 33, 33, 2, 37, True),       # nothing aligned: rows of P start at odd byte offsets
    (1, 2, 64, 64, 3, 20, False),      # Lr % 8 != 0
    (1, 1, 77, 77, 1, 1, True),
]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from instantrestore_amd import ops as _ops
    _ops._lib.lib()
    return _ops


def _rand(shape, dtype, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype)


def _np64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _ids(cases):
    return [f"B{c[0]}H{c[1]}L{c[2]}Ls{c[3]}N{c[4]}Lr{c[5]}s{int(c[6])}" for c in cases]


def _case_inputs(case, dtype, seed=5):
    B, H, Lq, Ls, N, Lr, inc = case
    Cc = H * 64
    gen = torch.Generator().manual_seed(seed)
    q = _rand((B, Lq, Cc), dtype, gen, 1.5)
    k, v = _rand((B, Ls, Cc), dtype, gen, 1.5), _rand((B, Ls, Cc), dtype, gen)
    rk = _rand((B, N, Lr, Cc), dtype, gen, 1.5) if N else None
    rv = _rand((B, N, Lr, Cc), dtype, gen) if N else None
    return q, k, v, rk, rv


def _oracle_probs(q, k, v, rk, rv, H, inc, scale=0.125):
    n = lambda t: None if t is None else _np64(t)
    _, p = O.shared_attention_np(_np64(q), _np64(k), _np64(v), n(rk), n(rv), H, scale, False, inc, return_probs=True)
    return p


def _gpu_lse(ops, q, k, v, rk, rv, H, inc, **kw):
    d = lambda t: None if t is None else t.cuda()
    qd, kd, vd, rkd, rvd = d(q), d(k), d(v), d(rk), d(rv)
    _, lse = ops.shared_attention(qd, kd, vd, rkd, rvd, heads=H, scale=0.125, include_self=inc, return_lse=True, **kw)
    return qd, kd, rkd, lse


def _row_counts(Lq):
    return sorted({min(r, Lq) for r in (1, 5, 68, min(200, Lq))})


def _indices(B, Lq, R, seed):
    """seeded (B, R) int32 indices with forced duplicates (several landmarks fall on one token at the small layers)"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, Lq, size=(B, R))
    if R >= 2:
        idx[:, 1] = idx[:, 0]
    if R >= 5:
        idx[:, -1] = idx[:, 2]
        idx[:, R // 2] = idx[:, 0]
    return torch.from_numpy(idx.astype(np.int32))


def _gather(p, idx):
    """(B, H, L, Lkv) array or tensor -> (B, H, R, Lkv), one index list per batch entry"""
    if isinstance(p, np.ndarray):
        return np.stack([p[b][:, idx[b].numpy()] for b in range(p.shape[0])])
    return torch.stack([p[b][:, idx[b].to(p.device).long()] for b in range(p.shape[0])])


def _oracle_side(q, k, rk, H, inc, scale=0.125, presc=False):
    """(E, delta) of tests/prob_bounds.py's reference B for the 16-bit inputs of a call (``q`` pre-scaled with scale = ln 2 and ``presc``)"""
    return PB.oracle_side(_np64(q), PB.pack_keys(k.cpu(), None if rk is None else rk.cpu(), inc), H, scale, presc)


def _check_forms(got, P0, p_ref_rows, dtype, R, what, E_rows, delta_rows, klass="plain"):
    """items 1-5 of the module docstring on one set of rows; returns the maxima against the oracle"""
    assert got["none"].dtype == dtype and got["head_mean"].dtype == torch.float32 and got["map"].dtype == torch.float32
    assert torch.equal(got["none"], P0), f"{what}: form none is not the dump's rows"
    mean0 = P0.double().mean(dim=1)
    hm = got["head_mean"].double()
    d1 = (hm - mean0).abs()
    bound1 = UNIT[dtype] * mean0 * (1 + 1e-3) + 1e-7
    sum_hm = got["head_mean"].double().sum(dim=1)
    d2 = (got["map"].double() - sum_hm).abs()
    bound2 = R * 2.0 ** -23 * sum_hm
    ref_hm = p_ref_rows.mean(axis=1)
    ref_map = ref_hm.sum(axis=1)
    e0 = float(np.abs(got["none"].float().cpu().numpy() - p_ref_rows).max())
    e1 = float(np.abs(got["head_mean"].cpu().numpy() - ref_hm).max())
    e2 = float(np.abs(got["map"].cpu().numpy() - ref_map).max())
    print(f"attn_rows {what} R={R}: vs oracle none {e0:.3e} head_mean {e1:.3e} map {e2:.3e} (bounds {TOL[dtype]:.0e}, {TOL[dtype]:.0e}, {R * TOL[dtype]:.1e}); "
          f"head_mean vs none max ratio to bound {float((d1 / bound1).max()):.3f}; map vs head_mean max |d| {float(d2.max()):.3e}")
    assert bool((d1 <= bound1).all()), f"{what}: head_mean vs none, worst ratio {float((d1 / bound1).max())}"
    assert bool((d2 <= bound2).all()), f"{what}: map vs head_mean, worst {float(d2.max())}"
    assert np.isfinite(got["none"].float().cpu().numpy()).all()
    assert e0 <= TOL[dtype] and e1 <= TOL[dtype] and e2 <= R * TOL[dtype], (what, e0, e1, e2)
    PB.check_probs(got["none"], p_ref_rows, E_rows, dtype, f"{what} R={R} none", delta=delta_rows, klass=klass)
    cal, der, ref = PB.head_mean_terms(*PB.terms(p_ref_rows, E_rows, None, delta_rows, klass), p_ref_rows)
    PB.check_terms(got["head_mean"], ref, cal, der, f"{what} R={R} head_mean", klass, "head_meanB")
    cal2, der2, ref2 = PB.map_terms(cal, der, ref)
    PB.check_terms(got["map"], ref2, cal2, der2, f"{what} R={R} map", klass, "mapB")
    return e0, e1, e2


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES + ODD_CASES, ids=_ids(CASES + ODD_CASES))
def test_three_forms_against_the_dump_and_the_oracle(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    q, k, v, rk, rv = _case_inputs(case, dtype)
    p_ref = _oracle_probs(q, k, v, rk, rv, H, inc)
    E, delta = _oracle_side(q, k, rk, H, inc)
    qd, kd, rkd, lse = _gpu_lse(ops, q, k, v, rk, rv, H, inc)
    dump = ops.attn_probs(qd, kd, rkd, lse, heads=H, scale=0.125, include_self=inc)
    for R in _row_counts(Lq):
        idx = _indices(B, Lq, R, seed=100 + R)
        got = {f: ops.attn_rows(qd, kd, rkd, lse, idx.cuda(), heads=H, scale=0.125, include_self=inc, reduce=f) for f in FORMS}
        lkv = p_ref.shape[-1]
        assert got["none"].shape == (B, H, R, lkv) and got["head_mean"].shape == (B, R, lkv) and got["map"].shape == (B, lkv)
        _check_forms(got, _gather(dump, idx), _gather(p_ref, idx), dtype, R, f"{_ids([case])[0]} {dtype}", _gather(E, idx), _gather(delta, idx))
        # the same list from the CPU, and a shared (R,) list: both are conveniences of the wrapper over the same call
        again = ops.attn_rows(qd, kd, rkd, lse, idx.long(), heads=H, scale=0.125, include_self=inc, reduce="none")
        assert torch.equal(again, got["none"])
        shared = ops.attn_rows(qd, kd, rkd, lse, idx[0], heads=H, scale=0.125, include_self=inc, reduce="head_mean")
        assert torch.equal(shared[0], got["head_mean"][0])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], ODD_CASES[0]], ids=_ids([CASES[0], CASES[3], ODD_CASES[0]]))
def test_out_of_range_indices_give_zero_rows(ops, case, dtype):
    B, H, Lq, Ls, N, Lr, inc = case
    q, k, v, rk, rv = _case_inputs(case, dtype, seed=8)
    qd, kd, rkd, lse = _gpu_lse(ops, q, k, v, rk, rv, H, inc)
    R = min(40, Lq)
    idx = _indices(B, Lq, R, seed=9)
    bad = idx.clone()
    bad[:, 3], bad[:, 17], bad[:, R - 1] = -1, Lq, 2 ** 31 - 1
    keep = torch.ones(R, dtype=torch.bool)
    keep[[3, 17, R - 1]] = False
    for f in FORMS[:2]:
        a = ops.attn_rows(qd, kd, rkd, lse, idx.cuda(), heads=H, scale=0.125, include_self=inc, reduce=f)
        z = ops.attn_rows(qd, kd, rkd, lse, bad.cuda(), heads=H, scale=0.125, include_self=inc, reduce=f)
        rows = -2
        assert torch.equal(z.index_select(z.dim() + rows, torch.nonzero(keep).flatten().cuda()),
                           a.index_select(a.dim() + rows, torch.nonzero(keep).flatten().cuda())), f
        assert float(z.index_select(z.dim() + rows, torch.nonzero(~keep).flatten().cuda()).abs().max()) == 0.0, f
    # the map adds nothing for them: it equals the map of the list without those entries
    m_bad = ops.attn_rows(qd, kd, rkd, lse, bad.cuda(), heads=H, scale=0.125, include_self=inc, reduce="map")
    hm = ops.attn_rows(qd, kd, rkd, lse, bad.cuda(), heads=H, scale=0.125, include_self=inc, reduce="head_mean")
    s = hm.double().sum(1)
    assert bool(((m_bad.double() - s).abs() <= R * 2.0 ** -23 * s).all())


def test_nothing_is_written_outside_the_output(ops):
    """canary: the buffer behind each form's output keeps its fill (partial row block, key tails, aligned and unaligned rows)"""
    from instantrestore_amd import _lib
    for case, dtype in ((CASES[0], torch.float16), (ODD_CASES[0], torch.bfloat16), (CASES[3], torch.bfloat16)):
        B, H, Lq, Ls, N, Lr, inc = case
        q, k, v, rk, rv = _case_inputs(case, dtype)
        qd, kd, rkd, lse = _gpu_lse(ops, q, k, v, rk, rv, H, inc)
        lkv = (Ls if inc else 0) + N * Lr
        args, *_keep = ops._probs_args(qd, kd, rkd, lse, H, 0.125, inc)
        args.tuning = 0
        for R in (5, min(68, Lq)):
            idx = _indices(B, Lq, R, seed=3).cuda()
            for red, (n, dt) in enumerate(((B * H * R * lkv, dtype), (B * R * lkv, torch.float32), (B * lkv, torch.float32))):
                big = torch.full((n + 65536,), 7.0, dtype=dt, device="cuda")
                _lib.check(_lib.lib().ir_attn_rows(C.byref(args), idx.data_ptr(), R, red, big.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream), "rows")
                torch.cuda.synchronize()
                assert bool((big[n:] == 7.0).all()), f"stores past the end of the output (reduce {red}, R {R}, {case})"
                assert bool((big[:n] <= (R if red == 2 else 1.0) * 1.01).all()), f"unwritten elements inside the output (reduce {red}, R {R}, {case})"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", [CASES[0], CASES[5], ODD_CASES[0]], ids=_ids([CASES[0], CASES[5], ODD_CASES[0]]))
def test_repeatable_and_batch_invariant(ops, case, dtype):
    """two runs are equal, and entry b alone (its own q, K, lse, index list) equals its slice of the batched call, in all forms"""
    B, H, Lq, Ls, N, Lr, inc = case
    assert B > 1
    q, k, v, rk, rv = _case_inputs(case, dtype, seed=12)
    qd, kd, rkd, lse = _gpu_lse(ops, q, k, v, rk, rv, H, inc)
    for R in (5, min(68, Lq)):
        idx = _indices(B, Lq, R, seed=21).cuda()
        for f in FORMS:
            a = ops.attn_rows(qd, kd, rkd, lse, idx, heads=H, scale=0.125, include_self=inc, reduce=f)
            assert torch.equal(a, ops.attn_rows(qd, kd, rkd, lse, idx, heads=H, scale=0.125, include_self=inc, reduce=f))
            assert torch.equal(a, ops.attn_rows(qd, kd, rkd, lse, idx, heads=H, scale=0.125, include_self=inc, reduce=f, batch_invariant=True))
            for b in range(B):
                one = ops.attn_rows(qd[b:b + 1].contiguous(), kd[b:b + 1].contiguous(), None if rkd is None else rkd[b:b + 1].contiguous(),
                                    lse[b:b + 1].contiguous(), idx[b:b + 1].contiguous(), heads=H, scale=0.125, include_self=inc, reduce=f)
                assert torch.equal(one[0], a[b]), (f, b)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 2, 72, 3, 40), (1, 2, 300, 2, 136)], ids=["L72", "L300"])
def test_prescaled_q(ops, dtype, shape):
    """IR_FLAG_Q_PRESCALED: bit-equal to the dump's rows under the same flag, and within TOL of the oracle run with scale = ln 2"""
    B, H, L, N, Lr = shape
    Cc = H * 64
    gen = torch.Generator().manual_seed(11)
    q = _rand((B, L, Cc), dtype, gen, 1.5)
    qs = (q.float() * (0.125 * 1.4426950408889634)).to(dtype).cuda()          # what the fused q/k/v projection hands over
    k, v = _rand((B, L, Cc), dtype, gen, 1.5).cuda(), _rand((B, L, Cc), dtype, gen).cuda()
    rk, rv = _rand((B, N, Lr, Cc), dtype, gen, 1.5).cuda(), _rand((B, N, Lr, Cc), dtype, gen).cuda()
    _, lse = ops.shared_attention(qs, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True, q_prescaled=True)
    dump = ops.attn_probs(qs, k, rk, lse, heads=H, scale=0.125, include_self=True, q_prescaled=True)
    p_ref = _oracle_probs(qs, k, v, rk, rv, H, True, scale=0.6931471805599453)
    R = min(68, L)
    idx = _indices(B, L, R, seed=31)
    got = {f: ops.attn_rows(qs, k, rk, lse, idx.cuda(), heads=H, scale=0.125, include_self=True, reduce=f, q_prescaled=True) for f in FORMS}
    E, delta = _oracle_side(qs, k, rk, H, True, scale=0.6931471805599453, presc=True)
    _check_forms(got, _gather(dump, idx), _gather(p_ref, idx), dtype, R, f"prescaled {shape} {dtype}", _gather(E, idx), _gather(delta, idx), klass="presc")


def test_capturable_and_follows_the_index_tensor(ops):
    """one torch.cuda.graph on one stream holding the rows call; the index tensor is overwritten in place; the replay equals an
    eager call with the new list"""
    dtype = torch.bfloat16
    case = CASES[2]
    B, H, Lq, Ls, N, Lr, inc = case
    q, k, v, rk, rv = _case_inputs(case, dtype, seed=14)
    qd, kd, rkd, lse = _gpu_lse(ops, q, k, v, rk, rv, H, inc)
    R = 68
    idx = _indices(B, Lq, R, seed=1).cuda()
    new = _indices(B, Lq, R, seed=2).cuda()
    assert not torch.equal(idx, new)
    for f in FORMS:
        static_idx = idx.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.attn_rows(qd, kd, rkd, lse, static_idx, heads=H, scale=0.125, include_self=inc, reduce=f)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.attn_rows(qd, kd, rkd, lse, static_idx, heads=H, scale=0.125, include_self=inc, reduce=f)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.attn_rows(qd, kd, rkd, lse, idx, heads=H, scale=0.125, include_self=inc, reduce=f)), f
        static_idx.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.attn_rows(qd, kd, rkd, lse, new, heads=H, scale=0.125, include_self=inc, reduce=f)), f
        del graph


def test_through_the_plugin_surface(ops):
    """SharedAttnProcessor on the host Attention: ``attention_rows`` is the gather of the ``attention_probs`` the same call
    dumps; without the dump the same rows come out and no (B, H, L, Lkv) tensor is formed; the layer output does not change"""
    from face_replace.models.attn_processors import SharedAttnProcessor
    from instantrestore_amd.attention import Attention
    torch.manual_seed(4)
    B, H, L, N = 2, 2, 256, 4
    Cc = H * 64
    for train_input in (True, False):
        proc = SharedAttnProcessor(self_attn_idx=0, save_self_attentions=True, use_adain=True, train_input=train_input)
        attn = Attention(query_dim=Cc, heads=H, dim_head=64, processor=proc).cuda()
        x = torch.randn(B, L, Cc, device="cuda")
        rk = torch.randn(B, N, L, Cc, device="cuda", dtype=torch.bfloat16)
        rv = torch.randn(B, N, L, Cc, device="cuda", dtype=torch.bfloat16)
        idx = _indices(B, L, 68, seed=6)
        run = lambda: attn(x, ref_keys=[rk], ref_values=[rv])
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y_plain = run()
            assert proc.attention_rows is None
            proc.attention_rows_index, proc.attention_rows_reduce = idx, "none"
            y_both = run()
            S = N + int(train_input)
            assert proc.attention_probs.shape == (B, H, L, S * L) and proc.attention_rows.shape == (B, H, 68, S * L)
            assert torch.equal(proc.attention_rows, _gather(proc.attention_probs, idx))
            rows_both = proc.attention_rows
            proc.save_self_attentions, proc.attention_probs = False, None
            y_rows = run()
            assert proc.attention_probs is None and torch.equal(proc.attention_rows, rows_both)
            proc.attention_rows_reduce = "map"
            run()
            assert proc.attention_rows.shape == (B, S * L) and proc.attention_rows.dtype == torch.float32
            assert float((proc.attention_rows.sum(-1) - 68).abs().max()) <= 68 * 8e-3      # 68 rows, each a probability distribution
        assert torch.equal(y_plain, y_both) and torch.equal(y_plain, y_rows)


def test_example_landmark_maps_switch(capsys):
    """examples/synthetic_inference.py --landmark-maps: every shared layer with at least 68 tokens prints its map"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "synthetic_inference.py")
    spec = importlib.util.spec_from_file_location("synthetic_inference_rows", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--identities", "2", "--refs", "3", "--px", "256", "--small", "--landmark-maps", "--dtype", "bf16"])
    text = capsys.readouterr().out
    assert out.shape == (2, 256, 256, 3)
    assert text.count("landmark map (2, ") == 6 and "picture (32, 128)" in text and "picture (16, 64)" in text, text


def test_1024px_layer_where_the_dump_cannot_exist(ops):
    """cfg 5's top shared layer at one identity (L = Ls = Lr = 16384, N = 4, H = 5, bf16): the dump would need 13.4 GB; the rows
    call allocates its output and nothing else.  The reference values of the 68 rows (scores, their own float64 LSE,
    probabilities) are computed here with NumPy and held to the bounds of item 4."""
    dtype = torch.bfloat16
    B, H, L, N, R = 1, 5, 16384, 4, 68
    Cc = H * 64
    g = torch.Generator(device="cuda").manual_seed(2)
    q = (torch.randn(B, L, Cc, device="cuda", generator=g) * 1.2).to(dtype)
    k = torch.randn(B, L, Cc, device="cuda", generator=g).to(dtype)
    v = torch.randn(B, L, Cc, device="cuda", generator=g).to(dtype)
    rk = torch.randn(B, N, L, Cc, device="cuda", generator=g).to(dtype)
    rv = torch.randn(B, N, L, Cc, device="cuda", generator=g).to(dtype)
    _, lse = ops.shared_attention(q, k, v, rk, rv, heads=H, scale=0.125, include_self=True, return_lse=True)
    idx = _indices(B, L, R, seed=5).cuda()
    lkv = (N + 1) * L
    # float64 reference of the chosen rows only
    ii = idx[0].long()
    qr = _np64(q[0, ii]).reshape(R, H, 64).transpose(1, 0, 2)                               # (H, R, 64)
    kext = np.concatenate([_np64(k[0])] + [_np64(rk[0, n]) for n in range(N)], axis=0)      # (Lkv, C)
    kext = kext.reshape(lkv, H, 64).transpose(1, 2, 0)                                      # (H, 64, Lkv)
    s = np.matmul(qr, kext) * 0.125
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    p_ref = (e / e.sum(-1, keepdims=True))[None]                                            # (1, H, R, Lkv)
    got = {}
    sizes = {"none": B * H * R * lkv * 2, "head_mean": B * R * lkv * 4, "map": B * lkv * 4}
    for f in FORMS:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        got[f] = ops.attn_rows(q, k, rk, lse, idx, heads=H, scale=0.125, include_self=True, reduce=f)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        print(f"attn_rows 1024px {f}: peak memory rise {rise} bytes for an output of {sizes[f]}")
        assert rise <= sizes[f] + (1 << 20), (f, rise, sizes[f])
    assert got["none"].shape == (B, H, R, lkv)
    # items 2-4 (item 1 needs the dump); the rows of one index are equal among its duplicates
    P0 = got["none"]
    assert torch.equal(P0[:, :, 0], P0[:, :, 1])
    mean0 = P0.double().mean(dim=1)
    d1 = (got["head_mean"].double() - mean0).abs()
    assert bool((d1 <= UNIT[dtype] * mean0 * (1 + 1e-3) + 1e-7).all())
    sum_hm = got["head_mean"].double().sum(dim=1)
    assert bool(((got["map"].double() - sum_hm).abs() <= R * 2.0 ** -23 * sum_hm).all())
    ref_hm = p_ref.mean(axis=1)
    e0 = float(np.abs(P0.float().cpu().numpy() - p_ref).max())
    e1 = float(np.abs(got["head_mean"].cpu().numpy() - ref_hm).max())
    e2 = float(np.abs(got["map"].cpu().numpy() - ref_hm.sum(axis=1)).max())
    print(f"attn_rows 1024px bf16 R=68: vs float64 none {e0:.3e} head_mean {e1:.3e} map {e2:.3e}")
    assert e0 <= TOL[dtype] and e1 <= TOL[dtype] and e2 <= R * TOL[dtype], (e0, e1, e2)
