"""tests/out_bounds.py without a GPU.  An fp32 emulation of the kernels' lazy walk - 64-key tiles, the running reference moved only
when the row max outgrows it by 2^6 (or, for the forms that check after the exponentials, when an 8-key partial sum exceeds 2^11),
P rounded to the 16-bit type ahead of P.V, the AdaIN fold per segment into a total that is rescaled with the reference, K/V-range
pieces merged by (O, m, l) - stays inside the bound on every input set of tests/test_gpu_out_walks.py; planted defects in exactly
that code leave it by more than 4 bounds; and the inputs do what the GPU tests rely on: every (shape, family) pair moves the
reference after the first tile on at least 10 % of its rows, "ramp" on every row, N(0, 1) on none - which is why the files
whose inputs are plain ``randn`` cannot see this code.

Where a defect can show.  "acc" (the accumulator not scaled at a row's last move) and "key" (one key lost: the family's dominant
key where it has one - what an off-by-one at a tile, segment, count or piece boundary loses - else the walk's last key) apply to
every set; "tot" (the fold total not scaled at that move) needs the fold and a move behind the first folded segment; "affine"
(the last reference folded with its neighbour's affine) needs the fold and two references; "merge" (a piece merged with the other
piece's maximum) needs the two pieces.  A (shape, family) pair is held to each defect over the variants - dtype, fold, rule - in
which the defect's code runs at all; the pairs in which it never runs (no reference, a walk whose moves all lie in the first
segment) are counted and printed."""
import numpy as np
import pytest
import torch

import lse_bounds as LB
import lse_cases as LC
import out_bounds as OB
from key_bias_oracle import biased_attention_np
from oracle import shared_attn_oracle as O
from region_oracle import allowed_np, masked_attention_np

DTYPES = [torch.bfloat16, torch.float16]
f32 = np.float32


def _round(p, dtype):
    return torch.from_numpy(np.ascontiguousarray(p)).to(dtype).float().numpy()


def emulate(q, keys, vals, heads, tile_lists, n_seg, affine, dtype, bias=None, allowed=None, rule="max6", pieces=1, defect=None, at_tile=None, lost=None):
    """the lazy walk in fp32.  q (B, Lq, C), keys / vals (B, Lkv, C) float64 of 16-bit values; tile_lists[b]: (first key, one past
    the last, segment) per tile; affine (a, b) (B, N, C) of the LAST N segments or None; bias (B, Lkv) added to the scores (-inf
    masks); allowed bool (B, 1, Lq, Lkv).  Returns out (B, Lq, C) fp32, moves (B, H, Lq): moves of the reference after the row's
    first live tile (``lost[b]``: the key the defect "key" loses), moves_folded: those behind the first folded segment, last (B, H, Lq): the tile of the last move (-1: none), last_acc: the
    tile of the last move that met a non-empty accumulator"""
    B, Lq, C = q.shape
    d = C // heads
    out = np.zeros((B, Lq, C), dtype=f32)
    moves, moves_f, last, last_acc = (np.zeros((B, heads, Lq), dtype=np.int64) for _ in range(4))
    last -= 1
    last_acc -= 1
    fold = affine is not None
    for b in range(B):
        qh = q[b].reshape(Lq, heads, d).transpose(1, 0, 2)
        kh = keys[b].reshape(-1, heads, d).transpose(1, 2, 0)
        vh = np.ascontiguousarray(vals[b].reshape(-1, heads, d).transpose(1, 0, 2), dtype=f32)       # (H, Lkv, d)
        s = (np.matmul(qh, kh) * LC.QC).astype(f32)
        if bias is not None:
            s = np.where(np.isfinite(bias[b]) & (bias[b] > OB.MASKED), s + (bias[b] * LC.LOG2E).astype(f32), f32(-np.inf)).astype(f32)
        if allowed is not None:
            s = np.where(allowed[b], s, f32(-np.inf))
        tl = tile_lists[b]
        cut = [0, len(tl)] if pieces == 1 else [0, len(tl) // 2, len(tl)]
        parts = []
        for pc in range(len(cut) - 1):
            m = np.full((heads, Lq), -np.inf, dtype=f32)
            l, lseg = np.zeros((heads, Lq), dtype=f32), np.zeros((heads, Lq), dtype=f32)
            acc, tot = np.zeros((heads, Lq, d), dtype=f32), np.zeros((heads, Lq, d), dtype=f32)
            folded = False
            for ti in range(cut[pc], cut[pc + 1]):
                t0, t1, sg = tl[ti]
                st = s[..., t0:t1]
                mx = st.max(-1)
                start = np.isneginf(m) & np.isfinite(mx)
                with np.errstate(invalid="ignore", over="ignore"):
                    if rule == "max6":
                        move = (mx > m + f32(6)) | start
                    else:
                        pe = np.exp2(st - np.where(np.isneginf(m), f32(0), m)[..., None])
                        pad = (-pe.shape[-1]) % 8
                        grp = np.pad(pe, ((0, 0), (0, 0), (0, pad))).reshape(heads, Lq, -1, 8).sum(-1, dtype=f32)
                        move = (~(grp.max(-1) <= f32(2048)) & np.isfinite(mx) & (mx > m)) | start
                    real = move & ~start
                    m_new = np.where(move, np.maximum(m, mx), m)
                    alpha = np.where(move, np.where(start, f32(0), np.exp2(m - m_new)), f32(1)).astype(f32)
                moves[b] += real
                moves_f[b] += real & folded
                last[b] = np.where(real, ti, last[b])
                if not (fold and tl[ti - 1][2] != sg):                # the fold has just emptied the accumulator on a segment's first tile
                    last_acc[b] = np.where(real, ti, last_acc[b])
                hit = (at_tile[b] == ti) & real if at_tile is not None else np.zeros_like(real)
                acc *= np.where(hit & (defect == "acc"), f32(1), alpha)[..., None]
                tot *= np.where(hit & (defect == "tot"), f32(1), alpha)[..., None]
                l, lseg, m = l * alpha, lseg * alpha, m_new
                with np.errstate(invalid="ignore"):
                    p = np.where(np.isneginf(m)[..., None], f32(0), np.exp2(st - np.where(np.isneginf(m), f32(0), m)[..., None])).astype(f32)
                if defect == "key" and t0 <= lost[b] < t1:
                    p[..., lost[b] - t0] = 0
                ps = p.sum(-1, dtype=f32)
                l, lseg = l + ps, lseg + ps
                acc = acc + np.matmul(_round(p, dtype), vh[:, t0:t1])      # 16-bit x 16-bit products are exact in fp32; fp32 sums
                if fold and (ti + 1 == cut[pc + 1] or tl[ti + 1][2] != sg):
                    n = sg - (n_seg - affine[0].shape[1])
                    if n < 0:
                        tot = tot + acc
                    else:
                        if defect == "affine" and n == affine[0].shape[1] - 1:
                            n -= 1
                        a_s = affine[0][b, n].reshape(heads, 1, d).astype(f32)
                        b_s = affine[1][b, n].reshape(heads, 1, d).astype(f32)
                        tot = (tot + (a_s * acc + b_s * lseg[..., None]).astype(f32)).astype(f32)
                        folded = True
                    acc, lseg = np.zeros_like(acc), np.zeros_like(lseg)
            parts.append((tot if fold else acc, m, l))
        if len(parts) == 1:
            num, m, l = parts[0]
        else:
            (n1, m1, l1), (n2, m2, l2) = parts
            M = np.maximum(m1, m2)
            ma, mb = (m2, m1) if defect == "merge" else (m1, m2)
            with np.errstate(invalid="ignore"):
                w1 = np.where(np.isneginf(M), f32(0), np.exp2(ma - np.where(np.isneginf(M), f32(0), M))).astype(f32)
                w2 = np.where(np.isneginf(M), f32(0), np.exp2(mb - np.where(np.isneginf(M), f32(0), M))).astype(f32)
            num, l = w1[..., None] * n1 + w2[..., None] * n2, w1 * l1 + w2 * l2
        with np.errstate(invalid="ignore", divide="ignore"):
            o = np.where((l > 0)[..., None], num / np.where(l > 0, l, f32(1))[..., None], f32(0))
        out[b] = o.transpose(1, 0, 2).reshape(Lq, C)
    return out, moves, moves_f, last, last_acc


_PACKED = {}
SHORT = 72     # query axes up to this length are evaluated on every row
ROWS = 32      # rows per entry the sets are evaluated on (rows are independent: a sample of a long query axis checks the same code)


class Set:
    """one input set of the GPU file, every entry, on a sample of its rows where the query axis is longer than SHORT (every
    ceil(Lq / ROWS)-th row and the REGION case's dead rows), with its oracle: built once, left unchanged.  ``full=True``: every row of every entry; ``full=n``: n rows per entry"""

    def __init__(self, shape, family, kind, which, dtype, fold, presc, full=False):
        self.shape, self.family, self.kind, self.dtype, self.fold, self.presc = shape, family, kind, dtype, fold, presc
        B, H, Lq, Ls, N, Lr, inc = shape
        bias, counts, region = LC.case_mask(shape, kind, which, family)
        x = LC.inputs(shape, family, dtype, style=True, counts=counts)
        self.which = which
        ent = list(range(B))
        want = Lq if full is True or Lq <= SHORT else ROWS if not full else full
        rows = np.array(sorted(set(range(0, Lq, -(-Lq // want))) | ({7, Lq - 50} if Lq > 57 else set())))
        pk = (id(x), tuple(ent))
        if pk not in _PACKED:        # per input tensors: the packed float64 keys / values of the sampled entries and their fp32 affine
            sub = lambda t: None if t is None else t[ent]
            a, b = O.adain_affine_np(LC.np64(sub(x.v)), LC.np64(sub(x.rv)), H) if N else (None, None)
            _PACKED[pk] = (x, LB.pack_keys(sub(x.k), sub(x.rk), inc).numpy(), LB.pack_keys(sub(x.v), sub(x.rv), inc).numpy(),
                              None if a is None else (a.astype(f32).astype(np.float64), b.astype(f32).astype(np.float64)))
        _, self.keys, self.vals, aff = _PACKED[pk]
        qt = (x.qs if presc else x.q)[:, torch.from_numpy(rows)][ent]
        self.q = LC.np64(qt) / LC.QC if presc else LC.np64(qt)
        self.seg_lens = LC.seg_lens(shape)
        self.affine = aff if fold else None
        self.counts = None if counts is None else [counts[b] for b in ent]
        self.bias = None if bias is None else bias.double().numpy()[ent]
        if counts is not None:
            self.bias = OB.counts_bias(self.counts, self.seg_lens, N)
        self.allowed = None if region is None else allowed_np(region[0].numpy(), region[1].numpy())[ent][:, :, rows]
        self.tiles = [LC.tiles(shape, None if counts is None else counts[b]) for b in ent]
        dom = LC.dominant_key(shape, family, counts)
        self.lost = None if dom is None else [dom[b] for b in ent]                       # the defect "key"; None: the heaviest key
        self._ref = None
        self.name = f"{LC.sid(shape)}-{family}-{kind}{'-' + which if which else ''}-{'bf16' if dtype == torch.bfloat16 else 'f16'}-" \
                    f"{'fold' if fold else 'nofold'}-{'prescq' if presc else 'plainq'}"

    @property
    def ref(self):
        if self._ref is None:
            self._ref = OB.oracle_out_and_scales(self.q, self.keys, self.vals, self.shape[1], LC.SCALE, self.seg_lens, affine=self.affine,
                                                 bias=self.bias, allowed=self.allowed)
        return self._ref

    def heaviest(self):
        """per entry, the key with the largest probability in any of the rows"""
        lse = self.ref.lse
        out = []
        for b in range(self.q.shape[0]):
            H, d = self.shape[1], 64
            sc = np.matmul(self.q[b].reshape(-1, H, d).transpose(1, 0, 2), self.keys[b].reshape(-1, H, d).transpose(1, 2, 0)) * LC.SCALE
            sc = sc + (0.0 if self.bias is None else np.where(self.bias[b] > OB.MASKED, self.bias[b], -np.inf))
            sc = sc if self.allowed is None else np.where(self.allowed[b], sc, -np.inf)
            with np.errstate(invalid="ignore"):
                p = np.where(np.isfinite(lse[b])[..., None], np.exp(sc - np.where(np.isfinite(lse[b]), lse[b], 0.0)[..., None]), 0.0)
            out.append(int(p.max((0, 1)).argmax()))
        return out

    def run(self, **kw):
        if kw.get("defect") == "key" and self.lost is None:
            self.lost = self.heaviest()
        return emulate(self.q, self.keys, self.vals, self.shape[1], self.tiles, len(self.seg_lens), self.affine, self.dtype, bias=self.bias,
                       allowed=self.allowed, rule="sum11" if self.presc else "max6", lost=self.lost, **kw)

    def ratio(self, out):
        return OB.check_out(out, self.ref, self.dtype, self.name, frame=self.presc, enforce=False)


_SETS = {}


def _set(*key):
    """the set and its walk without a defect: (out, moves, moves behind a fold, tile of the last move), once"""
    if key not in _SETS:
        s = Set(*key)
        _SETS[key] = (s, s.run(pieces=2 if s.shape in LC.PIECES else 1))
    return _SETS[key]


def _sets(cases, prescs=(False, True)):
    for shape, family, kind, which in cases:
        for dtype in DTYPES:
            for fold in ((False, True) if shape[4] else (False,)):
                # plain Q under the 2^6 rule; the pre-scaled Q under the 2^11 partial-sum rule of the forms that check after the exponentials
                for presc in prescs:
                    yield _set(shape, family, kind, which, dtype, fold, presc)


CASES = LC.out_walk_cases()


# ---- helper semantics ---------------------------------------------------------------------------------------------------------------
def test_check_out_is_elementwise_and_dead_rows_are_exact(tmp_path, monkeypatch):
    s = Set(LC.REGION, "spike", "region", None, torch.bfloat16, True, False, full=True)
    ref = s.ref
    assert np.isneginf(ref.lse[:, :, 7]).all() and (ref.out[:, 7] == 0).all()            # a row that may attend nothing
    bnd, _, _ = OB.out_bound(torch.bfloat16, ref.A, ref.S, ref.scale, 2, ref.U)
    good = ref.out + 0.5 * bnd
    assert abs(OB.check_out(good, ref, torch.bfloat16, "half a bound") - 0.5) < 1e-9
    at = np.unravel_index(int(np.where(bnd > 0, bnd, np.inf).argmin()), bnd.shape)      # the element with the smallest bound
    bad = ref.out.copy()
    bad[at] += 2.0 * bnd[at]
    assert 2.0 * bnd[at] < 0.1 * bnd.max()                                               # a max-norm gate would not see it
    with pytest.raises(AssertionError, match="out off by"):
        OB.check_out(bad, ref, torch.bfloat16, "one element")
    dead = ref.out.copy()
    dead[0, 7, 5] = 1e-30
    with pytest.raises(AssertionError, match="not exactly 0"):
        OB.check_out(dead, ref, torch.bfloat16, "a dead row")
    nan = ref.out.copy()
    nan[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        OB.check_out(nan, ref, torch.bfloat16, "NaN")
    with pytest.raises(AssertionError):
        OB.check_out(ref.out[:, :5], ref, torch.bfloat16, "shape")
    log = tmp_path / "out.jsonl"
    monkeypatch.setenv("IR_PARITY_LOG", str(log))
    monkeypatch.setenv("IR_OUT_SOFT", "1")
    assert OB.check_out(bad, ref, torch.bfloat16, "soft: recorded, not failed") > 1.0
    with pytest.raises(AssertionError):
        OB.check_out(nan, ref, torch.bfloat16, "soft mode does not excuse NaN")
    import json
    rec = json.loads(log.read_text().splitlines()[0])
    assert rec["kind"] == "out" and rec["r"] > 1.0 and rec["r2"] > 0.0 and rec["at"] == [int(i) for i in at]
    # fp16's first term is 8 times smaller
    assert OB.U_P[torch.float16] * 8 == OB.U_P[torch.bfloat16] == 2.0 ** -8


def test_the_reference_is_the_oracles():
    """``oracle_out_and_scales`` against oracle.shared_attn_oracle (with and without AdaIN), tests/key_bias_oracle.py (bias, counts as
    a tail mask) and tests/region_oracle.py: the same float64 numbers to 1e-12; the row scales are ``lse_bounds.row_scale``"""
    f = LC.np64
    for shape, kind, which in ((LC.PIPE32[0], "plain", None), (LC.PIPE32[1], "plain", None), (LC.BIASED, "bias", "finite_one_entry_masked"),
                               (LC.BIASED, "bias", "scatter"), (LC.BIASED, "counts", None), (LC.REGION, "region", None)):
        B, H, Lq, Ls, N, Lr, inc = shape
        bias, counts, region = LC.case_mask(shape, kind, which)
        x = LC.inputs(shape, "n15", torch.bfloat16, style=True)
        keys, vals, sl = LB.pack_keys(x.k, x.rk, inc), LB.pack_keys(x.v, x.rv, inc), LC.seg_lens(shape)
        for fold in (False, True):
            aff = O.adain_affine_np(f(x.v), f(x.rv), H) if fold else None
            args = (f(x.q), f(x.k), f(x.v), f(x.rk), f(x.rv), H, LC.SCALE)
            if kind == "plain":
                ref = O.shared_attention_np(*args, fold, inc)
                got = OB.oracle_out_and_scales(f(x.q), keys, vals, H, LC.SCALE, sl, affine=aff)
                kb = None
            elif kind == "region":
                al = allowed_np(region[0].numpy(), region[1].numpy())
                ref, lse = masked_attention_np(*args, al, use_adain=fold, train_input=inc)
                got = OB.oracle_out_and_scales(f(x.q), keys, vals, H, LC.SCALE, sl, affine=aff, allowed=al)
                kb = "region"
            else:
                kb = bias.double().numpy() if counts is None else LC.tail_bias(shape, counts)
                ref, lse = biased_attention_np(*args, kb, use_adain=fold, train_input=inc)
                got = OB.oracle_out_and_scales(f(x.q), keys, vals, H, LC.SCALE, sl, affine=aff, bias=None if counts else kb, counts=counts)
            assert np.abs(got.out - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (shape, kind, fold)
            assert (got.A <= got.S).all() and (np.abs(got.out) <= got.S * (1 + 1e-12) + 1e-300).all()
            if kb is not None:
                assert np.array_equal(np.isneginf(lse), np.isneginf(got.lse))
                live = np.isfinite(lse)
                assert np.abs(lse[live] - got.lse[live]).max() <= 1e-12 * np.abs(lse[live]).max()
            if kb is None or isinstance(kb, np.ndarray):
                for frame, mine in ((False, got.scale), (True, got.scale_frame)):
                    assert np.abs(LB.row_scale(f(x.q), keys, LC.SCALE, got.lse, bias=kb, frame=frame) - mine).max() <= 1e-9
            if not fold:
                assert np.array_equal(got.A, got.S)


# ---- the inputs do what the GPU tests rely on ------------------------------------------------------------------------------------------
def _moves(shape, family, kind, which, presc, dtype=torch.bfloat16):
    s = Set(shape, family, kind, which, dtype, False, presc, full=128)           # every entry, 128 rows of each
    moves = s.run()[1]
    live = np.isfinite(s.ref.lse)
    return moves[live]


# "ramp" outside the plain long walks, by rule: the smallest share is the two-tile walk's (B1 H1 Lq128 Ls128, no reference): 0.79 / 0.25
RAMP_FLOOR = {False: 0.75, True: 0.25}


def test_every_relied_on_pair_moves_the_reference_and_plain_randn_does_not():
    """conditions of the inputs, per case of the GPU file: after the first tile the reference moves on at least 10 % of the rows under
    the 2^6 row-max rule, and - with the pre-scaled Q - under the 2^11 partial-sum rule, for every case the GPU file relies on
    (``lse_cases.relied_on``; under the 2^11 rule the "spike" and "peaky" recipes stay as they are and are not relied on: one key
    times 6 outgrows a reference by 11 exponent units on fewer rows).  The shares of the cases that are NOT relied on are printed;
    the GPU file marks them in its output and its records.  "ramp" moves the reference on every row of a plain walk of four tiles
    or more under the 2^6 rule, and on at least RAMP_FLOOR of the rows of every other case, masked kinds and the 2^11 rule
    included; N(0, 1) - what tests/test_gpu_key_bias.py, test_gpu_ref_lens.py, test_gpu_region.py and test_gpu_item_grid.py feed -
    on none."""
    low, ramp, others = [], [], []
    for shape, family, kind, which in CASES:
        for presc in (False, True):
            share = float((_moves(shape, family, kind, which, presc) > 0).mean())
            rec = (round(share, 3), LC.sid(shape), family, kind, which, "2^11" if presc else "2^6")
            if not LC.relied_on(shape, family, kind, which, presc):
                others.append(rec)
                continue
            low.append(rec)
            assert share >= 0.10, f"{rec}: the reference moves on {share:.3f} of the rows"
            if family == "ramp":
                ramp.append(rec)
                every = kind == "plain" and not presc and len(LC.tiles(shape)) >= 4
                assert share == 1.0 if every else share >= RAMP_FLOOR[presc], f"{rec}: ramp moves the reference on {share:.3f} of the rows"
    print("lowest shares of moving rows:", sorted(low)[:5])
    print("lowest ramp shares:", sorted(ramp)[:4])
    print("not relied on:", sorted(others))
    for shape in dict.fromkeys(s for s, _, _, _ in CASES):
        for presc in (False, True):
            for dtype in DTYPES:
                x = Set(shape, "n1", "plain", None, dtype, False, presc)
                assert int(x.run()[1].sum()) == 0, f"{LC.sid(shape)} N(0, 1) prescq={presc}: the reference moved"


# ---- achievability and discriminating power ---------------------------------------------------------------------------------------------
def test_the_emulated_walk_is_inside_the_bound():
    worst = {}
    n = 0
    for s, res in _sets(CASES):
        r = OB.check_out(res[0], s.ref, s.dtype, f"fp32 emulation on {s.name}", frame=s.presc)
        worst[s.dtype] = max(worst.get(s.dtype, (0.0, None)), (r, s.name))
        n += 1
    for dtype, (r, name) in worst.items():
        print(f"fp32 emulation of the lazy walk, {dtype}: largest ratio {r:.3f} of the bound on {name} ({n} sets in all)")
        assert r <= 1.0


DEFECTS = ["acc", "tot", "affine", "merge", "key"]


def test_planted_defects_leave_the_bound_and_are_invisible_on_plain_randn():
    """every defect, in EVERY variant (case, dtype, fold on / off) in which its code runs, leaves the bound by more than 4 bounds on at
    least one row: nothing is carried by the other dtype or by the other fold setting"""
    seen = {d: {} for d in DEFECTS}
    for s, (_, moves, moves_f, last, last_acc) in _sets(CASES, prescs=(False,)):
        two = s.shape in LC.PIECES
        var = (s.shape, s.family, s.kind, s.which, s.dtype, s.fold)
        for d in DEFECTS:
            # one-tile references: with the fold every move behind the self segment meets an emptied accumulator - "tot" is the defect there
            runs = {"acc": bool((last_acc >= 0).any()) and not (s.fold and s.shape[5] <= LC.KVB), "tot": s.fold and bool(moves_f.any()), "affine": s.fold and s.shape[4] >= 2,
                    "merge": two, "key": True}[d]
            if not runs:
                seen[d][var] = None
                continue
            seen[d][var] = s.ratio(s.run(pieces=2 if two else 1, defect=d, at_tile=last_acc if d == "acc" else last)[0])
    for d in DEFECTS:
        held = {k: v for k, v in seen[d].items() if v is not None}
        never = [k for k, v in seen[d].items() if v is None]
        for dtype in DTYPES:
            print(f"defect {d}, {dtype}: {sum(k[4] == dtype for k in held)} variants, smallest ratio "
                  f"{min(v for k, v in held.items() if k[4] == dtype):.1f}; its code never runs in {sum(k[4] == dtype for k in never)}")
        idle = [(LC.sid(k[0]),) + k[1:] for k in never if d in ("acc", "key") and LC.relied_on(k[0], k[1], k[2], k[3])
                and not (k[0] in LC.PIECES and k[1] == "at:piece_first")         # there the move IS the merge: defect "merge"
                and not (d == "acc" and k[5])]        # with the fold a move on a segment's first tile meets an empty accumulator: "tot"
        assert not idle, f"defect {d} never runs in {idle}"
        bad = {(LC.sid(k[0]),) + k[1:]: round(v, 2) for k, v in held.items() if not v > 4.0}
        assert not bad, f"defect {d} stays within 4 bounds in {bad}"
    # N(0, 1): the reference never moves, so the defects of the rescale code change nothing at all
    for shape in dict.fromkeys(s for s, _, _, _ in CASES):
        for dtype in DTYPES:
            for fold in ((False, True) if shape[4] else (False,)):
                s = Set(shape, "n1", "plain", None, dtype, fold, False)
                res = s.run()
                for d in ("acc", "tot"):
                    assert s.ratio(s.run(defect=d, at_tile=res[4] if d == "acc" else res[3])[0]) < 1.0, (LC.sid(shape), d)
