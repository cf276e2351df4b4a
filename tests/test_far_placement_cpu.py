"""The placement rule of tests/far_placement.py, proved for every layout tests/test_gpu_far_addresses.py runs - by enumerating
offsets, without an allocation and without a GPU.  This is what makes a 32-bit offset bug in a kernel show up in that module
as a mismatch and never as a memory fault: every truncated offset a kernel could form lands inside the one allocation and on
none of the call's tensors."""
import bisect
import itertools

import numpy as np
import pytest

import far_placement as FP
import test_gpu_far_addresses as G

ALLOC = G.ALLOC_BYTES
KEYS = sorted(G.LAYOUTS)


def test_the_allocation_is_at_most_eight_and_a_half_gib():
    assert ALLOC <= 17 << 29 and ALLOC % 16 == 0


@pytest.mark.parametrize("key", KEYS)
def test_every_layout_of_the_gpu_module_satisfies_the_rule(key):
    layout = G.LAYOUTS[key]
    placed = FP.place(ALLOC, 2, layout)
    assert set(placed) == {t[0] for t in layout}
    bases = {n: p.base for n, p in placed.items()}
    assert FP.violations(ALLOC, 2, layout, bases) == []
    for p in placed.values():          # what the GPU module hands to as_strided: every run inside the allocation
        assert p.entries.shape == p.shape[:-1]
        assert int(p.entries.min()) >= 0 and (int(p.entries.max()) + p.shape[-1]) * p.elem_size <= ALLOC
        assert (p.base * p.elem_size) % 16 == 0
    again = FP.place(ALLOC, 2, layout)  # the GPU test places the layout anew: the same bases
    assert {n: p.base for n, p in again.items()} == bases


def _naive_violations(alloc, layout, bases):
    """the rule once more in plain loops, sharing nothing with far_placement but the specification"""
    specs = []
    for t in layout:
        size = next((e for e in t[3:] if isinstance(e, int)), 2)
        specs.append((t[0], t[1], t[2], size))
    legit = []
    for name, shape, strides, size in specs:
        for idx in itertools.product(*(range(n) for n in shape[:-1])):
            o = sum(i * s for i, s in zip(idx, strides))
            legit.append(((bases[name] + o) * size, (bases[name] + o + shape[-1]) * size))
    legit.sort()
    starts = [a for a, _ in legit]
    bad = [("", (), "tensor outside") for a, b in legit if a < 0 or b > alloc]
    s32 = lambda x: (x + 2 ** 31) % 2 ** 32 - 2 ** 31
    for name, shape, strides, size in specs:
        width = shape[-1] * size
        for idx in itertools.product(*(range(n) for n in shape[:-1])):
            terms = [i * s for i, s in zip(idx, strides)]
            at = (bases[name] + sum(terms)) * size
            for mask in itertools.product((0, 1), repeat=len(terms)):
                part = sum(t for t, m in zip(terms, mask) if m)
                for p in (part, part + shape[-1] - 1):
                    for got in (p % 2 ** 32 * size, s32(p) * size, p * size % 2 ** 32, s32(p * size)):
                        short = p * size - got
                        if short == 0:
                            continue
                        lo, hi = at - short, at - short + width
                        if lo < 0 or hi > alloc:
                            bad.append((name, idx, "outside"))
                            continue
                        i = bisect.bisect_left(starts, hi) - 1
                        if i >= 0 and legit[i][1] > lo:
                            bad.append((name, idx, "legit"))
    return bad


SMALL = [k for k in KEYS if k.startswith(("fwd/pipe32_default/", "fwd/w128/all", "fwd_variant/w64x8_ragged/out_f32", "readout_long/", "linear/stats",
                                          "linear/skinny_k320/", "linear_mid/256x256/", "linear_mid/skinny_k320/f32", "adain/zero_invalid_refs/", "adain/adain_stats/", "tensor2im/", "freeu/"))]


@pytest.mark.parametrize("key", SMALL)
def test_plain_loops_agree_with_the_vectorised_check(key):
    layout = G.LAYOUTS[key]
    bases = {n: p.base for n, p in FP.place(ALLOC, 2, layout).items()}
    assert _naive_violations(ALLOC, layout, bases) == []


@pytest.mark.parametrize("kind,hits", [("A", (True, True, True, True)), ("B", (False, True, True, True)), ("C", (False, True, True, True))])
def test_each_far_stride_defeats_the_truncations_it_is_there_for(kind, hits):
    """A wraps every truncation; B and C leave ``p mod 2^32`` alone (no offset reaches 2^32 elements).  B sends the signed element
    offset negative (its byte offset wraps positive), C the signed byte offset of entry 1 and the signed element offset of entry 2"""
    count = 3 if kind == "C" else 2
    p = np.arange(count, dtype=np.int64) * G.FAR[kind]
    short = FP.truncation_shortfalls(p, 2)
    assert tuple(bool(row.any()) for row in short) == hits
    if kind != "A":
        assert (p - short[1] // 2 < 0).any()
    if kind == "C":
        assert p[1] * 2 - short[3][1] < 0 <= p[1] - short[1][1] // 2 and p[2] - short[1][2] // 2 < 0


def test_layouts_use_the_far_strides():
    for key in KEYS:
        if key.startswith(("fwd/", "readout/")) and not key.startswith("fwd_long"):
            strides = [s for t in G.LAYOUTS[key] for s in t[2]]
            assert max(strides) * 2 >= 1 << 31, key


NEGATIVE = [
    # (what, shape, strides, base, sentence the check must produce)
    ("A: a remainder smaller than the entry", (2, 200, 128), ((1 << 32) + 4096, 128, 1), 0, "lands in a legitimate region"),
    ("A: base too high for the second entry", (2, 200, 128), ((1 << 32) + G.D, 128, 1), 1 << 31, "outside the allocation"),
    ("B: base 0, the signed truncation goes below the allocation", (2, 200, 128), ((1 << 31) + G.D, 128, 1), 0, "leaves the allocation"),
    ("B: a remainder smaller than the entry", (2, 200, 128), ((1 << 31) + 4096, 128, 1), 1 << 31, "lands in a legitimate region"),
    ("B: base below 2^31 - remainder", (2, 200, 128), ((1 << 31) + G.D, 128, 1), (1 << 31) - 2 * G.D, "leaves the allocation"),
    ("C: three entries from base 0", (3, 72, 128), ((1 << 30) + G.D, 128, 1), 0, "leaves the allocation"),
    ("rows: a stride that divides 2^31 puts the wrapped row on a real one", (2, 300, 128), (128, (1 << 31) // 256, 1), 1 << 31,
     "lands in a legitimate region"),
    ("a base that is not 16-byte aligned", (2, 8, 128), ((1 << 32) + G.D, 128, 1), 4, "not 16-byte aligned"),
]


@pytest.mark.parametrize("case", NEGATIVE, ids=[c[0] for c in NEGATIVE])
def test_a_placement_that_breaks_the_rule_is_reported(case):
    what, shape, strides, base, sentence = case
    layout = [("t", shape, strides)]
    bad = FP.violations(ALLOC, 2, layout, {"t": base})
    assert any(sentence in b for b in bad), (what, bad)
    assert _naive_violations(ALLOC, layout, {"t": base}) != [] or "aligned" in sentence
    if what.startswith(("A: base", "B: base", "C:")):       # the same strides are fine at the base that place() finds
        good = FP.place(ALLOC, 2, layout)["t"].base
        assert good != base and FP.violations(ALLOC, 2, layout, {"t": good}) == []
    elif "aligned" not in sentence:                         # a remainder or a row stride that no base can mend
        with pytest.raises(ValueError):
            FP.place(ALLOC, 2, layout)


def test_the_two_placements_of_the_issue_hold_for_small_entries():
    """base 0 with entry stride 2^32 + 4096 elements, and base 2^31 with entry stride 2^31 + 4096: fine while an entry spans less
    than 4096 elements, which is why this module's strides add 2^23 instead"""
    small = (2, 8, 128)
    assert FP.violations(ALLOC, 2, [("t", small, ((1 << 32) + 4096, 128, 1))], {"t": 0}) == []
    assert FP.violations(ALLOC, 2, [("t", small, ((1 << 31) + 4096, 128, 1))], {"t": 1 << 31}) == []
    assert FP.place(ALLOC, 2, [("t", small, ((1 << 32) + 4096, 128, 1))])["t"].base == 0
    assert FP.place(ALLOC, 2, [("t", small, ((1 << 31) + 4096, 128, 1))])["t"].base == 1 << 31


def test_place_refuses_strides_that_admit_no_base():
    with pytest.raises(ValueError):
        FP.place(ALLOC, 2, [("t", (3, 8, 128), ((1 << 32) + G.D, 128, 1))])          # the third entry is past any 8.5 GiB
    with pytest.raises(ValueError):
        FP.place(ALLOC, 2, [("t", (2, 300, 128), (128, (1 << 31) // 256, 1))])        # the wrapped row IS another row


def test_two_tensors_never_share_bytes_or_wrong_images():
    layout = [("a", (2, 200, 128), ((1 << 32) + G.D, 128, 1)), ("b", (2, 200, 128), ((1 << 32) + G.D, 128, 1))]
    placed = FP.place(ALLOC, 2, layout)
    assert placed["a"].base != placed["b"].base
    # b where a's truncated second entry lands: reported
    bad = FP.violations(ALLOC, 2, layout, {"a": 0, "b": G.D})
    assert any("a: a truncated offset lands in a legitimate region" in s for s in bad), bad
