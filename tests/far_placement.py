"""Where the tensors of one kernel call go inside ONE large allocation so that a 32-bit offset bug reads or writes the wrong bytes
INSIDE that allocation - a mismatch, never a memory fault.  Pure Python and numpy: nothing of the GPU, no allocation.

A tensor is ``(name, shape, strides)`` in elements, optionally followed by its element size in bytes (default: the call's) and
by ``(other name, element offset)`` to pin its base that far behind another tensor's (column ranges of the same wide rows).
Its last axis has stride 1: one index of the leading axes is a RUN of ``shape[-1]`` contiguous elements (a token row of all heads).

THE RULE.  Take every run of every tensor and every element offset ``p`` a correct kernel may form on the way to it from the view's
base: each of the batch / reference / row terms ``index * stride`` and every sum of them (the in-run offset up to the run's last
element included).  Take each of four truncations of ``p``:

    p mod 2^32          p as a signed 32-bit value          (p * size) mod 2^32 bytes          (p * size) as signed 32 bits

A kernel that truncates ``p`` lands ``p - trunc(p)`` short of the run.  Either that is 0 (the truncation is harmless here), or the
whole run's image at the wrong place lies inside ``[0, allocation)`` and touches NO run of any tensor of the call, inputs and
outputs alike.  A wrapped read then returns fill pattern (NaN) and a wrapped write lands on fill pattern that the scan sees.

WHAT THE RULE DOES NOT COVER.  It is about truncated OFFSETS.  A kernel that truncates a STRIDE (or twice the stride, in bytes) and
multiplies by the index afterwards, ``(int)(stride * 2) * n``, falls short by ``n`` times the stride's own shortfall - 2^33 bytes
for a stride of 2^30 + d elements at ``n = 2`` - and nothing here proves that such an image stays inside the allocation.  Not every
32-bit bug is fault-free under these placements; the ones that truncate a formed offset are.

:func:`violations` checks the rule for given bases; :func:`place` searches bases that satisfy it and returns, per tensor, the
base and the absolute offset of every run."""
import itertools

import numpy as np

FILL16 = 0x7FC0                      # NaN in fp16 and in bf16
ANCHORS = (0, 1 << 32, 1 << 31, 3 << 31, 1 << 30, 3 << 30, 5 << 30, 7 << 30)    # byte offsets a base search starts from


def _spec(t, elem_size):
    name, shape, strides = t[0], tuple(int(x) for x in t[1]), tuple(int(x) for x in t[2])
    size, rel = elem_size, None
    for extra in t[3:]:
        if isinstance(extra, tuple):
            rel = extra
        elif extra is not None:
            size = int(extra)
    assert len(shape) == len(strides) >= 1 and strides[-1] == 1 and all(s >= 0 for s in strides) and all(n >= 1 for n in shape), t
    return name, shape, strides, size, rel


def run_offsets(shape, strides):
    """element offset of every run from the view's base, shape ``shape[:-1]``"""
    o = np.zeros(shape[:-1], dtype=np.int64)
    for ax, (n, s) in enumerate(zip(shape[:-1], strides[:-1])):
        idx = np.arange(n, dtype=np.int64) * s
        o = o + idx.reshape([-1 if a == ax else 1 for a in range(len(shape) - 1)])
    return o


def _s32(x):
    return ((x + (1 << 31)) % (1 << 32)) - (1 << 31)


def truncation_shortfalls(p, size):
    """bytes by which each of the four truncations of the element offsets ``p`` falls short of ``p`` (0: harmless), stacked"""
    pb = p * size
    return np.stack([(p - p % (1 << 32)) * size, (p - _s32(p)) * size, pb - pb % (1 << 32), pb - _s32(pb)])


def _images(shape, strides, size):
    """(byte offsets of the runs from the base, byte offsets of every wrong image of a run from the base), both flat"""
    lead, width = shape[:-1], shape[-1]
    axes = [np.arange(n, dtype=np.int64) * s for n, s in zip(lead, strides[:-1])]
    grid = np.meshgrid(*axes, indexing="ij") if axes else []
    terms = [g.reshape(-1) for g in grid]
    full = sum(terms) if terms else np.zeros(1, dtype=np.int64)
    wrong = []
    for mask in itertools.product((0, 1), repeat=len(terms)):
        part = sum((t for t, m in zip(terms, mask) if m), np.zeros_like(full))
        for p in (part, part + (width - 1)):
            short = truncation_shortfalls(p, size)
            for row in short:
                hit = row != 0
                if hit.any():
                    wrong.append(full[hit] * size - row[hit])
    wrong = np.unique(np.concatenate(wrong)) if wrong else np.zeros(0, dtype=np.int64)
    return full * size, wrong


def _merge(starts, width):
    """sorted disjoint intervals covering ``[s, s + width)`` for every start"""
    if len(starts) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    s = np.sort(starts)
    e = s + width
    cut = np.ones(len(s), dtype=bool)
    cut[1:] = s[1:] > np.maximum.accumulate(e)[:-1]
    first = np.flatnonzero(cut)
    return s[first], np.maximum.reduceat(e, first)


def _union(parts):
    parts = [p for p in parts if len(p[0])]
    if not parts:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    s = np.concatenate([p[0] for p in parts])
    e = np.concatenate([p[1] for p in parts])
    order = np.argsort(s, kind="stable")
    s, e = s[order], e[order]
    cut = np.ones(len(s), dtype=bool)
    cut[1:] = s[1:] > np.maximum.accumulate(e)[:-1]
    first = np.flatnonzero(cut)
    return s[first], np.maximum.reduceat(e, first)


def _touch(a, b):
    """indices of the intervals of ``a`` that overlap some interval of ``b`` (both sorted and disjoint)"""
    if len(a[0]) == 0 or len(b[0]) == 0:
        return np.zeros(0, dtype=np.int64)
    i = np.searchsorted(b[0], a[1], side="left") - 1          # the last interval of b that starts before this one ends
    return np.flatnonzero((i >= 0) & (b[1][np.maximum(i, 0)] > a[0]))


def _layout(spec, base_bytes):
    """(the byte intervals the tensor occupies at this base, the byte intervals of every wrong image of one of its runs)"""
    name, shape, strides, size, _ = spec
    runs, wrong = _images(shape, strides, size)
    w = shape[-1] * size
    legit = _merge(runs + base_bytes, w)
    images = _merge(wrong + base_bytes, w)
    return legit, images


def violations(alloc_bytes, elem_size, tensors, bases):
    """the rule's violations as a list of sentences (empty: the placement keeps every truncated access inside the allocation
    and off every tensor of the call).  ``bases``: ``{name: base in elements of that tensor}``."""
    specs = [_spec(t, elem_size) for t in tensors]
    lay = {}
    out = []
    for sp in specs:
        b = int(bases[sp[0]]) * sp[3]
        if b % 16:
            out.append(f"{sp[0]}: base byte {b} is not 16-byte aligned")
        lay[sp[0]] = _layout(sp, b)
    legit_all = _union([lay[sp[0]][0] for sp in specs])
    names = [sp[0] for sp in specs]
    for i, a in enumerate(names):
        la = lay[a][0]
        if la[0][0] < 0 or la[1][-1] > alloc_bytes:
            out.append(f"{a}: occupies bytes [{la[0][0]}, {la[1][-1]}) outside the allocation of {alloc_bytes}")
        for b in names[i + 1:]:
            if len(_touch(la, lay[b][0])):
                out.append(f"{a} overlaps {b}")
        im = lay[a][1]
        if len(im[0]):
            if im[0][0] < 0 or im[1][-1] > alloc_bytes:
                out.append(f"{a}: a truncated offset leaves the allocation (image bytes [{im[0][0]}, {im[1][-1]}) of {alloc_bytes})")
            hit = _touch(im, legit_all)
            if len(hit):
                out.append(f"{a}: a truncated offset lands in a legitimate region (image at byte {im[0][hit[0]]})")
    return out


class Placed:
    """one tensor's place: ``base`` (elements from the allocation's start), ``entries`` (absolute element offset of every run,
    shape ``shape[:-1]``), and what :func:`torch.as_strided` needs"""

    def __init__(self, spec, base):
        self.name, self.shape, self.strides, self.elem_size, _ = spec
        self.base = int(base)
        self.entries = run_offsets(self.shape, self.strides) + self.base


def place(alloc_bytes, elem_size, tensors, step_bytes=1 << 16, tries=4096):
    """bases that satisfy the rule: ``{name: Placed}``.  Tensors are taken in order; each (with the tensors pinned to it) gets
    the first base ``anchor + cursor`` that keeps it inside the allocation, off everything placed so far and off every wrong
    image, its own included.  Raises ``ValueError`` when the strides admit no such base."""
    specs = [_spec(t, elem_size) for t in tensors]
    groups = []
    for sp in specs:
        if sp[4] is None:
            groups.append([sp])
        else:
            next(g for g in groups if any(m[0] == sp[4][0] for m in g)).append(sp)
    legit_all = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    image_all = legit_all
    bases, cursor = {}, 0
    for group in groups:
        rel0 = []                                     # each member's (spec, runs, images) relative to the leader's base byte 0
        local = {group[0][0]: 0}
        for sp in group:
            if sp[4] is not None:
                local[sp[0]] = local[sp[4][0]] + sp[4][1] * sp[3]
            legit, images = _layout(sp, local[sp[0]])
            rel0.append((sp, legit, images))
        g_legit = _union([r[1] for r in rel0])
        g_image = _union([r[2] for r in rel0])
        if len(_touch(g_image, g_legit)):
            raise ValueError(f"{group[0][0]}: a truncated offset lands on the tensor itself whatever its base (strides {group[0][2]})")
        lo = min(g_legit[0][0], g_image[0][0] if len(g_image[0]) else 0)
        hi = max(g_legit[1][-1], g_image[1][-1] if len(g_image[0]) else 0)
        found = None
        for k in range(tries):
            for anchor in ANCHORS:
                b = anchor + cursor + k * step_bytes
                if b + lo < 0 or b + hi > alloc_bytes:
                    continue
                gl, gi = (g_legit[0] + b, g_legit[1] + b), (g_image[0] + b, g_image[1] + b)
                if len(_touch(gl, legit_all)) or len(_touch(gl, image_all)) or len(_touch(gi, legit_all)):
                    continue
                found = b
                break
            if found is not None:
                cursor += k * step_bytes
                break
        if found is None:
            raise ValueError(f"{group[0][0]}: no base inside {alloc_bytes} bytes satisfies the rule (strides {group[0][2]})")
        legit_all = _union([legit_all, (g_legit[0] + found, g_legit[1] + found)])
        image_all = _union([image_all, (g_image[0] + found, g_image[1] + found)])
        for sp, _, _ in rel0:
            bb = found + local[sp[0]]
            assert bb % sp[3] == 0
            bases[sp[0]] = bb // sp[3]
        extent = int(min(g_legit[1][-1], 1 << 26))
        cursor += (extent + 8191) // 4096 * 4096
    bad = violations(alloc_bytes, elem_size, tensors, bases)
    if bad:
        raise ValueError("; ".join(bad))
    return {sp[0]: Placed(sp, bases[sp[0]]) for sp in specs}
