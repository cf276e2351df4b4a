"""Per-identity cache of harvested reference K/V.

The reference recomputes the K/V of the reference faces for every restored frame
(``Pix2Pix_Turbo.forward`` -> ``get_conditioning_keys_values``, pix2pix_turbo.py:297-298): N of
the N+1 UNet forwards, N of the N+1 VAE encodes and an unused VAE decode (:277-279) per frame,
although the references of one identity never change.  This cache keeps, per identity, the nine
``(1, N, L, C)`` key tensors and nine value tensors produced by
:func:`instantrestore_amd.kv_harvest.get_conditioning_keys_values`; a batch is assembled by
concatenation along the identity axis (one copy of the cached tensors per batch, instead of N UNet
forwards per identity).  Behaviour-preserving for inference callers: the K/V handed to the main
UNet are the same tensors the reference would have recomputed (up to the reference's own RNG:
``randn_like`` noise at t=1, pix2pix_turbo.py:248 - caching freezes one draw).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Hashable, List, Sequence, Tuple

import torch

KV = Tuple[List[torch.Tensor], ...]   # (keys, values) or (keys, values, stats): stats[l] = (mean, std) fp32 (1, N, H, 64)


class _TableList(list):
    """the key tables of one :meth:`ReferenceKVCache.assemble_tables` set; also holds what ``refill_tables`` rewrites - the set's
    one pointer block (``buf``), its pinned staging tensor and the valid counts"""


class ReferenceKVCache:
    def __init__(self, max_identities: int = 64):
        if max_identities < 1:
            raise ValueError("max_identities must be >= 1")
        self.max_identities = max_identities
        self._store: "OrderedDict[Hashable, KV]" = OrderedDict()
        self._lens = {}   # identity -> per-layer token counts of its references (set_ref_lens); absent: every reference is full
        self.hits = 0
        self.misses = 0

    def __len__(self) -> int:
        return len(self._store)

    def __contains__(self, identity: Hashable) -> bool:
        return identity in self._store

    def get_or_compute(self, identity: Hashable, compute: Callable[[], KV]) -> KV:
        """``compute()`` must return ``(keys, values)`` for ONE identity: lists of ``(1, N, L, C)`` - or ``(keys, values,
        stats)`` as ``get_conditioning_keys_values(..., with_stats=True)`` does: the AdaIN content statistics of the reference
        V's (``(mean, std)`` per layer, fp32 ``(1, N, H, 64)``) are constant per identity too and are cached with them."""
        if identity in self._store:
            self._store.move_to_end(identity)
            self.hits += 1
            return self._store[identity]
        self.misses += 1
        res = compute()
        if not isinstance(res, (tuple, list)) or len(res) not in (2, 3):
            # harvest_reference_kv(with_events=True) returns (keys, values, events[, stats]): events are not cacheable and
            # must not be mistaken for statistics - accept the two documented forms only
            raise ValueError("compute() must return (keys, values) or (keys, values, stats); harvest with with_events=False")
        keys, values = res[0], res[1]
        stats = res[2] if len(res) > 2 else None
        if stats is not None:      # statistics still in the GEMM-partials form (ops.RefStatsPartials): a cache entry holds them finished
            stats = [st.finished() if hasattr(st, "finished") else st for st in stats]
        if len(keys) != len(values) or any(k.shape[0] != 1 or k.shape != v.shape for k, v in zip(keys, values)):
            raise ValueError("compute() must return matching lists of (1, N, L, C) tensors")
        if stats is not None:
            def _is_stat(st):
                return st is None or (isinstance(st, (tuple, list)) and len(st) == 2 and
                                      all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] == 1 for t in st))
            if len(stats) != len(keys) or not all(_is_stat(st) for st in stats):
                raise ValueError("stats must be a per-layer list of None or (mean, std) fp32 tensors of shape (1, N, H, 64)")
        # compact copies: the harvested tensors are strided views of the capture layers' fused (B*N, L, 3C) projection
        # output - caching the views would pin that whole buffer (dead Q third, every other identity of the batch) per
        # entry and eviction would free nothing.  One entry = 2 * 9 layers * N * L * C * 2 bytes.
        entry = ([k.detach().clone(memory_format=torch.contiguous_format) for k in keys],
                 [v.detach().clone(memory_format=torch.contiguous_format) for v in values])
        if stats is not None:
            entry = entry + ([None if st is None else (st[0].detach().clone(), st[1].detach().clone()) for st in stats],)
        self._store[identity] = entry
        self._lens.pop(identity, None)   # a recomputed entry is full again
        while len(self._store) > self.max_identities:
            self._lens.pop(self._store.popitem(last=False)[0], None)
        return entry

    def set_ref_lens(self, identity: Hashable, ref_lens) -> None:
        """per-layer token counts of a cached identity's references: a list with, per layer, ``N`` integers (or an int tensor of ``N``
        elements, e.g. a row of ``ops.compact_refs``' counts - read back once, here) or ``None`` for a layer whose references are
        full.  The entry's tensors keep their shape: the token axis is the capacity, the kept rows lie in front.  ``None`` drops
        the counts.  :meth:`assemble_tables` hands them to the attention call as ``ref_lens``."""
        entry = self._store[identity]
        if ref_lens is None:
            self._lens.pop(identity, None)
            return
        if len(ref_lens) != len(entry[0]):
            raise ValueError(f"set_ref_lens(): {len(entry[0])} layers are cached, got counts for {len(ref_lens)}")
        rows = []
        for l, c in enumerate(ref_lens):
            n, cap = int(entry[0][l].shape[1]), int(entry[0][l].shape[2])
            if c is None:
                rows.append([cap] * n)
                continue
            c = [int(x) for x in (c.reshape(-1).tolist() if isinstance(c, torch.Tensor) else c)]
            if len(c) != n or any(x < 0 or x > cap for x in c):
                raise ValueError(f"set_ref_lens(): layer {l} needs {n} counts in [0, {cap}], got {c}")
            rows.append(c)
        self._lens[identity] = rows

    def set_ref_stats(self, identity: Hashable, stats) -> None:
        """replace the AdaIN content statistics of a cached identity: a per-layer list of ``(mean, std)`` fp32 ``(1, N, H, 64)``
        pairs (or ``None`` for a layer without).  For statistics taken with other weights than the capture's - after
        ``ops.compact_refs`` the kept-token statistics are ``ops.token_stats_weighted(packed_v, heads=H, lens=lens)`` - which
        :meth:`assemble` / :meth:`assemble_tables` / :meth:`refill_tables` then carry as they carry any others.  The pairs are
        cloned; an entry cached without statistics gains them."""
        entry = self._store[identity]
        if len(stats) != len(entry[0]):
            raise ValueError(f"set_ref_stats(): {len(entry[0])} layers are cached, got statistics for {len(stats)}")
        new = []
        for l, st in enumerate(stats):
            if st is None:
                new.append(None)
                continue
            n, heads = int(entry[1][l].shape[1]), int(entry[1][l].shape[3]) // 64
            if not (isinstance(st, (tuple, list)) and len(st) == 2 and
                    all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == (1, n, heads, 64) for t in st)):
                raise ValueError(f"set_ref_stats(): layer {l} needs a (mean, std) pair of fp32 (1, {n}, {heads}, 64) tensors")
            new.append((st[0].detach().clone(), st[1].detach().clone()))
        self._store[identity] = (entry[0], entry[1], new)

    def _count_rows(self, identities, entries, counts, n_refs: int):
        """host side of the per-layer ``(B, N)`` counts: an identity's own counts, the capacity for one without, 0 for a slot it does
        not have"""
        out = []
        for l in range(len(entries[0][0])):
            cap = int(entries[0][0][l].shape[2])
            out.append([(self._lens[i][l] if i in self._lens else [cap] * c) + [0] * (n_refs - c) for i, c in zip(identities, counts)])
        return out

    def assemble(self, identities: Sequence[Hashable]) -> KV:
        """``(B, N, L, C)`` lists for a batch of cached identities (raises KeyError on a miss)."""
        entries = [self._store[i] for i in identities]
        for i in identities:
            self._store.move_to_end(i)
        n_layers = len(entries[0][0])
        keys = [torch.cat([e[0][l] for e in entries], dim=0) for l in range(n_layers)]
        values = [torch.cat([e[1][l] for e in entries], dim=0) for l in range(n_layers)]
        with_stats = [len(e) > 2 for e in entries]
        if any(with_stats) and not all(with_stats):
            raise ValueError("assemble(): some of these identities were cached with AdaIN content statistics and some without; "
                             "cache them the same way (the statistics would otherwise be dropped silently)")
        if all(with_stats):
            stats = [None if any(e[2][l] is None for e in entries) else
                     (torch.cat([e[2][l][0] for e in entries], dim=0), torch.cat([e[2][l][1] for e in entries], dim=0))
                     for l in range(n_layers)]
            return keys, values, stats
        return keys, values

    def _table_plan(self, identities: Sequence[Hashable], n_max: int = 0):
        """host side of :meth:`assemble_tables` / :meth:`refill_tables`: the entries (LRU order touched as :meth:`assemble`
        touches it), every identity's reference count, N and whether the identities carry statistics"""
        entries = [self._store[i] for i in identities]
        for i in identities:
            self._store.move_to_end(i)
        counts = [int(e[0][0].shape[1]) for e in entries]
        with_stats = [len(e) > 2 for e in entries]
        if any(with_stats) and not all(with_stats):
            raise ValueError("assemble_tables(): some of these identities were cached with AdaIN content statistics and some without; "
                             "cache them the same way (the statistics would otherwise be dropped silently)")
        return entries, counts, max(max(counts), n_max), all(with_stats)

    @staticmethod
    def _table_words(entries, counts, n_refs: int, lens_rows):
        """the int64 words of one table set: 2 * layers * B * N addresses (keys of every layer, then values; an unused slot points
        at its identity's reference 0), then the B valid counts packed as int32 pairs, then the layers * B * N per-reference token
        counts (``lens_rows``: :meth:`_count_rows`) packed the same way"""
        n_layers = len(entries[0][0])
        words = []
        for side in (0, 1):
            for l in range(n_layers):
                for e, c in zip(entries, counts):
                    t = e[side][l]
                    if t.data_ptr() % 16 or t.stride(-1) != 1 or t.stride(2) % 8 or (t.stride(1) * t.element_size()) % 16:
                        raise ValueError("assemble_tables(): a cached entry is not 16-byte aligned")
                    words += [t[0, n if n < c else 0].data_ptr() for n in range(n_refs)]
        valid = counts + [0] * (len(counts) % 2)
        words += [valid[i] | (valid[i + 1] << 32) for i in range(0, len(valid), 2)]     # little-endian int32 pairs
        flat = [c for layer in lens_rows for row in layer for c in row]
        flat += [0] * (len(flat) % 2)
        words += [flat[i] | (flat[i + 1] << 32) for i in range(0, len(flat), 2)]
        return words

    @staticmethod
    def _table_stats(entries, counts, n_refs: int, l: int):
        """layer l's content statistics (B, N, H, 64): concatenated; an unused slot gets (0, 0), what the harvest writes for a
        zero-filled reference"""
        if any(e[2][l] is None for e in entries):
            return None
        def pad(t, c):
            return t if c == n_refs else torch.cat([t, t.new_zeros((1, n_refs - c) + tuple(t.shape[2:]))], dim=1)
        return (torch.cat([pad(e[2][l][0], c) for e, c in zip(entries, counts)], dim=0),
                torch.cat([pad(e[2][l][1], c) for e, c in zip(entries, counts)], dim=0))

    def assemble_tables(self, identities: Sequence[Hashable]):
        """:meth:`assemble` without the copy: per layer an :class:`instantrestore_amd.ops.RefKVTable` of pointers INTO the cached
        entries instead of a dense ``(B, N, L, C)`` tensor.  Nothing of K/V size is allocated or moved: the pointer arrays of all
        layers (keys and values), the valid counts and the per-reference token counts live in one int64 device tensor filled by one host-to-device copy, and each
        table keeps the entries it points into alive (an evicted or invalidated identity stays readable while a table holds it).

        Identities cached with different numbers of references may share a batch: ``N`` is the largest count, unused slots point at
        their identity's reference 0 and carry content statistics (0, 0), and ``valid`` says how many references each identity has.

        Returns ``(keys, values, stats, valid)``: ``stats`` as :meth:`assemble` returns them (``None`` when the identities were
        cached without), ``valid`` an int32 ``(B,)`` device tensor to hand over as ``ref_valid`` when the counts differ, ``None``
        when every identity has ``N`` references (the call then is the dense call's, kernel for kernel).

        Per-reference token counts ride beside the tables: ``keys.ref_lens`` is a list with one int32 ``(B, N)`` device tensor per
        layer - an identity's :meth:`set_ref_lens` counts, ``len_ref`` for an identity without, 0 for a slot it does not have -
        to hand over as ``ref_lens`` INSTEAD of ``ref_valid`` (a missing slot is then absent, not zero-filled; without ``ref_lens``
        those slots keep the meaning they have today).  They are views into the set's one pointer block: no copy of their own, and
        :meth:`refill_tables` refills them in place with the same upload.  Counts given to :meth:`set_ref_lens` AFTER this call reach
        the device with the next :meth:`refill_tables`, not before.  The list hangs on the returned key list: hand ``keys`` itself (not
        ``list(keys)``) to :meth:`refill_tables`."""
        from .ops import RefKVTable, _PinnedStage

        entries, counts, n_refs, with_stats = self._table_plan(identities)
        n_layers, B = len(entries[0][0]), len(entries)
        words = self._table_words(entries, counts, n_refs, self._count_rows(identities, entries, counts, n_refs))
        first = entries[0][0][0]
        buf = torch.empty(len(words), dtype=torch.int64, device=first.device)
        if first.is_cuda:
            stage = _PinnedStage(len(words))
            with torch.cuda.device(first.device):
                stage.upload(words, buf)
        else:
            stage = None
            buf.copy_(torch.tensor(words, dtype=torch.int64))
        ptrs = buf[:2 * n_layers * B * n_refs].view(2, n_layers, B, n_refs)
        tables = []
        for side in (0, 1):
            tables.append([RefKVTable(ptrs[side, l], e0.shape[2], e0.shape[3], e0.stride(2), e0.dtype, [e[side][l] for e in entries])
                           for l, e0 in enumerate(entries[0][side])])
            for l, t in enumerate(tables[-1]):
                if any(e[side][l].shape[2:] != entries[0][side][l].shape[2:] or e[side][l].dtype != t.dtype or
                       e[side][l].stride(2) != t.row_stride for e in entries):
                    raise ValueError("assemble_tables(): the identities' cached tensors differ in length, width, dtype or row stride")
        valid_all = buf[2 * n_layers * B * n_refs:].view(torch.int32)[:B]
        stats = [self._table_stats(entries, counts, n_refs, l) for l in range(n_layers)] if with_stats else None
        keys = _TableList(tables[0])
        keys.buf, keys.stage, keys.valid_all = buf, stage, valid_all
        n_ptr, n_valid = 2 * n_layers * B * n_refs, (B + 1) // 2
        lens = buf[n_ptr + n_valid:].view(torch.int32)[:n_layers * B * n_refs].view(n_layers, B, n_refs)   # views: the block's one upload fills them
        keys.ref_lens = [lens[l] for l in range(n_layers)]
        return keys, tables[1], stats, (valid_all if min(counts) < n_refs else None)

    def refill_tables(self, tables, identities: Sequence[Hashable]) -> None:
        """point the set returned by :meth:`assemble_tables` at other identities IN PLACE - pointer arrays, valid counts and
        statistics keep their addresses, so a captured step that reads them serves the new identities on its next replay.  One
        host-to-device copy of the pointer block - addresses, valid counts and the per-reference token counts of ``keys.ref_lens``
        (the identities' :meth:`set_ref_lens` counts as they are now) - plus the statistics' few KB.  Same batch size; no identity may have more
        references than the set's N, and a set assembled without ``valid`` takes identities of exactly N references only."""
        keys, values, stats, valid = tables
        n_layers, (B, n_refs) = len(keys), keys[0].shape[:2]
        entries, counts, n_now, with_stats = self._table_plan(identities, n_refs)
        if len(entries) != B or n_now != n_refs or len(entries[0][0]) != n_layers:
            raise ValueError(f"refill_tables(): the set holds {B} identities of up to {n_refs} references in {n_layers} layers")
        if valid is None and min(counts) < n_refs:
            raise ValueError("refill_tables(): this set was assembled without valid counts (every identity had N references); "
                             "assemble a new one for identities with fewer")
        if with_stats != (stats is not None):
            raise ValueError("refill_tables(): the set and the identities differ in whether they carry AdaIN content statistics")
        if not isinstance(keys, _TableList) or not hasattr(keys, "ref_lens"):
            raise ValueError("refill_tables(): pass the key list assemble_tables() returned itself (it carries the set's pointer block and counts)")
        words = self._table_words(entries, counts, n_refs, self._count_rows(identities, entries, counts, n_refs))
        if keys.stage is not None:
            with torch.cuda.device(keys.buf.device):
                keys.stage.upload(words, keys.buf)
        else:
            keys.buf.copy_(torch.tensor(words, dtype=torch.int64))
        for side, tabs in ((0, keys), (1, values)):
            for l, t in enumerate(tabs):
                t.tensors = [e[side][l] for e in entries]
        if stats is not None:
            for l, st in enumerate(stats):
                new = self._table_stats(entries, counts, n_refs, l)
                if (st is None) != (new is None):
                    raise ValueError("refill_tables(): layer %d: statistics present on one side only" % l)
                if st is not None:
                    st[0].copy_(new[0])
                    st[1].copy_(new[1])

    def nbytes(self, identity: Hashable) -> int:
        """device bytes held for one cached identity"""
        e = self._store[identity]
        extra = [t for st in (e[2] if len(e) > 2 else []) if st is not None for t in st]
        return sum(t.untyped_storage().nbytes() for t in e[0] + e[1] + extra)

    def invalidate(self, identity: Hashable = None) -> None:
        if identity is None:
            self._store.clear()
            self._lens.clear()
        else:
            self._store.pop(identity, None)
            self._lens.pop(identity, None)
