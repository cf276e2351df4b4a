"""Tensor-level entry points of the HIP hot path.

Thin, allocation-only wrappers: they check devices / dtypes / strides, allocate outputs with
torch (device memory and streams are PyTorch-ROCm plumbing) and hand raw pointers, element
strides and the current HIP stream to the C ABI (``include/instantrestore_hip.h``).  Nothing
here computes anything, and nothing falls back to torch math: a CPU tensor or a missing
library is an error.

Layouts are the reference's own, consumed IN PLACE (no head-split copies, no ``cat``):
``q, k_self, v_self``: ``(B, L, H*64)``; ``ref_k, ref_v``: ``(B, N, Lr, H*64)`` exactly as
``Pix2Pix_Turbo.get_conditioning_keys_values`` hands them over (pix2pix_turbo.py:265-266).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import collections
import threading
from typing import Optional, Tuple

import torch

from . import _lib

HEAD_DIM = 64
ADAIN_EPS = 1e-5  # attn_processors.py:10,245

_DT = {torch.float16: _lib.IR_DTYPE_F16, torch.bfloat16: _lib.IR_DTYPE_BF16}
# measurement hook (bench.py): (predicate(q, ref_k, adain) -> bool, list collecting (start, end) HIP events recorded
# on the launch stream around the matching ir_shared_attn_fwd calls) or None
EVENT_SINK = None


def _dtype_code(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(
            f"the fused HIP path computes in fp16/bf16 (got {t.dtype}); run the model under "
            "torch.autocast (as face_replace/inference/test.py:83 does) or cast it to bf16/fp16"
        ) from None


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the handle without a torch.cuda.Stream object around it


def _stream() -> int:
    """the calling thread's current HIP stream on the current device, as the integer the C ABI takes.  Through torch's raw
    accessor where this torch has it (what its own compiled kernels use): ``torch.cuda.current_stream()`` builds a Stream object
    per call, ~7 us of the ~30 us a launch costs the host - a fifth of an eager one-identity step (tools/gpu_host_overhead.py)"""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _on_tensor_device(fn):
    """HIP launches go to the calling thread's CURRENT device: make that the device of the tensors
    (so a caller holding cuda:1 tensors while cuda:0 is current gets the right device and stream)."""

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = None
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, (torch.Tensor, RefKVTable)) and a.is_cuda:
                dev = a.device
                break
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)

    return wrapper


def _need_gpu(*ts: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "instantrestore_amd ops run on the MI355X only; got a CPU tensor "
                "(there is no CPU fallback - the CPU restatement lives in oracle/ and is test-only)"
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def _tok(t: torch.Tensor, heads: int, name: str) -> torch.Tensor:
    """(B, L, H*64) view usable in place; falls back to .contiguous() only for exotic strides."""
    if t.dim() != 3 or t.shape[-1] != heads * HEAD_DIM:
        raise ValueError(f"{name}: expected (B, L, {heads * HEAD_DIM}), got {tuple(t.shape)}")
    if t.stride(-1) != 1 or t.stride(0) % 8 or t.stride(1) % 8 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def _ref(t, heads: int, name: str):
    if _is_table(t):      # a pointer table is used as it is (from_tensors checked strides and alignment); never densified
        if t.shape[-1] != heads * HEAD_DIM:
            raise ValueError(f"{name}: expected a table of (L, {heads * HEAD_DIM}) entries, got {tuple(t.shape)}")
        return t
    if t.dim() != 4 or t.shape[-1] != heads * HEAD_DIM:
        raise ValueError(f"{name}: expected (B, N, L, {heads * HEAD_DIM}), got {tuple(t.shape)}")
    if t.stride(-1) != 1 or any(t.stride(i) % 8 for i in range(3)) or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def _grid_pointers(grid, valid=None):
    """``grid`` (B rows of N ``(L, C)`` tensors) -> (B x N addresses, (L, C, row stride, dtype, device), the tensors).  ``None`` is
    allowed only in slots ``n >= valid[b]``; such a slot gets the address of the row's reference 0 (of the grid's first tensor
    when the whole row is empty): a readable address that a call with ``valid_refs`` never uses."""
    rows = [list(r) for r in grid]
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("RefKVTable: grid must be B non-empty rows of N entries each")
    if valid is not None and len(valid) != len(rows):
        raise ValueError(f"RefKVTable: {len(valid)} valid counts for {len(rows)} rows")
    tensors = [t for r in rows for t in r if t is not None]
    if not tensors:
        raise ValueError("RefKVTable: no tensor in the grid")
    first = tensors[0]
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError("RefKVTable: every entry must be an (L, C) tensor with a contiguous channel axis")
        if t.dtype != first.dtype or t.device != first.device:
            raise ValueError(f"RefKVTable: mixed dtype / device ({t.dtype} on {t.device} vs {first.dtype} on {first.device})")
        if t.shape != first.shape:
            raise ValueError(f"RefKVTable: mixed shapes {tuple(t.shape)} vs {tuple(first.shape)} (every entry has the same L and C)")
        if t.stride(0) != first.stride(0):
            raise ValueError(f"RefKVTable: mixed row strides {t.stride(0)} vs {first.stride(0)}")
        if t.stride(0) % 8:
            raise ValueError(f"RefKVTable: row stride {t.stride(0)} is not a multiple of 8 elements")
        if t.data_ptr() % 16:
            raise ValueError(f"RefKVTable: an entry at address {t.data_ptr():#x} is not 16-byte aligned")
    ptrs = []
    for b, r in enumerate(rows):
        nv = len(r) if valid is None else int(valid[b])
        if not 0 <= nv <= len(r):
            raise ValueError(f"RefKVTable: valid count {nv} of row {b} outside [0, {len(r)}]")
        row = []
        for n, t in enumerate(r):
            if t is None:
                if n < nv:
                    raise ValueError(f"RefKVTable: entry [{b}][{n}] is None but row {b} has {nv} valid references")
                t = r[0] if r[0] is not None else first
            row.append(t.data_ptr())
        ptrs.append(row)
    return ptrs, (first.shape[0], first.shape[1], first.stride(0), first.dtype, first.device), tensors


class _PinnedStage:
    """one pinned host tensor that feeds ``copy_(non_blocking=True)`` uploads: before the host rewrites it, the previous upload
    from it has to have run (an event recorded behind that copy; a few KB, long done in practice)"""

    __slots__ = ("host", "event")

    def __init__(self, numel: int):
        self.host = torch.empty(numel, dtype=torch.int64, pin_memory=True)
        self.event = None

    def upload(self, values, dst: torch.Tensor) -> None:
        if self.event is not None:
            self.event.synchronize()
        self.host.copy_(torch.as_tensor(values, dtype=torch.int64).reshape(-1))
        dst.copy_(self.host.view(dst.shape), non_blocking=True)     # on the current stream
        self.event = None
        if not torch.cuda.is_current_stream_capturing():    # (a captured copy re-reads the staging tensor at every replay: fill outside)
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(dst.device))


class RefKVTable:
    """The reference K (or V) of one layer as a TABLE of device pointers instead of one dense ``(B, N, L, C)`` tensor
    (``ir_shared_attn_table_args``): ``ptrs`` is an int64 ``(B, N)`` tensor on the entries' device, ``ptrs[b, n]`` the address of
    the ``(L, C)`` matrix of reference ``n`` of batch entry ``b`` - which may live anywhere (a per-identity cache entry, a slice
    of a pool, the K third of a fused ``(L, 3C)`` projection output), as long as all entries share dtype, ``L``, ``C`` and the row
    stride and are 16-byte aligned.  Nothing of K/V size is allocated or copied.  ``shape`` / ``dtype`` / ``device`` are those of
    the dense tensor it stands for; ``tensors`` keeps the entries alive.

    The kernels read the table when they run: after :meth:`fill_` a replayed graph attends to the new entries."""

    __slots__ = ("ptrs", "shape", "dtype", "device", "row_stride", "tensors", "_stage")

    def __init__(self, ptrs: torch.Tensor, length: int, channels: int, row_stride: int, dtype: torch.dtype, tensors):
        if ptrs.dtype != torch.int64 or ptrs.dim() != 2 or not ptrs.is_contiguous():
            raise ValueError("RefKVTable: ptrs must be a contiguous int64 (B, N) tensor")
        self.ptrs = ptrs
        self.shape = torch.Size((ptrs.shape[0], ptrs.shape[1], int(length), int(channels)))
        self.dtype, self.device, self.row_stride = dtype, ptrs.device, int(row_stride)
        self.tensors = list(tensors)
        self._stage = None

    @classmethod
    def from_tensors(cls, grid, valid=None) -> "RefKVTable":
        """``grid``: ``B`` rows of ``N`` ``(L, C)`` tensors (same device, dtype, L, C and row stride; ``data_ptr() % 16 == 0``).
        ``valid`` (optional, ``B`` counts): slots ``n >= valid[b]`` may be ``None``; pass the same counts to the attention call as
        ``valid_refs``.  One small host-to-device copy on the current stream."""
        ptrs, (length, channels, row_stride, dtype, device), tensors = _grid_pointers(grid, valid)
        host = torch.tensor(ptrs, dtype=torch.int64)
        table = cls(host if device.type == "cpu" else torch.empty(host.shape, dtype=torch.int64, device=device),
                    length, channels, row_stride, dtype, tensors)
        if device.type != "cpu":
            with torch.cuda.device(device):
                table._upload(ptrs)
        return table

    def _upload(self, ptrs) -> None:
        if self._stage is None:
            self._stage = _PinnedStage(self.ptrs.numel())
        self._stage.upload(ptrs, self.ptrs)

    def fill_(self, grid, valid=None) -> "RefKVTable":
        """point the table at other entries of the same geometry, IN PLACE (``ptrs`` keeps its address: a captured graph that
        reads it follows): one pinned staging tensor, one ``copy_(non_blocking=True)`` on the current stream"""
        ptrs, (length, channels, row_stride, dtype, device), tensors = _grid_pointers(grid, valid)
        if (len(ptrs), len(ptrs[0]), length, channels) != tuple(self.shape) or row_stride != self.row_stride or dtype != self.dtype \
                or device != self.device:
            raise ValueError(f"RefKVTable.fill_: the entries do not match the table ({tuple(self.shape)}, row stride {self.row_stride}, "
                             f"{self.dtype} on {self.device})")
        if self.device.type == "cpu":
            self.ptrs.copy_(torch.tensor(ptrs, dtype=torch.int64))
        else:
            with torch.cuda.device(self.device):
                self._upload(ptrs)
        self.tensors = list(tensors)
        return self

    @property
    def is_cuda(self) -> bool:
        return self.device.type == "cuda"

    def dim(self) -> int:
        return 4

    def record_stream(self, stream) -> None:
        self.ptrs.record_stream(stream)
        for t in self.tensors:
            t.record_stream(stream)


def _is_table(t) -> bool:
    return isinstance(t, RefKVTable)


def _nseg(include_self: bool, ref_k) -> int:
    """the K/V segments of a call: ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1``"""
    return (1 if include_self else 0) + (ref_k.shape[1] if ref_k is not None else 0)


def _fill_args(q, k_self, v_self, ref_k, ref_v, heads, scale, include_self, adain, out, lse, split=True,
               q_prescaled=False, valid_refs=None, batch_invariant=False, key_bias=None, ref_lens=None, q_allow=None, key_region=None):
    if ref_lens is not None:   # validated before anything else is touched
        _check_ref_lens(ref_lens, q, ref_k, valid_refs, key_bias)
    regions = q_allow is not None or key_region is not None
    if regions:
        lkv = (k_self.shape[1] if include_self else 0) + (ref_k.shape[1] * ref_k.shape[2] if ref_k is not None else 0)
        _check_regions(q_allow, key_region, q, lkv, key_bias, ref_lens)
    a = _lib.SharedAttnRegionArgs() if regions else _lib.SharedAttnRaggedArgs() if ref_lens is not None else _lib.SharedAttnBiasArgs() if key_bias is not None else _lib.SharedAttnTableArgs() if _is_table(ref_k) else _lib.SharedAttnArgs()
    a.struct_size = C.sizeof(a)
    a.dtype = _dtype_code(q)
    a.flags = (_lib.IR_FLAG_INCLUDE_SELF if include_self else 0) | (_lib.IR_FLAG_Q_PRESCALED if q_prescaled else 0)
    if out is not None and out.dtype == torch.float32:
        a.flags |= _lib.IR_FLAG_OUT_F32
    if batch_invariant:   # ABI v10: the library's batch-invariant plan; the A/B tuning hook does not apply to it
        a.flags |= _lib.IR_FLAG_BATCH_INVARIANT
    a.tuning = 0 if batch_invariant else _TUNING
    a.batch, a.len_q, _ = q.shape
    a.heads = heads
    a.scale = float(scale)
    a.q = q.data_ptr()
    a.q_sb, a.q_sl, a.q_sh = q.stride(0), q.stride(1), HEAD_DIM
    if include_self:
        a.len_self = k_self.shape[1]
        a.k_self, a.v_self = k_self.data_ptr(), v_self.data_ptr()
        a.ks_sb, a.ks_sl, a.ks_sh = k_self.stride(0), k_self.stride(1), HEAD_DIM
        a.vs_sb, a.vs_sl, a.vs_sh = v_self.stride(0), v_self.stride(1), HEAD_DIM
    if _is_table(ref_k):     # ir_shared_attn_table_args: k_ref / v_ref stay NULL, the batch and reference strides 0
        a.n_refs, a.len_ref = ref_k.shape[1], ref_k.shape[2]
        a.k_ref_table, a.v_ref_table = ref_k.ptrs.data_ptr(), ref_v.ptrs.data_ptr()
        a.kr_sl, a.kr_sh, a.vr_sl, a.vr_sh = ref_k.row_stride, HEAD_DIM, ref_v.row_stride, HEAD_DIM
    elif ref_k is not None:
        a.n_refs, a.len_ref = ref_k.shape[1], ref_k.shape[2]
        a.k_ref, a.v_ref = ref_k.data_ptr(), ref_v.data_ptr()
        a.kr_sb, a.kr_sn, a.kr_sl, a.kr_sh = ref_k.stride(0), ref_k.stride(1), ref_k.stride(2), HEAD_DIM
        a.vr_sb, a.vr_sn, a.vr_sl, a.vr_sh = ref_v.stride(0), ref_v.stride(1), ref_v.stride(2), HEAD_DIM
    if adain is not None:
        a.adain_a, a.adain_b = adain[0].data_ptr(), adain[1].data_ptr()
    if key_bias is not None:
        lkv = (k_self.shape[1] if include_self else 0) + (ref_k.shape[1] * ref_k.shape[2] if ref_k is not None else 0)
        _check_key_bias(key_bias, q, heads, lkv)
        a.key_bias = key_bias.data_ptr()
        a.kb_sb, a.kb_sh = key_bias.stride(0), (key_bias.stride(1) if key_bias.dim() == 3 else 0)
        a._keepbias = key_bias
        if valid_refs is not None and _is_table(ref_k):
            raise ValueError("key_bias with valid_refs on a RefKVTable call: slots n >= valid_refs[b] of the table are not readable, and the kernel "
                             "with a key bias walks every reference (mask them in the bias and fill the slots, or pass dense tensors)")
        valid_refs = None   # dense: the promise is about the DATA (all-zero references) - walking the zeros gives the same numbers
    if ref_lens is not None:
        a.ref_lens, a.rl_sb = ref_lens.data_ptr(), ref_lens.stride(0)
        a._keeplens = ref_lens
    if regions:
        a.q_allow, a.qa_sb = q_allow.data_ptr(), q_allow.stride(0)
        a.key_region, a.kg_sb = key_region.data_ptr(), key_region.stride(0)
        a._keepregions = (q_allow, key_region)
        if valid_refs is not None and _is_table(ref_k):
            raise ValueError("q_allow / key_region with valid_refs on a RefKVTable call: slots n >= valid_refs[b] of the table are not readable, and the "
                             "kernel with regions walks every reference (give those keys a region nobody may attend and fill the slots, or pass dense tensors)")
        valid_refs = None   # dense: the promise is about the DATA (all-zero references) - walking the zeros gives the same numbers
    if valid_refs is not None and ref_k is not None:
        if valid_refs.dtype != torch.int32 or valid_refs.device != q.device or valid_refs.numel() != q.shape[0] or not valid_refs.is_contiguous():
            raise ValueError(f"valid_refs must be a contiguous int32 ({q.shape[0]},) tensor on {q.device}")
        a.valid_refs = valid_refs.data_ptr()
    if out is not None:
        a.out = out.data_ptr()
        a.o_sb, a.o_sl, a.o_sh = out.stride(0), out.stride(1), HEAD_DIM
    if lse is not None:
        a.lse = lse.data_ptr()
    if out is not None and split and not batch_invariant:  # scratch for the remainder split (ir_shared_attn_workspace_bytes)
        ws = _workspace(q.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        a._keepalive = ws
    return a


def _check_ref_lens(rl, q, ref_k, valid_refs=None, key_bias=None) -> None:
    """``ref_lens``: int32 ``(B, N)`` on q's device, last axis contiguous (the row stride goes to the kernel as it is); not together
    with ``valid_refs`` or ``key_bias``"""
    if not isinstance(rl, torch.Tensor) or rl.dtype != torch.int32:
        raise ValueError(f"ref_lens must be an int32 tensor, got {getattr(rl, 'dtype', type(rl))}")
    if ref_k is None:
        raise ValueError("ref_lens given without references")
    want = (q.shape[0], ref_k.shape[1])
    if tuple(rl.shape) != want:
        raise ValueError(f"ref_lens must have shape (B, N) = {want}, got {tuple(rl.shape)}")
    if rl.device != q.device:
        raise ValueError(f"ref_lens is on {rl.device}, q on {q.device}")
    if rl.stride(-1) != 1 or rl.stride(0) < want[1]:
        raise ValueError("ref_lens: the reference axis must be contiguous (stride 1) and the rows at least N apart")
    if valid_refs is not None:
        raise ValueError("ref_lens with valid_refs: a count of 0 says the reference is absent, valid_refs says it is zero-filled - pass one of the two")
    if key_bias is not None:
        raise ValueError("ref_lens with key_bias: the bias indexes the packed uniform key axis; counts together with a bias are a follow-up")


def _check_regions(q_allow, key_region, q, lkv: int, key_bias=None, ref_lens=None) -> None:
    """``q_allow``: uint32 (or int32 storage of the same bits) ``(B, Lq)``; ``key_region``: int32 ``(B, Lkv)``; both on q's device, last
    axis contiguous (the row strides go to the kernel as they are); both or neither; not together with ``key_bias`` or ``ref_lens``"""
    if q_allow is None or key_region is None:
        raise ValueError("q_allow and key_region must be given together")
    if not isinstance(q_allow, torch.Tensor) or q_allow.dtype not in (torch.int32, torch.uint32):
        raise ValueError(f"q_allow must be an int32 or uint32 tensor (one 32-bit word per query row), got {getattr(q_allow, 'dtype', type(q_allow))}")
    if not isinstance(key_region, torch.Tensor) or key_region.dtype != torch.int32:
        raise ValueError(f"key_region must be an int32 tensor, got {getattr(key_region, 'dtype', type(key_region))}")
    B, Lq = q.shape[0], q.shape[1]
    if tuple(q_allow.shape) != (B, Lq):
        raise ValueError(f"q_allow must have shape (B, Lq) = {(B, Lq)}, got {tuple(q_allow.shape)}")
    if tuple(key_region.shape) != (B, lkv):
        raise ValueError(f"key_region must have shape (B, Lkv) = {(B, lkv)} over the extended key axis, got {tuple(key_region.shape)}")
    for name, t in (("q_allow", q_allow), ("key_region", key_region)):
        if t.device != q.device:
            raise ValueError(f"{name} is on {t.device}, q on {q.device}")
        if t.stride(-1) != 1 or t.stride(0) < t.shape[1]:
            raise ValueError(f"{name}: the last axis must be contiguous (stride 1) and the rows at least its length apart")
    if key_bias is not None:
        raise ValueError("q_allow / key_region with key_bias: regions together with a bias are a follow-up (one C operand carries either)")
    if ref_lens is not None:
        raise ValueError("q_allow / key_region with ref_lens: key_region indexes the packed uniform key axis; regions together with counts are a follow-up")


def region_masks(q_labels, key_labels, allow, *, self_len: int = 0, self_free: bool = True):
    """The pair ``(q_allow, key_region)`` of :func:`shared_attention` from integer class labels and a rule.

    ``q_labels`` ``(B, Lq)``, ``key_labels`` ``(B, Lkv)`` over the packed extended key axis: integer tensors (any integer dtype).
    ``allow``: a ``(C, C)`` bool matrix - ``allow[c, d]``: a query of class ``c`` may attend keys of class ``d`` - or a ``(C,)``
    integer tensor of bitmasks (bit ``d`` of ``allow[c]``).  ``C <= 32``.
    ``self_free`` (with ``self_len`` > 0 leading keys of the query's own picture): those keys get region 31 whatever their label and
    every row gets bit 31, so a token always sees its own picture; classes are then limited to 31 (region 31 is taken), and bit 31 of
    a bitmask rule is dropped.
    A key label outside ``[0, C)`` becomes region -1: nobody's.  A query label outside ``[0, C)`` gives a row that sees only what
    ``self_free`` grants (nothing at all without it: zeros, ``lse = -inf``).
    Returns ``q_allow`` int32 ``(B, Lq)`` (the storage of the 32-bit words) and ``key_region`` int32 ``(B, Lkv)``, on the labels'
    device.  Plain torch elementwise work and one gather, no host sync."""
    ql, kl = torch.as_tensor(q_labels), torch.as_tensor(key_labels)
    for name, t in (("q_labels", ql), ("key_labels", kl)):
        if t.dim() != 2 or t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
            raise ValueError(f"{name} must be an integer (B, L) tensor, got {t.dtype} {tuple(t.shape)}")
    if ql.shape[0] != kl.shape[0]:
        raise ValueError(f"q_labels and key_labels differ in batch: {ql.shape[0]} vs {kl.shape[0]}")
    dev = ql.device
    kl = kl.to(dev)
    rule = torch.as_tensor(allow).to(dev)
    free = bool(self_free) and int(self_len) > 0
    if not 0 <= int(self_len) <= kl.shape[1]:
        raise ValueError(f"self_len {self_len} outside [0, Lkv = {kl.shape[1]}]")
    C_ = rule.shape[0]
    most = _lib.IR_REGION_MAX - 1 if free else _lib.IR_REGION_MAX
    if C_ < 1 or C_ > most:
        raise ValueError(f"allow has {C_} classes: 1 .. {most} fit{' (self_free takes region 31)' if free else ''}")
    if rule.dim() == 2:
        if rule.dtype != torch.bool or rule.shape[1] != C_:
            raise ValueError(f"allow must be a (C, C) bool matrix or a (C,) tensor of bitmasks, got {rule.dtype} {tuple(rule.shape)}")
        words = (rule.to(torch.int64) << torch.arange(C_, device=dev, dtype=torch.int64)).sum(dim=1)
    elif rule.dim() == 1 and not (rule.dtype.is_floating_point or rule.dtype == torch.bool):
        words = rule.to(torch.int64) & ((1 << C_) - 1)   # bits of classes that do not exist (and bit 31 under self_free) are dropped
    else:
        raise ValueError(f"allow must be a (C, C) bool matrix or a (C,) tensor of bitmasks, got {rule.dtype} {tuple(rule.shape)}")
    ql64 = ql.to(torch.int64)
    q_ok = (ql64 >= 0) & (ql64 < C_)
    qa = torch.where(q_ok, words[ql64.clamp(0, C_ - 1)], torch.zeros((), dtype=torch.int64, device=dev))
    kl64 = kl.to(torch.int64)
    kr = torch.where((kl64 >= 0) & (kl64 < C_), kl64, torch.full((), -1, dtype=torch.int64, device=dev))
    if free:
        qa = qa | (1 << 31)
        kr[:, :int(self_len)] = _lib.IR_REGION_MAX - 1
    qa = torch.where(qa >= (1 << 31), qa - (1 << 32), qa)   # the same 32 bits as int32 storage
    return qa.to(torch.int32).contiguous(), kr.to(torch.int32).contiguous()


def _check_key_bias(kb, q, heads: int, lkv: int) -> None:
    """``key_bias``: fp32 ``(B, Lkv)`` or ``(B, H, Lkv)`` on q's device, last axis contiguous (the strides go to the kernel as they are)"""
    if not isinstance(kb, torch.Tensor) or kb.dtype != torch.float32:
        raise ValueError(f"key_bias must be a float32 tensor, got {getattr(kb, 'dtype', type(kb))}")
    want = ((q.shape[0], lkv), (q.shape[0], heads, lkv))
    if tuple(kb.shape) not in want:
        raise ValueError(f"key_bias must have shape (B, Lkv) = {want[0]} or (B, H, Lkv) = {want[1]} over the extended key axis, got {tuple(kb.shape)}")
    if kb.device != q.device:
        raise ValueError(f"key_bias is on {kb.device}, q on {q.device}")
    if kb.stride(-1) != 1 or any(st < 0 for st in kb.stride()):
        raise ValueError("key_bias: the key axis must be contiguous (stride 1) and no stride negative")


def key_bias(batch: int, len_self: int, n_refs: int, len_ref: int, include_self: bool, *, attention_mask=None, ref_weights=None,
             ref_token_keep=None, device=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fp32 ``(B, Lkv)`` bias row of :func:`shared_attention` over the extended key axis ``[self (iff include_self)] ++ ref 0 ++
    ... ++ ref N-1`` (``Lkv = include_self * len_self + n_refs * len_ref``), the sum of:

    ``ref_weights`` ``(B, N)``, values >= 0: ``log w`` on every key of the reference's segment - ``mass_n / mass_self`` scales by
    ``w_n``; 0 masks the reference (``-inf``).
    ``ref_token_keep`` bool: ``(B, N, len_ref)``, or ``(B, N, S, S)`` pooled by area to the layer's ``side = sqrt(len_ref)`` (a
    token is kept when >= 0.5 of its area is); dropped tokens are masked.
    ``attention_mask``: additive (diffusers' prepared form), ``(B, Lkv)`` or ``(B, 1, Lkv)`` over the extended length.

    Plain torch elementwise work, off the hot path, no sync.  ``out=``: refill that tensor in place (a captured step follows)."""
    B, N = int(batch), int(n_refs)
    ls = int(len_self) if include_self else 0
    lkv = ls + N * int(len_ref)
    if device is None:
        device = next((t.device for t in (out, attention_mask, ref_weights, ref_token_keep) if isinstance(t, torch.Tensor)), torch.device("cpu"))
    device = torch.device(device)
    row = torch.zeros((B, lkv), dtype=torch.float32, device=device)
    neg = float("-inf")
    if N > 0:
        refs = row[:, ls:].view(B, N, int(len_ref))
        if ref_weights is not None:
            w = torch.as_tensor(ref_weights).to(device=device, dtype=torch.float32)
            if tuple(w.shape) != (B, N):
                raise ValueError(f"ref_weights must have shape (B, N) = {(B, N)}, got {tuple(w.shape)}")
            if not w.is_cuda and bool((w < 0).any()):
                raise ValueError("ref_weights must be >= 0")
            refs += torch.log(w).unsqueeze(-1)   # log 0 = -inf: masked
        if ref_token_keep is not None:
            keep = torch.as_tensor(ref_token_keep).to(device=device)
            if keep.dtype != torch.bool:
                raise ValueError(f"ref_token_keep must be a bool tensor, got {keep.dtype}")
            if keep.dim() == 4:
                side = int(round(int(len_ref) ** 0.5))
                if keep.shape[:2] != (B, N) or side * side != int(len_ref) or keep.shape[2] != keep.shape[3]:
                    raise ValueError(f"ref_token_keep (B, N, S, S) needs a square layer (len_ref = {len_ref}) and shape ({B}, {N}, S, S), got {tuple(keep.shape)}")
                area = torch.nn.functional.adaptive_avg_pool2d(keep.to(torch.float32), side) if keep.shape[2] != side else keep.to(torch.float32)
                keep = (area >= 0.5).reshape(B, N, side * side)
            if tuple(keep.shape) != (B, N, int(len_ref)):
                raise ValueError(f"ref_token_keep must have shape (B, N, len_ref) = {(B, N, int(len_ref))} or (B, N, S, S), got {tuple(keep.shape)}")
            refs.masked_fill_(~keep, neg)
    elif ref_weights is not None or ref_token_keep is not None:
        raise ValueError("ref_weights / ref_token_keep given without references")
    if attention_mask is not None:
        m = torch.as_tensor(attention_mask).to(device=device)
        if m.dtype == torch.bool:
            raise ValueError("attention_mask must be additive (0 / -10000), not bool")
        if m.dim() == 3 and m.shape[1] == 1:
            m = m[:, 0]
        if tuple(m.shape) != (B, lkv):
            raise ValueError(f"attention_mask must have shape (B, Lkv) = {(B, lkv)} or (B, 1, Lkv) over the extended key axis, got {tuple(torch.as_tensor(attention_mask).shape)}")
        row += m.to(torch.float32)
    if out is not None:
        if out.dtype != torch.float32 or tuple(out.shape) != (B, lkv):
            raise ValueError(f"out must be fp32 {(B, lkv)}, got {out.dtype} {tuple(out.shape)}")
        out.copy_(row)
        return out
    return row


def _bi_workspace(a, device) -> None:
    """batch-invariant mode: a per-call scratch of exactly what the plan's pieces need (``ir_shared_attn_workspace_bytes_for``;
    none when every item runs whole), from torch's caching allocator on the current stream - so it follows that stream's
    ordering and, under graph capture, lives in the graph's pool like any other intermediate; the shared per-thread buffer of
    :func:`_workspace` (and its capture pinning) is not involved.  Set after ``seg_mass``: the masses size the pieces' partials."""
    nbytes = int(_lib.lib().ir_shared_attn_workspace_bytes_for(C.byref(a)))
    if nbytes > 0:
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        a._keepalive = ws


_WS = threading.local()
_WS_MAX_PER_THREAD = 8   # unpinned (device, stream) pairs a thread keeps scratch for; least recently used goes first


def _workspace(device: torch.device) -> torch.Tensor:
    """one scratch buffer per (device, stream, THREAD).  Launches on one stream are ordered, so one thread reuses its buffer
    safely; but ``ir_shared_attn_fwd`` issues two launches per call (the kernel, then the merge of its K/V-range pieces through
    this scratch), ctypes releases the GIL for the call, and threads that share a stream - torch's default stream is shared by
    all threads - can interleave: A's kernel, B's kernel, A's merge would read B's pieces.  A buffer per thread removes the
    hazard (69 MB each; tests/test_gpu_threads.py).

    Bounded (round 6): the buffers live in ``threading.local()`` - they are released with their thread, so a server that
    spawns a thread per request does not accumulate them - and a thread keeps at most ``_WS_MAX_PER_THREAD`` UNPINNED
    (device, stream) pairs, least recently used evicted.  A buffer handed out while its stream is being CAPTURED into a hipGraph
    is pinned for the life of the thread: the graph replays with the raw pointer, long after this call (bench.py's captured step;
    the first version of the bound evicted such a buffer and the replay faulted).  An evicted buffer goes back to torch's caching
    allocator, which keeps it off other streams until the work queued on its stream has run (``record_stream``)."""
    key = (device.index, _RAW_STREAM(device.index) if _RAW_STREAM is not None and device.index is not None
           else torch.cuda.current_stream(device).cuda_stream)
    cache = getattr(_WS, "cache", None)
    if cache is None:
        cache = _WS.cache = collections.OrderedDict()
        _WS.pinned = {}
    ws = _WS.pinned.get(key)
    if ws is not None:
        return ws
    capturing = torch.cuda.is_current_stream_capturing()
    ws = cache.get(key)
    if ws is None:
        ws = torch.empty(_lib.lib().ir_shared_attn_workspace_bytes() // 4, dtype=torch.float32, device=device)
        if not capturing:
            ws.record_stream(torch.cuda.current_stream(device))
        cache[key] = ws
    else:
        cache.move_to_end(key)
    if capturing:
        _WS.pinned[key] = cache.pop(key)
    while len(cache) > _WS_MAX_PER_THREAD:
        cache.popitem(last=False)
    return ws


def _forward_only(*ts) -> None:
    """the HIP path is the inference forward (test.py runs under ``torch.no_grad()``): a tensor that would
    need a backward through it must not pass silently - the result would carry no ``grad_fn``"""
    if torch.is_grad_enabled() and any(t is not None and not _is_table(t) and t.requires_grad for t in ts):
        raise NotImplementedError(
            "instantrestore_amd ops are forward-only (inference hot path): run under torch.no_grad() / "
            "inference_mode(); the training backward of the reference (coach.py) is out of scope")


def _prep(q, k_self, v_self, ref_k, ref_v, heads, include_self, adain):
    if ref_k is not None and ref_v is not None and _is_table(ref_k) != _is_table(ref_v):
        raise TypeError("ref_k and ref_v must both be RefKVTable objects or both be tensors")
    _need_gpu(q, k_self, v_self, ref_k, ref_v)
    _forward_only(q, k_self, v_self, ref_k, ref_v)
    q = _tok(q, heads, "q")
    if (ref_k is None) != (ref_v is None):
        raise ValueError("ref_k and ref_v must be given together")
    if ref_k is None and not include_self:
        raise ValueError("no references and include_self=False: empty key/value sequence")
    if include_self:
        k_self, v_self = _tok(k_self, heads, "k_self"), _tok(v_self, heads, "v_self")
        if k_self.shape != v_self.shape or k_self.shape[0] != q.shape[0]:
            raise ValueError("k_self / v_self shape mismatch")
    if ref_k is not None:
        ref_k, ref_v = _ref(ref_k, heads, "ref_k"), _ref(ref_v, heads, "ref_v")
        if ref_k.shape != ref_v.shape or ref_k.shape[0] != q.shape[0]:
            raise ValueError("ref_k / ref_v shape mismatch")
    for t in (k_self if include_self else None, v_self if include_self else None, ref_k, ref_v):
        if t is not None and t.dtype != q.dtype:
            raise TypeError(f"mixed dtypes on the fused path: q is {q.dtype}, a K/V tensor is {t.dtype}")
    if adain is not None:
        if ref_k is None:
            raise ValueError("AdaIN affine given without references")
        B, N = ref_k.shape[:2]
        for t in adain:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != B * N * heads * HEAD_DIM:
                raise ValueError("adain (a, b) must be contiguous fp32 of shape (B, N, H, 64)")
    return q, k_self, v_self, ref_k, ref_v


@_on_tensor_device
def shared_attention(q, k_self, v_self, ref_k=None, ref_v=None, *, heads: int, scale: float,
                     include_self: bool = True, adain: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                     return_lse: bool = False, split: bool = True, q_prescaled: bool = False,
                     out_dtype: Optional[torch.dtype] = None, valid_refs: Optional[torch.Tensor] = None,
                     return_mass: bool = False, batch_invariant: bool = False, key_bias: Optional[torch.Tensor] = None,
                     ref_lens: Optional[torch.Tensor] = None, q_allow: Optional[torch.Tensor] = None,
                     key_region: Optional[torch.Tensor] = None):
    """Fused extended self-attention (``ir_shared_attn_fwd``).

    Returns ``out`` (B, Lq, H*64) in q's dtype [, ``lse`` (B, H, Lq) fp32] [, ``mass`` (B, H, Lq, include_self + N) fp32:
    ``return_mass``, ABI v9 ``seg_mass`` - the attention mass of every K/V segment as a by-product of the same launch, what
    gradio_demo.py:119-127 reduces ``attention_probs`` to].  ``adain`` is the
    (a, b) pair from :func:`adain_stats`; the reference-V renormalisation happens inside the
    kernel's V staging.  ``q_prescaled``: ``q`` already holds ``Q * scale * log2(e)`` (``IR_FLAG_Q_PRESCALED``: the
    fused q/k/v projection folds the factor into its weights; ``scale`` stays the reference's ``attn.scale``).
    ``out_dtype=torch.float32`` returns the result before its rounding to 16 bit (``IR_FLAG_OUT_F32``, parity tests).
    ``valid_refs`` (ABI v8): int32 ``(B,)`` on the device - a PROMISE that references ``n >= valid_refs[b]`` are all-zero in
    ``ref_k`` and ``ref_v`` (``zero_invalid_refs``; pix2pix_turbo.py:269-273).  The kernels then close that suffix of the reference
    list analytically (every score exactly 0, every value row 0 or the AdaIN shift) instead of walking its tiles: same result,
    time proportional to the valid segments.  Zeroed, not masked: the tokens keep their exp(0) weight.
    ``batch_invariant`` (ABI v10, ``IR_FLAG_BATCH_INVARIANT``): the bytes of entry ``b`` of every output depend on entry ``b``'s
    inputs and the per-entry parameters only - not on the batch size or position, the other entries, the stream, capture,
    ``return_lse`` / ``return_mass`` or the tuning hook (:func:`shared_attention_plan` shows the plan).  ``split`` is ignored
    in this mode: the plan's K/V-range pieces are part of the result, and their scratch is allocated per call.
    ``ref_k`` / ``ref_v`` may be :class:`RefKVTable` objects (both or neither): the kernels then take every reference's base
    address from a device table instead of ``(B, N, L, C)`` tensors - same kernel, same pieces, same bytes as the dense call on
    ``torch.stack`` of the entries (:func:`attn_probs`, :func:`attn_segment_mass`, :func:`attn_rows` and
    :func:`shared_attention_kernel_name` take a table as ``ref_k`` too).  With ``valid_refs``, table slots ``n >= valid_refs[b]``
    are never read.
    ``key_bias`` (``ir_shared_attn_bias_args``): fp32 ``(B, Lkv)`` or ``(B, H, Lkv)`` on the device, added to the scaled scores before
    the softmax over the packed extended key axis (:func:`key_bias` builds the row from masks and per-reference weights).  A key
    at ``-inf`` or ``<= -10000`` is masked: probability exactly 0; a ``(b, h)`` with every key masked gives zeros, ``lse = -inf``
    and zero masses.  Read when the kernel runs (a captured call follows in-place updates).  Always the 32-row kernel.  With
    ``valid_refs``: a dense call drops the promise and walks the zeros (same numbers); a table call raises.  AdaIN statistics are
    not masked (the reference's ``adain`` knows no mask).  :func:`attn_probs`, :func:`attn_segment_mass` and :func:`attn_rows`
    take no bias - their ``exp(s - lse)`` would leave it out; ``return_mass`` is the read-back that honours it.
    ``ref_lens`` (``ir_shared_attn_ragged_args``): int32 ``(B, N)`` on the device, last axis contiguous - reference ``n`` of entry ``b``
    HAS ``clamp(ref_lens[b, n], 0, len_ref)`` keys, and ``len_ref`` (the tensors' token axis) is only the capacity of its segment.
    Keys behind the count do not exist: they are never used whatever lies there, ``lse`` and the masses are over the existing keys,
    a count of 0 is an absent reference (mass 0, its table slot never read), and a ``(b, h)`` without any key gives zeros,
    ``lse = -inf`` and zero masses.  Read when the kernel runs (a captured call follows in-place updates); always the 32-row kernel,
    time proportional to the tiles that exist.  :func:`compact_refs` packs kept tokens to the front and returns the counts.
    ``adain`` is taken as given - for a compacted reference pass the affine of the FULL reference (statistics before compaction).
    Raises with ``valid_refs`` (absent is not zero-filled) and with ``key_bias`` (the bias indexes the uniform key axis: a
    follow-up); the C ABI refuses ``n_refs == 0`` and tunings other than the default and the two 32-row forms, and
    :func:`attn_probs`, :func:`attn_segment_mass` and :func:`attn_rows` take no counts (``return_mass`` honours them).
    ``q_allow`` / ``key_region`` (``ir_shared_attn_region_args``, both or neither; :func:`region_masks` builds them from labels):
    per-QUERY masks in compact form.  ``key_region`` int32 ``(B, Lkv)`` gives every key of the packed extended key axis a region,
    ``q_allow`` int32 / uint32 ``(B, Lq)`` gives every query row the 32-bit set of regions it may attend (bit g = region g); one rule
    for all heads.  A pair that is not allowed has probability exactly 0; a key with a region outside ``[0, 31]`` is nobody's; a row
    with no allowed key gives zeros, ``lse = -inf`` and zero masses.  ``lse`` and the masses are over the allowed keys.  Read when
    the kernel runs (a captured call follows in-place updates); always the 32-row kernel, every tile walked.  With ``valid_refs``: a
    dense call drops the promise and walks the zeros; a table call raises.  Raises with ``key_bias`` and with ``ref_lens`` (regions
    together with a bias or with counts are a follow-up); the read-outs take no regions (``return_mass`` honours them).
    """
    q, k_self, v_self, ref_k, ref_v = _prep(q, k_self, v_self, ref_k, ref_v, heads, include_self, adain)
    if out_dtype not in (None, q.dtype, torch.float32):
        raise TypeError("out_dtype must be the compute dtype or torch.float32")
    out = torch.empty((q.shape[0], q.shape[1], heads * HEAD_DIM), dtype=out_dtype or q.dtype, device=q.device)
    lse = torch.empty((q.shape[0], heads, q.shape[1]), dtype=torch.float32, device=q.device) if return_lse else None
    args = _fill_args(q, k_self, v_self, ref_k, ref_v, heads, scale, include_self, adain, out, lse, split, q_prescaled, valid_refs,
                      batch_invariant, key_bias, ref_lens, q_allow, key_region)
    mass = None
    if return_mass:
        mass = torch.empty((q.shape[0], heads, q.shape[1], _nseg(include_self, ref_k)), dtype=torch.float32, device=q.device)
        args.seg_mass = mass.data_ptr()
    if batch_invariant:
        _bi_workspace(args, q.device)
    sink = EVENT_SINK
    if sink is not None and sink[0](q, ref_k, adain):   # bench.py: HIP events around chosen launches, in situ
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(_lib.lib().ir_shared_attn_fwd(C.byref(args), _stream()), "ir_shared_attn_fwd")
        e1.record()
        sink[1].append((e0, e1))
    else:
        _lib.check(_lib.lib().ir_shared_attn_fwd(C.byref(args), _stream()), "ir_shared_attn_fwd")
    res = (out,) + ((lse,) if return_lse else ()) + ((mass,) if return_mass else ())
    return res if len(res) > 1 else out


@_on_tensor_device
def time_shared_attention(q, k_self, v_self, ref_k=None, ref_v=None, *, heads: int, scale: float,
                          include_self: bool = True, adain=None, iters: int = 10, split: bool = True,
                          q_prescaled: bool = False, valid_refs: Optional[torch.Tensor] = None, return_mass: bool = False,
                          batch_invariant: bool = False, key_bias: Optional[torch.Tensor] = None,
                          ref_lens: Optional[torch.Tensor] = None, q_allow: Optional[torch.Tensor] = None,
                          key_region: Optional[torch.Tensor] = None) -> float:
    """Average ms per launch measured with HIP events on the launch stream (``bench.py``); ``valid_refs`` / ``return_mass`` /
    ``batch_invariant`` as in :func:`shared_attention` (the masses' finishing kernel is part of the timed launch)."""
    q, k_self, v_self, ref_k, ref_v = _prep(q, k_self, v_self, ref_k, ref_v, heads, include_self, adain)
    out = torch.empty((q.shape[0], q.shape[1], heads * HEAD_DIM), dtype=q.dtype, device=q.device)
    args = _fill_args(q, k_self, v_self, ref_k, ref_v, heads, scale, include_self, adain, out, None, split, q_prescaled, valid_refs,
                      batch_invariant, key_bias, ref_lens, q_allow, key_region)
    if return_mass:
        mass = torch.empty((q.shape[0], heads, q.shape[1], _nseg(include_self, ref_k)), dtype=torch.float32, device=q.device)
        args.seg_mass = mass.data_ptr()
    if batch_invariant:
        _bi_workspace(args, q.device)
    ms = C.c_float(0.0)
    _lib.check(_lib.lib().ir_time_shared_attn_fwd(C.byref(args), int(iters), _stream(), C.byref(ms)),
               "ir_time_shared_attn_fwd")
    return float(ms.value)


def bench_mfma_stream(dtype: torch.dtype = torch.bfloat16, zero_operands: bool = False, iters: int = 40000, launches: int = 5,
                      device: Optional[torch.device] = None) -> float:
    """TFLOP/s an MFMA-only stream of the attention kernels' instruction sustains on this device (``ir_bench_mfma_stream``):
    on pseudo-random operands the board's power cap sets it, on all-zero operands the clock does.  Measurement only."""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("bench_mfma_stream needs the GPU (no CPU fallback)")
    with torch.cuda.device(dev):
        nbytes = int(_lib.lib().ir_bench_mfma_stream_scratch_bytes())
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        out = C.c_float(0.0)
        _lib.check(_lib.lib().ir_bench_mfma_stream(_DT[dtype], 1 if zero_operands else 0, int(iters), int(launches), scratch.data_ptr(),
                                                   nbytes, _stream(), C.byref(out)), "ir_bench_mfma_stream")
    return float(out.value)


def shared_attention_kernel_name(q, k_self, v_self, ref_k=None, ref_v=None, *, heads: int, scale: float,
                                 include_self: bool = True, adain=None, q_prescaled: bool = False,
                                 valid_refs: Optional[torch.Tensor] = None, return_mass: bool = False,
                                 batch_invariant: bool = False, key_bias: Optional[torch.Tensor] = None,
                                 ref_lens: Optional[torch.Tensor] = None, q_allow: Optional[torch.Tensor] = None,
                                 key_region: Optional[torch.Tensor] = None) -> str:
    """which kernel the dispatcher launches for these tensors (reporting only; ``valid_refs`` / ``return_mass`` as in
    :func:`shared_attention` - they decide the 128-row kernel's form and whether the default rule takes it;
    ``batch_invariant``: the kernel and pieces of the batch-invariant plan)"""
    q, k_self, v_self, ref_k, ref_v = _prep(q, k_self, v_self, ref_k, ref_v, heads, include_self, adain)
    out = torch.empty((q.shape[0], q.shape[1], heads * HEAD_DIM), dtype=q.dtype, device=q.device)
    args = _fill_args(q, k_self, v_self, ref_k, ref_v, heads, scale, include_self, adain, out, None, True, q_prescaled, valid_refs,
                      batch_invariant, key_bias, ref_lens, q_allow, key_region)
    if return_mass:   # never written: the name is all this call computes
        mass = torch.empty((q.shape[0], heads, q.shape[1], _nseg(include_self, ref_k)), dtype=torch.float32, device=q.device)
        args.seg_mass = mass.data_ptr()
    return _lib.lib().ir_shared_attn_kernel_name(C.byref(args)).decode()


def shared_attention_plan(batch: int, len_q: int, heads: int, *, len_self: int = 0, n_refs: int = 0, len_ref: int = 0,
                          dtype: torch.dtype = torch.bfloat16, include_self: bool = True, adain: bool = False,
                          q_prescaled: bool = False, valid_refs: bool = False, return_mass: bool = False,
                          out_dtype: Optional[torch.dtype] = None, workspace_bytes: Optional[int] = None, key_bias: bool = False,
                          ref_lens: bool = False, regions: bool = False) -> dict:
    """the batch-invariant plan of a :func:`shared_attention` call of these sizes (``ir_shared_attn_plan``; host only - no tensor,
    no device): ``kernel`` (``IR_TUNE_*``), ``rows_per_item``, ``items_per_batch``, ``pieces_per_item``, ``workspace_bytes`` (the
    scratch of one launch over the batch, what :func:`shared_attention` allocates per call) and ``batch_per_launch`` - the entries
    one launch covers with a workspace of ``workspace_bytes`` bytes (default: the plan's own size).  ``ref_lens``: the call carries
    per-reference counts (the pieces are planned for full references); ``regions``: it carries ``q_allow`` / ``key_region`` (the
    32-row kernel at every len_q, cut as the bias form is)"""
    a = _lib.SharedAttnRegionArgs() if regions else _lib.SharedAttnRaggedArgs() if ref_lens else _lib.SharedAttnBiasArgs() if key_bias else _lib.SharedAttnArgs()   # key_bias: one more per-entry parameter (the 32-row kernel at every len_q)
    a.struct_size = C.sizeof(a)
    a.dtype = _DT[dtype]
    a.flags = _lib.IR_FLAG_BATCH_INVARIANT | (_lib.IR_FLAG_INCLUDE_SELF if include_self else 0) | \
        (_lib.IR_FLAG_Q_PRESCALED if q_prescaled else 0) | (_lib.IR_FLAG_OUT_F32 if out_dtype == torch.float32 else 0)
    a.batch, a.len_q, a.heads, a.scale = int(batch), int(len_q), int(heads), 0.125
    a.len_self = int(len_self) if include_self else 0
    a.n_refs, a.len_ref = int(n_refs), int(len_ref)
    # the checks of a launch look at the pointer fields (set or NULL, alignment) and never read through them: one aligned dummy
    c = HEAD_DIM * int(heads)
    dummy = 256
    a.q = a.out = dummy
    a.q_sb, a.q_sl, a.q_sh = int(len_q) * c, c, HEAD_DIM
    a.o_sb, a.o_sl, a.o_sh = int(len_q) * c, c, HEAD_DIM
    if include_self:
        a.k_self = a.v_self = dummy
        a.ks_sb = a.vs_sb = int(len_self) * c
        a.ks_sl = a.vs_sl = c
        a.ks_sh = a.vs_sh = HEAD_DIM
    if n_refs:
        a.k_ref = a.v_ref = dummy
        a.kr_sb = a.vr_sb = int(n_refs) * int(len_ref) * c
        a.kr_sn = a.vr_sn = int(len_ref) * c
        a.kr_sl = a.vr_sl = c
        a.kr_sh = a.vr_sh = HEAD_DIM
    if adain:
        a.adain_a = a.adain_b = dummy
    if valid_refs:
        a.valid_refs = dummy
    if return_mass:
        a.seg_mass = dummy
    if key_bias:
        a.key_bias = dummy
    if ref_lens:
        a.ref_lens, a.rl_sb = dummy, int(n_refs)
    if regions:
        a.q_allow, a.qa_sb = dummy, int(len_q)
        a.key_region, a.kg_sb = dummy, (int(len_self) if include_self else 0) + int(n_refs) * int(len_ref)
    L = _lib.lib()
    if workspace_bytes is None:
        workspace_bytes = int(L.ir_shared_attn_workspace_bytes_for(C.byref(a)))
    if workspace_bytes > 0:
        a.workspace, a.workspace_bytes = dummy, int(workspace_bytes)
    plan = _lib.SharedAttnPlan()
    plan.struct_size = C.sizeof(_lib.SharedAttnPlan)
    _lib.check(L.ir_shared_attn_plan(C.byref(a), C.byref(plan)), "ir_shared_attn_plan")
    return {n: int(getattr(plan, n)) for n, _ in _lib.SharedAttnPlan._fields_ if n != "struct_size"}


PROBS_KERNELS = {"auto": 0, "generic": 1, "lines64": 2, "lines32": 3, "lines32k128": 4, "lines64k128": 5, "lines32k256": 6}   # IR_PROBS_*


def _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled=False, batch_invariant=False, one_kernel=False):
    """the argument block of a read-out from the LSE.  ``one_kernel``: the entry point has one kernel, so the A/B hook of the
    forward (``tuning``) does not apply"""
    q, k_self, _, ref_k, _ = _prep(q, k_self, k_self, ref_k, ref_k, heads, include_self, None)
    B, Lq, _ = q.shape
    lkv = (k_self.shape[1] if include_self else 0) + (ref_k.shape[1] * ref_k.shape[2] if ref_k is not None else 0)
    if lse.dtype != torch.float32 or not lse.is_contiguous() or tuple(lse.shape) != (B, heads, Lq):
        raise ValueError("lse must be contiguous fp32 (B, H, Lq)")
    args = _fill_args(q, k_self, k_self, ref_k, ref_k, heads, scale, include_self, None, None, lse, True, q_prescaled, None,
                      batch_invariant)
    if one_kernel:
        args.tuning = 0
    return args, q, B, Lq, lkv, (q, k_self, ref_k, lse)


def _check_reduce(reduce: str, codes: dict) -> None:
    if reduce not in codes:
        raise ValueError(f"reduce must be one of {sorted(codes)}, got {reduce!r}")


def _all_rows(batch: int, len_q: int, device: torch.device) -> torch.Tensor:
    """``rows=None`` of a read-out - every query token, in order - as the index tensor :func:`_row_index` makes of a list"""
    return torch.arange(len_q, dtype=torch.int32, device=device).unsqueeze(0).expand(batch, -1).contiguous()


@_on_tensor_device
def attn_probs(q, k_self, ref_k, lse, *, heads: int, scale: float, include_self: bool = True, kernel: str = "auto",
               q_prescaled: bool = False, batch_invariant: bool = False) -> torch.Tensor:
    """Materialise ``attention_probs`` (B, H, Lq, Lkv) from the LSE of the fused forward
    (``ir_attn_probs``; the ``save_self_attentions`` dump path, attn_processors.py:258-261).
    ``kernel``: ``PROBS_KERNELS`` (benchmarks / A-B tests; "auto" is what the processors use).  ``q_prescaled``: ``q`` holds
    ``Q * scale * log2(e)`` (``IR_FLAG_Q_PRESCALED``; ``scale`` stays the reference's ``attn.scale``, the unit of ``lse``).
    ``batch_invariant`` (ABI v10): the kernel follows the per-entry parameters only (with an invariant ``lse``, so is every
    probability)."""
    args, q, B, Lq, lkv, _keep = _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled, batch_invariant)
    probs = torch.empty((B, heads, Lq, lkv), dtype=q.dtype, device=q.device)
    _lib.check(_lib.lib().ir_attn_probs_ex(C.byref(args), probs.data_ptr(), PROBS_KERNELS[kernel], _stream()), "ir_attn_probs")
    return probs


@_on_tensor_device
def attn_segment_mass(q, k_self, ref_k, lse, *, heads: int, scale: float, include_self: bool = True,
                      q_prescaled: bool = False, batch_invariant: bool = False) -> torch.Tensor:
    """Attention mass per K/V segment, fp32 (B, H, Lq, include_self + N), without the probability matrix
    (``ir_attn_segment_mass``): what gradio_demo.py:119-127 reduces ``attention_probs`` to.  ``batch_invariant`` as in
    :func:`attn_probs`."""
    args, q, B, Lq, _, _keep = _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled, batch_invariant)
    mass = torch.empty((B, heads, Lq, _nseg(include_self, ref_k)), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().ir_attn_segment_mass(C.byref(args), mass.data_ptr(), _stream()), "ir_attn_segment_mass")
    return mass


ROWS_REDUCE = {"none": _lib.IR_ROWS_NONE, "head_mean": _lib.IR_ROWS_HEAD_MEAN, "map": _lib.IR_ROWS_MAP}


def _row_index(rows, batch: int, len_q: int, device: torch.device) -> torch.Tensor:
    """``rows`` as the contiguous int32 ``(B, R)`` device tensor ``ir_attn_rows`` reads.  A CPU tensor is range-checked here; a
    device tensor is converted without a sync (the kernel turns an index outside ``[0, len_q)`` into an all-zero row)."""
    rows = torch.as_tensor(rows)
    if rows.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or rows.dim() not in (1, 2):
        raise ValueError(f"rows must be an integer tensor (R,) or (B, R), got {rows.dtype} {tuple(rows.shape)}")
    if rows.dim() == 2 and rows.shape[0] != batch:
        raise ValueError(f"rows: {rows.shape[0]} index lists for a batch of {batch}")
    if rows.shape[-1] < 1 or rows.shape[-1] > len_q:
        raise ValueError(f"rows: {rows.shape[-1]} indices per entry, expected 1 ... len_q = {len_q}")
    if not rows.is_cuda and (int(rows.min()) < 0 or int(rows.max()) >= len_q):
        raise ValueError(f"rows: indices must lie in [0, {len_q})")
    rows = rows.to(device=device, dtype=torch.int32, non_blocking=True)
    if rows.dim() == 1:
        rows = rows.unsqueeze(0).expand(batch, -1)
    return rows.contiguous()


@_on_tensor_device
def attn_rows(q, k_self, ref_k, lse, rows, *, heads: int, scale: float, include_self: bool = True, reduce: str = "none",
              q_prescaled: bool = False, batch_invariant: bool = False) -> torch.Tensor:
    """The probability rows of the query tokens ``rows`` from the LSE of the fused forward, without the ``(B, H, Lq, Lkv)``
    tensor (``ir_attn_rows``): what vis_utils.py:88-110 (``get_visualization_image``) reads out of ``attention_probs``.

    ``rows``: integer tensor ``(R,)`` (one list for the whole batch) or ``(B, R)``, on the CPU or the device; duplicates give
    repeated rows.  ``reduce``: ``"none"`` - ``attention_probs[:, :, rows]``, ``(B, H, R, Lkv)`` in q's dtype, bit for bit the rows
    of :func:`attn_probs`; ``"head_mean"`` - fp32 ``(B, R, Lkv)``, ``attn.mean(dim=1)[b][rows]``; ``"map"`` - fp32 ``(B, Lkv)``,
    the sum of those rows (the landmark heat map before its reshape, :func:`instantrestore_amd.attn_maps.landmark_picture`).
    ``q_prescaled`` as in :func:`attn_probs`.  Batch invariant by construction; ``batch_invariant`` is accepted and changes nothing."""
    _check_reduce(reduce, ROWS_REDUCE)
    args, q, B, Lq, lkv, _keep = _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled, batch_invariant, one_kernel=True)
    idx = _row_index(rows, B, Lq, q.device)
    R = idx.shape[1]
    if reduce == "none":
        out = torch.empty((B, heads, R, lkv), dtype=q.dtype, device=q.device)
    elif reduce == "head_mean":
        out = torch.empty((B, R, lkv), dtype=torch.float32, device=q.device)
    else:
        out = torch.empty((B, lkv), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().ir_attn_rows(C.byref(args), idx.data_ptr(), R, ROWS_REDUCE[reduce], out.data_ptr(), _stream()), "ir_attn_rows")
    return out


MATCH_REDUCE = {"none": _lib.IR_MATCH_PER_HEAD, "head_mean": _lib.IR_MATCH_HEAD_MEAN}


@_on_tensor_device
def attn_match(q, k_self, ref_k, lse, rows=None, *, heads: int, scale: float, include_self: bool = True, reduce: str = "none",
               q_prescaled: bool = False, batch_invariant: bool = False):
    """The best-matching key of every K/V segment for the query tokens ``rows`` from the LSE of the fused forward, without the
    ``(B, H, Lq, Lkv)`` tensor (``ir_attn_match``): ``attention_probs[..., segment].max(-1)`` / ``.argmax(-1)`` per segment of
    ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1``.

    ``rows``: ``None`` - every query token, in order - or an integer tensor ``(R,)`` / ``(B, R)`` as for :func:`attn_rows`
    (duplicates are rows like any other; a device index outside ``[0, Lq)`` gives ``index = -1``, ``prob = 0``).  Returns
    ``(index, prob)``: int32 and fp32, ``(B, H, R, S)`` with ``reduce="none"`` (per head), ``(B, R, S)`` with ``"head_mean"`` (of
    the head mean as :func:`attn_rows` forms it).  ``prob`` is the largest fp32 probability of the segment - rounded to q's dtype
    it is the maximum of :func:`attn_probs` there; the head-mean ``prob`` is the maximum of :func:`attn_rows`' head-mean row bit
    for bit - and ``index`` the lowest key, counted inside its segment, that attains it
    (:func:`instantrestore_amd.attn_maps.match_coordinates` turns it into ``(y, x)``).  ``q_prescaled`` as in :func:`attn_probs`.
    Batch invariant by construction; ``batch_invariant`` is accepted and changes nothing."""
    _check_reduce(reduce, MATCH_REDUCE)
    args, q, B, Lq, _, _keep = _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled, batch_invariant, one_kernel=True)
    idx = _all_rows(B, Lq, q.device) if rows is None else _row_index(rows, B, Lq, q.device)
    R = idx.shape[1]
    nseg = _nseg(include_self, ref_k)
    shape = (B, heads, R, nseg) if reduce == "none" else (B, R, nseg)
    index = torch.empty(shape, dtype=torch.int32, device=q.device)
    prob = torch.empty(shape, dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().ir_attn_match(C.byref(args), idx.data_ptr(), R, MATCH_REDUCE[reduce], index.data_ptr(), prob.data_ptr(), _stream()),
               "ir_attn_match")
    return index, prob


@_on_tensor_device
def attn_topk(q, k_self, ref_k, lse, rows=None, *, k: int, heads: int, scale: float, include_self: bool = True, reduce: str = "none",
              q_prescaled: bool = False, batch_invariant: bool = False):
    """The ``k`` best keys of every K/V segment for the query tokens ``rows`` from the LSE of the fused forward, without the
    ``(B, H, Lq, Lkv)`` tensor (``ir_attn_topk``): ``torch.topk(attention_probs[..., segment], k)`` per segment of
    ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1``, :func:`attn_match` with ranks.

    ``k``: ``1 ... IR_TOPK_MAX`` (8).  ``rows``: ``None`` - every query token, in order - or an integer tensor ``(R,)`` / ``(B, R)`` as
    for :func:`attn_match` (duplicates are rows like any other; a device index outside ``[0, Lq)`` gives ``index = -1``,
    ``prob = 0`` in every rank).  Returns ``(index, prob)``: int32 and fp32, ``(B, H, R, S, k)`` with ``reduce="none"`` (per head),
    ``(B, R, S, k)`` with ``"head_mean"`` (of the head mean as :func:`attn_rows` forms it).  Rank ``t`` holds the ``t``-th key of the
    segment under (fp32 probability descending, key ascending) - equal probabilities come in ascending key order - counted inside
    its segment; a segment with fewer than ``k`` keys ends in ``index = -1``, ``prob = 0``.  Rank 0 is :func:`attn_match` of the same
    call bit for bit; the head-mean ranks are a stable descending sort of :func:`attn_rows`' head-mean row segment.
    :func:`instantrestore_amd.attn_maps.topk_coordinates`, ``match_ambiguity``, ``topk_coverage`` and ``keep_from_topk`` read the
    result.  ``q_prescaled`` as in :func:`attn_probs`.  Batch invariant by construction; ``batch_invariant`` is accepted and changes
    nothing."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.IR_TOPK_MAX:
        raise ValueError(f"k must be an integer in 1 ... {_lib.IR_TOPK_MAX}, got {k!r}")
    _check_reduce(reduce, MATCH_REDUCE)
    args, q, B, Lq, _, _keep = _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled, batch_invariant, one_kernel=True)
    idx = _all_rows(B, Lq, q.device) if rows is None else _row_index(rows, B, Lq, q.device)
    R = idx.shape[1]
    nseg = _nseg(include_self, ref_k)
    shape = (B, heads, R, nseg, k) if reduce == "none" else (B, R, nseg, k)
    index = torch.empty(shape, dtype=torch.int32, device=q.device)
    prob = torch.empty(shape, dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().ir_attn_topk(C.byref(args), idx.data_ptr(), R, k, MATCH_REDUCE[reduce], index.data_ptr(), prob.data_ptr(), _stream()),
               "ir_attn_topk")
    return index, prob


TRANSFER_REDUCE = {"none": _lib.IR_TRANSFER_PER_HEAD, "head_mean": _lib.IR_TRANSFER_HEAD_MEAN}


def _transfer_payload(payload, batch: int, lkv: int, device: torch.device):
    """``payload`` checked against the call: the tensor as it is (never copied) and its batch / key strides in floats"""
    if not isinstance(payload, torch.Tensor) or payload.dtype != torch.float32:
        raise ValueError(f"payload must be an fp32 tensor, got {getattr(payload, 'dtype', type(payload))}")
    if payload.dim() not in (2, 3):
        raise ValueError(f"payload must be (Lkv, C), (1, Lkv, C) or (B, Lkv, C), got {tuple(payload.shape)}")
    if payload.device != device:
        raise ValueError(f"payload is on {payload.device}, the call on {device}")
    if payload.dim() == 3 and payload.shape[0] not in (1, batch):
        raise ValueError(f"payload: {payload.shape[0]} batch entries for a batch of {batch} (1 or {batch})")
    if payload.shape[-2] != lkv:
        raise ValueError(f"payload: {payload.shape[-2]} keys, the call has Lkv = {lkv}")
    nch = payload.shape[-1]
    if nch < 1 or nch > _lib.IR_TRANSFER_MAX_CHANNELS:
        raise ValueError(f"payload: {nch} channels, expected 1 ... {_lib.IR_TRANSFER_MAX_CHANNELS} (call again for more)")
    if payload.stride(-1) != 1:
        raise ValueError(f"payload: last-axis stride {payload.stride(-1)}, expected 1")
    sj = payload.stride(-2) if lkv > 1 else nch
    sb = payload.stride(0) if payload.dim() == 3 and payload.shape[0] == batch and batch > 1 else 0
    if sj < nch or sb < 0:
        raise ValueError(f"payload: key stride {sj} must be >= {nch} channels and the batch stride {sb} >= 0")
    return payload, sb, sj, nch


@_on_tensor_device
def attn_transfer(q, k_self, ref_k, lse, payload, rows=None, *, heads: int, scale: float, include_self: bool = True,
                  reduce: str = "none", normalize: bool = False, q_prescaled: bool = False, batch_invariant: bool = False):
    """Attention-weighted sums of a per-key payload for the query tokens ``rows`` from the LSE of the fused forward, without the
    ``(B, H, Lq, Lkv)`` tensor (``ir_attn_transfer``): ``einsum('bhij,bjc->bhic', attention_probs[..., segment], payload[:, segment])``
    per segment of ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1`` - the soft form of :func:`attn_match`.

    ``payload``: fp32 device tensor ``(Lkv, C)``, ``(1, Lkv, C)`` (one payload for the whole batch) or ``(B, Lkv, C)``, ``C <= 8``,
    last-axis stride 1; its key and batch strides are passed through, never copied
    (:func:`instantrestore_amd.attn_maps.coordinate_payload` / ``image_payload`` build the usual ones).  ``rows``: ``None`` - every
    query token, in order - or an integer tensor ``(R,)`` / ``(B, R)`` as for :func:`attn_match` (a device index outside ``[0, Lq)``
    gives sums 0, mass 0).  Returns ``(values, mass)``, fp32: ``(B, H, R, S, C)`` and ``(B, H, R, S)`` with ``reduce="none"``,
    ``(B, R, S, C)`` and ``(B, R, S)`` with ``"head_mean"`` - bit for bit ``((S_0 + S_1) + ...) * (1/H)`` of the per-head result.
    ``values`` are the UNNORMALISED sums (``values.sum(-2)`` is the expectation over all keys); ``normalize=True`` returns
    ``sums / mass`` - the expectation inside each segment - where ``mass > 0`` and 0 elsewhere.  The mass and every channel are
    summed over the same keys in the same order: a channel of ones IS the mass, a one-hot channel IS that key's fp32 probability
    (what :func:`attn_rows` rounds to q's dtype).  ``q_prescaled`` as in :func:`attn_probs`.  Batch invariant by construction;
    ``batch_invariant`` is accepted and changes nothing."""
    _check_reduce(reduce, TRANSFER_REDUCE)
    args, q, B, Lq, lkv, _keep = _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled, batch_invariant, one_kernel=True)
    payload, sb, sj, nch = _transfer_payload(payload, B, lkv, q.device)
    idx = _all_rows(B, Lq, q.device) if rows is None else _row_index(rows, B, Lq, q.device)
    R = idx.shape[1]
    nseg = _nseg(include_self, ref_k)
    shape = (B, heads, R, nseg) if reduce == "none" else (B, R, nseg)
    sums = torch.empty(shape + (nch,), dtype=torch.float32, device=q.device)
    mass = torch.empty(shape, dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().ir_attn_transfer(C.byref(args), payload.data_ptr(), sb, sj, nch, idx.data_ptr(), R, TRANSFER_REDUCE[reduce],
                                           sums.data_ptr(), mass.data_ptr(), _stream()), "ir_attn_transfer")
    if normalize:
        m = mass.unsqueeze(-1)
        sums = torch.where(m > 0, sums / m, torch.zeros_like(sums))
    return sums, mass


RECEIVED_REDUCE = {"none": _lib.IR_RECEIVED_PER_HEAD, "head_mean": _lib.IR_RECEIVED_HEAD_MEAN}


def _received_weights(weights, batch: int, len_q: int, device: torch.device):
    """``weights`` checked against the call: the tensor as it is (never copied), its batch / row strides in floats and its
    channel count.  ``(L,)`` / ``(B, L)`` are one channel; ``(L, C)``, ``(1, L, C)``, ``(B, L, C)`` carry ``C``"""
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32:
        raise ValueError(f"weights must be an fp32 tensor, got {getattr(weights, 'dtype', type(weights))}")
    if weights.dim() not in (1, 2, 3):
        raise ValueError(f"weights must be (L,), (B, L), (L, C), (1, L, C) or (B, L, C), got {tuple(weights.shape)}")
    if weights.device != device:
        raise ValueError(f"weights is on {weights.device}, the call on {device}")
    # two axes: (L, C) when the first one is the query axis, else (B, L); a shape that reads both ways is refused
    if weights.dim() == 2 and weights.shape[0] == len_q and tuple(weights.shape) == (batch, len_q):
        raise ValueError(f"weights {tuple(weights.shape)} reads as (L, C) and as (B, L) for a batch of {batch} and len_q = {len_q}: "
                         f"pass (1, L, C) or (B, L, 1)")
    one_channel = weights.dim() == 1 or (weights.dim() == 2 and weights.shape[0] != len_q)
    if one_channel:
        weights = weights.unsqueeze(-1)          # a view: the row stride stays what it was
    if weights.dim() == 3 and weights.shape[0] not in (1, batch):
        raise ValueError(f"weights: {weights.shape[0]} batch entries for a batch of {batch} (1 or {batch})")
    if weights.shape[-2] != len_q:
        raise ValueError(f"weights: {weights.shape[-2]} rows, the call has len_q = {len_q}")
    nch = weights.shape[-1]
    if nch < 1 or nch > _lib.IR_RECEIVED_MAX_CHANNELS:
        raise ValueError(f"weights: {nch} channels, expected 1 ... {_lib.IR_RECEIVED_MAX_CHANNELS} (call again for more)")
    if not one_channel and weights.stride(-1) != 1:
        raise ValueError(f"weights: last-axis stride {weights.stride(-1)}, expected 1")
    si = weights.stride(-2) if len_q > 1 else nch
    sb = weights.stride(0) if weights.dim() == 3 and weights.shape[0] == batch and batch > 1 else 0
    if si < nch or sb < 0:
        raise ValueError(f"weights: row stride {si} must be >= {nch} channels and the batch stride {sb} >= 0")
    return weights, sb, si, nch


@_on_tensor_device
def attn_received(q, k_self, ref_k, lse, weights=None, *, heads: int, scale: float, include_self: bool = True, reduce: str = "none",
                  q_prescaled: bool = False, batch_invariant: bool = False) -> torch.Tensor:
    """The attention every key RECEIVES from the query rows, from the LSE of the fused forward, without the ``(B, H, Lq, Lkv)``
    tensor (``ir_attn_received``): ``einsum('bhij,bic->bhjc', attention_probs, weights)`` - with ``weights=None`` one channel of
    ones, ``attention_probs.sum(dim=-2)[..., None]``.  The adjoint of :func:`attn_transfer`.

    ``weights``: ``None`` or an fp32 device tensor over the query axis - ``(L, C)``, ``(1, L, C)`` (one payload for the whole
    batch) or ``(B, L, C)``, ``C <= 8``, last-axis stride 1; ``(L,)`` / ``(B, L)`` are one channel.  A tensor of two axes is
    ``(L, C)`` when its first axis has ``len_q`` entries and ``(B, L)`` otherwise; one that reads both ways (``B == len_q``) is
    refused: pass three axes.  Its row and batch strides are passed through, never copied (an expanded batch axis is stride 0).  Returns fp32 ``(B, H, Lkv, C)`` with
    ``reduce="none"``, ``(B, Lkv, C)`` with ``"head_mean"`` - bit for bit ``((R_0 + R_1) + ...) * (1/H)`` of the per-head result -
    over the packed key axis ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1``
    (:func:`instantrestore_amd.attn_maps.received_maps` cuts it into pictures, ``keep_from_received`` into a ``keep`` mask for
    :func:`compact_refs`).  Every term is one fused multiply-add in a fixed order that follows ``len_q`` and ``reduce`` only: a
    one-hot channel at row ``i`` IS that row's fp32 probabilities (what :func:`attn_rows` rounds to q's dtype), ``None`` IS a
    channel of ones.  ``q_prescaled`` as in :func:`attn_probs`.  Batch invariant by construction; ``batch_invariant`` is accepted
    and changes nothing."""
    _check_reduce(reduce, RECEIVED_REDUCE)
    args, q, B, Lq, lkv, _keep = _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled, batch_invariant, one_kernel=True)
    if weights is None:
        wptr, sb, si, nch = None, 0, 1, 1
    else:
        weights, sb, si, nch = _received_weights(weights, B, Lq, q.device)
        wptr = weights.data_ptr()
    recv = torch.empty((B, heads, lkv, nch) if reduce == "none" else (B, lkv, nch), dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().ir_attn_received(C.byref(args), wptr, sb, si, nch, RECEIVED_REDUCE[reduce], recv.data_ptr(), _stream()),
               "ir_attn_received")
    return recv


@_on_tensor_device
def attn_key_match(q, k_self, ref_k, lse, *, heads: int, scale: float, include_self: bool = True, reduce: str = "none",
                   q_prescaled: bool = False, batch_invariant: bool = False):
    """The query row that looks hardest at every key, from the LSE of the fused forward, without the ``(B, H, Lq, Lkv)`` tensor
    (``ir_attn_key_match``): ``attention_probs.max(dim=-2)`` / ``.argmax(dim=-2)`` over ALL query rows.  The query-axis
    counterpart of :func:`attn_match`, and the second half of the mutual check
    (:func:`instantrestore_amd.attn_maps.mutual_matches`).

    Returns ``(index, prob)``: int32 and fp32, ``(B, H, Lkv)`` with ``reduce="none"`` (per head), ``(B, Lkv)`` with
    ``"head_mean"`` (of the head mean as :func:`attn_rows` forms it), over the packed key axis
    ``[self (iff include_self)] ++ ref 0 ++ ... ++ ref N-1`` (the axis of :func:`attn_received`).  ``prob`` is the largest fp32
    probability of the column - rounded to q's dtype it is the maximum of :func:`attn_probs` there; the head-mean ``prob`` is the
    column maximum of :func:`attn_rows`' head-mean rows bit for bit - and ``index`` the LOWEST query row that attains it.  The
    order (probability descending, row ascending) is total, so the result depends on no order of evaluation; a column of zeros
    gives ``index 0``, ``prob 0``.  :func:`instantrestore_amd.attn_maps.keep_from_key_match` turns ``prob`` into a ``keep`` mask
    for :func:`compact_refs`.  ``q_prescaled`` as in :func:`attn_probs`.  Batch invariant by construction; ``batch_invariant`` is
    accepted and changes nothing."""
    _check_reduce(reduce, MATCH_REDUCE)
    args, q, B, Lq, lkv, _keep = _probs_args(q, k_self, ref_k, lse, heads, scale, include_self, q_prescaled, batch_invariant, one_kernel=True)
    shape = (B, heads, lkv) if reduce == "none" else (B, lkv)
    index = torch.empty(shape, dtype=torch.int32, device=q.device)
    prob = torch.empty(shape, dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().ir_attn_key_match(C.byref(args), MATCH_REDUCE[reduce], index.data_ptr(), prob.data_ptr(), _stream()),
               "ir_attn_key_match")
    return index, prob


@_on_tensor_device
def adain_stats(v_self: torch.Tensor, ref_v: torch.Tensor, *, heads: int, eps: float = ADAIN_EPS):
    """AdaIN as a per-(b, n, head, channel) affine ``x*a + b`` (``ir_adain_stats``).

    ``v_self`` (B, L, H*64) supplies the style statistics, ``ref_v`` (B, N, Lr, H*64) the content
    statistics (attn_processors.py:9-10, 244-245: token axis, unbiased std, eps on both)."""
    if _is_table(ref_v):
        raise TypeError("adain_stats reads a dense ref_v (ir_adain_stats has no pointer-table form): with a RefKVTable take the affine "
                        "from cached content statistics (adain_stats_cached / adain_affine_from_partials)")
    _need_gpu(v_self, ref_v)
    _forward_only(v_self, ref_v)
    v_self, ref_v = _tok(v_self, heads, "v_self"), _ref(ref_v, heads, "ref_v")
    if v_self.dtype != ref_v.dtype:
        raise TypeError("v_self / ref_v dtype mismatch")
    B, Ls, _ = v_self.shape
    _, N, Lr, _ = ref_v.shape
    L = _lib.lib()
    nbytes = L.ir_adain_stats_workspace_bytes(B, heads, Ls, N, Lr)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=v_self.device)
    a = torch.empty((B, N, heads, HEAD_DIM), dtype=torch.float32, device=v_self.device)
    b = torch.empty_like(a)
    rc = L.ir_adain_stats(_dtype_code(v_self), B, heads, Ls, N, Lr,
                          v_self.data_ptr(), v_self.stride(0), v_self.stride(1), HEAD_DIM,
                          ref_v.data_ptr(), ref_v.stride(0), ref_v.stride(1), ref_v.stride(2), HEAD_DIM,
                          float(eps), a.data_ptr(), b.data_ptr(), ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "ir_adain_stats")
    return a, b


@_on_tensor_device
def adain_stats_cached(v_self: torch.Tensor, content_mean: torch.Tensor, content_std: torch.Tensor, *, heads: int,
                       eps: float = ADAIN_EPS):
    """The affine of :func:`adain_stats` from CACHED content statistics (``ir_adain_stats_cached``): ``content_mean`` /
    ``content_std`` are the fp32 ``(B, N, H, 64)`` outputs of :func:`token_stats` over the reference V's (the K/V-capture
    layer computes them once per identity); only ``v_self`` is read.  Bit-identical to ``adain_stats(v_self, ref_v)``."""
    _need_gpu(v_self, content_mean, content_std)
    _forward_only(v_self)
    v_self = _tok(v_self, heads, "v_self")
    B, Ls, _ = v_self.shape
    if content_mean.dim() != 4 or content_mean.shape != content_std.shape or content_mean.shape[0] != B or \
            tuple(content_mean.shape[2:]) != (heads, HEAD_DIM):
        raise ValueError(f"content statistics must be two (B, N, {heads}, 64) tensors")
    for t in (content_mean, content_std):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("content statistics must be contiguous fp32")
    N = content_mean.shape[1]
    L = _lib.lib()
    nbytes = L.ir_adain_stats_workspace_bytes(B, heads, Ls, 0, Ls)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=v_self.device)
    a = torch.empty((B, N, heads, HEAD_DIM), dtype=torch.float32, device=v_self.device)
    b = torch.empty_like(a)
    rc = L.ir_adain_stats_cached(_dtype_code(v_self), B, heads, Ls, N, v_self.data_ptr(), v_self.stride(0), v_self.stride(1),
                                 HEAD_DIM, content_mean.data_ptr(), content_std.data_ptr(), float(eps), a.data_ptr(),
                                 b.data_ptr(), ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "ir_adain_stats_cached")
    return a, b


@_on_tensor_device
def token_stats(x: torch.Tensor, *, heads: int):
    """mean and unbiased std over the token axis of x (B, M, L, H*64) -> two fp32 (B, M, H, 64)
    tensors (``ir_token_stats``)."""
    _need_gpu(x)
    x = _ref(x, heads, "x")
    B, M, Lx, _ = x.shape
    L = _lib.lib()
    nbytes = L.ir_adain_stats_workspace_bytes(B, heads, Lx, M - 1, Lx)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    mean = torch.empty((B, M, heads, HEAD_DIM), dtype=torch.float32, device=x.device)
    std = torch.empty_like(mean)
    rc = L.ir_token_stats(_dtype_code(x), B, heads, M, Lx,
                          x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), HEAD_DIM,
                          mean.data_ptr(), std.data_ptr(), ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "ir_token_stats")
    return mean, std


@_on_tensor_device
def token_stats_weighted(x: torch.Tensor, *, heads: int, weights: Optional[torch.Tensor] = None,
                         lens: Optional[torch.Tensor] = None, return_wsum: bool = False):
    """:func:`token_stats` over weighted or counted tokens (``ir_token_stats_weighted``): the mask-aware AdaIN statistics.

    ``x`` is ``(B, M, L, H*64)`` as for :func:`token_stats`.  ``weights`` is ``(B, M, L)`` fp32 >= 0 (or bool, converted once
    here; a batch dimension of size 1 is shared by the batch), ``lens`` int32 ``(B, M)``: token ``t`` of matrix ``(b, m)`` counts
    with ``w = weights[b, m, t]`` if ``t < lens[b, m]`` and not at all otherwise.  Returns the weighted mean and the unbiased std
    under reliability weights, two fp32 ``(B, M, H, 64)`` tensors (std without eps) - for a 0/1 mask the ``mean(dim=1)`` /
    ``std(dim=1)`` of the kept tokens alone - and with ``return_wsum`` the effective token count ``W`` as fp32 ``(B, M)``.
    A token of weight 0 or behind its count is never used, whatever its bytes; no token gives ``(0, 0)``, one token
    ``(x, 0)``.  With neither ``weights`` nor ``lens`` (or all-ones / ``lens == L``) the bytes of :func:`token_stats`."""
    _need_gpu(x, weights, lens)
    _forward_only(x, weights)
    x = _ref(x, heads, "x")
    B, M, Lx, _ = x.shape
    w_ptr, w_sb, w_sn = None, 0, 0
    if weights is not None:
        if weights.dim() != 3 or tuple(weights.shape[1:]) != (M, Lx) or weights.shape[0] not in (1, B):
            raise ValueError(f"weights: expected ({B}, {M}, {Lx}) (or a batch of 1), got {tuple(weights.shape)}")
        if weights.dtype == torch.bool:
            weights = weights.to(torch.float32)
        if weights.dtype != torch.float32:
            raise TypeError(f"weights must be float32 or bool, got {weights.dtype}")
        if weights.stride(2) != 1 or weights.stride(1) < Lx or weights.stride(0) < 0:
            weights = weights.contiguous()
        w_ptr, w_sn = weights.data_ptr(), weights.stride(1)
        w_sb = 0 if weights.shape[0] == 1 else weights.stride(0)
    l_ptr, ln_sb = None, 0
    if lens is not None:
        if lens.dtype != torch.int32:
            raise TypeError(f"lens must be int32, got {lens.dtype}")
        if tuple(lens.shape) != (B, M):
            raise ValueError(f"lens: expected ({B}, {M}), got {tuple(lens.shape)}")
        if lens.stride(1) != 1 or lens.stride(0) < M:
            lens = lens.contiguous()
        l_ptr, ln_sb = lens.data_ptr(), lens.stride(0)
    L = _lib.lib()
    nbytes = L.ir_token_stats_weighted_workspace_bytes(B, heads, M, Lx)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    mean = torch.empty((B, M, heads, HEAD_DIM), dtype=torch.float32, device=x.device)
    std = torch.empty_like(mean)
    wsum = torch.empty((B, M), dtype=torch.float32, device=x.device) if return_wsum else None
    rc = L.ir_token_stats_weighted(_dtype_code(x), B, heads, M, Lx,
                                   x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), HEAD_DIM,
                                   w_ptr, w_sb, w_sn, l_ptr, ln_sb, mean.data_ptr(), std.data_ptr(),
                                   wsum.data_ptr() if return_wsum else None, ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "ir_token_stats_weighted")
    return (mean, std, wsum) if return_wsum else (mean, std)


@_on_tensor_device
def adain_affine(style, content, *, eps: float = ADAIN_EPS):
    """The AdaIN affine from FINISHED statistics (``ir_adain_affine_from_stats``): ``style = (mean, std)`` of the degraded
    image's V - fp32 ``(B, H, 64)`` (or the ``(B, 1, H, 64)`` that :func:`token_stats` returns for one matrix) - and
    ``content = (mean, std)`` of the reference V's, fp32 ``(B, N, H, 64)``, both std without eps.  Returns ``(a, b)`` in the shape
    :func:`adain_stats` returns; ``token_stats(v_self)`` followed by this gives the bits of :func:`adain_stats_cached`."""
    (s_mean, s_std), (c_mean, c_std) = style, content
    _need_gpu(s_mean, s_std, c_mean, c_std)
    if c_mean.dim() != 4 or c_mean.shape[-1] != HEAD_DIM or c_mean.shape != c_std.shape:
        raise ValueError(f"content statistics must be two (B, N, H, 64) tensors, got {tuple(c_mean.shape)} / {tuple(c_std.shape)}")
    B, N, H, _ = c_mean.shape
    if s_mean.shape != s_std.shape or tuple(s_mean.shape) not in ((B, H, HEAD_DIM), (B, 1, H, HEAD_DIM)):
        raise ValueError(f"style statistics must be two ({B}, {H}, 64) tensors, got {tuple(s_mean.shape)} / {tuple(s_std.shape)}")
    for t in (s_mean, s_std, c_mean, c_std):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("statistics must be contiguous fp32")
    a = torch.empty((B, N, H, HEAD_DIM), dtype=torch.float32, device=c_mean.device)
    b = torch.empty_like(a)
    rc = _lib.lib().ir_adain_affine_from_stats(B, H, N, s_mean.data_ptr(), s_std.data_ptr(), c_mean.data_ptr(), c_std.data_ptr(),
                                               float(eps), a.data_ptr(), b.data_ptr(), _stream())
    _lib.check(rc, "ir_adain_affine_from_stats")
    return a, b


@_on_tensor_device
def adain_apply(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, *, heads: int) -> torch.Tensor:
    """``y = x*a + b`` over (B, N, L, H*64) (``ir_adain_apply``; op-level parity, ``adain()``)."""
    _need_gpu(x, a, b)
    x = _ref(x, heads, "x")
    B, N, Lx, _ = x.shape
    y = torch.empty_like(x, memory_format=torch.contiguous_format)
    rc = _lib.lib().ir_adain_apply(_dtype_code(x), B, heads, N, Lx,
                                   x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), HEAD_DIM,
                                   a.data_ptr(), b.data_ptr(),
                                   y.data_ptr(), y.stride(0), y.stride(1), y.stride(2), HEAD_DIM, _stream())
    _lib.check(rc, "ir_adain_apply")
    return y


def _region_labels(labels, B: int, M: int, Lx: int, n_regions: int):
    """int32 ``(B or 1, M, L)`` labels -> (tensor kept alive, pointer, lb_sb, lb_sn) of the C ABI's label rows"""
    n_regions = int(n_regions)
    if not 1 <= n_regions <= _lib.IR_ADAIN_REGIONS_MAX:
        raise ValueError(f"n_regions must be in [1, {_lib.IR_ADAIN_REGIONS_MAX}], got {n_regions}")
    if labels.dtype != torch.int32:
        raise TypeError(f"labels must be int32, got {labels.dtype}")
    if labels.dim() != 3 or tuple(labels.shape[1:]) != (M, Lx) or labels.shape[0] not in (1, B):
        raise ValueError(f"labels: expected ({B}, {M}, {Lx}) (or a batch of 1), got {tuple(labels.shape)}")
    if labels.stride(2) != 1 or labels.stride(1) < Lx or labels.stride(0) < 0:
        labels = labels.contiguous()
    return labels, labels.data_ptr(), (0 if labels.shape[0] == 1 else labels.stride(0)), labels.stride(1)


@_on_tensor_device
def token_stats_regions(x: torch.Tensor, labels: torch.Tensor, *, heads: int, n_regions: int, return_count: bool = False):
    """:func:`token_stats` per REGION label, every region in one pass over ``x`` (``ir_token_stats_labelled``): the per-region AdaIN
    statistics.

    ``x`` is ``(B, M, L, H*64)`` as for :func:`token_stats`, ``labels`` int32 ``(B, M, L)`` (a batch dimension of size 1 is shared
    by the batch; read in place, so a captured graph follows in-place updates).  Returns the mean and the unbiased std over the
    tokens of every region, two fp32 ``(B, n_regions, M, H, 64)`` tensors (std without eps; region-major, so
    ``(B * n_regions)`` is a batch of :func:`adain_affine`), and with ``return_count`` the token count as fp32
    ``(B, n_regions, M)``.  Region ``r`` holds the bytes of ``token_stats_weighted(x, weights=(labels == r))``.  A token whose
    label lies outside ``[0, n_regions)`` belongs to no region, whatever its bytes; an empty region gives ``(0, 0)`` and count 0,
    one token ``(x, 0)`` and count 1."""
    _need_gpu(x, labels)
    _forward_only(x)
    x = _ref(x, heads, "x")
    B, M, Lx, _ = x.shape
    labels, l_ptr, lb_sb, lb_sn = _region_labels(labels, B, M, Lx, n_regions)
    R = int(n_regions)
    L = _lib.lib()
    nbytes = L.ir_token_stats_labelled_workspace_bytes(B, heads, M, Lx, R)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    mean = torch.empty((B, R, M, heads, HEAD_DIM), dtype=torch.float32, device=x.device)
    std = torch.empty_like(mean)
    count = torch.empty((B, R, M), dtype=torch.float32, device=x.device) if return_count else None
    rc = L.ir_token_stats_labelled(_dtype_code(x), B, heads, M, Lx, R,
                                  x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), HEAD_DIM,
                                  l_ptr, lb_sb, lb_sn, mean.data_ptr(), std.data_ptr(),
                                  count.data_ptr() if return_count else None, ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "ir_token_stats_labelled")
    return (mean, std, count) if return_count else (mean, std)


@_on_tensor_device
def adain_apply_regions(x: torch.Tensor, labels: torch.Tensor, a: torch.Tensor, b: torch.Tensor, *, heads: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``y = x*a + b`` over ``(B, N, L, H*64)`` with the affine chosen PER TOKEN by its label (``ir_adain_apply_labelled``).

    ``a``, ``b``: fp32 ``(B, N, R + 1, H, 64)`` contiguous (:func:`adain_affine_regions`); token ``t`` of reference ``(b, n)`` takes
    slot ``labels[b, n, t]`` if that lies in ``[0, R)`` and slot ``R`` otherwise.  ``labels`` int32 ``(B, N, L)`` (a batch of 1 is
    shared).  ``out``: a ``(B, N, L, H*64)`` view to write (its own strides; a view into a wider buffer keeps the bytes around it),
    ``out is x`` works in place; any other overlap is undefined.  A token of region ``r`` gets the bytes of
    ``adain_apply(x, a[:, :, r], b[:, :, r])``."""
    _need_gpu(x, labels, a, b, out)
    _forward_only(x, a, b)
    if out is not None and out is not x and out.data_ptr() == x.data_ptr() and out.stride() == x.stride():
        out = x
    xin = _ref(x, heads, "x")
    if out is x and xin is not x:
        raise ValueError("adain_apply_regions in place: x must be 16-byte aligned with a contiguous channel axis and strides that are multiples of 8")
    B, N, Lx, _ = xin.shape
    if a.dim() != 5 or a.shape != b.shape or a.shape[0] != B or a.shape[1] != N or tuple(a.shape[3:]) != (heads, HEAD_DIM) or a.shape[2] < 2:
        raise ValueError(f"a, b: expected two ({B}, {N}, R + 1, {heads}, 64) tensors, got {tuple(a.shape)} / {tuple(b.shape)}")
    for t in (a, b):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("a, b must be contiguous fp32")
    R = a.shape[2] - 1
    labels, l_ptr, lb_sb, lb_sn = _region_labels(labels, B, N, Lx, R)
    if out is None:
        y = torch.empty_like(xin, memory_format=torch.contiguous_format)
    else:
        y = xin if out is x else out
        if y.shape != xin.shape or y.dtype != xin.dtype:
            raise ValueError(f"out: expected {tuple(xin.shape)} {xin.dtype}, got {tuple(y.shape)} {y.dtype}")
        if y.stride(-1) != 1 or any(y.stride(i) % 8 for i in range(3)) or y.data_ptr() % 16:
            raise ValueError("out must be 16-byte aligned with a contiguous channel axis and strides that are multiples of 8")
    rc = _lib.lib().ir_adain_apply_labelled(_dtype_code(xin), B, heads, N, Lx, R,
                                           xin.data_ptr(), xin.stride(0), xin.stride(1), xin.stride(2), HEAD_DIM,
                                           l_ptr, lb_sb, lb_sn, a.data_ptr(), b.data_ptr(),
                                           y.data_ptr(), y.stride(0), y.stride(1), y.stride(2), HEAD_DIM, _stream())
    _lib.check(rc, "ir_adain_apply_labelled")
    return y


def adain_affine_regions(style, content, style_global, content_global, *, min_tokens: int = 8, eps: float = ADAIN_EPS):
    """The per-region AdaIN affine table ``(a, b)``, two fp32 ``(B, N, R + 1, H, 64)`` tensors for :func:`adain_apply_regions`.

    ``style = (mean, std, count)`` of ``token_stats_regions(v_self.unsqueeze(1), ...)`` - ``(B, R, 1, H, 64)`` / ``(B, R, 1)`` -
    ``content = (mean, std, count)`` of the references - ``(B, R, N, H, 64)`` / ``(B, R, N)`` - and the globals are what
    :func:`token_stats` gives: ``style_global = (mean, std)`` ``(B, 1, H, 64)``, ``content_global`` ``(B, N, H, 64)``.
    Slot ``(b, n, r)`` uses the regional pair when ``style_count[b, r] >= min_tokens`` AND ``content_count[b, r, n] >= min_tokens``;
    otherwise BOTH sides take the global statistics (a ``torch.where`` on the device, no sync), so a fallen-back slot is the
    ordinary affine bit for bit and an absent region never gives the ``a ~ eps / sigma`` of ``(0, 0)`` statistics.  Slot ``R``
    (tokens of no region) is the ordinary affine.  Two :func:`adain_affine` calls."""
    s_mean, s_std, s_cnt = style
    c_mean, c_std, c_cnt = content
    (sg_mean, sg_std), (cg_mean, cg_std) = style_global, content_global
    if c_mean.dim() != 5 or c_mean.shape != c_std.shape or c_mean.shape[-1] != HEAD_DIM:
        raise ValueError(f"content statistics must be two (B, R, N, H, 64) tensors, got {tuple(c_mean.shape)} / {tuple(c_std.shape)}")
    B, R, N, H, _ = c_mean.shape
    if tuple(s_mean.shape) != (B, R, 1, H, HEAD_DIM) or s_std.shape != s_mean.shape:
        raise ValueError(f"style statistics must be two ({B}, {R}, 1, {H}, 64) tensors, got {tuple(s_mean.shape)} / {tuple(s_std.shape)}")
    if tuple(s_cnt.shape) != (B, R, 1) or tuple(c_cnt.shape) != (B, R, N):
        raise ValueError(f"counts must be ({B}, {R}, 1) and ({B}, {R}, {N}), got {tuple(s_cnt.shape)} / {tuple(c_cnt.shape)}")
    if tuple(cg_mean.shape) != (B, N, H, HEAD_DIM) or cg_std.shape != cg_mean.shape:
        raise ValueError(f"content_global must be two ({B}, {N}, {H}, 64) tensors, got {tuple(cg_mean.shape)} / {tuple(cg_std.shape)}")
    if sg_mean.shape != sg_std.shape or tuple(sg_mean.shape) not in ((B, H, HEAD_DIM), (B, 1, H, HEAD_DIM)):
        raise ValueError(f"style_global must be two ({B}, 1, {H}, 64) tensors, got {tuple(sg_mean.shape)} / {tuple(sg_std.shape)}")
    sg_mean, sg_std = sg_mean.reshape(B, 1, 1, H, HEAD_DIM), sg_std.reshape(B, 1, 1, H, HEAD_DIM)
    regional = ((s_cnt >= min_tokens) & (c_cnt >= min_tokens)).reshape(B, R, N, 1, 1)
    # one (style, content) pair per (b, r, n): the fallback of a slot replaces both of its sides
    pick = lambda reg, glob: torch.where(regional, reg, glob).reshape(B * R * N, H, HEAD_DIM).contiguous()
    st = (pick(s_mean, sg_mean), pick(s_std, sg_std))
    ct = (pick(c_mean, cg_mean.unsqueeze(1)).unsqueeze(1), pick(c_std, cg_std.unsqueeze(1)).unsqueeze(1))
    ar, br = adain_affine(st, ct, eps=eps)                                                          # (B*R*N, 1, H, 64)
    ag, bg = adain_affine((sg_mean.reshape(B, H, HEAD_DIM), sg_std.reshape(B, H, HEAD_DIM)), (cg_mean, cg_std), eps=eps)   # (B, N, H, 64)
    table = lambda reg, glob: torch.cat([reg.reshape(B, R, N, H, HEAD_DIM).permute(0, 2, 1, 3, 4), glob.unsqueeze(2)], dim=2).contiguous()
    return table(ar, ag), table(br, bg)


@_on_tensor_device
def zero_invalid_refs(k: torch.Tensor, v: torch.Tensor, valid_indices: torch.Tensor, *, heads: int) -> None:
    """In place: zero K and V of references ``n >= valid_indices[b]`` (``ir_zero_invalid_refs``;
    pix2pix_turbo.py:269-273 - zeroed, not masked)."""
    _need_gpu(k, v)
    if k.dim() != 4 or k.shape != v.shape or k.stride(-1) != 1 or v.stride(-1) != 1:
        raise ValueError("k, v must be (B, N, L, H*64) views with a contiguous channel axis")
    B, N, L, _ = k.shape
    valid = torch.as_tensor(valid_indices).to(device=k.device, dtype=torch.int32).contiguous()
    if valid.numel() != B:
        raise ValueError("valid_indices must have one entry per batch element")
    rc = _lib.lib().ir_zero_invalid_refs(B, heads, N, L, valid.data_ptr(),
                                         k.data_ptr(), k.stride(0), k.stride(1), k.stride(2), HEAD_DIM,
                                         v.data_ptr(), v.stride(0), v.stride(1), v.stride(2), HEAD_DIM, _stream())
    _lib.check(rc, "ir_zero_invalid_refs")


def _pool_keep(keep: torch.Tensor, B: int, N: int, len_ref: int) -> torch.Tensor:
    """bool ``(B, N, len_ref)`` from ``(B, N, len_ref)`` or ``(B, N, S, S)``: pooled by area to the layer's side, a token kept when
    >= 0.5 of its area is - the rule of :func:`key_bias` for ``ref_token_keep``"""
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool:
        raise ValueError(f"keep must be a bool tensor, got {getattr(keep, 'dtype', type(keep))}")
    if keep.dim() == 4:
        side = int(round(int(len_ref) ** 0.5))
        if keep.shape[:2] != (B, N) or side * side != int(len_ref) or keep.shape[2] != keep.shape[3]:
            raise ValueError(f"keep (B, N, S, S) needs a square layer (len_ref = {len_ref}) and shape ({B}, {N}, S, S), got {tuple(keep.shape)}")
        area = torch.nn.functional.adaptive_avg_pool2d(keep.to(torch.float32), side) if keep.shape[2] != side else keep.to(torch.float32)
        keep = (area >= 0.5).reshape(B, N, side * side)
    if tuple(keep.shape) != (B, N, int(len_ref)):
        raise ValueError(f"keep must have shape (B, N, len_ref) = {(B, N, int(len_ref))} or (B, N, S, S), got {tuple(keep.shape)}")
    return keep


@_on_tensor_device
def compact_refs(ref_k: torch.Tensor, ref_v: torch.Tensor, keep: torch.Tensor, *, heads: int, out=None):
    """Pack the kept tokens of every reference to the front of its segment (``ir_compact_ref_tokens``): returns ``(k, v, ref_lens)``
    - ``k`` / ``v`` of ``ref_k``'s shape whose rows ``0 .. ref_lens[b, n] - 1`` of reference ``(b, n)`` are the kept rows in their
    order (rows behind the count are not written: ``torch.empty`` bytes, or what ``out`` held), and ``ref_lens`` int32 ``(B, N)`` -
    the ``ref_lens`` of :func:`shared_attention`, which then walks the kept keys only.
    ``keep``: bool ``(B, N, len_ref)``, or ``(B, N, S, S)`` pooled as :func:`key_bias` pools ``ref_token_keep``.
    ``out=(k, v, ref_lens)``: refill those buffers (a captured step follows).  One launch, no host sync.  Runs once per identity;
    AdaIN statistics belong to the FULL reference - take them before compacting."""
    _need_gpu(ref_k, ref_v, keep)
    _forward_only(ref_k, ref_v)
    if _is_table(ref_k) or _is_table(ref_v):
        raise TypeError("compact_refs takes dense (B, N, L, C) tensors")
    ref_k, ref_v = _ref(ref_k, heads, "ref_k"), _ref(ref_v, heads, "ref_v")
    if ref_k.shape != ref_v.shape or ref_k.dtype != ref_v.dtype:
        raise ValueError("ref_k / ref_v shape or dtype mismatch")
    B, N, L, _ = ref_k.shape
    mask = _pool_keep(keep, B, N, L).to(torch.uint8).contiguous()
    if out is None:
        k, v = torch.empty_like(ref_k, memory_format=torch.contiguous_format), torch.empty_like(ref_v, memory_format=torch.contiguous_format)
        lens = torch.empty((B, N), dtype=torch.int32, device=ref_k.device)
    else:
        k, v, lens = out
        for t, src in ((k, ref_k), (v, ref_v)):
            if t.shape != src.shape or t.dtype != src.dtype or t.device != src.device or t.stride(-1) != 1 or any(t.stride(i) % 8 for i in range(3)) or t.data_ptr() % 16:
                raise ValueError("out k / v must match ref_k / ref_v in shape, dtype and device, with 16-byte aligned rows")
        if lens.dtype != torch.int32 or tuple(lens.shape) != (B, N) or lens.device != ref_k.device or lens.stride(-1) != 1 or lens.stride(0) < N:
            raise ValueError(f"out ref_lens must be int32 {(B, N)} on {ref_k.device}")
    _lib.check(_lib.lib().ir_compact_ref_tokens(
        _dtype_code(ref_k), B, heads, N, L,
        ref_k.data_ptr(), ref_k.stride(0), ref_k.stride(1), ref_k.stride(2), HEAD_DIM,
        ref_v.data_ptr(), ref_v.stride(0), ref_v.stride(1), ref_v.stride(2), HEAD_DIM,
        mask.data_ptr(),
        k.data_ptr(), k.stride(0), k.stride(1), k.stride(2), HEAD_DIM,
        v.data_ptr(), v.stride(0), v.stride(1), v.stride(2), HEAD_DIM,
        lens.data_ptr(), lens.stride(0), _stream()), "ir_compact_ref_tokens")
    return k, v, lens


@_on_tensor_device
def tensor2im_u8(x: torch.Tensor) -> torch.Tensor:
    """(B, 3, H, W) or (3, H, W) in [-1, 1] -> uint8 (B, H, W, 3) / (H, W, 3) on the device, with the
    exact rounding sequence of the reference's ``tensor2im(var, unnorm=True)`` (vis_utils.py:14-23)."""
    _need_gpu(x)
    squeeze = x.dim() == 3
    if squeeze:
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError("expected (B, C, H, W) or (C, H, W)")
    code = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}.get(x.dtype)
    if code is None:
        raise TypeError(f"tensor2im_u8: unsupported dtype {x.dtype}")
    B, Cc, H, W = x.shape
    out = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=x.device)
    rc = _lib.lib().ir_tensor2im_u8(code, B, Cc, H, W, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2),
                                    x.stride(3), out.data_ptr(), _stream())
    _lib.check(rc, "ir_tensor2im_u8")
    return out[0] if squeeze else out


LIN_AUTO, LIN_X_STATIONARY, LIN_TILED_FIRST = 0, 1, 2   # IR_LIN_* of include/instantrestore_hip.h
LIN_KERNELS = {"auto": 0, "x_stationary": 1, "256x128": 2, "128x128": 3, "128x64": 4, "256x64": 5, "64x128": 6, "128x256": 7, "256x256": 8,
               "128x128k2": 9}   # 9 (round 5): 128 x 128 tile, contraction split over two wave groups (K / 64 even)


def linear_supported(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> bool:
    """shapes / layouts ``ir_linear_fwd`` implements: K % 64 == 0 and N % 64 == 0 (LDS-tiled kernel), or K <= 320 / K = 640
    with N % 32 == 0 (X-stationary kernels)"""
    n, k = weight.shape
    if not (x.is_cuda and weight.dtype in _DT and (x.dtype == weight.dtype or x.dtype == torch.float32) and x.shape[-1] == k
            and weight.stride(1) == 1 and weight.stride(0) % 8 == 0 and x.numel() > 0
            and (bias is None or (bias.dtype == weight.dtype and bias.is_contiguous()))):
        return False
    rows = x.numel() // k
    key = (rows, n, k, bias is None)
    ok = _KERNEL_FOR.get(key)
    if ok is None:      # a pure function of the shape: asked once per shape, not once per launch
        if len(_KERNEL_FOR) > 4096:
            _KERNEL_FOR.clear()
        ok = _KERNEL_FOR[key] = _lib.lib().ir_linear_kernel_for(rows, n, k, 0 if bias is None else 1) >= 0
    return ok


_KERNEL_FOR = {}


def linear_kernel_for(rows: int, n: int, k: int, bias: bool, batch_invariant: bool = False) -> int:
    """IR_LIN_* id of the kernel the automatic choice launches for a shape (-1: unsupported); ``batch_invariant``: the one
    kernel ``linear(..., batch_invariant=True)`` launches for (N, K, bias) at any number of rows"""
    if batch_invariant:
        return int(_lib.lib().ir_linear_kernel_for_ex(int(rows), int(n), int(k), 1 if bias else 0, _lib.IR_LIN_BATCH_INVARIANT))
    return int(_lib.lib().ir_linear_kernel_for(int(rows), int(n), int(k), 1 if bias else 0))


STATS_MAX_CHUNKS = 256   # partials per matrix the merge kernels take (ir_adain_affine_from_partials): 16 384 tokens in 64-row blocks


def linear_stats_rows(rows: int, n: int, k: int, bias: bool) -> int:
    """rows per statistics block of ``linear(..., stats=...)`` for a shape (``ir_linear_stats_rows``); 0: the kernel that
    serves the shape cannot leave statistics behind (``M`` not a multiple of its row block, ``N % 64 != 0``)"""
    return int(_lib.lib().ir_linear_stats_rows(int(rows), int(n), int(k), 1 if bias else 0))


class ColumnStats:
    """partial token statistics of a column range of a projection output, as ``ir_linear_fwd_stats`` leaves them:
    ``ws`` fp32 ``(M / rows, heads, 128)`` = mean[64] | M2[64] per (row block, head); ``rows`` tokens per block"""

    __slots__ = ("ws", "rows", "heads")

    def __init__(self, ws: torch.Tensor, rows: int, heads: int):
        self.ws, self.rows, self.heads = ws, int(rows), int(heads)

    def record_stream(self, stream) -> None:
        self.ws.record_stream(stream)


class RefStatsPartials:
    """AdaIN CONTENT statistics of the reference V's of one layer, still in the form the K/V-capture layer's q/k/v GEMM left
    them in: ``part`` = partials over ``batch * n_refs`` token sets of ``length`` rows.  The shared layer's affine kernel
    merges them directly (one launch per layer instead of a merge on the capture side plus the affine); ``finished()`` gives
    the ``(mean, std)`` pair of ``(B, N, H, 64)`` tensors that a per-identity cache stores.  ``valid``: int32 ``(B,)`` device
    tensor when references ``n >= valid[b]`` were zero-filled by the harvest (statistics (0, 0)), else ``None``."""

    __slots__ = ("part", "batch", "n_refs", "length", "valid", "producer", "_finished")

    def __init__(self, part: ColumnStats, batch: int, n_refs: int, length: int, valid: Optional[torch.Tensor] = None,
                 producer: Optional["torch.cuda.Stream"] = None):
        """``producer``: the HIP stream the capture layer's GEMM wrote the partials on (``AttnProcessor.stream``); a merge
        launched on another stream first waits for everything enqueued there (``finished()`` on the main stream
        could read the partials before the capture stream's GEMM tail had written them when no event was handed over)."""
        self.part, self.batch, self.n_refs, self.length, self.valid = part, int(batch), int(n_refs), int(length), valid
        self.producer = producer
        self._finished = None

    def __setattr__(self, name, value):
        if name == "valid":     # the zero fill changes which references count as all-zero: a cached merge is stale
            object.__setattr__(self, "_finished", None)
        object.__setattr__(self, name, value)

    def record_stream(self, stream) -> None:
        self.part.ws.record_stream(stream)
        if self.valid is not None:
            self.valid.record_stream(stream)

    def sync_to_current(self) -> None:
        """order the current stream behind the partials' producer (no-op on the producer's own stream)"""
        if self.producer is None or not self.part.ws.is_cuda:
            return
        cur = torch.cuda.current_stream(self.part.ws.device)
        if cur != self.producer:
            cur.wait_stream(self.producer)
            self.record_stream(cur)

    def finished(self):
        """``(mean, std)`` of every reference V, fp32 ``(B, N, H, 64)``: merged once, then cached on the object"""
        if self._finished is not None:
            return self._finished
        self.sync_to_current()
        mean, std = token_stats_from_partials(self.part, self.batch * self.n_refs, self.length)
        mean, std = mean.reshape(self.batch, self.n_refs, *mean.shape[-2:]), std.reshape(self.batch, self.n_refs, *std.shape[-2:])
        if self.valid is not None:
            keep = (torch.arange(self.n_refs, device=mean.device)[None, :] < self.valid.reshape(-1, 1)).to(torch.float32)[:, :, None, None]
            mean, std = mean * keep, std * keep
        self._finished = (mean.contiguous(), std.contiguous())
        return self._finished


@_on_tensor_device
def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, scale_cols: int = 0,
           col_scale: float = 1.0, kernel: int = 0, stats: Optional[Tuple[int, int]] = None, batch_invariant: bool = False):
    """``F.linear(x, weight, bias)`` for ``x (..., K)``, 16-bit ``weight (N, K)`` (``ir_linear_fwd_ex``): fp32 accumulation,
    one rounding.  Raises for unsupported shapes.  ``scale_cols`` / ``col_scale``: the first ``scale_cols`` output columns
    are multiplied by ``col_scale`` in fp32 before that rounding.  ``x`` may be fp32: it is rounded to the weight's dtype
    while loaded (the autocast cast, fused).  ``kernel``: ``LIN_KERNELS`` (0 = the library's own choice).

    ``stats=(col0, cols)``: also return the partial token statistics of output columns ``[col0, col0 + cols)`` - whole
    heads - computed by the GEMM's own workgroups from the block they have just stored (``ir_linear_fwd_stats``; the AdaIN
    statistics without a pass over V): the result is ``(y, ColumnStats)``.  Check :func:`linear_stats_rows` first.

    ``batch_invariant`` (ABI v10, ``IR_LIN_BATCH_INVARIANT``): one kernel per (N, K, bias) at every number of rows and no split
    contraction - row ``r`` of ``y`` (and a 64-row statistics block) depends on row ``r`` of ``x``, ``weight`` and ``bias`` only.
    Not combinable with ``kernel``."""
    _need_gpu(x, weight, bias)
    _forward_only(x, weight, bias)
    if batch_invariant:
        if kernel:
            raise ValueError("batch_invariant: the kernel choice is the library's (kernel=0)")
        kernel = _lib.IR_LIN_BATCH_INVARIANT
    n, k = weight.shape
    x2 = x.reshape(-1, k)
    if x2.stride(1) != 1 or x2.stride(0) % 8 != 0:
        x2 = x2.contiguous()
    y = torch.empty((x2.shape[0], n), dtype=weight.dtype, device=x.device)
    if stats is not None:
        if kernel and not batch_invariant:
            raise ValueError("stats: the kernel choice is the library's (kernel=0)")
        col0, cols = int(stats[0]), int(stats[1])
        rows = linear_stats_rows(x2.shape[0], n, k, bias is not None)
        if rows <= 0 or cols <= 0 or cols % HEAD_DIM or col0 % HEAD_DIM:
            raise ValueError(f"linear(stats=...): shape ({x2.shape[0]}, {n}, {k}) / columns ({col0}, {cols}) cannot carry the statistics tail")
        ws = torch.empty((x2.shape[0] // rows, cols // HEAD_DIM, 128), dtype=torch.float32, device=x.device)
        if batch_invariant:
            rc = _lib.lib().ir_linear_fwd_stats_ex(_dtype_code(weight), 1 if x.dtype == torch.float32 else 0, x2.shape[0], n, k,
                                                   x2.data_ptr(), x2.stride(0), weight.data_ptr(), weight.stride(0),
                                                   None if bias is None else bias.data_ptr(), y.data_ptr(), n, int(scale_cols),
                                                   float(col_scale), col0, cols, ws.data_ptr(), ws.numel() * 4, int(kernel), _stream())
            _lib.check(rc, "ir_linear_fwd_stats_ex")
            return y.view(*x.shape[:-1], n), ColumnStats(ws, rows, cols // HEAD_DIM)
        rc = _lib.lib().ir_linear_fwd_stats(_dtype_code(weight), 1 if x.dtype == torch.float32 else 0, x2.shape[0], n, k, x2.data_ptr(),
                                            x2.stride(0), weight.data_ptr(), weight.stride(0),
                                            None if bias is None else bias.data_ptr(), y.data_ptr(), n, int(scale_cols),
                                            float(col_scale), col0, cols, ws.data_ptr(), ws.numel() * 4, _stream())
        _lib.check(rc, "ir_linear_fwd_stats")
        return y.view(*x.shape[:-1], n), ColumnStats(ws, rows, cols // HEAD_DIM)
    rc = _lib.lib().ir_linear_fwd_ex(_dtype_code(weight), 1 if x.dtype == torch.float32 else 0, x2.shape[0], n, k, x2.data_ptr(), x2.stride(0), weight.data_ptr(),
                                     weight.stride(0), None if bias is None else bias.data_ptr(), y.data_ptr(), n,
                                     int(scale_cols), float(col_scale), int(kernel), _stream())
    _lib.check(rc, "ir_linear_fwd_ex")
    return y.view(*x.shape[:-1], n)


@_on_tensor_device
def adain_affine_from_partials(style: ColumnStats, batch: int, len_self: int, n_refs: int, len_ref: int, *,
                               content: Optional[ColumnStats] = None, content_mean: Optional[torch.Tensor] = None,
                               content_std: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None,
                               eps: float = ADAIN_EPS):
    """The AdaIN affine ``(a, b)`` of :func:`adain_stats` from the partials the projections left behind
    (``ir_adain_affine_from_partials``): ``style`` from the shared layer's q/k/v GEMM over ``batch`` sets of ``len_self``
    tokens; the content statistics either as the K/V-capture layer's partials (``content``, ``batch * n_refs`` sets of
    ``len_ref`` tokens) or finished (``content_mean`` / ``content_std``, fp32 ``(B, N, H, 64)``).  ``valid``: int32 ``(B)``
    on the device, references ``n >= valid[b]`` count as zero-filled."""
    H = style.heads
    dev = style.ws.device
    if (content is None) == (content_mean is None or content_std is None):
        raise ValueError("content statistics: either `content` partials or content_mean + content_std")
    if content is not None and content.heads != H:
        raise ValueError("style / content head counts differ")
    for t in (content_mean, content_std):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (batch, n_refs, H, HEAD_DIM)):
            raise ValueError(f"content statistics must be contiguous fp32 ({batch}, {n_refs}, {H}, 64)")
    if style.ws.shape[0] * style.rows != batch * len_self or (content is not None and content.ws.shape[0] * content.rows != batch * n_refs * len_ref):
        raise ValueError("partials do not cover batch x len rows")
    if valid is not None and (valid.dtype != torch.int32 or valid.device != dev or valid.numel() != batch or not valid.is_contiguous()):
        raise ValueError(f"valid must be a contiguous int32 ({batch},) tensor on {dev}")
    a = torch.empty((batch, n_refs, H, HEAD_DIM), dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    rc = _lib.lib().ir_adain_affine_from_partials(
        batch, H, n_refs, len_self, len_ref, style.ws.data_ptr(), style.rows,
        None if content is None else content.ws.data_ptr(), 0 if content is None else content.rows,
        None if content_mean is None else content_mean.data_ptr(), None if content_std is None else content_std.data_ptr(),
        None if valid is None else valid.data_ptr(), float(eps), a.data_ptr(), b.data_ptr(), _stream())
    _lib.check(rc, "ir_adain_affine_from_partials")
    return a, b


@_on_tensor_device
def token_stats_from_partials(part: ColumnStats, n_sets: int, length: int):
    """mean and unbiased std over the tokens of ``n_sets`` matrices of ``length`` rows from their partials
    (``ir_token_stats_from_partials``): two fp32 ``(n_sets, H, 64)`` tensors, what :func:`token_stats` returns per matrix"""
    if part.ws.shape[0] * part.rows != n_sets * length:
        raise ValueError("partials do not cover n_sets x length rows")
    mean = torch.empty((n_sets, part.heads, HEAD_DIM), dtype=torch.float32, device=part.ws.device)
    std = torch.empty_like(mean)
    rc = _lib.lib().ir_token_stats_from_partials(n_sets, part.heads, length, part.ws.data_ptr(), part.rows, mean.data_ptr(),
                                                 std.data_ptr(), _stream())
    _lib.check(rc, "ir_token_stats_from_partials")
    return mean, std


_ANY_DT = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}


@_on_tensor_device
def freeu_fourier_filter(x: torch.Tensor, threshold: int, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FreeU's skip-feature filter on (B, C, H, W) (``ir_freeu_fourier_filter``; replaces
    ``fourier_filter(x.float(), threshold, scale).to(x.dtype)``, block.py:3514,3518).  Result has
    ``x``'s dtype; ``out=x`` filters in place."""
    _need_gpu(x, out)
    if x.dim() != 4:
        raise ValueError("expected (B, C, H, W)")
    code = _ANY_DT.get(x.dtype)
    if code is None:
        raise TypeError(f"freeu_fourier_filter: unsupported dtype {x.dtype}")
    B, Cc, H, W = x.shape
    if not (x.stride(3) == 1 and x.stride(2) == W and (B == 1 or x.stride(0) == Cc * x.stride(1))):
        x = x.contiguous()
    if out is None:
        out = torch.empty((B, Cc, H, W), dtype=x.dtype, device=x.device)
    elif out.shape != x.shape or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor of x's shape and dtype")
    rc = _lib.lib().ir_freeu_fourier_filter(code, B * Cc, H, W, x.data_ptr(), x.stride(1), out.data_ptr(), H * W,
                                            int(threshold), float(scale), _stream())
    _lib.check(rc, "ir_freeu_fourier_filter")
    return out


def lanczos_coeffs(in_size: int, out_size: int):
    """Pillow's LANCZOS tap tables for one axis, computed on the host by the library
    (``ir_lanczos_coeffs``): ``(bounds (out, 2) int32, kk (out, ksize) int32)`` CPU tensors."""
    L = _lib.lib()
    ksize = L.ir_lanczos_ksize(int(in_size), int(out_size))
    if ksize <= 0:
        _lib.check(ksize, "ir_lanczos_ksize")
    bounds = torch.empty((out_size, 2), dtype=torch.int32)
    kk = torch.empty((out_size, ksize), dtype=torch.int32)
    _lib.check(L.ir_lanczos_coeffs(int(in_size), int(out_size), bounds.data_ptr(), kk.data_ptr()), "ir_lanczos_coeffs")
    return bounds, kk


def preprocess_lanczos(descs, size: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """Launch ``ir_preprocess_lanczos_u8`` over a ctypes array of ``_lib.ImageDesc`` (built by
    ``instantrestore_amd.preprocess``); returns ``(n, 3, size, size)`` in ``dtype``."""
    code = _ANY_DT.get(dtype)
    if code is None:
        raise TypeError(f"preprocess: unsupported output dtype {dtype}")
    n = len(descs)
    with torch.cuda.device(device):
        out = torch.empty((n, 3, size, size), dtype=dtype, device=device)
        rc = _lib.lib().ir_preprocess_lanczos_u8(descs, n, int(size), code, out.data_ptr(), _stream())
    _lib.check(rc, "ir_preprocess_lanczos_u8")
    return out


_TUNING = int(os.environ.get("IR_ATTN_VARIANT", "0") or 0)


def tuning_supports_prescaled_q() -> bool:
    """``IR_FLAG_Q_PRESCALED`` is implemented by the default dispatch and by the kernels it picks from (tuning 0, 11, 13, 16, 18;
    the development build's ablations 20-28 take the flag explicitly); under any other A/B ``tuning`` the processors keep the plain q (the C ABI rejects the combination)"""
    return _TUNING in (0, 11, 13, 16, 18)


def set_attn_variant(variant: int) -> int:
    """tuning hook for benchmarks / A-B tests: the value goes into the per-call ``tuning`` field of the C ABI's
    argument block (``IR_TUNE_*`` in include/instantrestore_hip.h; 0 = default dispatch, 16 = 128-row kernel (one wave per SIMD; pre-scaled Q only), 13 / 12 = 64-row kernel in 8- / 4-wave workgroups, 10 / 14 = pipelined 32-row kernel, 11 = its
    pre-scaled-Q form).  ``IR_ATTN_VARIANT=<n>`` in the environment sets the initial value.  Returns the previous one.
    The C library itself holds no such state."""
    global _TUNING
    prev, _TUNING = _TUNING, int(variant)
    return prev
