"""The segment-span limit of the attention forward (include/instantrestore_hip.h, ``IR_ATTN_SEG_BYTES_MAX``), without a GPU.

The forward kernels walk one (b, segment, head) of K or V through a buffer descriptor and form its byte offsets in ``int``.  The
largest of them is the offset of the tile behind the segment's last whole 64-key tile, ``64 * ceil(len / 64) * row_stride * 2``,
and one 128-byte head row behind it bounds the descriptor's ``(len - 1) * row_stride * 2 + 128`` as well, so the rule is

    64 * ceil(len / 64) * row_stride * 2 + 128  <=  2**31 - 1.

The addresses below are never dereferenced: the smallest refused stride and the largest accepted one are told apart by the
host-only ``ir_shared_attn_kernel_name`` first, and only the REFUSED call is then handed to the launching entry points."""
import ctypes as C

import pytest

from test_ref_table_cpu import _args

UNSUPPORTED = -2
LIMIT = 2 ** 31 - 1
LENGTHS = [1, 64, 72, 300, 4096, 65536]      # one row, a whole tile, ragged tiles, the 64x64- and 256x256-token layers
FIELDS = ["ks_sl", "vs_sl", "kr_sl", "vr_sl"]


def _padded_span(length, stride):
    """the bytes the rule bounds: the segment's whole 64-key tiles and one head row"""
    return 64 * ((length + 63) // 64) * stride * 2 + 128


def _edge(length):
    """(largest accepted, smallest refused) row stride in elements: neighbouring multiples of 8, worked out from the rule alone"""
    most = (LIMIT - 128) // (64 * ((length + 63) // 64) * 2) // 8 * 8
    assert _padded_span(length, most) <= LIMIT < _padded_span(length, most + 8)
    return most, most + 8


def _call(lib_mod, table, field, length, stride):
    a = _args(lib_mod, table=table, L=64)
    if field in ("ks_sl", "vs_sl"):
        a.len_self = length
    else:
        a.len_ref = length
    setattr(a, field, stride)
    return a


@pytest.mark.parametrize("table", [False, True], ids=["dense", "tables"])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("length", LENGTHS)
def test_the_largest_accepted_and_the_smallest_refused_stride(length, field, table):
    from instantrestore_amd import _lib
    lib = _lib.lib()
    most, over = _edge(length)
    ok, bad = _call(_lib, table, field, length, most), _call(_lib, table, field, length, over)
    name = lib.ir_shared_attn_kernel_name(C.byref(ok))
    assert name != b"", lib.ir_last_error_string()
    assert name == lib.ir_shared_attn_kernel_name(C.byref(_call(_lib, table, field, length, 64)))       # the stride picks no kernel
    assert lib.ir_shared_attn_kernel_name(C.byref(bad)) == b""
    msg = lib.ir_last_error_string().decode()
    assert f"{field} {over}" in msg and str(LIMIT) in msg and f"at most {most} elements" in msg, msg
    # the descriptor's own span, as the issue of the limit states it
    assert (length - 1) * most * 2 + 128 <= LIMIT
    # only now the launching entry points, on the refused call alone: they return before any launch
    ms = C.c_float(0)
    assert lib.ir_shared_attn_fwd(C.byref(bad), None) == UNSUPPORTED and field in lib.ir_last_error_string().decode()
    assert lib.ir_time_shared_attn_fwd(C.byref(bad), 1, None, C.byref(ms)) == UNSUPPORTED
    assert lib.ir_shared_attn_workspace_bytes_for(C.byref(bad)) == 0
    bad.flags |= _lib.IR_FLAG_BATCH_INVARIANT
    plan = _lib.SharedAttnPlan()
    plan.struct_size = C.sizeof(plan)
    assert lib.ir_shared_attn_plan(C.byref(bad), C.byref(plan)) == UNSUPPORTED
    ok.flags |= _lib.IR_FLAG_BATCH_INVARIANT
    assert lib.ir_shared_attn_plan(C.byref(ok), C.byref(plan)) == 0


def test_a_segment_that_the_call_does_not_use_is_not_measured():
    """ks_sl / vs_sl without IR_FLAG_INCLUDE_SELF and kr_sl / vr_sl without references are never walked"""
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a = _args(_lib, table=False, flags=0)
    a.ks_sl = a.vs_sl = 1 << 40
    assert lib.ir_shared_attn_kernel_name(C.byref(a)) != b"", lib.ir_last_error_string()
    a = _args(_lib, table=False, N=0)
    a.n_refs = a.len_ref = 0
    a.k_ref = a.v_ref = None
    a.kr_sb = a.kr_sn = a.vr_sb = a.vr_sn = 0
    a.kr_sl = a.vr_sl = 1 << 40
    assert lib.ir_shared_attn_kernel_name(C.byref(a)) != b"", lib.ir_last_error_string()


def test_batch_reference_and_head_strides_are_not_limited():
    from instantrestore_amd import _lib
    lib = _lib.lib()
    a = _args(_lib, table=False)
    for f in ("q_sb", "ks_sb", "vs_sb", "o_sb", "kr_sb", "vr_sb", "kr_sn", "vr_sn", "q_sh", "ks_sh", "vs_sh", "kr_sh", "vr_sh", "o_sh",
              "q_sl", "o_sl"):                  # ... and the row strides of q and out, which no descriptor walks
        setattr(a, f, (1 << 40) + 8)
    assert lib.ir_shared_attn_kernel_name(C.byref(a)) != b"", lib.ir_last_error_string()
