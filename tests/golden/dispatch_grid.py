"""The grid of calls whose dispatch tests/golden/dispatch_golden.npz pins (make_golden_dispatch.py writes it from the library
of the commit before the dispatch became one function; tests/test_dispatch_golden_cpu.py replays it).  Host only: every
pointer field points into one host buffer that is never read.

Run as a script it prints, as JSON, ``[kernel name, error text]`` of every call of the grid, in grid order, for the library that
``IR_LIB_PATH`` names (default: the built one).  ``IR_ATTN_W128`` is read once per process, so each of its settings needs a
process of its own."""
import ctypes as C
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BATCHES = (1, 8, 32)
SHAPES = ((256, 20), (1024, 10), (4096, 5), (4096, 10), (16384, 5))   # (Lq, heads)
N_REFS = (0, 4)
TUNINGS = (0, 1, 5, 7, 10, 11, 12, 13, 14, 16, 18)
W128_ENV = (None, "0", "1")   # IR_ATTN_W128 of the three recordings
FLAGS = tuple(itertools.product((False, True), repeat=5))   # include_self, AdaIN, pre-scaled, valid_refs, seg_mass


def grid():
    """(B, Lq, H, N, len_ref, (inc, adain, presc, valid, mass), tuning, batch_invariant); the flag with tuning 0 only"""
    for B, (L, H), N, short, fl in itertools.product(BATCHES, SHAPES, N_REFS, (0, 8), FLAGS):
        for tuning in TUNINGS:
            yield B, L, H, N, L - short, fl, tuning, False
        yield B, L, H, N, L - short, fl, 0, True


def make_args(_lib, ptr, B, L, H, N, len_ref, fl, tuning, bi):
    inc, adain, presc, valid, mass = fl
    a = _lib.SharedAttnArgs()
    a.struct_size = C.sizeof(a)
    a.dtype, a.batch, a.heads, a.len_q, a.scale = 1, B, H, L, 0.125
    a.flags = (_lib.IR_FLAG_INCLUDE_SELF if inc else 0) | (_lib.IR_FLAG_Q_PRESCALED if presc else 0) | \
              (_lib.IR_FLAG_BATCH_INVARIANT if bi else 0)
    a.tuning = tuning
    ch = H * 64
    a.q = a.out = a.workspace = ptr
    a.workspace_bytes = 1 << 26
    a.q_sb = a.o_sb = L * ch
    a.q_sl = a.o_sl = ch
    a.q_sh = a.o_sh = 64
    if inc:
        a.len_self = L
        a.k_self = a.v_self = ptr
        a.ks_sb = a.vs_sb = L * ch
        a.ks_sl = a.vs_sl = ch
        a.ks_sh = a.vs_sh = 64
    a.n_refs, a.len_ref = N, len_ref
    if N > 0:
        a.k_ref = a.v_ref = ptr
        a.kr_sb = a.vr_sb = N * len_ref * ch
        a.kr_sn = a.vr_sn = len_ref * ch
        a.kr_sl = a.vr_sl = ch
        a.kr_sh = a.vr_sh = 64
    if adain:
        a.adain_a = a.adain_b = ptr
    if valid:
        a.valid_refs = ptr
    if mass:
        a.seg_mass = ptr
    return a


def record():
    """[name, error text] per grid entry; the error text (ir_last_error_string) only where the name is empty: a refused call"""
    sys.path.insert(0, REPO)
    from instantrestore_amd import _lib
    lib = _lib.lib()
    buf = (C.c_char * 4096)()
    ptr = C.cast(C.byref(buf, 64 - C.addressof(buf) % 64), C.c_void_p)
    out = []
    for entry in grid():
        name = lib.ir_shared_attn_kernel_name(C.byref(make_args(_lib, ptr, *entry))).decode()
        out.append([name, "" if name else lib.ir_last_error_string().decode()])
    return out


def record_in_children(lib_path=None):
    """the whole grid in three fresh child processes: IR_ATTN_W128 unset, 0, 1"""
    import subprocess
    res = []
    for w128 in W128_ENV:
        env = dict(os.environ)
        for k in ("IR_ATTN_W128", "IR_ATTN_VARIANT", "IR_ATTN_FORCE_SPLIT"):
            env.pop(k, None)
        if w128 is not None:
            env["IR_ATTN_W128"] = w128
        if lib_path is not None:
            env["IR_LIB_PATH"] = lib_path
        r = subprocess.run([sys.executable, "-B", os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res.append(json.loads(r.stdout))
    return res


if __name__ == "__main__":
    print(json.dumps(record()))
