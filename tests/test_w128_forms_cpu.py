"""The 128-row kernel's valid_refs / seg_mass forms, as the C ABI reports them (CPU-only box: kernel names, no launch).

``ir_shared_attn_kernel_name`` runs the parameter checks of a launch (``build_attn_params``: alignment, strides, lengths - it
only copies the pointers, never reads through them) and restates the dispatch.  Held to: IR_TUNE_W128 takes ``valid_refs`` and
``seg_mass`` and says so in the name; the default rule keeps such calls on the 64-row kernel at cfg 2's top layer (the outputs
of existing callers keep their bits); ``IR_ATTN_W128=1`` - read once per process, so a fresh child - sends them to the 128-row
kernel."""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W128, W64 = "shared_attn_fwd_w128_kernel", "shared_attn_fwd_w64_kernel<64 rows/wave, 8 waves"

_BUF = (C.c_char * 4096)()   # host memory for the pointer fields: 64-byte aligned, never dereferenced


def _args(B, H, L, N, *, inc=True, adain=True, tuning=0, valid=False, mass=False, Lr=None):
    from instantrestore_amd import _lib
    Lr = L if Lr is None else Lr
    ptr = C.cast(C.byref(_BUF, 64 - C.addressof(_BUF) % 64), C.c_void_p)
    a = _lib.SharedAttnArgs()
    a.struct_size = C.sizeof(a)
    a.dtype, a.batch, a.heads, a.len_q, a.scale = 1, B, H, L, 0.125
    a.flags = (_lib.IR_FLAG_INCLUDE_SELF if inc else 0) | _lib.IR_FLAG_Q_PRESCALED
    a.tuning = tuning
    C_ = H * 64
    a.q = a.out = ptr
    a.q_sb = a.o_sb = L * C_
    a.q_sl = a.o_sl = C_
    a.q_sh = a.o_sh = 64
    if inc:
        a.len_self = L
        a.k_self = a.v_self = ptr
        a.ks_sb = a.vs_sb = L * C_
        a.ks_sl = a.vs_sl = C_
        a.ks_sh = a.vs_sh = 64
    a.n_refs, a.len_ref = N, Lr
    a.k_ref = a.v_ref = ptr
    a.kr_sb = a.vr_sb = N * Lr * C_
    a.kr_sn = a.vr_sn = Lr * C_
    a.kr_sl = a.vr_sl = C_
    a.kr_sh = a.vr_sh = 64
    if adain:
        a.adain_a = a.adain_b = ptr
    if valid:
        a.valid_refs = ptr
    if mass:
        a.seg_mass = ptr
    return a


def _name(**kw):
    from instantrestore_amd import _lib
    return _lib.lib().ir_shared_attn_kernel_name(C.byref(_args(**kw))).decode()


CFG2_TOP = dict(B=8, H=5, L=4096, N=4)      # cfg 2's top layer: 64x64 tokens, four references


def test_tuning_16_takes_valid_refs_and_seg_mass():
    for adain in (False, True):
        fold = "AdaIN ratio-frame fold" in _name(**CFG2_TOP, adain=adain, tuning=16)
        assert fold == adain
        n = _name(**CFG2_TOP, adain=adain, tuning=16, valid=True)
        assert n.startswith(W128) and "zero suffix in closed form" in n and "segment masses" not in n, n
        assert ("AdaIN ratio-frame fold" in n) == adain
        n = _name(**CFG2_TOP, adain=adain, tuning=16, mass=True)
        assert n.startswith(W128) and "segment masses" in n and "zero suffix" not in n, n
        n = _name(**CFG2_TOP, adain=adain, tuning=16, valid=True, mass=True)
        assert n.startswith(W128) and "zero suffix in closed form" in n and "segment masses" in n, n
    # without the self segment, and at the 32x32-token class
    assert "zero suffix" in _name(B=2, H=10, L=1024, N=4, inc=False, tuning=16, valid=True)
    # the plain call keeps its name
    plain = _name(**CFG2_TOP, tuning=16)
    assert plain.startswith(W128) and "zero suffix" not in plain and "segment masses" not in plain


def test_tuning_16_still_refuses_ragged_segments():
    from instantrestore_amd import _lib
    assert _name(B=1, H=1, L=4096, N=2, Lr=4000, tuning=16, valid=True) == ""
    assert b"multiples of 64" in _lib.lib().ir_last_error_string()


def test_default_rule_keeps_these_calls_on_the_64_row_kernel():
    if os.environ.get("IR_ATTN_W128") is not None:   # the variable overrides the rule under test
        return
    assert _name(**CFG2_TOP).startswith(W128)              # the plain call: the 128-row kernel, as before
    for kw in (dict(valid=True), dict(mass=True), dict(valid=True, mass=True)):
        for adain in (False, True):
            n = _name(**CFG2_TOP, adain=adain, **kw)
            assert n.startswith(W64), (kw, n)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_w128_forms_cpu as T
for kw in (dict(valid=True), dict(mass=True), dict(valid=True, mass=True)):
    print(T._name(**T.CFG2_TOP, **kw))
    print(T._name(B=2, H=10, L=1024, N=4, **kw))
"""


def test_env_override_sends_them_to_the_128_row_kernel():
    env = dict(os.environ, IR_ATTN_W128="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    names = r.stdout.strip().splitlines()
    assert len(names) == 6
    for i, n in enumerate(names):
        assert n.startswith(W128), n
        assert ("zero suffix in closed form" in n) == (i // 2 != 1)
        assert ("segment masses" in n) == (i // 2 != 0)


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_forms_object_keeps_the_compiler_out_of_the_accumulator_registers(tmp_path):
    """the rule tests/test_build_guards.py holds shared_attn_fwd_w128.hip to, for the FORMS instantiations in their own object: no
    compiler-generated v_accvgpr_* / AGPR operand outside the asm blocks, no scratch, no VGPR spill, 256 AGPRs"""
    import re
    if not os.path.exists(HIPCC):
        import pytest
        pytest.skip("needs hipcc")
    out = tmp_path / "forms.s"
    src = os.path.join(REPO, "instantrestore_amd", "csrc", "shared_attn_fwd_w128_forms.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), src],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    inasm, cur, bad, kernels = False, None, [], set()
    for line in open(out):
        m = re.match(r"^(_ZN\S*shared_attn_fwd_w128_kernel\S*):", line)
        if m:
            cur = m.group(1)
            kernels.add(cur)
        if ";;#ASMSTART" in line:
            inasm = True
            continue
        if ";;#ASMEND" in line:
            inasm = False
            continue
        code = line.split(";")[0]
        if cur and not inasm and (re.search(r"v_accvgpr|\ba\d+\b|a\[\d+", code) or "scratch_" in code):
            bad.append((cur[-30:], line.strip()))
    text = open(out).read()
    assert len(kernels) == 4 and all(k.endswith("Lb1EEEv11AttnKParams") for k in kernels), kernels   # bf16 / f16 x fold / plain, FORMS
    assert not bad, bad[:10]
    assert text.count(".vgpr_spill_count: 0") == 4 and text.count(".agpr_count:     256") == 4
    assert text.count(".private_segment_fixed_size: 0") >= 4
