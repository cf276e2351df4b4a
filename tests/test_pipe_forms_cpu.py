"""The 32-row attention kernel (csrc/shared_attn_fwd_pipe.hip) names its forms - FormExact ... FormPostCheck, WithKeyBias,
WithRefCounts - and holds no experiment path: round 1's `ABL` bit mask, the register-staging, builtin-DMA and straight-schedule
branches and their tuning values 3, 4, 6, 9 are gone.  Pure text, plus one check through the built library: the kernel-name strings
of every 32-row tuning value are the ones the build before that change printed."""
import ctypes as C
import pathlib
import re

import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
CSRC = REPO / "instantrestore_amd" / "csrc"
TUNINGS = (7, 10, 11, 14, 18, 0)
KINDS = ("plain", "prescaled", "key_bias", "ref_lens")

# ir_shared_attn_kernel_name of a 650-row call (B 2, H 2, self block + 2 references of 650 keys, bf16), recorded from the build of
# the commit before the forms were named; "" = the call is refused
_P = "shared_attn_fwd_pipe_kernel<4 waves, "
_EQK, _PRQ, _PRK = _P + "lazy max, early QK", _P + "lazy max, pre-scaled Q", _P + "lazy max, pre-scaled Q (Q rounded in the kernel)"
_B, _R = ", key bias (reference follows every max)>", ", ragged refs (per-reference counts)>"
RECORDED = {
    "plain": {7: _P + "exact rescale>", 10: _P + "lazy max>", 11: _PRK + ">", 14: _EQK + ">", 18: "", 0: _EQK + ">"},
    "prescaled": {7: "", 10: "", 11: _PRQ + ">", 14: "", 18: _P + "pre-scaled Q, reference checked after the exponentials>", 0: _PRQ + ">"},
    "key_bias": {7: "", 10: "", 11: _PRK + _B, 14: _EQK + _B, 18: "", 0: _EQK + _B},
    "ref_lens": {7: "", 10: "", 11: _PRK + _R, 14: _EQK + _R, 18: "", 0: _EQK + _R},
}


def _call(lib_mod, kind, tuning, L=650, B=2, H=2, N=2):
    """a valid self + N-reference call on addresses that are never dereferenced (the name is formed before any launch)"""
    a = lib_mod.SharedAttnRaggedArgs()
    a.struct_size = C.sizeof(a)
    c = 64 * H
    a.dtype, a.batch, a.heads, a.len_q, a.len_self, a.scale, a.tuning = 1, B, H, L, L, 0.125, tuning
    a.flags = 1 | (2 if kind == "prescaled" else 0)
    a.q = a.out = a.k_self = a.v_self = a.k_ref = a.v_ref = 4096
    a.q_sb = a.o_sb = a.ks_sb = a.vs_sb = L * c
    a.q_sl = a.o_sl = a.ks_sl = a.vs_sl = a.kr_sl = a.vr_sl = c
    a.q_sh = a.o_sh = a.ks_sh = a.vs_sh = a.kr_sh = a.vr_sh = 64
    a.n_refs, a.len_ref = N, L
    a.kr_sb = a.vr_sb = N * L * c
    a.kr_sn = a.vr_sn = L * c
    if kind == "key_bias":
        a.key_bias, a.kb_sb = 4100, (1 + N) * L
    if kind == "ref_lens":
        a.ref_lens, a.rl_sb = 4100, N
    return a


def names(lib_mod):
    lib = lib_mod.lib()
    return {kind: {t: lib.ir_shared_attn_kernel_name(C.byref(_call(lib_mod, kind, t))).decode() for t in TUNINGS} for kind in KINDS}


def test_the_kernel_source_selects_by_name_and_holds_no_experiment_path():
    text = (CSRC / "shared_attn_fwd_pipe.hip").read_text()
    for gone in ("ABL", "kreg", "stage_write", "issue_loads", "NOPIPE"):
        assert gone not in text, gone
    for form in ("FormExact", "FormLazy", "FormPresc", "FormEarlyQK", "FormPostCheck", "WithKeyBias", "WithRefCounts"):
        assert len(re.findall(r"\bstruct %s\b" % form, text)) == 1, form
    assert "IR_PIPE_DEV_" not in (CSRC / "ir_kernels.h").read_text()


@pytest.mark.parametrize("tuning", [3, 4, 6, 9])
def test_the_retired_tuning_values_are_refused(tuning):
    from instantrestore_amd import _lib
    for kind in KINDS:
        assert _lib.lib().ir_shared_attn_kernel_name(C.byref(_call(_lib, kind, tuning))) == b"", (kind, tuning)


def test_the_name_strings_are_the_recorded_ones():
    from instantrestore_amd import _lib
    got = names(_lib)
    assert got == RECORDED
    assert sum(1 for kind in KINDS for t in TUNINGS if got[kind][t]) == 14   # (the refusals among them are recorded too, not the subject)


if __name__ == "__main__":   # prints what the loaded build (IR_LIB_PATH) names: how RECORDED was taken
    import pprint
    import sys
    sys.path.insert(0, str(REPO))
    from instantrestore_amd import _lib
    pprint.pprint(names(_lib), width=200)
