"""The read-out kernels (attn_probs.hip, attn_rows.hip, attn_match.hip) take their QK block from csrc/ir_readout.h: the lane map
and the probability expression that hold the three bit for bit to each other exist once.  Pure text, no build."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parent.parent / "instantrestore_amd" / "csrc"
READOUTS = ("attn_probs.hip", "attn_rows.hip", "attn_match.hip")
INCLUDE = re.compile(r'#include\s+"ir_readout\.h"')


def _text(name):
    return (CSRC / name).read_text()


def test_keymap_is_defined_in_the_header_only():
    assert "int keymap(" in _text("ir_readout.h")
    for name in READOUTS:
        assert "int keymap(" not in _text(name), name


def test_probability_expression_is_in_the_header_only():
    pat = re.compile(r"__builtin_fmaf\([^;]*scale_log2")
    assert pat.search(_text("ir_readout.h"))
    for name in READOUTS:
        assert not pat.search(_text(name)), name


def test_every_readout_includes_the_header():
    for name in READOUTS:
        assert INCLUDE.search(_text(name)), name


def test_no_forward_kernel_includes_the_header():
    forward = sorted(CSRC.glob("shared_attn_fwd*")) + sorted((CSRC / "w128").glob("*"))
    assert len([f for f in forward if f.name.startswith("shared_attn_fwd")]) >= 8
    for f in forward:
        if f.is_file() and f.suffix != ".pyc":
            assert "ir_readout.h" not in f.read_text(errors="replace"), f.name
