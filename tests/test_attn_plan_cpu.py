"""The work plan of the attention forward (instantrestore_amd/csrc/ir_attn_plan.h) pinned by literals.

The header is plain C++17 with nothing of HIP in it: a stand-alone program that includes it alone is built with the host compiler
(once more under -fsanitize=address,undefined) and prints the plan of each row below.  The expected numbers were derived by hand
from the formulas the three kernel launchers carried before they shared this header.  Workspace: 69,206,016 B
(ir_shared_attn_workspace_bytes()) unless the row says otherwise."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "instantrestore_amd", "csrc")
WS = 69206016

PROGRAM = r"""
#include "ir_attn_plan.h"
#include <stdio.h>
// stands in for the float pointers of the kernel argument block: an offset in floats from the workspace's start, or null
struct Ptr {
  long off;
  Ptr(decltype(nullptr) = nullptr) : off(-1) {}
  explicit Ptr(long o) : off(o) {}
  Ptr operator+(size_t n) const { return Ptr(off + (long)n); }
  bool operator!=(decltype(nullptr)) const { return off >= 0; }
  bool operator==(const Ptr& o) const { return off == o.off; }
};
struct FakeParams { int nqb, sk_items, sk_ix, sk_full, sk_k; Ptr ws, ws_o, ws_ml, ws_cum, seg_cum; };
static void row(int rows, int slots, int B, int H, int Lq, int ntiles, bool ws, int nseg, int fixed_k, int force_k) {
  const IrAttnPlanIn in = {B, H, Lq, ntiles, rows, slots, ws, ws ? (size_t)%dULL : 0, nseg, fixed_k, force_k};
  const IrAttnPlan pl = ir_attn_plan(in);
  FakeParams p = {};
  p.ws = Ptr(0L);
  p.seg_cum = nseg > 0 ? Ptr(0L) : Ptr();
  ir_attn_plan_apply(pl, p);
  const bool applied = p.nqb == pl.nqb && p.sk_items == pl.items && p.sk_ix == pl.ix && p.sk_full == pl.full && p.sk_k == pl.k &&
                       p.ws_o == Ptr(0L) && p.ws_ml == Ptr((long)pl.ml_off) && p.ws_cum == (nseg > 0 ? Ptr((long)pl.cum_off) : Ptr());
  printf("%%d %%d %%d %%d %%d %%d %%d %%zu %%zu %%zu %%zu %%d\n", pl.nqb, pl.items, pl.ix, pl.full, pl.rem, pl.k, pl.grid,
         pl.piece_bytes, pl.ml_off, pl.cum_off, pl.ws_needed, (int)applied);
}
int main() {
  row(512, 32, 8, 5, 4096, 320, true, 0, 0, 0);
  row(512, 32, 8, 5, 4096, 320, true, 5, 0, 0);
  row(512, 32, 1, 5, 4096, 320, true, 0, 0, 0);
  row(512, 32, 8, 5, 4096, 320, false, 0, 0, 0);
  row(512, 32, 8, 5, 4096, 320, true, 0, 7, 0);
  row(128, 64, 8, 10, 1024, 80, true, 0, 0, 0);
  row(128, 64, 1, 10, 1024, 80, true, 0, 0, 0);
  row(128, 64, 8, 20, 256, 20, true, 0, 0, 0);
  row(512, 32, 1, 5, 4096, 320, true, 0, 0, 3);
  printf("%%zu %%zu %%d %%d %%d %%d\n", (size_t)kIrXcds * kIrWsPiecesPerXcd * ir_attn_piece_bytes(kIrMaxItemRows, 0),
         ir_attn_partials_bytes(320, 7, ir_attn_piece_bytes(512, 0)), kIrXcds, kIrPartialRowFloats, kIrPieceMinTiles, kIrBiCus);
  return 0;
}
""" % WS

# ix, full, rem, k, grid, ml offset, cum offset (floats)
EXPECT = [
    (40, 32, 8, 4, 512, 8388608, 8650752),
    None,                                        # seg_mass over 5 segments: same k and grid as the row above
    (5, 0, 5, 6, 240, 7864320, 8110080),
    (40, 40, 0, 1, 320, 0, 0),                   # no workspace
    (40, 0, 40, 7, 2240, None, None),            # fixed 7 pieces: workspace needed 302,776,320 B
    (80, 64, 16, 4, 1024, 4194304, 4325376),
    (10, 0, 10, 6, 480, 3932160, 4055040),
    (40, 40, 0, 1, 320, 0, 0),
    (5, 0, 5, 3, None, None, None),              # forced pieces = 3 on the third row's shape
]


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and (shutil.which(c) or os.path.exists(c)):
            return c
    pytest.fail("no host C++ compiler found")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("attn_plan")
    src = d / "plan_main.cpp"
    src.write_text(PROGRAM)
    out = {}
    for tag, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = d / f"plan_{tag}"
        r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and run.stderr == "", (tag, run.returncode, run.stderr[-3000:])
        out[tag] = run.stdout
    return out


def test_the_header_builds_alone_and_runs_clean_under_the_sanitizers(programs):
    assert programs["sanitized"] == programs["plain"]


def test_plans_equal_the_hand_derived_literals(programs):
    lines = programs["plain"].strip().splitlines()
    rows = [dict(zip(("nqb", "items", "ix", "full", "rem", "k", "grid", "piece_bytes", "ml", "cum", "ws_needed", "applied"),
                     map(int, ln.split()))) for ln in lines[:-1]]
    assert len(rows) == len(EXPECT)
    for i, (r, want) in enumerate(zip(rows, EXPECT)):
        assert r["applied"] == 1, i
        assert r["grid"] == 8 * (r["full"] + r["rem"] * r["k"]) and r["full"] + r["rem"] == r["ix"] == -(-r["items"] // 8), (i, r)
        if want is None:
            continue
        got = (r["ix"], r["full"], r["rem"], r["k"], r["grid"], r["ml"], r["cum"])
        assert all(w is None or g == w for g, w in zip(got, want)), (i, got, want)
    assert (rows[1]["k"], rows[1]["grid"]) == (rows[0]["k"], rows[0]["grid"])
    assert rows[1]["piece_bytes"] == 512 * (66 + 5) * 4 and rows[0]["piece_bytes"] == 512 * 66 * 4
    assert rows[4]["ws_needed"] == 302776320
    assert (rows[8]["full"], rows[8]["rem"], rows[8]["k"]) == (0, rows[8]["ix"], 3)
    # the recommended workspace, the batch-invariant scratch of the fixed-plan row, the named constants
    assert lines[-1].split() == ["69206016", "302776320", "8", "66", "8", "256"]


def test_the_library_reports_the_same_workspace():
    from instantrestore_amd import _lib
    assert _lib.lib().ir_shared_attn_workspace_bytes() == WS
