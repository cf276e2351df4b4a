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
static const size_t kWs = %dULL;   // ir_shared_attn_workspace_bytes()
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
static void row_ws(const char* tag, int rows, int slots, int B, int H, int Lq, int ntiles, size_t ws_bytes, int nseg, int fixed_k, int force_k) {
  const IrAttnPlanIn in = {B, H, Lq, ntiles, rows, slots, ws_bytes > 0, ws_bytes, nseg, fixed_k, force_k};
  const IrAttnPlan pl = ir_attn_plan(in);
  FakeParams p = {};
  p.ws = Ptr(0L);
  p.seg_cum = nseg > 0 ? Ptr(0L) : Ptr();
  ir_attn_plan_apply(pl, p);
  const bool applied = p.nqb == pl.nqb && p.sk_items == pl.items && p.sk_ix == pl.ix && p.sk_full == pl.full && p.sk_k == pl.k &&
                       p.ws_o == Ptr(0L) && p.ws_ml == Ptr((long)pl.ml_off) && p.ws_cum == (nseg > 0 ? Ptr((long)pl.cum_off) : Ptr());
  printf("%%s%%d %%d %%d %%d %%d %%d %%d %%zu %%zu %%zu %%zu %%d\n", tag, pl.nqb, pl.items, pl.ix, pl.full, pl.rem, pl.k, pl.grid,
         pl.piece_bytes, pl.ml_off, pl.cum_off, pl.ws_needed, (int)applied);
}
static void row(int rows, int slots, int B, int H, int Lq, int ntiles, bool ws, int nseg, int fixed_k, int force_k) {
  row_ws("", rows, slots, B, H, Lq, ntiles, ws ? kWs : 0, nseg, fixed_k, force_k);
}
// the item grids of tests/test_gpu_item_grid.py: printed with a tag, compared with GRID_EXPECT
static void grid_row(int rows, int slots, int B, int H, int Lq, size_t ws_bytes, int nseg, int ntiles = 16) {
  row_ws("grid ", rows, slots, B, H, Lq, ntiles, ws_bytes, nseg, 0, 0);
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
  grid_row(512, 32, 47, 3, 600, kWs, 0);   // set A: the 128- and the 8-wave 64-row kernel
  grid_row(256, 64, 59, 3, 700, kWs, 0);   // set B: the 4-wave 64-row kernel
  grid_row(128, 64, 37, 3, 650, kWs, 0);   // set C: the 32-row kernel's forms
  grid_row(512, 32, 47, 3, 600, kWs, 3);   // sets A and C with the masses of three segments
  grid_row(128, 64, 37, 3, 650, kWs, 3);
  grid_row(512, 32, 47, 3, 600, 8650752ULL, 0);   // set A with a caller's workspace of exactly the split's size ...
  grid_row(512, 32, 47, 3, 600, 8650751ULL, 0);   // ... and one byte short: 7 pieces per XCD, the 4 remainder items stay whole
  grid_row(512, 32, 47, 3, 600, kWs, 0, 64);      // the same sets on 64 K/V tiles (the bf16 runs)
  grid_row(256, 64, 59, 3, 700, kWs, 0, 64);
  grid_row(128, 64, 37, 3, 650, kWs, 0, 64);
  grid_row(512, 32, 47, 3, 600, kWs, 3, 64);
  grid_row(128, 64, 37, 3, 650, kWs, 3, 64);
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

# The item grids of tests/test_gpu_item_grid.py (the "grid" rows of the program; 16 K/V tiles, so at most 16 / 8 = 2 pieces), by hand:
#   set A  B 47, H 3, Lq 600, 512-row items on 32 slots: nqb 2, items 282, ix = ceil(282 / 8) = 36 = one round of 32 + 4;
#          cap = 69,206,016 / 135,168 / 8 = 64 pieces per XCD >= 4 * 2; one round of 8 pieces: 1/2 + 0.024 < 1, so k = 2;
#          grid 8 * (32 + 4 * 2) = 320; partial rows 8 * 4 * 2 * 512 = 32,768: ml at 32,768 * 64 = 2,097,152 floats, cum 2 * 32,768 further
#          = 2,162,688; 64 pieces of 512 * 66 * 4 = 135,168 B = 8,650,752 B.  XCD 7 starts at item 252: 30 of its 36 exist
#   set B  B 59, H 3, Lq 700, 256-row items on 64 slots: nqb 3, items 531, ix 67 = 64 + 3, k = 2, grid 8 * (64 + 6) = 560; partial rows
#          8 * 3 * 2 * 256 = 12,288: ml 786,432, cum 786,432 + 24,576 = 811,008; 48 pieces of 67,584 B = 3,244,032 B
#   set C  B 37, H 3, Lq 650, 128-row items on 64 slots: nqb 6, items 666, ix 84 = 64 + 20, k = 2 (40 pieces: one round), grid
#          8 * (64 + 40) = 832; partial rows 8 * 20 * 2 * 128 = 40,960: ml 2,621,440, cum 2,621,440 + 81,920 = 2,703,360; 320 pieces of
#          33,792 B = 10,813,440 B
#   masses of 3 segments: pieces of rows * 69 * 4 B (141,312 / 35,328), same cut and offsets; 64 * 141,312 = 9,043,968 B and
#          320 * 35,328 = 11,304,960 B
#   set A on 8,650,752 B: cap = 64 / 8 = 8 = 4 * 2, k stays 2; on 8,650,751 B: 63 / 8 = 7 < 8: no k >= 2 fits, whole items, grid 288
#   64 tiles (the bf16 runs of the GPU test): up to 64 / 8 = 8 pieces.  Sets A and B: 4 k and 3 k pieces fit one round of 32 / 64
#          slots for every k <= 8, so the cost is 1/k + 0.012 k: 0.221 at k = 8 (k = 7: 0.227).  A: grid 8 * (32 + 32) = 512, partial
#          rows 8 * 4 * 8 * 512 = 131,072: ml 8,388,608, cum + 262,144 = 8,650,752, 256 pieces = 34,603,008 B (with masses: cap =
#          489 / 8 = 61 >= 32; 256 * 141,312 = 36,175,872 B).  B: grid 8 * (64 + 24) = 704, partial rows 49,152: ml 3,145,728, cum
#          3,244,032, 192 pieces = 12,976,128 B.  Set C: 20 k pieces on 64 slots take ceil(20 k / 64) rounds: k = 2 0.524, 3 0.369
#          (one round), 4 0.548, 5 0.460, 6 0.405, 7 0.513, 8 0.471, so k = 3: grid 8 * (64 + 60) = 992, partial rows 61,440: ml
#          3,932,160, cum + 122,880 = 4,055,040, 480 pieces = 16,220,160 B (with masses 480 * 35,328 = 16,957,440 B)
# nqb, items, ix, full, rem, k, grid, piece bytes, ml offset, cum offset (floats), bytes needed
GRID_EXPECT = [
    (2, 282, 36, 32, 4, 2, 320, 135168, 2097152, 2162688, 8650752),
    (3, 531, 67, 64, 3, 2, 560, 67584, 786432, 811008, 3244032),
    (6, 666, 84, 64, 20, 2, 832, 33792, 2621440, 2703360, 10813440),
    (2, 282, 36, 32, 4, 2, 320, 141312, 2097152, 2162688, 9043968),
    (6, 666, 84, 64, 20, 2, 832, 35328, 2621440, 2703360, 11304960),
    (2, 282, 36, 32, 4, 2, 320, 135168, 2097152, 2162688, 8650752),
    (2, 282, 36, 36, 0, 1, 288, 135168, 0, 0, 0),
    (2, 282, 36, 32, 4, 8, 512, 135168, 8388608, 8650752, 34603008),
    (3, 531, 67, 64, 3, 8, 704, 67584, 3145728, 3244032, 12976128),
    (6, 666, 84, 64, 20, 3, 992, 33792, 3932160, 4055040, 16220160),
    (2, 282, 36, 32, 4, 8, 512, 141312, 8388608, 8650752, 36175872),
    (6, 666, 84, 64, 20, 3, 992, 35328, 3932160, 4055040, 16957440),
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
    lines = [ln for ln in programs["plain"].strip().splitlines() if not ln.startswith("grid ")]
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


def test_item_grid_plans_equal_the_hand_derived_literals(programs):
    got = [tuple(map(int, ln.split()[1:])) for ln in programs["plain"].strip().splitlines() if ln.startswith("grid ")]
    assert len(got) == len(GRID_EXPECT)
    for i, (g, want) in enumerate(zip(got, GRID_EXPECT)):
        assert g[:-1] == want and g[-1] == 1, (i, g, want)
    # what tests/test_gpu_item_grid.py says of the last XCD's chunk: items it owns, and of those how many in the remainder round
    for (_, items, ix, full, _, _, _, _, _, _, _), owned, in_rem in zip(GRID_EXPECT[:3], (30, 62, 78), (0, 0, 14)):
        assert items - 7 * ix == owned and max(0, owned - full) == in_rem


def test_the_library_reports_the_same_workspace():
    from instantrestore_amd import _lib
    assert _lib.lib().ir_shared_attn_workspace_bytes() == WS
