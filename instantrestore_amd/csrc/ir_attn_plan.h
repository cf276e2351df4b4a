// ir_attn_plan.h - the work plan of one attention forward launch, once for every kernel family (plain C++17: nothing of HIP, so
// a host compiler builds it alone - tests/test_attn_plan_cpu.py).
//
// items = B * H * ceil(Lq / rows) work items; every XCD owns ix = ceil(items / 8) consecutive ones and has `slots` concurrently
// resident workgroups (the launcher's own rule: CUs per XCD x workgroups per CU).  Whole rounds of the slots run their items'
// full K/V range; the `rem` items of the last, partly filled round are cut into k K/V-range pieces so that the round ends early.
// A piece leaves fp32 partials in the caller's workspace - per row 64 of O, the running max and the row sum, and with seg_mass
// the cumulative value of every segment - which the combine kernel merges in piece order.
#pragma once
#include <stddef.h>

constexpr int kIrXcds = 8;                  // XCD chunks of the item list (an MI355X's count; the kernels' remap is built on it)
constexpr int kIrPartialRowFloats = 64 + 2; // fp32 partials of one row of a piece: O, (raw running max, row sum)
constexpr int kIrPieceMinTiles = 8;         // a piece walks at least 8 K/V tiles.  (Round 3 tried 5-tile pieces for the 16x16-token
                                            // class - 320 items of 20 tiles on 512 slots, cut in three: 47 us against 37 us unsplit,
                                            // profiles/r3_layer_classes_cfg2_presc.txt: prologue, partials and combine cost more)
constexpr int kIrBiCus = 256;               // batch-invariant plan: one batch entry fills 256 CUs (a constant, not the device's count)
constexpr int kIrWsPiecesPerXcd = 64;       // ir_shared_attn_workspace_bytes(): pieces per XCD the recommended workspace holds ...
constexpr int kIrMaxItemRows = 512;         // ... of the largest work item of any kernel

static inline size_t ir_attn_piece_bytes(int rows, int nseg_cum) { return (size_t)rows * (kIrPartialRowFloats + nseg_cum) * sizeof(float); }

// partials of `pieces` pieces of each of `items` consecutive work items, in whole XCD chunks
static inline size_t ir_attn_partials_bytes(size_t items, int pieces, size_t piece_bytes) {
  return kIrXcds * ((items + kIrXcds - 1) / kIrXcds) * (size_t)pieces * piece_bytes;
}

// Remainder split: `rem` items of the last, partially filled round (per XCD) on `slots` concurrently
// resident workgroups.  Cutting each into k K/V-range pieces makes the round last ceil(rem*k/slots)/k of an
// item; pick the k that minimises it (plus a small per-piece charge for the fp32 partials and the combine),
// within the piece-length floor `kmax` and the workspace capacity `cap_pieces` (pieces per XCD).
static inline int ir_pick_split(int rem, int slots, int kmax, long cap_pieces) {
  int best_k = 1;
  double best = 1.0;   // k = 1: one round of whole items
  for (int k = 2; k <= kmax && (long)rem * k <= cap_pieces; ++k) {
    const int rounds = (rem * k + slots - 1) / slots;
    const double t = (double)rounds / k + 0.012 * k;
    if (t < best - 1e-9) { best = t; best_k = k; }
  }
  return best_k;
}

struct IrAttnPlanIn {
  int B, H, Lq, ntiles;
  int rows;          // query rows per work item
  int slots;         // resident workgroup slots per XCD
  bool ws_present;   // no workspace: never split
  size_t ws_bytes;
  int nseg;          // seg_mass: segments whose cumulative value a piece stores; 0 without
  int fixed_k;       // > 0: a fixed plan (batch-invariant mode): EVERY item in fixed_k pieces (1: whole items), workspace sized by the caller
  int force_k;       // > 1: the measurement knob IR_ATTN_FORCE_SPLIT of the 32-row launcher: every item in force_k pieces where they fit
};

struct IrAttnPlan {
  int nqb, items, ix;      // query blocks per (b, h); work items; items per XCD
  int full, rem, k;        // per XCD: whole items, cut items, pieces per cut item (k = 1: rem = 0)
  int grid;                // workgroups
  size_t piece_bytes;
  size_t ml_off, cum_off;  // float offsets of the (max, sum) and the cumulative-value areas behind the O partials
  size_t ws_needed;        // bytes of all three areas
};

static inline IrAttnPlan ir_attn_plan(const IrAttnPlanIn& in) {
  IrAttnPlan pl;
  pl.nqb = (in.Lq + in.rows - 1) / in.rows;
  pl.items = in.B * in.H * pl.nqb;
  pl.ix = (pl.items + kIrXcds - 1) / kIrXcds;
  pl.piece_bytes = ir_attn_piece_bytes(in.rows, in.nseg);
  const long cap = (long)(in.ws_bytes / pl.piece_bytes / kIrXcds);   // pieces per XCD the workspace holds
  int full = (pl.ix / in.slots) * in.slots, k = 1;
  if (in.fixed_k > 0) {
    k = in.fixed_k;
    full = k > 1 ? 0 : pl.ix;
  } else {
    if (in.ws_present && pl.ix > full) k = ir_pick_split(pl.ix - full, in.slots, in.ntiles / kIrPieceMinTiles, cap);
    if (k <= 1) { full = pl.ix; k = 1; }
    if (in.force_k > 1 && in.ws_present && in.ntiles >= 2 * in.force_k && (long)pl.ix * in.force_k <= cap) { full = 0; k = in.force_k; }
  }
  pl.full = full;
  pl.rem = pl.ix - full;
  pl.k = k;
  pl.grid = kIrXcds * (pl.full + pl.rem * k);
  const size_t prows = (size_t)kIrXcds * pl.rem * k * in.rows;   // partial rows of the launch
  pl.ml_off = prows * 64;
  pl.cum_off = pl.ml_off + prows * 2;
  pl.ws_needed = prows / in.rows * pl.piece_bytes;
  return pl;
}

// the plan into the kernel argument block (AttnKParams: nqb, sk_*, ws_*).  ws_cum is set with seg_mass only: nothing else reads it
template <typename Params>
static inline void ir_attn_plan_apply(const IrAttnPlan& pl, Params& p) {
  p.nqb = pl.nqb;
  p.sk_items = pl.items;
  p.sk_ix = pl.ix;
  p.sk_full = pl.full;
  p.sk_k = pl.k;
  p.ws_o = p.ws;
  p.ws_ml = p.ws + pl.ml_off;
  p.ws_cum = p.seg_cum != nullptr ? p.ws + pl.cum_off : nullptr;
}
