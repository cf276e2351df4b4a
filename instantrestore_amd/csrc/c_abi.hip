// c_abi.hip - the extern "C" surface declared in include/instantrestore_hip.h.
// Argument validation, parameter-block construction, launches. No exceptions, no global state
// other than a thread-local error string.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../include/instantrestore_hip.h"
#include "ir_kernels.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool stride_ok(int64_t s) { return s >= 0 && (s % 8) == 0; }  // keeps every head row 16-B aligned

// The forward kernels walk a K/V segment through a buffer descriptor with 32-bit byte offsets, formed in `int`: the row stride in
// bytes, (len - 1) * row_bytes + 128 (num_records), 64 * row_bytes per tile, tile * 64 * row_bytes for a piece that starts inside
// the segment, and the 128-row kernel's offset of the tile behind a run, which reaches the segment's whole tiles:
// 64 * ceil(len / 64) * row_bytes.  That last one, plus the 128 bytes of a head row, bounds them all; it has to fit a positive int.
// 0 when it does, else the largest row stride (elements, a multiple of 8) that fits at this length.
int64_t seg_stride_limit(int32_t len, int64_t sl) {
  const int64_t rows = ((int64_t)len + IR_KV_TILE - 1) / IR_KV_TILE * IR_KV_TILE;
  if (rows * sl * 2 + 128 <= IR_ATTN_SEG_BYTES_MAX) return 0;
  return (IR_ATTN_SEG_BYTES_MAX - 128) / (rows * 2) / 8 * 8;
}

// `fwd`: the call is (or describes) a launch of the attention forward, whose segment-span limit applies; the read-out entry points
// (ir_attn_probs*, ir_attn_segment_mass, ir_attn_rows, ir_attn_match, ir_attn_transfer, ir_attn_received, ir_attn_topk, ir_attn_key_match) address K through 64-bit pointers and take any stride
bool attn_block_size_ok(uint32_t n) {
  return n == sizeof(ir_shared_attn_args) || n == sizeof(ir_shared_attn_table_args) || n == sizeof(ir_shared_attn_bias_args) ||
         n == sizeof(ir_shared_attn_ragged_args) || n == sizeof(ir_shared_attn_region_args);
}

int build_attn_params(const ir_shared_attn_args* a, AttnKParams* p, bool need_out, bool fwd) {
  if (a == nullptr) return fail(IR_ERR_INVALID_ARG, "args is NULL");
  // the block up to and including seg_mass (no pointer tables), ir_shared_attn_table_args, ir_shared_attn_bias_args,
  // ir_shared_attn_ragged_args or ir_shared_attn_region_args; nothing in between
  if (!attn_block_size_ok(a->struct_size))
    return fail(IR_ERR_INVALID_ARG, "struct_size %u != %zu, %zu, %zu, %zu or %zu (ABI mismatch)", a->struct_size, sizeof(ir_shared_attn_args),
                sizeof(ir_shared_attn_table_args), sizeof(ir_shared_attn_bias_args), sizeof(ir_shared_attn_ragged_args), sizeof(ir_shared_attn_region_args));
  const ir_shared_attn_table_args* ta = a->struct_size >= sizeof(ir_shared_attn_table_args) ? (const ir_shared_attn_table_args*)a : nullptr;
  const ir_shared_attn_bias_args* ba = a->struct_size >= sizeof(ir_shared_attn_bias_args) ? (const ir_shared_attn_bias_args*)a : nullptr;
  const ir_shared_attn_ragged_args* ra = a->struct_size >= sizeof(ir_shared_attn_ragged_args) ? (const ir_shared_attn_ragged_args*)a : nullptr;
  const ir_shared_attn_region_args* ga = a->struct_size == sizeof(ir_shared_attn_region_args) ? (const ir_shared_attn_region_args*)a : nullptr;
  const uint32_t* qallow = ga != nullptr ? ga->q_allow : nullptr;
  const int32_t* kregion = ga != nullptr ? ga->key_region : nullptr;
  const float* kbias = ba != nullptr ? ba->key_bias : nullptr;
  const int32_t* rlens = ra != nullptr ? ra->ref_lens : nullptr;
  const void* const* ktab = ta != nullptr ? ta->k_ref_table : nullptr;
  const void* const* vtab = ta != nullptr ? ta->v_ref_table : nullptr;
  const bool tables = ktab != nullptr;
  if (a->dtype != IR_DTYPE_F16 && a->dtype != IR_DTYPE_BF16)
    return fail(IR_ERR_UNSUPPORTED, "dtype %d: only fp16 (0) and bf16 (1) are implemented", a->dtype);
  if (a->batch <= 0 || a->heads <= 0 || a->len_q <= 0) return fail(IR_ERR_INVALID_ARG, "batch/heads/len_q must be > 0");
  if (a->n_refs < 0 || a->len_self < 0 || a->len_ref < 0) return fail(IR_ERR_INVALID_ARG, "negative length");
  const bool inc = (a->flags & IR_FLAG_INCLUDE_SELF) != 0;
  if ((a->flags & ~(IR_FLAG_INCLUDE_SELF | IR_FLAG_Q_PRESCALED | IR_FLAG_OUT_F32 | IR_FLAG_BATCH_INVARIANT)) != 0) return fail(IR_ERR_INVALID_ARG, "unknown flag bits 0x%x", a->flags);
  if ((a->flags & IR_FLAG_BATCH_INVARIANT) && a->tuning != IR_TUNE_DEFAULT)
    return fail(IR_ERR_INVALID_ARG, "IR_FLAG_BATCH_INVARIANT chooses its own kernel: tuning must be 0 (got %d)", a->tuning);
  if (a->reserved != 0) return fail(IR_ERR_INVALID_ARG, "reserved must be 0");
  if (!ir_attn_variant_available(a->tuning)) return fail(IR_ERR_UNSUPPORTED, "tuning value %d is not available in this build", a->tuning);
  if (inc && a->len_self <= 0) return fail(IR_ERR_INVALID_ARG, "INCLUDE_SELF with len_self == 0");
  if (a->n_refs > 0 && a->len_ref <= 0) return fail(IR_ERR_INVALID_ARG, "n_refs > 0 with len_ref == 0");
  if (!inc && a->n_refs == 0) return fail(IR_ERR_INVALID_ARG, "empty key/value sequence");
  if (a->q == nullptr || (need_out && a->out == nullptr)) return fail(IR_ERR_INVALID_ARG, "q/out is NULL");
  if (inc && (a->k_self == nullptr || a->v_self == nullptr)) return fail(IR_ERR_INVALID_ARG, "k_self/v_self is NULL");
  if ((ktab == nullptr) != (vtab == nullptr)) return fail(IR_ERR_INVALID_ARG, "k_ref_table and v_ref_table must both be set or both be NULL");
  if (tables) {
    if (a->k_ref != nullptr || a->v_ref != nullptr) return fail(IR_ERR_INVALID_ARG, "k_ref_table / v_ref_table given: k_ref and v_ref must be NULL");
    if (a->n_refs == 0) return fail(IR_ERR_INVALID_ARG, "k_ref_table / v_ref_table need n_refs > 0");
    if (a->kr_sb != 0 || a->kr_sn != 0 || a->vr_sb != 0 || a->vr_sn != 0)
      return fail(IR_ERR_INVALID_ARG, "k_ref_table / v_ref_table given: the strides kr_sb, kr_sn, vr_sb, vr_sn must be 0 (the tables hold every base address)");
    if (((reinterpret_cast<uintptr_t>(ktab) | reinterpret_cast<uintptr_t>(vtab)) & 7u) != 0) return fail(IR_ERR_UNSUPPORTED, "k_ref_table / v_ref_table must be 8-byte aligned");
  }
  if (a->n_refs > 0 && !tables && (a->k_ref == nullptr || a->v_ref == nullptr)) return fail(IR_ERR_INVALID_ARG, "k_ref/v_ref is NULL");
  if ((a->adain_a == nullptr) != (a->adain_b == nullptr)) return fail(IR_ERR_INVALID_ARG, "adain_a and adain_b must both be set or both be NULL");
  if (a->adain_a != nullptr && a->n_refs == 0) return fail(IR_ERR_INVALID_ARG, "AdaIN affine without references");
  if (a->valid_refs != nullptr && (reinterpret_cast<uintptr_t>(a->valid_refs) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "valid_refs must be 4-byte aligned");
  if (a->seg_mass != nullptr && (reinterpret_cast<uintptr_t>(a->seg_mass) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "seg_mass must be 4-byte aligned");
  if (kbias != nullptr) {
    if (!fwd)
      return fail(IR_ERR_UNSUPPORTED, "key_bias: ir_attn_probs[_ex], ir_attn_segment_mass, ir_attn_rows, ir_attn_match, ir_attn_transfer, ir_attn_received, ir_attn_topk and ir_attn_key_match do not take a key bias yet (their exp(s - lse) would "
                  "leave it out); the forward's seg_mass by-product does");
    if ((reinterpret_cast<uintptr_t>(kbias) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "key_bias must be 4-byte aligned");
    if (ba->kb_sb < 0 || ba->kb_sh < 0) return fail(IR_ERR_INVALID_ARG, "key_bias strides kb_sb %lld, kb_sh %lld must be >= 0", (long long)ba->kb_sb, (long long)ba->kb_sh);
    if (a->valid_refs != nullptr && a->n_refs > 0)
      return fail(IR_ERR_UNSUPPORTED, "key_bias together with valid_refs: the closed form of the zero-filled suffix assumes score 0 on its keys (pass "
                  "valid_refs = NULL and let the kernel walk the zeros, or mask those references in the bias)");
    if (a->tuning != IR_TUNE_DEFAULT && a->tuning != IR_TUNE_PIPE32_PRESCALE_Q && a->tuning != IR_TUNE_PIPE32_EARLYQK)
      return fail(IR_ERR_UNSUPPORTED, "key_bias: tuning %d has no BIAS form (IR_TUNE_DEFAULT, IR_TUNE_PIPE32_PRESCALE_Q or IR_TUNE_PIPE32_EARLYQK: the "
                  "32-row kernel runs every call with a key bias)", a->tuning);
  }
  if (rlens != nullptr) {
    if (!fwd)
      return fail(IR_ERR_UNSUPPORTED, "ref_lens: ir_attn_probs[_ex], ir_attn_segment_mass, ir_attn_rows, ir_attn_match, ir_attn_transfer, ir_attn_received, ir_attn_topk and ir_attn_key_match do not take per-reference counts yet (they would "
                  "walk the tails behind the counts); the forward's seg_mass by-product does");
    if ((reinterpret_cast<uintptr_t>(rlens) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "ref_lens must be 4-byte aligned");
    if (a->n_refs == 0) return fail(IR_ERR_UNSUPPORTED, "ref_lens with n_refs == 0: there is no reference to count");
    if (ra->rl_sb < a->n_refs) return fail(IR_ERR_INVALID_ARG, "ref_lens row stride rl_sb %lld must be >= n_refs %d", (long long)ra->rl_sb, a->n_refs);
    if (a->valid_refs != nullptr)
      return fail(IR_ERR_UNSUPPORTED, "ref_lens together with valid_refs: a count of 0 says the reference is absent, valid_refs says it is zero-filled "
                  "(exp(0) per key) - pass one of the two");
    if (kbias != nullptr)
      return fail(IR_ERR_UNSUPPORTED, "ref_lens together with key_bias: the bias indexes the packed uniform key axis (len_ref keys per reference); counts "
                  "with a bias are a follow-up");
    if (a->tuning != IR_TUNE_DEFAULT && a->tuning != IR_TUNE_PIPE32_PRESCALE_Q && a->tuning != IR_TUNE_PIPE32_EARLYQK)
      return fail(IR_ERR_UNSUPPORTED, "ref_lens: tuning %d has no RAGGED form (IR_TUNE_DEFAULT, IR_TUNE_PIPE32_PRESCALE_Q or IR_TUNE_PIPE32_EARLYQK: the "
                  "32-row kernel runs every call with per-reference counts)", a->tuning);
  }
  if ((qallow == nullptr) != (kregion == nullptr)) return fail(IR_ERR_INVALID_ARG, "q_allow and key_region must both be set or both be NULL");
  if (qallow != nullptr) {
    if (!fwd)
      return fail(IR_ERR_UNSUPPORTED, "q_allow / key_region: ir_attn_probs[_ex], ir_attn_segment_mass, ir_attn_rows, ir_attn_match, ir_attn_transfer, ir_attn_received, ir_attn_topk and ir_attn_key_match do not take "
                  "regions yet (their exp(s - lse) would count the pairs the forward left out); the forward's seg_mass by-product does");
    if (((reinterpret_cast<uintptr_t>(qallow) | reinterpret_cast<uintptr_t>(kregion)) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "q_allow and key_region must be 4-byte aligned");
    const int64_t lkv = (inc ? (int64_t)a->len_self : 0) + (int64_t)a->n_refs * a->len_ref;
    if (ga->qa_sb < a->len_q) return fail(IR_ERR_INVALID_ARG, "q_allow row stride qa_sb %lld must be >= len_q %d", (long long)ga->qa_sb, a->len_q);
    if (ga->kg_sb < lkv) return fail(IR_ERR_INVALID_ARG, "key_region row stride kg_sb %lld must be >= Lkv %lld", (long long)ga->kg_sb, (long long)lkv);
    if (kbias != nullptr)
      return fail(IR_ERR_UNSUPPORTED, "q_allow / key_region together with key_bias: one C operand carries either the bias or the region test; regions with a "
                  "bias are a follow-up");
    if (rlens != nullptr)
      return fail(IR_ERR_UNSUPPORTED, "q_allow / key_region together with ref_lens: key_region indexes the packed uniform key axis (len_ref keys per reference); "
                  "regions with counts are a follow-up");
    if (a->valid_refs != nullptr && a->n_refs > 0)
      return fail(IR_ERR_UNSUPPORTED, "q_allow / key_region together with valid_refs: the closed form of the zero-filled suffix gives every row its keys (pass "
                  "valid_refs = NULL and let the kernel walk the zeros, or give those keys a region nobody may attend)");
    if (a->tuning != IR_TUNE_DEFAULT && a->tuning != IR_TUNE_PIPE32_PRESCALE_Q && a->tuning != IR_TUNE_PIPE32_EARLYQK)
      return fail(IR_ERR_UNSUPPORTED, "q_allow / key_region: tuning %d has no REGION form (IR_TUNE_DEFAULT, IR_TUNE_PIPE32_PRESCALE_Q or IR_TUNE_PIPE32_EARLYQK: the "
                  "32-row kernel runs every call with regions)", a->tuning);
  }
  const void* ptrs[] = {a->q, a->k_self, a->v_self, a->k_ref, a->v_ref, a->out, a->adain_a, a->adain_b};
  for (const void* q : ptrs)
    if (q != nullptr && !aligned16(q)) return fail(IR_ERR_UNSUPPORTED, "pointer %p is not 16-byte aligned", q);
  const int64_t strides[] = {a->q_sb, a->q_sl, a->q_sh, a->ks_sb, a->ks_sl, a->ks_sh, a->vs_sb, a->vs_sl, a->vs_sh,
                             a->kr_sb, a->kr_sn, a->kr_sl, a->kr_sh, a->vr_sb, a->vr_sn, a->vr_sl, a->vr_sh,
                             a->o_sb, a->o_sl, a->o_sh};
  for (int64_t s : strides)
    if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "stride %lld must be a non-negative multiple of 8 elements", (long long)s);
  if (fwd) {
    const struct { const char* name; int64_t sl; int32_t len; bool used; } segs[] = {
        {"ks_sl", a->ks_sl, a->len_self, inc}, {"vs_sl", a->vs_sl, a->len_self, inc},
        {"kr_sl", a->kr_sl, a->len_ref, a->n_refs > 0}, {"vr_sl", a->vr_sl, a->len_ref, a->n_refs > 0}};
    for (const auto& g : segs) {
      const int64_t most = g.used ? seg_stride_limit(g.len, g.sl) : 0;
      if (most != 0)
        return fail(IR_ERR_UNSUPPORTED, "%s %lld: the forward addresses a K/V segment with 32-bit byte offsets, so its whole 64-key tiles and a head row may span "
                    "at most %lld bytes (IR_ATTN_SEG_BYTES_MAX): at %d keys the row stride is at most %lld elements",
                    g.name, (long long)g.sl, (long long)IR_ATTN_SEG_BYTES_MAX, g.len, (long long)most);
    }
  }

  memset(p, 0, sizeof(*p));
  p->q = a->q; p->k_self = a->k_self; p->v_self = a->v_self; p->k_ref = a->k_ref; p->v_ref = a->v_ref;
  p->aa = a->adain_a; p->ab = a->adain_b; p->out = a->out; p->lse = a->lse;
  p->valid = a->n_refs > 0 ? a->valid_refs : nullptr;
  p->seg_cum = need_out ? a->seg_mass : nullptr;   // a by-product of the forward launch only (ir_attn_probs / _segment_mass ignore it)
  p->nseg_out = (inc ? 1 : 0) + a->n_refs;
  p->q_sb = a->q_sb; p->q_sl = a->q_sl; p->q_sh = a->q_sh;
  p->ks_sb = a->ks_sb; p->ks_sl = a->ks_sl; p->ks_sh = a->ks_sh;
  p->vs_sb = a->vs_sb; p->vs_sl = a->vs_sl; p->vs_sh = a->vs_sh;
  p->kr_sb = a->kr_sb; p->kr_sn = a->kr_sn; p->kr_sl = a->kr_sl; p->kr_sh = a->kr_sh;
  p->vr_sb = a->vr_sb; p->vr_sn = a->vr_sn; p->vr_sl = a->vr_sl; p->vr_sh = a->vr_sh;
  p->o_sb = a->o_sb; p->o_sl = a->o_sl; p->o_sh = a->o_sh;
  p->B = a->batch; p->H = a->heads; p->Lq = a->len_q; p->Ls = a->len_self; p->N = a->n_refs; p->Lr = a->len_ref;
  if (tables) {   // the tables in the dense fields, strided by entries (AttnKParams.ref_tables): batch_slice and every kernel index them as they index K / V
    p->k_ref = ktab; p->v_ref = vtab; p->ref_tables = 1;
    p->kr_sb = p->vr_sb = (int64_t)a->n_refs * 4; p->kr_sn = p->vr_sn = 4;
  }
  p->include_self = inc ? 1 : 0;
  if (kbias != nullptr) { p->key_bias = kbias; p->kb_sb = ba->kb_sb; p->kb_sh = ba->kb_sh; }
  if (rlens != nullptr) { p->ref_lens = rlens; p->rl_sb = ra->rl_sb; }
  if (qallow != nullptr) { p->q_allow = qallow; p->qa_sb = ga->qa_sb; p->key_region = kregion; p->kg_sb = ga->kg_sb; }
  p->q_prescaled = (a->flags & IR_FLAG_Q_PRESCALED) ? 1 : 0;
  p->out_f32 = (a->flags & IR_FLAG_OUT_F32) ? 1 : 0;
  if (p->q_prescaled && ((a->tuning >> 5) != 0 || !ir_attn_variant(a->tuning)->presc_q))   // (the availability test above found the row)
    return fail(IR_ERR_UNSUPPORTED, "IR_FLAG_Q_PRESCALED is implemented by the W128, W64X8, PIPE32_PRESCALE_Q and PIPE32_POSTCHECK kernels only");
  if (a->tuning == IR_TUNE_W128 && !p->q_prescaled)
    return fail(IR_ERR_UNSUPPORTED, "IR_TUNE_W128 needs IR_FLAG_Q_PRESCALED");
  if (!p->q_prescaled && a->tuning == IR_TUNE_PIPE32_POSTCHECK)
    return fail(IR_ERR_UNSUPPORTED, "IR_TUNE_PIPE32_POSTCHECK needs IR_FLAG_Q_PRESCALED (its scores must already carry the reference)");
  p->tiles_self = inc ? (a->len_self + IR_KV_TILE - 1) / IR_KV_TILE : 0;
  p->tiles_ref = a->n_refs > 0 ? (a->len_ref + IR_KV_TILE - 1) / IR_KV_TILE : 0;
  p->ntiles = p->tiles_self + a->n_refs * p->tiles_ref;
  p->lkv = (inc ? a->len_self : 0) + a->n_refs * a->len_ref;
  p->scale = a->scale;
  p->scale_log2 = a->scale * 1.4426950408889634f;
  if (a->workspace != nullptr && !aligned16(a->workspace)) return fail(IR_ERR_UNSUPPORTED, "workspace must be 16-byte aligned");
  p->ws = (float*)a->workspace;
  p->ws_bytes = a->workspace != nullptr ? (size_t)a->workspace_bytes : 0;
  if (a->tuning == IR_TUNE_W128 && !ir_attn_w128_supports(*p))
    return fail(IR_ERR_UNSUPPORTED, "IR_TUNE_W128 takes segment lengths that are multiples of 64 keys (valid_refs and seg_mass included)");
  const int64_t blocks = (int64_t)a->batch * a->heads * ((a->len_q + 127) / 128);
  if (blocks > 0x7fffffffLL) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  return IR_OK;
}

bool batch_invariant(const ir_shared_attn_args* a) { return (a->flags & IR_FLAG_BATCH_INVARIANT) != 0; }

// ABI v10: the batch-invariant plan of a call whose AttnKParams are built; seg_mass counts wherever it is asked for (it sizes the pieces'
// partials, never the kernel or the cut)
IrAttnBiPlan bi_plan_of(const ir_shared_attn_args* a, const AttnKParams& p0) {
  AttnKParams p = p0;
  p.seg_cum = (float*)a->seg_mass;
  IrAttnBiPlan pl;
  ir_attn_bi_plan(p, &pl);
  return pl;
}

// batch entries per launch that the caller's workspace holds (0: not even one)
int bi_batch_per_launch(const IrAttnBiPlan& pl, int batch, size_t ws_bytes) {
  if (pl.pieces <= 1 || ir_attn_bi_workspace_bytes(pl, batch) <= ws_bytes) return batch;
  const size_t chunk_items = kIrXcds * (ws_bytes / ir_attn_partials_bytes(kIrXcds, pl.pieces, pl.piece_bytes));   // whole XCD chunks of items
  const size_t nb = chunk_items / (size_t)pl.items;
  return nb < (size_t)batch ? (int)nb : batch;
}

// the part of a call that covers batch entries [b0, b0 + nb): every pointer moved by b0 entries (pointer tables: by b0 * N table entries)
AttnKParams batch_slice(const AttnKParams& p, int b0, int nb) {
  AttnKParams q = p;
  q.B = nb;
  q.q = (const char*)p.q + (int64_t)b0 * p.q_sb * 2;
  if (p.k_self != nullptr) { q.k_self = (const char*)p.k_self + (int64_t)b0 * p.ks_sb * 2; q.v_self = (const char*)p.v_self + (int64_t)b0 * p.vs_sb * 2; }
  if (p.k_ref != nullptr) { q.k_ref = (const char*)p.k_ref + (int64_t)b0 * p.kr_sb * 2; q.v_ref = (const char*)p.v_ref + (int64_t)b0 * p.vr_sb * 2; }
  if (p.aa != nullptr) { q.aa = p.aa + (int64_t)b0 * p.N * p.H * 64; q.ab = p.ab + (int64_t)b0 * p.N * p.H * 64; }
  q.out = (char*)p.out + (int64_t)b0 * p.o_sb * (p.out_f32 ? 4 : 2);
  if (p.lse != nullptr) q.lse = p.lse + (int64_t)b0 * p.H * p.Lq;
  if (p.seg_cum != nullptr) q.seg_cum = p.seg_cum + (int64_t)b0 * p.H * p.Lq * p.nseg_out;
  if (p.valid != nullptr) q.valid = p.valid + b0;
  if (p.key_bias != nullptr) q.key_bias = p.key_bias + (int64_t)b0 * p.kb_sb;
  if (p.ref_lens != nullptr) q.ref_lens = p.ref_lens + (int64_t)b0 * p.rl_sb;
  if (p.q_allow != nullptr) { q.q_allow = p.q_allow + (int64_t)b0 * p.qa_sb; q.key_region = p.key_region + (int64_t)b0 * p.kg_sb; }
  return q;
}

// the forward launch of a validated call: the default dispatch (tuning), or the batch-invariant plan over as many launches as the
// workspace needs (each entry's plan is the same in every one of them)
int launch_fwd(const ir_shared_attn_args* a, const AttnKParams& p, hipStream_t s) {
  if (!batch_invariant(a)) {
    const hipError_t e = ir_launch_shared_attn_fwd(p, a->dtype, a->tuning, s);
    if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "shared_attn_fwd launch: %s", hipGetErrorString(e));
    return IR_OK;
  }
  IrAttnBiPlan pl;
  ir_attn_bi_plan(p, &pl);
  const int per = bi_batch_per_launch(pl, p.B, p.ws_bytes);
  if (per <= 0)
    return fail(IR_ERR_WORKSPACE, "batch-invariant plan (%d pieces per item): workspace %zu < %zu bytes for one batch entry, %zu for the whole batch "
                "(ir_shared_attn_workspace_bytes_for)", pl.pieces, p.ws_bytes, ir_attn_bi_workspace_bytes(pl, 1), ir_attn_bi_workspace_bytes(pl, p.B));
  for (int b0 = 0; b0 < p.B; b0 += per) {
    const AttnKParams q = batch_slice(p, b0, p.B - b0 < per ? p.B - b0 : per);
    const hipError_t e = ir_launch_shared_attn_fwd_bi(q, a->dtype, pl, s);
    if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "shared_attn_fwd (batch-invariant) launch: %s", hipGetErrorString(e));
  }
  return IR_OK;
}

// The parameter block of a read-out of the forward's LSE (ir_attn_probs_ex, ir_attn_segment_mass, ir_attn_rows, ir_attn_match,
// ir_attn_transfer, ir_attn_received, ir_attn_topk, ir_attn_key_match).
// `single_kernel`: the name of an entry point that has one kernel and refuses a tuning value, or nullptr.  A key bias,
// per-reference counts and regions are refused for the whole family in build_attn_params (!fwd)
int build_readout_params(const ir_shared_attn_args* args, AttnKParams* p, const char* single_kernel) {
  if (single_kernel != nullptr) {
    if (args == nullptr) return fail(IR_ERR_INVALID_ARG, "args is NULL");
    if (attn_block_size_ok(args->struct_size) && args->tuning != IR_TUNE_DEFAULT)
      return fail(IR_ERR_UNSUPPORTED, "%s has one kernel: tuning must be 0 (got %d)", single_kernel, args->tuning);
  }
  const int rc = build_attn_params(args, p, false, false);
  if (rc != IR_OK) return rc;
  if (p->q_prescaled) p->scale_log2 = 1.0f;   // IR_FLAG_Q_PRESCALED: the products of q and k ARE the exponents (`scale` is the LSE's unit only)
  return IR_OK;
}

// What ir_attn_rows, ir_attn_match, ir_attn_transfer and ir_attn_topk check of their own arguments, in the order all of them make the checks: every NULL, n_rows, the
// form (0 .. n_forms - 1, `forms` names them), every alignment
struct OutArg { const char* name; const void* ptr; unsigned align; };
template <size_t N>
int check_row_readout(const ir_shared_attn_args* args, const int32_t* row_index, int32_t n_rows, int32_t reduce, int32_t n_forms, const char* forms,
                      const OutArg (&outs)[N]) {
  if (row_index == nullptr) return fail(IR_ERR_INVALID_ARG, "row_index is NULL");
  for (const OutArg& o : outs)
    if (o.ptr == nullptr) return fail(IR_ERR_INVALID_ARG, "%s is NULL", o.name);
  if (args->lse == nullptr) return fail(IR_ERR_INVALID_ARG, "lse is NULL");
  if (n_rows < 1 || n_rows > args->len_q) return fail(IR_ERR_INVALID_ARG, "n_rows %d outside [1, len_q = %d]", n_rows, args->len_q);
  if (reduce < 0 || reduce >= n_forms) return fail(IR_ERR_UNSUPPORTED, "reduce %d: %s", reduce, forms);
  if ((reinterpret_cast<uintptr_t>(row_index) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "row_index must be 4-byte aligned");
  for (const OutArg& o : outs)
    if ((reinterpret_cast<uintptr_t>(o.ptr) & (o.align - 1)) != 0) return fail(IR_ERR_UNSUPPORTED, "%s must be %u-byte aligned", o.name, o.align);
  return IR_OK;
}

}  // namespace

extern "C" {

int ir_abi_version(void) { return IR_ABI_VERSION; }

const char* ir_build_info(void) { return "instantrestore_hip gfx950 (CDNA4) hipcc " __VERSION__ " built " __DATE__; }

const char* ir_last_error_string(void) { return g_err; }

// The kernel a call launches, in words: ir_attn_choose's (or the batch-invariant plan's) choice, formatted with the call's fold /
// valid_refs / seg_mass / pre-scaled flags.  No dispatch rule lives here.
const char* ir_shared_attn_kernel_name(const ir_shared_attn_args* args) {
  AttnKParams p;
  if (build_attn_params(args, &p, false, true) != IR_OK) return "";
  // the launch takes seg_mass only with an output (need_out); for reporting the by-product counts wherever it is asked for - it
  // decides the 128-row kernel's form and whether the default rule takes that kernel.  Never dereferenced here
  p.seg_cum = (float*)args->seg_mass;
  const bool bi = batch_invariant(args), fold = p.aa != nullptr;
  const IrAttnChoice c = bi ? ir_attn_choose_bi(p) : ir_attn_choose(p, args->tuning);
  const char* head = nullptr;        // the name up to the fold
  const char* fold_text = ", AdaIN fold";
  bool forms = false;                // the 128-row kernel's default-mode names say which of its forms run
  switch (c.family) {
    case IR_FAM_REFUSED: return "";
    case IR_FAM_W128: case IR_FAM_W128_FORMS:
      head = "shared_attn_fwd_w128_kernel<128 rows/wave, one wave per SIMD, hand-placed stream, pre-scaled Q";
      fold_text = ", AdaIN ratio-frame fold";
      forms = !bi;
      break;
    case IR_FAM_W64X8:   // (the batch-invariant name does not say how Q arrives)
      head = p.q_prescaled && !bi ? "shared_attn_fwd_w64_kernel<64 rows/wave, 8 waves, pre-scaled Q (reference through the MFMA C operand, checked after the exponentials)"
                                  : "shared_attn_fwd_w64_kernel<64 rows/wave, 8 waves";
      fold_text = ", AdaIN ratio-frame fold";
      break;
    case IR_FAM_W64X4:
      head = "shared_attn_fwd_w64_kernel<64 rows/wave, 4 waves";
      fold_text = ", AdaIN ratio-frame fold";
      break;
    case IR_FAM_PIPE32:
      switch (c.form) {
        case IR_PIPE_EXACT: head = "shared_attn_fwd_pipe_kernel<4 waves, exact rescale"; fold_text = ""; break;
        case IR_PIPE_LAZY: head = "shared_attn_fwd_pipe_kernel<4 waves, lazy max"; fold_text = ""; break;
        case IR_PIPE_PRESC:
          if (p.q_prescaled) head = "shared_attn_fwd_pipe_kernel<4 waves, lazy max, pre-scaled Q";
          else { head = "shared_attn_fwd_pipe_kernel<4 waves, lazy max, pre-scaled Q (Q rounded in the kernel)"; fold_text = ""; }
          break;
        case IR_PIPE_EARLYQK: head = "shared_attn_fwd_pipe_kernel<4 waves, lazy max, early QK"; break;
        case IR_PIPE_POSTCHECK: head = "shared_attn_fwd_pipe_kernel<4 waves, pre-scaled Q, reference checked after the exponentials"; break;
        default: break;
      }
      break;
    default: break;
  }
  if (head == nullptr) return "shared_attn_fwd (tuning variant)";
  static thread_local char name[320];
  int n = snprintf(name, sizeof(name), "%s%s%s%s%s%s%s%s>", head, fold ? fold_text : "", forms && p.valid != nullptr ? ", zero suffix in closed form" : "",
                   forms && p.seg_cum != nullptr ? ", segment masses" : "", bi && c.family == IR_FAM_W128_FORMS ? ", forms" : "",
                   p.key_bias != nullptr ? ", key bias (reference follows every max)" : "", p.ref_lens != nullptr ? ", ragged refs (per-reference counts)" : "",
                   p.q_allow != nullptr ? ", regions (per-query masks, reference per row)" : "");
  if (bi) {   // the plan's cut; the name does not change with seg_mass (the output does not either)
    const IrAttnBiPlan pl = bi_plan_of(args, p);
    snprintf(name + n, sizeof(name) - n, " [batch-invariant: %d piece%s per %d-row item]", pl.pieces, pl.pieces > 1 ? "s" : "", pl.rows);
  }
  return name;
}

size_t ir_shared_attn_workspace_bytes(void) {   // the largest remainder split of any kernel
  return (size_t)kIrXcds * kIrWsPiecesPerXcd * ir_attn_piece_bytes(kIrMaxItemRows, 0);
}

size_t ir_shared_attn_workspace_bytes_for(const ir_shared_attn_args* args) {
  AttnKParams p;
  if (build_attn_params(args, &p, false, true) != IR_OK) return 0;
  if (!batch_invariant(args)) return ir_shared_attn_workspace_bytes();
  return ir_attn_bi_workspace_bytes(bi_plan_of(args, p), p.B);
}

int ir_shared_attn_plan(const ir_shared_attn_args* args, ir_shared_attn_plan_info* plan) {
  if (plan == nullptr) return fail(IR_ERR_INVALID_ARG, "plan is NULL");
  if (plan->struct_size != sizeof(ir_shared_attn_plan_info))
    return fail(IR_ERR_INVALID_ARG, "plan struct_size %u != %zu (ABI mismatch)", plan->struct_size, sizeof(ir_shared_attn_plan_info));
  AttnKParams p;
  const int rc = build_attn_params(args, &p, false, true);
  if (rc != IR_OK) return rc;
  if (!batch_invariant(args)) return fail(IR_ERR_INVALID_ARG, "ir_shared_attn_plan reports the IR_FLAG_BATCH_INVARIANT plan (the default dispatch plans per launch)");
  const IrAttnBiPlan pl = bi_plan_of(args, p);
  plan->kernel = pl.kernel;
  plan->rows_per_item = pl.rows;
  plan->items_per_batch = pl.items;
  plan->pieces_per_item = pl.pieces;
  plan->batch_per_launch = bi_batch_per_launch(pl, p.B, p.ws_bytes);
  plan->workspace_bytes = ir_attn_bi_workspace_bytes(pl, p.B);
  return IR_OK;
}

int ir_shared_attn_fwd(const ir_shared_attn_args* args, void* stream) {
  AttnKParams p;
  const int rc = build_attn_params(args, &p, true, true);
  if (rc != IR_OK) return rc;
  return launch_fwd(args, p, (hipStream_t)stream);
}

int ir_time_shared_attn_fwd(const ir_shared_attn_args* args, int32_t iters, void* stream, float* ms_per_launch) {
  if (ms_per_launch == nullptr || iters <= 0) return fail(IR_ERR_INVALID_ARG, "iters/ms_per_launch");
  AttnKParams p;
  const int rc = build_attn_params(args, &p, true, true);
  if (rc != IR_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(IR_ERR_LAUNCH, "hipEventCreate failed");
  hipError_t e = hipEventRecord(e0, s);
  for (int i = 0; i < iters && e == hipSuccess; ++i)
    e = batch_invariant(args) ? (launch_fwd(args, p, s) == IR_OK ? hipSuccess : hipErrorLaunchFailure)
                              : ir_launch_shared_attn_fwd(p, args->dtype, args->tuning, s);
  if (e == hipSuccess) e = hipEventRecord(e1, s);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "timed launch: %s", hipGetErrorString(e));
  *ms_per_launch = ms / (float)iters;
  return IR_OK;
}

size_t ir_bench_mfma_stream_scratch_bytes(void) { return (size_t)1024 * 512 * sizeof(float); }   // up to 1024 CUs

int ir_bench_mfma_stream(int32_t dtype, int32_t zero_operands, int32_t iters, int32_t launches, void* scratch, size_t scratch_bytes,
                         void* stream, float* tflops) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d: fp16 (0) / bf16 (1)", dtype);
  if (iters <= 0 || launches <= 0 || tflops == nullptr || scratch == nullptr) return fail(IR_ERR_INVALID_ARG, "iters/launches/scratch/tflops");
  const int blocks = ir_device_cus();   // one 8-wave workgroup per CU = two waves per SIMD
  if (blocks > 1024 || scratch_bytes < (size_t)blocks * 512 * sizeof(float)) return fail(IR_ERR_WORKSPACE, "scratch %zu < %zu bytes", scratch_bytes, (size_t)blocks * 512 * sizeof(float));
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(IR_ERR_LAUNCH, "hipEventCreate failed");
  hipError_t e = hipSuccess;
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = ir_launch_bench_mfma_stream(dtype, zero_operands, iters, blocks, (float*)scratch, s);   // untimed: clocks settle
  if (e == hipSuccess) e = hipEventRecord(e0, s);
  for (int i = 0; i < launches && e == hipSuccess; ++i) e = ir_launch_bench_mfma_stream(dtype, zero_operands, iters, blocks, (float*)scratch, s);
  if (e == hipSuccess) e = hipEventRecord(e1, s);
  if (e == hipSuccess) e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "mfma stream: %s", hipGetErrorString(e));
  const double flops = (double)launches * iters * 16.0 * 32768.0 * (double)blocks * 8.0;   // 2 * 32 * 32 * 16 per MFMA, 8 waves per workgroup
  *tflops = (float)(flops / ((double)ms * 1e-3) / 1e12);
  return IR_OK;
}

int ir_attn_probs_ex(const ir_shared_attn_args* args, void* probs, int32_t kernel, void* stream) {
  AttnKParams p;
  const int rc = build_readout_params(args, &p, nullptr);
  if (rc != IR_OK) return rc;
  if (probs == nullptr || args->lse == nullptr) return fail(IR_ERR_INVALID_ARG, "probs/lse is NULL");
  if (kernel < IR_PROBS_AUTO || kernel > IR_PROBS_LINES32_K256) return fail(IR_ERR_UNSUPPORTED, "attn_probs kernel %d", kernel);
  p.probs = probs;
  if (kernel >= IR_PROBS_LINES64 && !ir_attn_probs_uses_lines(p))
    return fail(IR_ERR_UNSUPPORTED, "the line kernel needs len_self, len_ref (and so Lkv) to be multiples of 8 and probs 16-byte aligned");
  const hipError_t e = ir_launch_attn_probs(p, args->dtype, kernel, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "attn_probs launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_attn_probs(const ir_shared_attn_args* args, void* probs, void* stream) { return ir_attn_probs_ex(args, probs, IR_PROBS_AUTO, stream); }

int ir_attn_segment_mass(const ir_shared_attn_args* args, float* mass, void* stream) {
  AttnKParams p;
  const int rc = build_readout_params(args, &p, nullptr);
  if (rc != IR_OK) return rc;
  if (mass == nullptr || args->lse == nullptr) return fail(IR_ERR_INVALID_ARG, "mass/lse is NULL");
  const hipError_t e = ir_launch_attn_segment_mass(p, args->dtype, mass, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "attn_segment_mass launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_attn_rows(const ir_shared_attn_args* args, const int32_t* row_index, int32_t n_rows, int32_t reduce, void* out, void* stream) {
  AttnKParams p;
  int rc = build_readout_params(args, &p, "ir_attn_rows");
  if (rc != IR_OK) return rc;
  const OutArg outs[] = {{"out", out, 16}};
  rc = check_row_readout(args, row_index, n_rows, reduce, 3, "IR_ROWS_NONE (0), IR_ROWS_HEAD_MEAN (1) or IR_ROWS_MAP (2)", outs);
  if (rc != IR_OK) return rc;
  const hipError_t e = ir_launch_attn_rows(p, args->dtype, row_index, n_rows, reduce, out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "attn_rows launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_attn_match(const ir_shared_attn_args* args, const int32_t* row_index, int32_t n_rows, int32_t reduce, int32_t* index, float* prob,
                  void* stream) {
  AttnKParams p;
  int rc = build_readout_params(args, &p, "ir_attn_match");
  if (rc != IR_OK) return rc;
  const OutArg outs[] = {{"index", index, 4}, {"prob", prob, 4}};
  rc = check_row_readout(args, row_index, n_rows, reduce, 2, "IR_MATCH_PER_HEAD (0) or IR_MATCH_HEAD_MEAN (1)", outs);
  if (rc != IR_OK) return rc;
  if (ir_attn_match_items(p, n_rows, reduce) > kMatchMaxItems) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  const hipError_t e = ir_launch_attn_match(p, args->dtype, row_index, n_rows, reduce, index, prob, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "attn_match launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_attn_transfer(const ir_shared_attn_args* args, const float* payload, int64_t pay_sb, int64_t pay_sj, int32_t channels,
                     const int32_t* row_index, int32_t n_rows, int32_t reduce, float* sums, float* mass, void* stream) {
  AttnKParams p;
  int rc = build_readout_params(args, &p, "ir_attn_transfer");
  if (rc != IR_OK) return rc;
  const OutArg outs[] = {{"payload", payload, 4}, {"sums", sums, 4}};
  rc = check_row_readout(args, row_index, n_rows, reduce, 2, "IR_TRANSFER_PER_HEAD (0) or IR_TRANSFER_HEAD_MEAN (1)", outs);
  if (rc != IR_OK) return rc;
  if (mass != nullptr && (reinterpret_cast<uintptr_t>(mass) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "mass must be 4-byte aligned");
  if (channels < 1 || channels > IR_TRANSFER_MAX_CHANNELS)
    return fail(IR_ERR_UNSUPPORTED, "channels %d outside [1, IR_TRANSFER_MAX_CHANNELS = %d] (call again for more)", channels, IR_TRANSFER_MAX_CHANNELS);
  if (pay_sb < 0) return fail(IR_ERR_INVALID_ARG, "pay_sb %lld must be >= 0 (0: one payload for every batch entry)", (long long)pay_sb);
  if (pay_sj < channels) return fail(IR_ERR_INVALID_ARG, "pay_sj %lld must be >= channels %d", (long long)pay_sj, channels);
  if (ir_attn_transfer_items(p, n_rows, reduce) > kTransferMaxItems) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  const hipError_t e = ir_launch_attn_transfer(p, args->dtype, payload, pay_sb, pay_sj, channels, row_index, n_rows, reduce, sums, mass, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "attn_transfer launch: %s", hipGetErrorString(e));
  return IR_OK;
}

// The checks of its own arguments, in this order (the header states it): NULL recv, NULL lse, channels, NULL weights with
// channels != 1, the strides, the form, the alignments, the item count
int ir_attn_received(const ir_shared_attn_args* args, const float* weights, int64_t w_sb, int64_t w_si, int32_t channels,
                     int32_t reduce, float* recv, void* stream) {
  AttnKParams p;
  const int rc = build_readout_params(args, &p, "ir_attn_received");
  if (rc != IR_OK) return rc;
  if (recv == nullptr) return fail(IR_ERR_INVALID_ARG, "recv is NULL");
  if (args->lse == nullptr) return fail(IR_ERR_INVALID_ARG, "lse is NULL");
  if (channels < 1 || channels > IR_RECEIVED_MAX_CHANNELS)
    return fail(IR_ERR_UNSUPPORTED, "channels %d outside [1, IR_RECEIVED_MAX_CHANNELS = %d] (call again for more)", channels, IR_RECEIVED_MAX_CHANNELS);
  if (weights == nullptr && channels != 1) return fail(IR_ERR_INVALID_ARG, "weights is NULL (one channel of ones): channels must be 1 (got %d)", channels);
  if (w_sb < 0) return fail(IR_ERR_INVALID_ARG, "w_sb %lld must be >= 0 (0: one payload for every batch entry)", (long long)w_sb);
  if (w_si < (weights != nullptr ? channels : 0)) return fail(IR_ERR_INVALID_ARG, "w_si %lld must be >= channels %d", (long long)w_si, channels);
  if (reduce != IR_RECEIVED_PER_HEAD && reduce != IR_RECEIVED_HEAD_MEAN)
    return fail(IR_ERR_UNSUPPORTED, "reduce %d: IR_RECEIVED_PER_HEAD (0) or IR_RECEIVED_HEAD_MEAN (1)", reduce);
  if ((reinterpret_cast<uintptr_t>(weights) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "weights must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(recv) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "recv must be 4-byte aligned");
  if (ir_attn_received_items(p, channels, reduce) > kReceivedMaxItems) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  const hipError_t e = ir_launch_attn_received(p, args->dtype, weights, w_sb, w_si, channels, reduce, recv, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "attn_received launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_attn_topk(const ir_shared_attn_args* args, const int32_t* row_index, int32_t n_rows, int32_t k, int32_t reduce,
                 int32_t* index, float* prob, void* stream) {
  AttnKParams p;
  int rc = build_readout_params(args, &p, "ir_attn_topk");
  if (rc != IR_OK) return rc;
  const OutArg outs[] = {{"index", index, 4}, {"prob", prob, 4}};
  rc = check_row_readout(args, row_index, n_rows, reduce, 2, "IR_MATCH_PER_HEAD (0) or IR_MATCH_HEAD_MEAN (1)", outs);
  if (rc != IR_OK) return rc;
  if (k < 1 || k > IR_TOPK_MAX) return fail(IR_ERR_UNSUPPORTED, "k %d outside [1, IR_TOPK_MAX = %d]", k, IR_TOPK_MAX);
  if (ir_attn_topk_items(p, n_rows, reduce) > kTopkMaxItems) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  const hipError_t e = ir_launch_attn_topk(p, args->dtype, row_index, n_rows, k, reduce, index, prob, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "attn_topk launch: %s", hipGetErrorString(e));
  return IR_OK;
}

// The checks of its own arguments, in this order (the header states it): NULL index, NULL prob, NULL lse, the form, the
// alignments, the item count
int ir_attn_key_match(const ir_shared_attn_args* args, int32_t reduce, int32_t* index, float* prob, void* stream) {
  AttnKParams p;
  const int rc = build_readout_params(args, &p, "ir_attn_key_match");
  if (rc != IR_OK) return rc;
  if (index == nullptr) return fail(IR_ERR_INVALID_ARG, "index is NULL");
  if (prob == nullptr) return fail(IR_ERR_INVALID_ARG, "prob is NULL");
  if (args->lse == nullptr) return fail(IR_ERR_INVALID_ARG, "lse is NULL");
  if (reduce != IR_MATCH_PER_HEAD && reduce != IR_MATCH_HEAD_MEAN)
    return fail(IR_ERR_UNSUPPORTED, "reduce %d: IR_MATCH_PER_HEAD (0) or IR_MATCH_HEAD_MEAN (1)", reduce);
  if ((reinterpret_cast<uintptr_t>(index) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "index must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(prob) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "prob must be 4-byte aligned");
  if (ir_attn_key_match_items(p, reduce) > kKeyMatchMaxItems) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  const hipError_t e = ir_launch_attn_key_match(p, args->dtype, reduce, index, prob, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "attn_key_match launch: %s", hipGetErrorString(e));
  return IR_OK;
}

static int adain_nchunk(int32_t len_self, int32_t len_ref) {
  const int a = (len_self + IR_ADAIN_ROWS - 1) / IR_ADAIN_ROWS;
  const int b = (len_ref + IR_ADAIN_ROWS - 1) / IR_ADAIN_ROWS;
  const int m = a > b ? a : b;
  return m > 0 ? m : 1;
}

size_t ir_adain_stats_workspace_bytes(int32_t batch, int32_t heads, int32_t len_self, int32_t n_refs, int32_t len_ref) {
  if (batch <= 0 || heads <= 0 || n_refs < 0) return 0;
  return (size_t)batch * (size_t)(1 + n_refs) * (size_t)heads * (size_t)adain_nchunk(len_self, len_ref) * 128u * sizeof(float);
}

int ir_adain_stats(int32_t dtype, int32_t batch, int32_t heads, int32_t len_self, int32_t n_refs, int32_t len_ref,
                   const void* v_self, int64_t vs_sb, int64_t vs_sl, int64_t vs_sh,
                   const void* v_ref, int64_t vr_sb, int64_t vr_sn, int64_t vr_sl, int64_t vr_sh,
                   float eps, float* a, float* b, void* workspace, size_t workspace_bytes, void* stream) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (batch <= 0 || heads <= 0 || len_self <= 0 || n_refs <= 0 || len_ref <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!v_self || !v_ref || !a || !b || !workspace) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (!aligned16(v_self) || !aligned16(v_ref)) return fail(IR_ERR_UNSUPPORTED, "v_self/v_ref must be 16-byte aligned");
  const int64_t st[] = {vs_sb, vs_sl, vs_sh, vr_sb, vr_sn, vr_sl, vr_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "stride %lld must be a non-negative multiple of 8", (long long)s);
  const size_t need = ir_adain_stats_workspace_bytes(batch, heads, len_self, n_refs, len_ref);
  if (workspace_bytes < need) return fail(IR_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  AdainKParams p;
  memset(&p, 0, sizeof(p));
  p.v_self = v_self; p.v_ref = v_ref;
  p.vs_sb = vs_sb; p.vs_sl = vs_sl; p.vs_sh = vs_sh;
  p.vr_sb = vr_sb; p.vr_sn = vr_sn; p.vr_sl = vr_sl; p.vr_sh = vr_sh;
  p.ws = (float*)workspace; p.a = a; p.b = b;
  p.B = batch; p.H = heads; p.Ls = len_self; p.N = n_refs; p.Lr = len_ref;
  p.nchunk = adain_nchunk(len_self, len_ref);
  p.eps = eps;
  const hipError_t e = ir_launch_adain_stats(p, dtype, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "adain_stats launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_adain_stats_cached(int32_t dtype, int32_t batch, int32_t heads, int32_t len_self, int32_t n_refs,
                          const void* v_self, int64_t vs_sb, int64_t vs_sl, int64_t vs_sh,
                          const float* content_mean, const float* content_std,
                          float eps, float* a, float* b, void* workspace, size_t workspace_bytes, void* stream) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (batch <= 0 || heads <= 0 || len_self <= 0 || n_refs <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!v_self || !content_mean || !content_std || !a || !b || !workspace) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (!aligned16(v_self)) return fail(IR_ERR_UNSUPPORTED, "v_self must be 16-byte aligned");
  const int64_t st[] = {vs_sb, vs_sl, vs_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "stride %lld must be a non-negative multiple of 8", (long long)s);
  const size_t need = ir_adain_stats_workspace_bytes(batch, heads, len_self, 0, len_self);
  if (workspace_bytes < need) return fail(IR_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  AdainKParams p;
  memset(&p, 0, sizeof(p));
  p.v_self = v_self; p.v_ref = v_self;
  p.vs_sb = vs_sb; p.vs_sl = vs_sl; p.vs_sh = vs_sh;
  p.ws = (float*)workspace; p.a = a; p.b = b;
  p.B = batch; p.H = heads; p.Ls = len_self; p.N = n_refs; p.Lr = len_self;
  p.nchunk = adain_nchunk(len_self, len_self);
  p.eps = eps;
  p.cmean = content_mean; p.cstd = content_std;
  const hipError_t e = ir_launch_adain_stats_cached(p, dtype, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "adain_stats_cached launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_token_stats(int32_t dtype, int32_t batch, int32_t heads, int32_t n_mats, int32_t len,
                   const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                   float* mean, float* std, void* workspace, size_t workspace_bytes, void* stream) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (batch <= 0 || heads <= 0 || n_mats <= 0 || len <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!x || !mean || !std || !workspace) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (!aligned16(x)) return fail(IR_ERR_UNSUPPORTED, "x must be 16-byte aligned");
  const int64_t st[] = {x_sb, x_sn, x_sl, x_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "stride %lld must be a non-negative multiple of 8", (long long)s);
  const size_t need = ir_adain_stats_workspace_bytes(batch, heads, len, n_mats - 1, len);
  if (workspace_bytes < need) return fail(IR_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  // matrix 0 of every batch entry plays the "self" role of the partial kernel, 1.. the "refs"
  AdainKParams p;
  memset(&p, 0, sizeof(p));
  p.v_self = x; p.v_ref = (const char*)x + x_sn * 2;
  p.vs_sb = x_sb; p.vs_sl = x_sl; p.vs_sh = x_sh;
  p.vr_sb = x_sb; p.vr_sn = x_sn; p.vr_sl = x_sl; p.vr_sh = x_sh;
  p.ws = (float*)workspace; p.a = mean; p.b = std;
  p.B = batch; p.H = heads; p.Ls = len; p.N = n_mats - 1; p.Lr = len;
  p.nchunk = adain_nchunk(len, len);
  const hipError_t e = ir_launch_token_stats(p, dtype, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "token_stats launch: %s", hipGetErrorString(e));
  return IR_OK;
}

static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

size_t ir_token_stats_weighted_workspace_bytes(int32_t batch, int32_t heads, int32_t n_mats, int32_t len) {
  if (batch <= 0 || heads <= 0 || n_mats <= 0 || len <= 0) return 0;
  return (size_t)batch * (size_t)n_mats * (size_t)heads * (size_t)adain_nchunk(len, len) * IR_ADAIN_W_STRIDE * sizeof(float);
}

// Checked in this order (the header states it): dtype, sizes, NULL x / mean / std / workspace, the 16-byte rule of x, the
// weights' strides, the counts' stride, the 4-byte alignments, the grid, the workspace
int ir_token_stats_weighted(int32_t dtype, int32_t batch, int32_t heads, int32_t n_mats, int32_t len,
                            const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                            const float* weights, int64_t w_sb, int64_t w_sn, const int32_t* lens, int64_t ln_sb,
                            float* mean, float* std, float* wsum, void* workspace, size_t workspace_bytes, void* stream) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d: only fp16 (0) and bf16 (1) are implemented", dtype);
  if (batch <= 0 || heads <= 0 || n_mats <= 0 || len <= 0)
    return fail(IR_ERR_INVALID_ARG, "batch %d, heads %d, n_mats %d and len %d must be > 0", batch, heads, n_mats, len);
  if (x == nullptr) return fail(IR_ERR_INVALID_ARG, "x is NULL");
  if (mean == nullptr) return fail(IR_ERR_INVALID_ARG, "mean is NULL");
  if (std == nullptr) return fail(IR_ERR_INVALID_ARG, "std is NULL");
  if (workspace == nullptr) return fail(IR_ERR_INVALID_ARG, "workspace is NULL");
  if (!aligned16(x)) return fail(IR_ERR_UNSUPPORTED, "x must be 16-byte aligned");
  const int64_t st[] = {x_sb, x_sn, x_sl, x_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "x stride %lld must be a non-negative multiple of 8", (long long)s);
  if (weights != nullptr) {
    if (w_sn < len) return fail(IR_ERR_INVALID_ARG, "weights matrix stride w_sn %lld must be >= len %d", (long long)w_sn, len);
    if (w_sb < 0) return fail(IR_ERR_INVALID_ARG, "weights batch stride w_sb %lld must be >= 0", (long long)w_sb);
  }
  if (lens != nullptr && ln_sb < n_mats) return fail(IR_ERR_INVALID_ARG, "lens row stride ln_sb %lld must be >= n_mats %d", (long long)ln_sb, n_mats);
  if (!aligned4(weights)) return fail(IR_ERR_UNSUPPORTED, "weights must be 4-byte aligned");
  if (!aligned4(lens)) return fail(IR_ERR_UNSUPPORTED, "lens must be 4-byte aligned");
  if (!aligned4(mean)) return fail(IR_ERR_UNSUPPORTED, "mean must be 4-byte aligned");
  if (!aligned4(std)) return fail(IR_ERR_UNSUPPORTED, "std must be 4-byte aligned");
  if (!aligned4(wsum)) return fail(IR_ERR_UNSUPPORTED, "wsum must be 4-byte aligned");
  if ((int64_t)batch * n_mats > 65535 || heads > 65535) return fail(IR_ERR_UNSUPPORTED, "grid too large: batch * n_mats and heads must be <= 65535");
  const size_t need = ir_token_stats_weighted_workspace_bytes(batch, heads, n_mats, len);
  if (workspace_bytes < need) return fail(IR_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  TokenStatsWKParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.x_sb = x_sb; p.x_sn = x_sn; p.x_sl = x_sl; p.x_sh = x_sh;
  p.weights = weights; p.w_sb = w_sb; p.w_sn = w_sn;
  p.lens = lens; p.ln_sb = ln_sb;
  p.ws = (float*)workspace; p.mean = mean; p.std = std; p.wsum = wsum;
  p.B = batch; p.M = n_mats; p.H = heads; p.len = len;
  p.nchunk = adain_nchunk(len, len);
  const hipError_t e = ir_launch_token_stats_weighted(p, dtype, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "token_stats_weighted launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_adain_affine_from_stats(int32_t batch, int32_t heads, int32_t n_refs,
                               const float* style_mean, const float* style_std, const float* content_mean, const float* content_std,
                               float eps, float* a, float* b, void* stream) {
  if (batch <= 0 || heads <= 0 || n_refs <= 0) return fail(IR_ERR_INVALID_ARG, "batch %d, heads %d and n_refs %d must be > 0", batch, heads, n_refs);
  if (style_mean == nullptr || style_std == nullptr) return fail(IR_ERR_INVALID_ARG, "style_mean / style_std is NULL");
  if (content_mean == nullptr || content_std == nullptr) return fail(IR_ERR_INVALID_ARG, "content_mean / content_std is NULL");
  if (a == nullptr || b == nullptr) return fail(IR_ERR_INVALID_ARG, "a / b is NULL");
  if (!aligned4(style_mean) || !aligned4(style_std) || !aligned4(content_mean) || !aligned4(content_std) || !aligned4(a) || !aligned4(b))
    return fail(IR_ERR_UNSUPPORTED, "style_mean, style_std, content_mean, content_std, a and b must be 4-byte aligned");
  if ((int64_t)batch * n_refs * heads > (0x7fffffffLL / 64) * 256) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  const hipError_t e = ir_launch_adain_affine_from_stats(style_mean, style_std, content_mean, content_std, eps, a, b, batch, n_refs, heads,
                                                         (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "adain_affine_from_stats launch: %s", hipGetErrorString(e));
  return IR_OK;
}

size_t ir_token_stats_labelled_workspace_bytes(int32_t batch, int32_t heads, int32_t n_mats, int32_t len, int32_t n_regions) {
  if (batch <= 0 || heads <= 0 || n_mats <= 0 || len <= 0 || n_regions <= 0 || n_regions > IR_ADAIN_REGIONS_MAX) return 0;
  return (size_t)batch * (size_t)n_mats * (size_t)n_regions * (size_t)heads * (size_t)adain_nchunk(len, len) * IR_ADAIN_W_STRIDE * sizeof(float);
}

// Checked in this order (the header states it): dtype, sizes, n_regions, NULL x / labels / mean / std / workspace, the 16-byte
// rule of x, the labels' strides, the 4-byte alignments, the grid, the workspace
int ir_token_stats_labelled(int32_t dtype, int32_t batch, int32_t heads, int32_t n_mats, int32_t len, int32_t n_regions,
                           const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                           const int32_t* labels, int64_t lb_sb, int64_t lb_sn,
                           float* mean, float* std, float* count, void* workspace, size_t workspace_bytes, void* stream) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d: only fp16 (0) and bf16 (1) are implemented", dtype);
  if (batch <= 0 || heads <= 0 || n_mats <= 0 || len <= 0)
    return fail(IR_ERR_INVALID_ARG, "batch %d, heads %d, n_mats %d and len %d must be > 0", batch, heads, n_mats, len);
  if (n_regions < 1 || n_regions > IR_ADAIN_REGIONS_MAX)
    return fail(IR_ERR_INVALID_ARG, "n_regions %d must be in [1, %d]", n_regions, IR_ADAIN_REGIONS_MAX);
  if (x == nullptr) return fail(IR_ERR_INVALID_ARG, "x is NULL");
  if (labels == nullptr) return fail(IR_ERR_INVALID_ARG, "labels is NULL");
  if (mean == nullptr) return fail(IR_ERR_INVALID_ARG, "mean is NULL");
  if (std == nullptr) return fail(IR_ERR_INVALID_ARG, "std is NULL");
  if (workspace == nullptr) return fail(IR_ERR_INVALID_ARG, "workspace is NULL");
  if (!aligned16(x)) return fail(IR_ERR_UNSUPPORTED, "x must be 16-byte aligned");
  const int64_t st[] = {x_sb, x_sn, x_sl, x_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "x stride %lld must be a non-negative multiple of 8", (long long)s);
  if (lb_sn < len) return fail(IR_ERR_INVALID_ARG, "labels matrix stride lb_sn %lld must be >= len %d", (long long)lb_sn, len);
  if (lb_sb < 0) return fail(IR_ERR_INVALID_ARG, "labels batch stride lb_sb %lld must be >= 0", (long long)lb_sb);
  if (!aligned4(labels)) return fail(IR_ERR_UNSUPPORTED, "labels must be 4-byte aligned");
  if (!aligned4(mean)) return fail(IR_ERR_UNSUPPORTED, "mean must be 4-byte aligned");
  if (!aligned4(std)) return fail(IR_ERR_UNSUPPORTED, "std must be 4-byte aligned");
  if (!aligned4(count)) return fail(IR_ERR_UNSUPPORTED, "count must be 4-byte aligned");
  if ((int64_t)batch * n_mats > 65535 || heads > 65535 || (int64_t)batch * n_mats * n_regions * heads > 0x7fffffffLL)
    return fail(IR_ERR_UNSUPPORTED, "grid too large: batch * n_mats and heads must be <= 65535, batch * n_mats * n_regions * heads < 2^31");
  const size_t need = ir_token_stats_labelled_workspace_bytes(batch, heads, n_mats, len, n_regions);
  if (workspace_bytes < need) return fail(IR_ERR_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
  TokenStatsRKParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.x_sb = x_sb; p.x_sn = x_sn; p.x_sl = x_sl; p.x_sh = x_sh;
  p.labels = labels; p.lb_sb = lb_sb; p.lb_sn = lb_sn;
  p.ws = (float*)workspace; p.mean = mean; p.std = std; p.count = count;
  p.B = batch; p.M = n_mats; p.H = heads; p.len = len; p.R = n_regions;
  p.nchunk = adain_nchunk(len, len);
  const hipError_t e = ir_launch_token_stats_regions(p, dtype, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "token_stats_regions launch: %s", hipGetErrorString(e));
  return IR_OK;
}

// Checked in this order (the header states it): dtype, sizes, n_regions, NULL x / y / a / b / labels, the 16-byte rule of x and
// y, the labels' strides, the 4-byte alignments
int ir_adain_apply_labelled(int32_t dtype, int32_t batch, int32_t heads, int32_t n_refs, int32_t len, int32_t n_regions,
                           const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                           const int32_t* labels, int64_t lb_sb, int64_t lb_sn, const float* a, const float* b,
                           void* y, int64_t y_sb, int64_t y_sn, int64_t y_sl, int64_t y_sh, void* stream) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d: only fp16 (0) and bf16 (1) are implemented", dtype);
  if (batch <= 0 || heads <= 0 || n_refs <= 0 || len <= 0)
    return fail(IR_ERR_INVALID_ARG, "batch %d, heads %d, n_refs %d and len %d must be > 0", batch, heads, n_refs, len);
  if (n_regions < 1 || n_regions > IR_ADAIN_REGIONS_MAX)
    return fail(IR_ERR_INVALID_ARG, "n_regions %d must be in [1, %d]", n_regions, IR_ADAIN_REGIONS_MAX);
  if (x == nullptr) return fail(IR_ERR_INVALID_ARG, "x is NULL");
  if (y == nullptr) return fail(IR_ERR_INVALID_ARG, "y is NULL");
  if (a == nullptr || b == nullptr) return fail(IR_ERR_INVALID_ARG, "a / b is NULL");
  if (labels == nullptr) return fail(IR_ERR_INVALID_ARG, "labels is NULL");
  if (!aligned16(x) || !aligned16(y)) return fail(IR_ERR_UNSUPPORTED, "x / y must be 16-byte aligned");
  const int64_t st[] = {x_sb, x_sn, x_sl, x_sh, y_sb, y_sn, y_sl, y_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "stride %lld must be a non-negative multiple of 8", (long long)s);
  if (lb_sn < len) return fail(IR_ERR_INVALID_ARG, "labels matrix stride lb_sn %lld must be >= len %d", (long long)lb_sn, len);
  if (lb_sb < 0) return fail(IR_ERR_INVALID_ARG, "labels batch stride lb_sb %lld must be >= 0", (long long)lb_sb);
  if (!aligned4(labels) || !aligned4(a) || !aligned4(b)) return fail(IR_ERR_UNSUPPORTED, "labels, a and b must be 4-byte aligned");
  AdainApplyRKParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.y = y; p.a = a; p.b = b;
  p.labels = labels; p.lb_sb = lb_sb; p.lb_sn = lb_sn;
  p.x_sb = x_sb; p.x_sn = x_sn; p.x_sl = x_sl; p.x_sh = x_sh;
  p.y_sb = y_sb; p.y_sn = y_sn; p.y_sl = y_sl; p.y_sh = y_sh;
  p.B = batch; p.H = heads; p.N = n_refs; p.L = len; p.R = n_regions;
  const hipError_t e = ir_launch_adain_apply_regions(p, dtype, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "adain_apply_regions launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_adain_apply(int32_t dtype, int32_t batch, int32_t heads, int32_t n_refs, int32_t len,
                   const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                   const float* a, const float* b,
                   void* y, int64_t y_sb, int64_t y_sn, int64_t y_sl, int64_t y_sh, void* stream) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (batch <= 0 || heads <= 0 || n_refs <= 0 || len <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!x || !y || !a || !b) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (!aligned16(x) || !aligned16(y)) return fail(IR_ERR_UNSUPPORTED, "x/y must be 16-byte aligned");
  const int64_t st[] = {x_sb, x_sn, x_sl, x_sh, y_sb, y_sn, y_sl, y_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "stride %lld must be a non-negative multiple of 8", (long long)s);
  AdainApplyKParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.y = y; p.a = a; p.b = b;
  p.x_sb = x_sb; p.x_sn = x_sn; p.x_sl = x_sl; p.x_sh = x_sh;
  p.y_sb = y_sb; p.y_sn = y_sn; p.y_sl = y_sl; p.y_sh = y_sh;
  p.B = batch; p.H = heads; p.N = n_refs; p.L = len;
  const hipError_t e = ir_launch_adain_apply(p, dtype, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "adain_apply launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_zero_invalid_refs(int32_t batch, int32_t heads, int32_t n_refs, int32_t len, const int32_t* valid,
                         void* k, int64_t k_sb, int64_t k_sn, int64_t k_sl, int64_t k_sh,
                         void* v, int64_t v_sb, int64_t v_sn, int64_t v_sl, int64_t v_sh, void* stream) {
  if (batch <= 0 || heads <= 0 || n_refs <= 0 || len <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!valid || !k || !v) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (!aligned16(k) || !aligned16(v)) return fail(IR_ERR_UNSUPPORTED, "k/v must be 16-byte aligned");
  const int64_t st[] = {k_sb, k_sn, k_sl, k_sh, v_sb, v_sn, v_sl, v_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "stride %lld must be a non-negative multiple of 8", (long long)s);
  ZeroRefsKParams p;
  memset(&p, 0, sizeof(p));
  p.k = k; p.v = v; p.valid = valid;
  p.k_sb = k_sb; p.k_sn = k_sn; p.k_sl = k_sl; p.k_sh = k_sh;
  p.v_sb = v_sb; p.v_sn = v_sn; p.v_sl = v_sl; p.v_sh = v_sh;
  p.B = batch; p.H = heads; p.N = n_refs; p.L = len;
  const hipError_t e = ir_launch_zero_refs(p, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "zero_refs launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_compact_ref_tokens(int32_t dtype, int32_t batch, int32_t heads, int32_t n_refs, int32_t len_ref,
                          const void* k_in, int64_t ki_sb, int64_t ki_sn, int64_t ki_sl, int64_t ki_sh,
                          const void* v_in, int64_t vi_sb, int64_t vi_sn, int64_t vi_sl, int64_t vi_sh,
                          const uint8_t* keep,
                          void* k_out, int64_t ko_sb, int64_t ko_sn, int64_t ko_sl, int64_t ko_sh,
                          void* v_out, int64_t vo_sb, int64_t vo_sn, int64_t vo_sl, int64_t vo_sh,
                          int32_t* ref_lens, int64_t rl_sb, void* stream) {
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d", dtype);
  if (batch <= 0 || heads <= 0 || n_refs <= 0 || len_ref <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!k_in || !v_in || !keep || !k_out || !v_out || !ref_lens) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (!aligned16(k_in) || !aligned16(v_in) || !aligned16(k_out) || !aligned16(v_out)) return fail(IR_ERR_UNSUPPORTED, "k/v must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(ref_lens) & 3u) != 0) return fail(IR_ERR_UNSUPPORTED, "ref_lens must be 4-byte aligned");
  if (rl_sb < n_refs) return fail(IR_ERR_INVALID_ARG, "ref_lens row stride rl_sb %lld must be >= n_refs %d", (long long)rl_sb, n_refs);
  const int64_t st[] = {ki_sb, ki_sn, ki_sl, ki_sh, vi_sb, vi_sn, vi_sl, vi_sh, ko_sb, ko_sn, ko_sl, ko_sh, vo_sb, vo_sn, vo_sl, vo_sh};
  for (int64_t s : st) if (!stride_ok(s)) return fail(IR_ERR_UNSUPPORTED, "stride %lld must be a non-negative multiple of 8", (long long)s);
  if ((int64_t)batch * n_refs > 0x7fffffffLL) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  {
    // no aliasing: the byte span of each output (first to last element the strides reach) must not meet the span of an input or of the
    // other output - a kernel that reads rows another workgroup has already overwritten would not be deterministic.  Spans, not
    // elements: outputs interleaved with anything else in one allocation are refused too
    struct Span { uintptr_t lo, hi; };
    auto span = [&](const void* base, int64_t sb, int64_t sn, int64_t sl, int64_t sh) {
      const int64_t last = (int64_t)(batch - 1) * sb + (int64_t)(n_refs - 1) * sn + (int64_t)(len_ref - 1) * sl + (int64_t)(heads - 1) * sh + 64;
      return Span{reinterpret_cast<uintptr_t>(base), reinterpret_cast<uintptr_t>(base) + (uintptr_t)last * 2};
    };
    auto meet = [](Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; };
    const Span ki = span(k_in, ki_sb, ki_sn, ki_sl, ki_sh), vi = span(v_in, vi_sb, vi_sn, vi_sl, vi_sh);
    const Span ko = span(k_out, ko_sb, ko_sn, ko_sl, ko_sh), vo = span(v_out, vo_sb, vo_sn, vo_sl, vo_sh);
    if (meet(ko, ki) || meet(ko, vi) || meet(vo, ki) || meet(vo, vi) || meet(ko, vo))
      return fail(IR_ERR_INVALID_ARG, "ir_compact_ref_tokens: the byte spans of the outputs must not overlap the inputs or each other (no aliasing)");
  }
  CompactRefsKParams p;
  memset(&p, 0, sizeof(p));
  p.k_in = k_in; p.v_in = v_in; p.k_out = k_out; p.v_out = v_out; p.keep = keep; p.ref_lens = ref_lens; p.rl_sb = rl_sb;
  p.ki_sb = ki_sb; p.ki_sn = ki_sn; p.ki_sl = ki_sl; p.ki_sh = ki_sh;
  p.vi_sb = vi_sb; p.vi_sn = vi_sn; p.vi_sl = vi_sl; p.vi_sh = vi_sh;
  p.ko_sb = ko_sb; p.ko_sn = ko_sn; p.ko_sl = ko_sl; p.ko_sh = ko_sh;
  p.vo_sb = vo_sb; p.vo_sn = vo_sn; p.vo_sl = vo_sl; p.vo_sh = vo_sh;
  p.B = batch; p.H = heads; p.N = n_refs; p.L = len_ref;
  const hipError_t e = ir_launch_compact_refs(p, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "compact_refs launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_tensor2im_u8(int32_t dtype, int32_t batch, int32_t channels, int32_t height, int32_t width, const void* x,
                    int64_t x_sb, int64_t x_sc, int64_t x_sh, int64_t x_sw, void* out_u8, void* stream) {
  if (dtype < 0 || dtype > 2) return fail(IR_ERR_UNSUPPORTED, "dtype %d (0 f16, 1 bf16, 2 f32)", dtype);
  if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!x || !out_u8) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  const hipError_t e = ir_launch_tensor2im(x, out_u8, dtype, x_sb, x_sc, x_sh, x_sw, batch, channels, height, width,
                                           (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "tensor2im launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_lanczos_ksize(int32_t in_size, int32_t out_size) {
  if (in_size <= 0 || out_size <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  return ir_host_lanczos_ksize(in_size, out_size);
}

int ir_lanczos_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* kk) {
  if (in_size <= 0 || out_size <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!bounds || !kk) return fail(IR_ERR_INVALID_ARG, "NULL table");
  ir_host_lanczos_coeffs(in_size, out_size, bounds, kk);
  return IR_OK;
}

int ir_preprocess_lanczos_u8(const ir_image_desc* images, int32_t n_images, int32_t size, int32_t out_dtype,
                             void* out, void* stream) {
  if (out_dtype < 0 || out_dtype > 2) return fail(IR_ERR_UNSUPPORTED, "out_dtype %d (0 f16, 1 bf16, 2 f32)", out_dtype);
  if (!images || !out || n_images <= 0 || size <= 0) return fail(IR_ERR_INVALID_ARG, "NULL pointer or empty batch");
  for (int i = 0; i < n_images; ++i) {
    const ir_image_desc& d = images[i];
    if (!d.src || !d.bounds_h || !d.kk_h || !d.bounds_v || !d.kk_v || !d.tmp)
      return fail(IR_ERR_INVALID_ARG, "image %d: NULL pointer", i);
    if (d.in_h <= 0 || d.in_w <= 0 || d.src_row_bytes < (int64_t)d.in_w * 3)
      return fail(IR_ERR_INVALID_ARG, "image %d: bad source geometry", i);
    if (d.out_h < size || d.out_w < size || d.crop_top < 0 || d.crop_left < 0 || d.crop_top + size > d.out_h ||
        d.crop_left + size > d.out_w)
      return fail(IR_ERR_INVALID_ARG, "image %d: crop %dx%d at (%d,%d) outside the %dx%d resized image", i, size, size,
                  d.crop_top, d.crop_left, d.out_h, d.out_w);
    if (d.ksize_h <= 0 || d.ksize_v <= 0 || d.row_first < 0 || d.row_count <= 0 || d.row_first + d.row_count > d.in_h)
      return fail(IR_ERR_INVALID_ARG, "image %d: bad tap tables / row range", i);
    if (d.col_first < 0 || d.col_count <= 0 || d.col_first + d.col_count > d.in_w)
      return fail(IR_ERR_INVALID_ARG, "image %d: bad column range", i);
    if ((int64_t)d.col_count * 3 > 60000) return fail(IR_ERR_UNSUPPORTED, "image %d: more than 20000 source columns under the crop", i);
    if (reinterpret_cast<uintptr_t>(d.tmp) & 3u) return fail(IR_ERR_UNSUPPORTED, "image %d: tmp must be 4-byte aligned", i);
  }
  for (int first = 0; first < n_images; first += kPreprocessImagesPerLaunch) {
    PreprocessKParams p;
    memset(&p, 0, sizeof(p));
    p.n = n_images - first < kPreprocessImagesPerLaunch ? n_images - first : kPreprocessImagesPerLaunch;
    p.size = size;
    p.first_image = first;
    p.tmp_pitch = (size * 3 + 3) & ~3;
    int max_rows = 0, max_span = 0, max_ksv = 0;
    for (int i = 0; i < p.n; ++i) {
      const ir_image_desc& d = images[first + i];
      ResampleImageK& k = p.img[i];
      k.src = (const unsigned char*)d.src; k.src_row_bytes = d.src_row_bytes;
      k.bounds_h = d.bounds_h; k.kk_h = d.kk_h; k.bounds_v = d.bounds_v; k.kk_v = d.kk_v;
      k.tmp = (unsigned char*)d.tmp; k.ksize_h = d.ksize_h; k.ksize_v = d.ksize_v;
      k.crop_top = d.crop_top; k.crop_left = d.crop_left; k.row_first = d.row_first; k.row_count = d.row_count;
      k.col_first = d.col_first; k.col_count = d.col_count; k.in_h = d.in_h; k.in_w = d.in_w; k.out_w = d.out_w;
      if (d.row_count > max_rows) max_rows = d.row_count;
      if (d.col_count * 3 > max_span) max_span = d.col_count * 3;
      if (d.ksize_v > max_ksv) max_ksv = d.ksize_v;
    }
    const hipError_t e = ir_launch_preprocess(p, max_rows, max_span, max_ksv, out_dtype, out, (hipStream_t)stream);
    if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "preprocess launch: %s", hipGetErrorString(e));
  }
  return IR_OK;
}

int ir_freeu_fourier_filter(int32_t dtype, int64_t planes, int32_t height, int32_t width, const void* x,
                            int64_t x_plane_stride, void* out, int64_t out_plane_stride, int32_t threshold,
                            float scale, void* stream) {
  if (dtype < 0 || dtype > 2) return fail(IR_ERR_UNSUPPORTED, "dtype %d (0 f16, 1 bf16, 2 f32)", dtype);
  if (!x || !out) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (planes <= 0 || height <= 0 || width <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if ((int64_t)height * width > 4096) return fail(IR_ERR_UNSUPPORTED, "plane %dx%d: at most 4096 elements", height, width);
  if (threshold < 1 || 2 * threshold > height || 2 * threshold > width)
    return fail(IR_ERR_INVALID_ARG, "threshold %d outside [1, min(H,W)/2]", threshold);
  if (x_plane_stride < (int64_t)height * width || out_plane_stride < (int64_t)height * width)
    return fail(IR_ERR_INVALID_ARG, "plane stride smaller than a plane");
  if ((planes + 3) / 4 > 0x7fffffffLL) return fail(IR_ERR_UNSUPPORTED, "grid too large");
  const hipError_t e = ir_launch_freeu_fourier(x, out, dtype, planes, height, width, x_plane_stride, out_plane_stride,
                                               threshold, scale, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "freeu launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_linear_fwd(int32_t dtype, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                  int64_t w_ld, const void* bias, void* y, int64_t y_ld, void* stream) {
  return ir_linear_fwd_scaled(dtype, 0, m, n, k, x, x_ld, w, w_ld, bias, y, y_ld, 0, 1.0f, stream);
}

int ir_linear_fwd_scaled(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                         int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                         void* stream) {
  return ir_linear_fwd_ex(dtype, x_is_f32, m, n, k, x, x_ld, w, w_ld, bias, y, y_ld, scale_cols, col_scale, IR_LIN_AUTO, stream);
}

static bool x_stationary_covers(int32_t n, int32_t k, const void* bias) {
  return ((k % 64 == 0 && k <= 320) || k == 640) && n % 32 == 0 && (bias == nullptr || n <= kLinearMaxBiasN);
}

// ABI v10 (IR_LIN_BATCH_INVARIANT): one kernel per (N, K, bias) whatever M is, and never a split contraction - every element of y
// is the same fp32 sum in the same order at any number of rows
static int linear_kernel_batch_invariant(int32_t n, int32_t k, int32_t has_bias) {
  static const int dummy = 0;
  if (k % 64 == 0 && n % 64 == 0) return IR_LIN_TILED_FIRST + IR_LIN_TILE_256x256;
  return x_stationary_covers(n, k, has_bias ? (const void*)&dummy : nullptr) ? IR_LIN_X_STATIONARY : -1;
}

int ir_linear_kernel_for_ex(int64_t m, int32_t n, int32_t k, int32_t has_bias, int32_t selector) {
  if (selector == IR_LIN_AUTO) return ir_linear_kernel_for(m, n, k, has_bias);
  if (selector == IR_LIN_BATCH_INVARIANT) return m > 0 ? linear_kernel_batch_invariant(n, k, has_bias) : -1;
  return -1;
}

int ir_linear_kernel_for(int64_t m, int32_t n, int32_t k, int32_t has_bias) {
  static const int dummy = 0;
  const bool xs = x_stationary_covers(n, k, has_bias ? (const void*)&dummy : nullptr);
  const bool tiled = (k % 64 == 0) && (n % 64 == 0);
  if (!xs && !tiled) return -1;
  if (!tiled) return IR_LIN_X_STATIONARY;
  // the X-stationary kernels read X once (and cast fp32 activations once) and win where that is the traffic that
  // matters: large M.  From profiles/r3_gemm_probe_final.txt: at 131072 rows they lead (K = 320: 122 vs 167 us), at 32768
  // rows the 256x256 tile leads or ties (32768 x 960 x 320: 33 vs 43 us; x 1920 x 640: 100 vs 100; x 640 x 640: 39-46 vs 44-54)
  if (xs && m >= 65536) return IR_LIN_X_STATIONARY;
  return IR_LIN_TILED_FIRST + ir_linear_tiled_pick(m, n, k);
}

static int linear_fwd_impl(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                           int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                           int32_t kernel, int32_t st_col0, int32_t st_cols, float* st_ws, size_t st_ws_bytes, void* stream);

int ir_linear_fwd_ex(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                     int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                     int32_t kernel, void* stream) {
  return linear_fwd_impl(dtype, x_is_f32, m, n, k, x, x_ld, w, w_ld, bias, y, y_ld, scale_cols, col_scale, kernel, 0, 0, nullptr, 0, stream);
}

static int stats_rows_of(int kernel) {   // every projection kernel gives a wave 64 rows of Y: the statistics block
  if (kernel == IR_LIN_X_STATIONARY) return 64;
  if (kernel >= IR_LIN_TILED_FIRST && kernel < IR_LIN_TILED_FIRST + IR_LIN_TILE_COUNT) return 64;
  return 0;
}

int ir_linear_stats_rows(int64_t m, int32_t n, int32_t k, int32_t has_bias) {
  if (m <= 0 || n <= 0 || k <= 0 || (n % 64) != 0) return 0;
  const int rows = stats_rows_of(ir_linear_kernel_for(m, n, k, has_bias));
  return (rows > 0 && (m % rows) == 0) ? rows : 0;
}

int ir_linear_fwd_stats(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                        int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                        int32_t stats_col0, int32_t stats_cols, float* stats_ws, size_t stats_ws_bytes, void* stream) {
  if (stats_ws == nullptr) return fail(IR_ERR_INVALID_ARG, "stats_ws is NULL (use ir_linear_fwd_scaled for a call without statistics)");
  return linear_fwd_impl(dtype, x_is_f32, m, n, k, x, x_ld, w, w_ld, bias, y, y_ld, scale_cols, col_scale, IR_LIN_AUTO, stats_col0, stats_cols,
                         stats_ws, stats_ws_bytes, stream);
}

int ir_linear_fwd_stats_ex(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                           int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                           int32_t stats_col0, int32_t stats_cols, float* stats_ws, size_t stats_ws_bytes, int32_t kernel, void* stream) {
  if (stats_ws == nullptr) return fail(IR_ERR_INVALID_ARG, "stats_ws is NULL (use ir_linear_fwd_ex for a call without statistics)");
  if (kernel != IR_LIN_AUTO && kernel != IR_LIN_BATCH_INVARIANT)
    return fail(IR_ERR_INVALID_ARG, "ir_linear_fwd_stats_ex: kernel %d (IR_LIN_AUTO or IR_LIN_BATCH_INVARIANT)", kernel);
  return linear_fwd_impl(dtype, x_is_f32, m, n, k, x, x_ld, w, w_ld, bias, y, y_ld, scale_cols, col_scale, kernel, stats_col0, stats_cols,
                         stats_ws, stats_ws_bytes, stream);
}

int ir_adain_affine_from_partials(int32_t batch, int32_t heads, int32_t n_refs, int32_t len_self, int32_t len_ref,
                                  const float* style_ws, int32_t style_rows, const float* content_ws, int32_t content_rows,
                                  const float* content_mean, const float* content_std, const int32_t* valid, float eps,
                                  float* a, float* b, void* stream) {
  if (batch <= 0 || heads <= 0 || n_refs <= 0 || len_self <= 0 || len_ref <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!style_ws || !a || !b) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (style_rows <= 0 || (len_self % style_rows) != 0) return fail(IR_ERR_INVALID_ARG, "len_self %d is not a multiple of style_rows %d", len_self, style_rows);
  if (content_ws != nullptr) {
    if (content_rows <= 0 || (len_ref % content_rows) != 0) return fail(IR_ERR_INVALID_ARG, "len_ref %d is not a multiple of content_rows %d", len_ref, content_rows);
  } else if (!content_mean || !content_std) {
    return fail(IR_ERR_INVALID_ARG, "content statistics: either content_ws or content_mean + content_std");
  }
  if (len_self / style_rows > ir_adain_partials_max_chunks() || (content_ws != nullptr && len_ref / content_rows > ir_adain_partials_max_chunks()))
    return fail(IR_ERR_UNSUPPORTED, "more than %d partials per matrix (token axis too long for the merge kernel: use ir_adain_stats)", ir_adain_partials_max_chunks());
  AdainPartialsKParams p;
  memset(&p, 0, sizeof(p));
  p.style_ws = style_ws; p.content_ws = content_ws; p.cmean = content_mean; p.cstd = content_std; p.valid = valid;
  p.a = a; p.b = b; p.B = batch; p.H = heads; p.N = n_refs; p.Ls = len_self; p.Lr = len_ref;
  p.style_rows = style_rows; p.content_rows = content_ws != nullptr ? content_rows : 1; p.eps = eps;
  const hipError_t e = ir_launch_adain_affine_partials(p, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "adain_affine_partials launch: %s", hipGetErrorString(e));
  return IR_OK;
}

int ir_token_stats_from_partials(int32_t n_sets, int32_t heads, int32_t len, const float* ws, int32_t rows, float* mean, float* std,
                                 void* stream) {
  if (n_sets <= 0 || heads <= 0 || len <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (!ws || !mean || !std) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (rows <= 0 || (len % rows) != 0) return fail(IR_ERR_INVALID_ARG, "len %d is not a multiple of rows %d", len, rows);
  if (len / rows > ir_adain_partials_max_chunks()) return fail(IR_ERR_UNSUPPORTED, "more than %d partials per matrix", ir_adain_partials_max_chunks());
  const hipError_t e = ir_launch_token_stats_partials(ws, rows, n_sets, heads, len, mean, std, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "token_stats_partials launch: %s", hipGetErrorString(e));
  return IR_OK;
}

static int linear_fwd_impl(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                           int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                           int32_t kernel, int32_t st_col0, int32_t st_cols, float* st_ws, size_t st_ws_bytes, void* stream) {
  if (scale_cols < 0 || scale_cols > n || (scale_cols % 32) != 0) return fail(IR_ERR_INVALID_ARG, "scale_cols %d: a multiple of 32 in [0, N]", scale_cols);
  if (dtype != IR_DTYPE_F16 && dtype != IR_DTYPE_BF16) return fail(IR_ERR_UNSUPPORTED, "dtype %d: fp16 (0) / bf16 (1)", dtype);
  if (!x || !w || !y) return fail(IR_ERR_INVALID_ARG, "NULL pointer");
  if (m <= 0 || n <= 0 || k <= 0) return fail(IR_ERR_INVALID_ARG, "sizes must be > 0");
  if (kernel == IR_LIN_AUTO) kernel = ir_linear_kernel_for(m, n, k, bias != nullptr);
  else if (kernel == IR_LIN_BATCH_INVARIANT) kernel = linear_kernel_batch_invariant(n, k, bias != nullptr);
  if (kernel < 0) return fail(IR_ERR_UNSUPPORTED, "K = %d, N = %d: K must be a multiple of 64 and N of 64 (of 32 for K <= 320 or K = 640)", k, n);
  if (kernel == IR_LIN_X_STATIONARY) {
    if (!x_stationary_covers(n, k, bias))
      return fail(IR_ERR_UNSUPPORTED, "X-stationary kernel: K in {64,...,320} or 640, N %% 32 == 0, N <= %d with bias (K = %d, N = %d)", kLinearMaxBiasN, k, n);
  } else if (kernel < IR_LIN_TILED_FIRST || kernel >= IR_LIN_TILED_FIRST + IR_LIN_TILE_COUNT) {
    return fail(IR_ERR_INVALID_ARG, "kernel %d: 0 auto, 1 X-stationary, %d..%d tiled", kernel, IR_LIN_TILED_FIRST, IR_LIN_TILED_FIRST + IR_LIN_TILE_COUNT - 1);
  } else if (k % 64 != 0 || !ir_linear_tiled_cfg_ok(kernel - IR_LIN_TILED_FIRST, n)) {
    return fail(IR_ERR_UNSUPPORTED, "tiled kernel %d: K %% 64 == 0 and N a multiple of the tile width (K = %d, N = %d)", kernel, k, n);
  }
  if (m > 0x7fffffffLL - 256) return fail(IR_ERR_UNSUPPORTED, "M too large");
  if (x_ld < k || w_ld < k || y_ld < n || (x_ld % 8) || (w_ld % 8) || (y_ld % 8))
    return fail(IR_ERR_UNSUPPORTED, "leading dimensions must cover a row and be multiples of 8 elements");
  if (!aligned16(x) || !aligned16(w) || !aligned16(y) || (bias != nullptr && !aligned16(bias)))
    return fail(IR_ERR_UNSUPPORTED, "pointers must be 16-byte aligned");
  if ((int64_t)n * w_ld * 2 >= (1LL << 31)) return fail(IR_ERR_UNSUPPORTED, "weight larger than 2 GiB");
  if (256 * x_ld * 2 >= (1LL << 31)) return fail(IR_ERR_UNSUPPORTED, "x_ld too large");
  if (256 * y_ld * 2 >= (1LL << 31)) return fail(IR_ERR_UNSUPPORTED, "y_ld too large");   // a wave's 64 rows of Y sit behind one 32-bit buffer range
  LinearKParams p;
  p.x = x; p.w = w; p.bias = bias; p.y = y; p.x_ld = x_ld; p.w_ld = w_ld; p.y_ld = y_ld;
  p.M = (int32_t)m; p.N = n; p.K = k; p.nsplit = 1;
  p.scale_cols = scale_cols; p.col_scale = col_scale; p.x_f32 = x_is_f32 ? 1 : 0;
  p.st_ws = nullptr; p.st_col0 = 0; p.st_cols = 0;
  if (st_ws != nullptr) {   // token statistics of columns [st_col0, st_col0 + st_cols) as the kernel's tail
    const int rows = stats_rows_of(kernel);
    if (st_col0 < 0 || st_cols <= 0 || (st_col0 % 64) != 0 || (st_cols % 64) != 0 || st_col0 + st_cols > n || (n % 64) != 0)
      return fail(IR_ERR_INVALID_ARG, "statistics columns [%d, %d + %d): whole heads (multiples of 64) inside N = %d, N %% 64 == 0", st_col0, st_col0, st_cols, n);
    if (rows <= 0 || (m % rows) != 0) return fail(IR_ERR_UNSUPPORTED, "statistics tail: M = %lld is not a multiple of the kernel's %d-row blocks (ir_linear_stats_rows)", (long long)m, rows);
    const size_t need = (size_t)(m / rows) * (size_t)(st_cols / 64) * 128 * sizeof(float);
    if (st_ws_bytes < need) return fail(IR_ERR_WORKSPACE, "stats_ws %zu < %zu bytes", st_ws_bytes, need);
    // the K = 640 X-stationary kernel re-reads the rows it has just stored (ir_wave_col_stats): every 128-byte line of the
    // statistics columns must belong to ONE workgroup's column range, i.e. rows of y start on a line and so does column st_col0
    if (kernel == IR_LIN_X_STATIONARY && k == 640 && (((y_ld * 2) % 128) != 0 || (((uintptr_t)y + (uintptr_t)st_col0 * 2) % 128) != 0))
      return fail(IR_ERR_UNSUPPORTED, "statistics tail at K = 640: y + stats_col0 must be 128-byte aligned and y_ld a multiple of 64 elements");
    p.st_ws = st_ws; p.st_col0 = st_col0; p.st_cols = st_cols;
  }
  const hipError_t e =
      kernel == IR_LIN_X_STATIONARY ? ir_launch_linear_skinny(p, dtype, (hipStream_t)stream)
                                    : ir_launch_linear_tiled(p, dtype, kernel - IR_LIN_TILED_FIRST, (hipStream_t)stream);
  if (e != hipSuccess) return fail(IR_ERR_LAUNCH, "linear launch: %s", hipGetErrorString(e));
  return IR_OK;
}

}  // extern "C"
