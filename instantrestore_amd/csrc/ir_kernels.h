// ir_kernels.h - kernel parameter blocks and host-side launchers (internal; the public
// interface is include/instantrestore_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ir_attn_plan.h"

#define IR_KV_TILE 64          // keys per K/V tile
#define IR_ADAIN_ROWS 256      // token rows per AdaIN partial-statistics workgroup
#define IR_ADAIN_W_STRIDE 136  // floats per chunk partial of the weighted statistics: mean[64] | M2[64] | W, W2, 6 of padding

// Parameter block of the fused attention kernels (passed by value as the kernel argument).
struct AttnKParams {
  const void* q;
  const void* k_self;
  const void* v_self;
  const void* k_ref;
  const void* v_ref;
  const float* aa;  // AdaIN scale  (B,N,H,64) or nullptr
  const float* ab;  // AdaIN shift
  void* out;
  float* lse;
  void* probs;      // attn_probs kernel only
  const int32_t* valid;   // ABI v8 (ir_shared_attn_args.valid_refs): references n >= valid[b] are all-zero in k_ref / v_ref: the default
                          // kernels (64-row, pipelined 32-row) close them analytically instead of walking their tiles; nullptr: walk all
  int64_t q_sb, q_sl, q_sh;
  int64_t ks_sb, ks_sl, ks_sh;
  int64_t vs_sb, vs_sl, vs_sh;
  int64_t kr_sb, kr_sn, kr_sl, kr_sh;
  int64_t vr_sb, vr_sn, vr_sl, vr_sh;
  int64_t o_sb, o_sl, o_sh;
  int B, H, Lq, Ls, N, Lr;
  int include_self;   // 0/1
  int q_prescaled;    // IR_FLAG_Q_PRESCALED: q holds Q * scale * log2(e)   (the 64-row kernel's QS instantiation, the 32-row kernel's PRESC forms)
  int out_f32;        // IR_FLAG_OUT_F32: fp32 output, o_s* in fp32 elements (every product kernel + combine)
  int tiles_self;     // ceil(Ls/64) if include_self else 0
  int tiles_ref;      // ceil(Lr/64)
  int ntiles;         // include_self*tiles_self + N*tiles_ref
  int nqb;            // query blocks per (b,h)
  int lkv;            // include_self*Ls + N*Lr
  float scale;
  float scale_log2;   // scale * log2(e)
  // remainder split (pipelined kernel): each XCD owns sk_ix consecutive work items; the first
  // sk_full of them (whole rounds of the XCD's workgroup slots) run their full K/V range, each
  // of the remaining sk_ix - sk_full is cut into sk_k pieces along the K/V tiles whose partial
  // (O, m, l) go to ws_o / ws_ml and are merged by the combine kernel.  sk_k <= 1: no split.
  float* ws;          // caller's workspace (or nullptr: never split)
  size_t ws_bytes;
  float* ws_o;        // [piece][QB rows][64] fp32, unnormalised O relative to m
  float* ws_ml;       // [piece][QB rows][2]  (raw running max, row sum)
  int sk_items;       // B*H*nqb
  int sk_ix;          // ceil(sk_items / 8)
  int sk_full;
  int sk_k;
  // ABI v9 (ir_shared_attn_args.seg_mass): attention mass per K/V segment as a BY-PRODUCT of the forward kernels.  At every segment
  // boundary of its K/V walk a kernel already holds the row sums (the AdaIN fold needs them); it stores the CUMULATIVE log-sum-exp
  // through segment s - a number that does not depend on the running reference - into seg_cum[b,h,row,s] (natural log; pieces of a
  // split item: log2 units into ws_cum, merged by the combine kernel), and seg_mass_finish_kernel turns the S cumulative values of
  // a row into S masses in place.  nullptr: off (nothing but one uniform test per SEGMENT, none per tile).
  float* seg_cum;     // (B, H, Lq, nseg_out) fp32 or nullptr
  float* ws_cum;      // [piece][QB rows][nseg_out]
  int nseg_out;       // include_self + N
  // sk_k on ENTRY to a kernel launcher: 0 = the launcher plans the remainder split itself (default dispatch); > 0 = a fixed plan
  // (ABI v10 batch-invariant mode, ir_attn_bi_plan): every item in sk_k pieces (1: whole items), workspace sized by the caller
  // pointer tables (ir_shared_attn_table_args.k_ref_table / v_ref_table): k_ref / v_ref then hold the TABLES - device arrays of B*N
  // device pointers - and kr_sb, kr_sn (vr_sb, vr_sn) their strides in 2-byte elements (4 N and 4: eight bytes per entry), so the dense
  // expression k_ref + b * kr_sb + n * kr_sn is the address of entry [b*N + n] and the kernels' one extra step is to read the
  // segment's base address there (ir_ref_entry).  No kernel argument of its own for the tables: the attention kernels have no
  // SGPRs to spare.  Read by the kernels when they run, never by the dispatch or the plans
  int ref_tables;     // 0/1
  // additive key bias (ir_shared_attn_bias_args): bias[b,h,j] = key_bias[b * kb_sb + h * kb_sh + j] over the packed extended key
  // axis, added to scale * <q,k> before the softmax; nullptr: none.  Read by the BIAS forms of the 32-row kernel only
  // (shared_attn_fwd_pipe_bias.hip); appended, so no other kernel's arguments move
  const float* key_bias;
  int64_t kb_sb, kb_sh;
  // per-reference token counts (ir_shared_attn_ragged_args): reference n of entry b has clamp(ref_lens[b * rl_sb + n], 0, Lr) keys;
  // Lr is the capacity of a segment (allocation, strides).  nullptr: every reference has Lr keys.  Read by the RAGGED forms of the
  // 32-row kernel only (shared_attn_fwd_pipe_ragged.hip), when they run; appended, so no other kernel's arguments move
  const int32_t* ref_lens;
  int64_t rl_sb;
  // region-restricted attention (ir_shared_attn_region_args): row i of entry b may attend key j iff key_region[b * kg_sb + j] is in
  // [0, 31] and bit key_region[..] of q_allow[b * qa_sb + i] is set; one rule for all heads.  nullptr (both): none.  Read by the REGION
  // forms of the 32-row kernel only (shared_attn_fwd_pipe_region.hip), when they run; appended, so no other kernel's arguments move
  const uint32_t* q_allow;
  int64_t qa_sb;
  const int32_t* key_region;
  int64_t kg_sb;
};

// The base address (head 0, token 0) of a reference segment from `at` = k_ref + b * kr_sb + n * kr_sn: `at` itself in the dense
// layout, the pointer stored at `at` in a pointer-table call.  Wave-uniform, outside every inner loop; read through the constant
// address space (one scalar load: the tables do not change while a kernel runs)
#ifdef __HIPCC__
template <typename T>
__device__ __forceinline__ const T* ir_ref_entry(const T* at, int tables) {
  typedef const __attribute__((address_space(4))) uint64_t* ConstTable;
  return tables ? (const T*)(uintptr_t)*(ConstTable)(uintptr_t)at : at;
}
#endif

// what a kernel launcher gives ir_attn_plan (ir_attn_plan.h): the call, its own rows per item and slots rule
static inline IrAttnPlanIn ir_attn_plan_in(const AttnKParams& p, int rows, int slots, int force_k = 0) {
  return {p.B, p.H, p.Lq, p.ntiles, rows, slots, p.ws != nullptr, p.ws_bytes, p.seg_cum != nullptr ? p.nseg_out : 0, p.sk_k, force_k};
}

// ---- the dispatch of the attention forward (shared_attn_fwd.hip: kAttnVariants, ir_attn_choose) ----
enum IrAttnFamily {
  IR_FAM_REFUSED = 0,   // the launch returns hipErrorInvalidValue
  IR_FAM_W128,          // 128 rows per wave, one wave per SIMD (shared_attn_fwd_w128.hip) ...
  IR_FAM_W128_FORMS,    // ... its valid_refs / seg_mass instantiation
  IR_FAM_W64X8,         // 64 rows per wave, 8-wave (512-row) workgroups (shared_attn_fwd_w64.hip) ...
  IR_FAM_W64X4,         // ... 4 waves
  IR_FAM_PIPE32,        // software-pipelined 32-row kernel (shared_attn_fwd_pipe.hip), in one of its forms
  IR_FAM_DEV            // -DIR_ABLATIONS builds: the straight-line kernel with its `>> 5` ablation bits, the 64-row kernel's ablations
};
enum IrPipeForm {   // the product forms of the 32-row kernel (shared_attn_fwd_pipe.hip: one Form... struct each; launch_t maps these to them)
  IR_PIPE_NONE = 0,
  IR_PIPE_EXACT,        // exact (every-change) rescale
  IR_PIPE_LAZY,         // + lazy max
  IR_PIPE_PRESC,        // + pre-scaled Q, reference through the MFMA C operand
  IR_PIPE_EARLYQK,      // LAZY with the next tile's QK^T issued before the row max
  IR_PIPE_POSTCHECK     // PRESC with the reference checked after the exponentials (no row max on ordinary tiles; K ring of 3)
};
struct IrAttnVariant {   // one tuning value (IR_TUNE_*)
  int id;
  IrAttnFamily family;   // (IR_TUNE_DEFAULT: what the default rules fall back to)
  IrPipeForm form;
  bool presc_q;          // takes IR_FLAG_Q_PRESCALED
  bool seg_mass;         // carries the seg_mass by-product
  bool product;          // false: -DIR_ABLATIONS builds only
};
struct IrAttnChoice {
  IrAttnFamily family;
  IrPipeForm form;       // IR_FAM_PIPE32 only
};
const IrAttnVariant* ir_attn_variant(int tuning);                      // nullptr: not available in this build
IrAttnChoice ir_attn_choose(const AttnKParams& p, int tuning);         // what ir_launch_shared_attn_fwd runs
IrAttnChoice ir_attn_choose_bi(const AttnKParams& p);                  // what the batch-invariant plan runs

// ABI v10 (IR_FLAG_BATCH_INVARIANT): the kernel and the cut of every work item into K/V-range pieces, from per-item parameters only
struct IrAttnBiPlan {
  int kernel;          // IR_TUNE_W128 (16), IR_TUNE_W64X8 (13), IR_TUNE_PIPE32_PRESCALE_Q (11) or IR_TUNE_PIPE32_EARLYQK (14)
  int rows;            // query rows per work item
  int items;           // work items per batch entry
  int pieces;          // K/V-range pieces per item (1: whole items)
  size_t piece_bytes;  // fp32 partials of one piece (O, max, sum, and the cumulative segment values with seg_mass)
};
void ir_attn_bi_plan(const AttnKParams& p, IrAttnBiPlan* pl);
size_t ir_attn_bi_workspace_bytes(const IrAttnBiPlan& pl, int batch);   // scratch of one launch over `batch` entries
hipError_t ir_launch_shared_attn_fwd_bi(const AttnKParams& p, int dtype, const IrAttnBiPlan& pl, hipStream_t s);

struct AdainKParams {
  const void* v_self;
  const void* v_ref;
  int64_t vs_sb, vs_sl, vs_sh;
  int64_t vr_sb, vr_sn, vr_sl, vr_sh;
  float* ws;          // partial statistics: [B*(1+N)][H][nchunk][2][64] (mean, M2)
  float* a;
  float* b;
  int B, H, Ls, N, Lr;
  int nchunk;         // max(ceil(Ls/ROWS), ceil(Lr/ROWS))
  float eps;
  // ir_adain_stats_cached: content statistics (mean, unbiased std) of every reference V, (B, N, H, 64) fp32, computed once
  // per identity (ir_token_stats in the K/V-capture layer); only V_self is read here
  const float* cmean;
  const float* cstd;
};

struct AdainApplyKParams {
  const void* x;
  void* y;
  const float* a;
  const float* b;
  int64_t x_sb, x_sn, x_sl, x_sh;
  int64_t y_sb, y_sn, y_sl, y_sh;
  int B, H, N, L;
};

struct ZeroRefsKParams {
  void* k;
  void* v;
  const int32_t* valid;
  int64_t k_sb, k_sn, k_sl, k_sh;
  int64_t v_sb, v_sn, v_sl, v_sh;
  int B, H, N, L;
};

// launchers (defined next to their kernels); dtype: 0 = f16, 1 = bf16. Return hipError_t.
hipError_t ir_launch_shared_attn_fwd(const AttnKParams& p, int dtype, int variant, hipStream_t s);
hipError_t ir_launch_shared_attn_fwd_pipe(const AttnKParams& p, int dtype, IrPipeForm form, hipStream_t s);
hipError_t ir_launch_shared_attn_fwd_pipe_bias(const AttnKParams& p, int dtype, IrPipeForm form, hipStream_t s);   // key_bias: PRESC / EARLYQK (shared_attn_fwd_pipe_bias.hip)
hipError_t ir_launch_shared_attn_fwd_pipe_ragged(const AttnKParams& p, int dtype, IrPipeForm form, hipStream_t s);   // ref_lens: PRESC / EARLYQK (shared_attn_fwd_pipe_ragged.hip)
hipError_t ir_launch_shared_attn_fwd_pipe_region(const AttnKParams& p, int dtype, IrPipeForm form, hipStream_t s);   // q_allow / key_region: PRESC / EARLYQK (shared_attn_fwd_pipe_region.hip)
hipError_t ir_launch_shared_attn_combine(const AttnKParams& p, int dtype, int qb, int rem, hipStream_t s);
hipError_t ir_launch_shared_attn_fwd_w64(const AttnKParams& p, int dtype, hipStream_t s);
hipError_t ir_launch_shared_attn_fwd_w64x8(const AttnKParams& p, int dtype, hipStream_t s);
// round 6: one wave per SIMD, 128 query rows per wave, hand-placed instruction stream (shared_attn_fwd_w128.hip)
hipError_t ir_launch_shared_attn_fwd_w128(const AttnKParams& p, int dtype, hipStream_t s);
hipError_t ir_launch_shared_attn_fwd_w128_forms(const AttnKParams& p, int dtype, hipStream_t s);   // valid_refs / seg_mass (shared_attn_fwd_w128_forms.hip)
bool ir_attn_w128_supports(const AttnKParams& p);   // pre-scaled Q, whole 64-key tiles (valid_refs / seg_mass included)
bool ir_attn_default_is_w128(const AttnKParams& p);
#ifdef IR_ABLATIONS   // energy / timing ablations of the 64-row QS kernel (tuning values 20 + index; shared_attn_fwd_w64.hip)
hipError_t ir_launch_shared_attn_fwd_w64_abl(const AttnKParams& p, int dtype, int index, hipStream_t s);
int ir_w64_abl_count(void);
int ir_w64_abl_mask(int index);
#endif
hipError_t ir_launch_seg_mass_finish(const AttnKParams& p, hipStream_t s);   // cumulative log-sum-exp -> masses, in place
bool ir_attn_default_is_w64(const AttnKParams& p);
bool ir_attn_variant_available(int variant);

// variant: 0 = automatic (line kernel when every segment length is a multiple of 8), 1 = round 1's 2-byte-store kernel,
// 2 / 3 = the line kernel with 64 / 32 query rows per wave
hipError_t ir_launch_attn_probs(const AttnKParams& p, int dtype, int variant, hipStream_t s);
int ir_device_cus();   // compute units of the current device (256 when the query fails); attn_probs.hip
bool ir_attn_probs_uses_lines(const AttnKParams& p);
hipError_t ir_launch_attn_segment_mass(const AttnKParams& p, int dtype, float* mass, hipStream_t s);
// attn_rows.hip: the probability rows of `n_rows` chosen query tokens per batch entry (row_index: int32 (B, n_rows) on the device),
// as they are or reduced over heads / over heads and rows; `reduce` is IR_ROWS_* of the public header
constexpr int kRowsNone = 0, kRowsHeadMean = 1, kRowsMap = 2;
hipError_t ir_launch_attn_rows(const AttnKParams& p, int dtype, const int32_t* row_index, int n_rows, int reduce, void* out, hipStream_t s);
// attn_match.hip: per K/V segment, the largest probability of each of `n_rows` chosen query tokens and the key that attains it
// (index int32, prob fp32: (B, H, n_rows, S) per head, (B, n_rows, S) of the head mean); `reduce` is IR_MATCH_* of the public header.
// One wave per item, four items per workgroup: ir_attn_match_items is the item count, at most kMatchMaxItems
constexpr int kMatchPerHead = 0, kMatchHeadMean = 1;
constexpr int64_t kMatchMaxItems = 0x7fffffffLL - 3;
int64_t ir_attn_match_items(const AttnKParams& p, int n_rows, int reduce);
hipError_t ir_launch_attn_match(const AttnKParams& p, int dtype, const int32_t* row_index, int n_rows, int reduce, int32_t* index, float* prob,
                                hipStream_t s);
// attn_transfer.hip: per K/V segment, the attention-weighted sums of a per-key fp32 payload (`channels` floats per key of the packed
// extended key axis, batch / key strides pay_sb / pay_sj in floats) and the segment's mass for `n_rows` chosen query tokens
// (sums fp32 (B, H, n_rows, S, channels) / (B, n_rows, S, channels), mass fp32 without the last axis, or nullptr); `reduce` is
// IR_TRANSFER_* of the public header.  The items of ir_attn_match: one wave each, at most kTransferMaxItems
constexpr int kTransferPerHead = 0, kTransferHeadMean = 1;
constexpr int kTransferMaxChannels = 8;
constexpr int64_t kTransferMaxItems = 0x7fffffffLL - 3;
int64_t ir_attn_transfer_items(const AttnKParams& p, int n_rows, int reduce);
hipError_t ir_launch_attn_transfer(const AttnKParams& p, int dtype, const float* payload, int64_t pay_sb, int64_t pay_sj, int channels,
                                   const int32_t* row_index, int n_rows, int reduce, float* sums, float* mass, hipStream_t s);
// attn_received.hip: per key of the packed extended key axis, the sum over ALL query rows of p * w for a per-row fp32 payload
// (`channels` floats per row, batch / row strides w_sb / w_si in floats; nullptr: one channel of ones), recv fp32
// (B, H, Lkv, channels) / (B, Lkv, channels); `reduce` is IR_RECEIVED_* of the public header.  One wave per item (a group of keys
// of one segment), at most kReceivedMaxItems
constexpr int kReceivedPerHead = 0, kReceivedHeadMean = 1;
constexpr int kReceivedMaxChannels = 8;
constexpr int64_t kReceivedMaxItems = 0x7fffffffLL - 3;
int64_t ir_attn_received_items(const AttnKParams& p, int channels, int reduce);
hipError_t ir_launch_attn_received(const AttnKParams& p, int dtype, const float* weights, int64_t w_sb, int64_t w_si, int channels, int reduce,
                                   float* recv, hipStream_t s);
// attn_topk.hip: per K/V segment, the `k` largest probabilities of each of `n_rows` chosen query tokens and the keys that attain
// them under (probability descending, key ascending) (index int32, prob fp32: (B, H, n_rows, S, k) per head, (B, n_rows, S, k) of
// the head mean); `reduce` is IR_MATCH_* of the public header, rank 0 is attn_match.hip's result.  The items of ir_attn_match: one
// wave each, at most kTopkMaxItems
constexpr int kTopkMax = 8;
constexpr int64_t kTopkMaxItems = kMatchMaxItems;
int64_t ir_attn_topk_items(const AttnKParams& p, int n_rows, int reduce);
hipError_t ir_launch_attn_topk(const AttnKParams& p, int dtype, const int32_t* row_index, int n_rows, int k, int reduce, int32_t* index, float* prob,
                               hipStream_t s);
// attn_key_match.hip: per key of the packed extended key axis, the largest probability over ALL query rows and the lowest row that
// attains it (index int32, prob fp32: (B, H, Lkv) per head, (B, Lkv) of the head mean); `reduce` is IR_MATCH_* of the public
// header.  One wave per item (a group of keys of one segment), at most kKeyMatchMaxItems
constexpr int kKeyMatchPerHead = 0, kKeyMatchHeadMean = 1;
constexpr int64_t kKeyMatchMaxItems = 0x7fffffffLL - 3;
int64_t ir_attn_key_match_items(const AttnKParams& p, int reduce);
hipError_t ir_launch_attn_key_match(const AttnKParams& p, int dtype, int reduce, int32_t* index, float* prob, hipStream_t s);
hipError_t ir_launch_adain_stats(const AdainKParams& p, int dtype, hipStream_t s);
hipError_t ir_launch_token_stats(const AdainKParams& p, int dtype, hipStream_t s);
hipError_t ir_launch_adain_stats_cached(const AdainKParams& p, int dtype, hipStream_t s);
// adain_weighted.hip: token statistics over weighted / counted tokens (ir_token_stats_weighted), the affine from finished statistics
struct TokenStatsWKParams {
  const void* x;             // (B, M, len, H, 64), strides in elements
  int64_t x_sb, x_sn, x_sl, x_sh;
  const float* weights;      // w[b, m, t] = weights[b * w_sb + m * w_sn + t], or nullptr (= 1)
  int64_t w_sb, w_sn;
  const int32_t* lens;       // c[b, m] = clamp(lens[b * ln_sb + m], 0, len), or nullptr (= len)
  int64_t ln_sb;
  float* ws;                 // chunk partials: [B*M][H][nchunk][IR_ADAIN_W_STRIDE]
  float* mean;               // fp32 (B, M, H, 64)
  float* std;
  float* wsum;               // fp32 (B, M), or nullptr
  int B, M, H, len, nchunk;
};
hipError_t ir_launch_token_stats_weighted(const TokenStatsWKParams& p, int dtype, hipStream_t s);
hipError_t ir_launch_adain_affine_from_stats(const float* smean, const float* sstd, const float* cmean, const float* cstd, float eps,
                                             float* a, float* b, int B, int N, int H, hipStream_t s);
// adain_regions.hip: token statistics per region label in one pass (ir_token_stats_labelled), the apply with a per-token affine slot
struct TokenStatsRKParams {
  const void* x;             // (B, M, len, H, 64), strides in elements
  int64_t x_sb, x_sn, x_sl, x_sh;
  const int32_t* labels;     // label[b, m, t] = labels[b * lb_sb + m * lb_sn + t]; outside [0, R): no region
  int64_t lb_sb, lb_sn;
  float* ws;                 // chunk partials: [B*M][R][H][nchunk][IR_ADAIN_W_STRIDE]
  float* mean;               // fp32 (B, R, M, H, 64)
  float* std;
  float* count;              // fp32 (B, R, M), or nullptr
  int B, M, H, len, R, nchunk;
};
struct AdainApplyRKParams {
  const void* x;
  void* y;
  const float* a;            // fp32 (B, N, R + 1, H, 64); slot R: tokens of no region
  const float* b;
  const int32_t* labels;     // label[b, n, t] = labels[b * lb_sb + n * lb_sn + t]
  int64_t lb_sb, lb_sn;
  int64_t x_sb, x_sn, x_sl, x_sh;
  int64_t y_sb, y_sn, y_sl, y_sh;
  int B, H, N, L, R;
};
hipError_t ir_launch_token_stats_regions(const TokenStatsRKParams& p, int dtype, hipStream_t s);
hipError_t ir_launch_adain_apply_regions(const AdainApplyRKParams& p, int dtype, hipStream_t s);
// round 4: the affine / the plain token statistics from the partials the projection GEMMs leave behind (ir_colstats.h)
struct AdainPartialsKParams {
  const float* style_ws;     // partials of V_self: [(b * Ls / style_rows + c)][H][128]
  const float* content_ws;   // partials of the reference V's: [((b * N + n) * Lr / content_rows + c)][H][128], or nullptr
  const float* cmean;        // ... then the finished content statistics (B, N, H, 64): mean, unbiased std (no eps)
  const float* cstd;
  const int32_t* valid;      // optional (B): references n >= valid[b] were zero-filled: statistics (0, 0)
  float* a;
  float* b;
  int B, H, N, Ls, Lr, style_rows, content_rows;
  float eps;
};
hipError_t ir_launch_adain_affine_partials(const AdainPartialsKParams& p, hipStream_t s);
hipError_t ir_launch_token_stats_partials(const float* ws, int rows, int nsets, int H, int len, float* mean, float* std, hipStream_t s);
// benchmark hook (bench_hooks.hip): one launch of an MFMA-only stream, `blocks` workgroups x 8 waves x iters x 16 MFMAs
hipError_t ir_launch_bench_mfma_stream(int dtype, int zero, int iters, int blocks, float* out, hipStream_t s);
int ir_adain_partials_max_chunks(void);   // partials per matrix the merge kernels hold in registers (len / rows <= this)
hipError_t ir_launch_adain_apply(const AdainApplyKParams& p, int dtype, hipStream_t s);
hipError_t ir_launch_zero_refs(const ZeroRefsKParams& p, hipStream_t s);
// compact_refs.hip: stable compaction of the kept token rows of every reference to the front of its output segment
struct CompactRefsKParams {
  const void* k_in;
  const void* v_in;
  void* k_out;
  void* v_out;
  const uint8_t* keep;   // (B, N, L) contiguous, non-zero = kept
  int32_t* ref_lens;     // (B, N) rows rl_sb apart: the counts
  int64_t rl_sb;
  int64_t ki_sb, ki_sn, ki_sl, ki_sh;
  int64_t vi_sb, vi_sn, vi_sl, vi_sh;
  int64_t ko_sb, ko_sn, ko_sl, ko_sh;
  int64_t vo_sb, vo_sn, vo_sl, vo_sh;
  int B, H, N, L;
};
hipError_t ir_launch_compact_refs(const CompactRefsKParams& p, hipStream_t s);
hipError_t ir_launch_tensor2im(const void* x, void* out, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                               int B, int C, int H, int W, hipStream_t s);

// ---- image_io.hip: the caller's input transform and FreeU's skip-feature filter ----------------
struct ResampleImageK {
  const unsigned char* src;   // (in_h, in_w, 3) uint8, pixel stride 3 bytes
  int64_t src_row_bytes;
  const int32_t* bounds_h;    // (out_w, 2): first source column, tap count
  const int32_t* kk_h;        // (ksize_h, out_w) 22-bit fixed-point taps, TRANSPOSED (tap-major)
  const int32_t* bounds_v;    // (out_h, 2)
  const int32_t* kk_v;        // (out_h, ksize_v)
  unsigned char* tmp;         // (row_count, size, 3): horizontal pass of the crop's columns
  int32_t ksize_h, ksize_v;
  int32_t crop_top, crop_left;
  int32_t row_first, row_count;  // source rows the crop's vertical taps touch
  int32_t col_first, col_count;  // source columns the crop's horizontal taps touch
  int32_t in_h, in_w, out_w;
};
constexpr int kPreprocessImagesPerLaunch = 16;
struct PreprocessKParams {
  ResampleImageK img[kPreprocessImagesPerLaunch];
  int32_t n, size, first_image, tmp_pitch;  // tmp rows are tmp_pitch bytes apart (multiple of 4)
};
hipError_t ir_launch_preprocess(const PreprocessKParams& p, int max_rows, int max_span_bytes, int max_ksize_v, int dtype,
                                void* out, hipStream_t s);
hipError_t ir_launch_freeu_fourier(const void* x, void* out, int dtype, int64_t planes, int H, int W, int64_t sp_in,
                                   int64_t sp_out, int thr, float scale, hipStream_t s);
int ir_host_lanczos_ksize(int in_size, int out_size);

// ---- linear_skinny.hip: Y = X W^T (+ bias) for K <= 320 (X-stationary, W streamed) ---------------
constexpr int kLinearMaxBiasN = 4096;
struct LinearKParams {
  const void* x;     // (M, K) rows x_ld elements apart
  const void* w;     // (N, K) rows w_ld elements apart (torch Linear weight)
  const void* bias;  // (N) or nullptr
  void* y;           // (M, N) rows y_ld elements apart
  int64_t x_ld, w_ld, y_ld;
  int32_t M, N, K, nsplit;
  int32_t x_f32;        // x is fp32 (x_ld in fp32 elements): cast to the 16-bit type while loading the resident fragments
  int32_t scale_cols;   // output columns [0, scale_cols) are multiplied by col_scale in fp32 before the rounding
  float col_scale;      // (scale_cols % 32 == 0; 0 = none): the softmax scale * log2(e) on the q third of a fused q/k/v
  // round 4: token statistics of a column range (the V third of a fused q/k/v output) as the kernel's tail (ir_colstats.h):
  // one (mean[64], M2[64]) partial per (64-row block, head); ws == nullptr: off
  float* st_ws;
  int32_t st_col0, st_cols;
};
hipError_t ir_launch_linear_skinny(const LinearKParams& p, int dtype, hipStream_t s);

// ---- linear_tiled.hip: LDS-tiled Y = X W^T (+ bias) for any K % 64 == 0, N % 64 == 0 (K = 1280, small-M shapes) ----
enum {   // tile shapes (rows x columns of Y per workgroup); values are the `kernel` argument of ir_linear_fwd_ex minus 2
  IR_LIN_TILE_256x128 = 0,   // 8 waves
  IR_LIN_TILE_128x128 = 1,   // 4 waves
  IR_LIN_TILE_128x64 = 2,    // 2 waves
  IR_LIN_TILE_256x64 = 3,    // 4 waves
  IR_LIN_TILE_64x128 = 4,    // 2 waves
  IR_LIN_TILE_128x256 = 5,   // 4 waves, 64 x 128 per wave
  IR_LIN_TILE_256x256 = 6,   // 8 waves, 64 x 128 per wave, wave groups one phase apart (matrix phase beside load phase on every SIMD)
  IR_LIN_TILE_128x128_K2 = 7,   // round 5: 128 x 128 with the contraction split over two 4-wave groups (K / 64 even), fixed-order sum through LDS
  IR_LIN_TILE_COUNT = 8
};
hipError_t ir_launch_linear_tiled(const LinearKParams& p, int dtype, int cfg, hipStream_t s);
int ir_linear_tiled_pick(int64_t M, int N, int K);
bool ir_linear_tiled_cfg_ok(int cfg, int N);
void ir_host_lanczos_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* kk);
