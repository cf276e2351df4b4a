/*
 * instantrestore_hip.h - C ABI of the MI355X (gfx950) hot path of InstantRestore.
 *
 * This is the drop-in boundary of the build: a plain-C interface (raw device pointers,
 * explicit strides, a hipStream_t passed as void*) that the Python host side binds with
 * ctypes (instantrestore_amd/_lib.py) and that a maintainer of the reference would bind from
 * face_replace/models/attn_processors.py.  The reference itself is pure
 * PyTorch and has no FFI; each entry point below names the reference code it replaces.
 *
 * Conventions
 *   - every function returns 0 on success and a negative ir_status on failure; nothing is
 *     thrown across the ABI; ir_last_error_string() describes the last failure of the
 *     calling thread;
 *   - all device work is enqueued asynchronously on `stream` (a hipStream_t; NULL = the
 *     legacy default stream); nothing synchronises, nothing allocates;
 *   - the caller owns every buffer; the library keeps no state between calls (no process-wide
 *     switches: kernel selection for benchmarks is the per-call `tuning` field of the args);
 *   - tensors are described by a base pointer plus strides IN ELEMENTS; the innermost
 *     (head_dim) axis is always contiguous and head_dim is always IR_HEAD_DIM = 64
 *     (SD-Turbo: attention_head_dim [5,10,20,20] x 64 channels);
 *   - element type of q/k/v/out is selected by ir_dtype (fp16 or bf16, 2 bytes); softmax
 *     statistics, AdaIN statistics and all accumulation are fp32.
 */
#ifndef INSTANTRESTORE_HIP_H
#define INSTANTRESTORE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IR_ABI_VERSION 10
#define IR_HEAD_DIM 64

typedef enum ir_status {
  IR_OK = 0,
  IR_ERR_INVALID_ARG = -1, /* NULL pointer, negative size, bad stride, bad struct_size, a broken rule of a pointer-table call */
  IR_ERR_UNSUPPORTED = -2, /* dtype / head_dim / alignment the kernels do not implement */
  IR_ERR_LAUNCH = -3,      /* hipLaunchKernel reported an error (see ir_last_error_string) */
  IR_ERR_WORKSPACE = -4    /* workspace too small */
} ir_status;

typedef enum ir_dtype { IR_DTYPE_F16 = 0, IR_DTYPE_BF16 = 1 } ir_dtype;

/* flags of ir_shared_attn_args.flags */
#define IR_FLAG_INCLUDE_SELF 1u /* train_input: self K/V block precedes the reference blocks */
#define IR_FLAG_Q_PRESCALED 2u  /* q already holds Q * scale * log2(e) (the fused q/k/v projection applies the factor to its
                                   fp32 accumulator before the one rounding to 16 bit, ir_linear_fwd col_scale): the
                                   scores leave the matrix pipe in the exp2 domain and the kernel saves one multiply-add
                                   per score.  `scale` is still the reference's attn.scale (used for the LSE). */
#define IR_FLAG_OUT_F32 4u      /* out is fp32 (strides in fp32 elements): the result of the SAME kernel the call would launch
                                   otherwise, stored BEFORE its rounding to the 16-bit type - parity instrumentation
                                   (tests show the pre-rounding error of the kernel that ships) */
#define IR_FLAG_BATCH_INVARIANT 8u /* ABI v10, opt-in: the bytes of every output of batch entry b (out, lse, seg_mass) depend on
                                   entry b's own inputs and the per-entry parameters only (dtype, len_q, heads, segment lengths,
                                   n_refs, INCLUDE_SELF, AdaIN on/off, Q_PRESCALED, valid_refs given or not, key_bias given or not, ref_lens given or not, OUT_F32) - not on
                                   the batch size, the entry's position, other entries, the stream, graph capture, the workspace,
                                   whether lse / seg_mass are asked for, IR_ATTN_W128 or the device's CU count.  The kernel and a
                                   fixed cut of every item into K/V-range pieces (merged in piece order) are chosen from those
                                   parameters alone (ir_shared_attn_plan).  Not combinable with a non-zero `tuning`. */

/*
 * ir_shared_attn_fwd - fused extended self-attention (flash-style, no probability matrix).
 *
 * Replaces the body of SharedAttnProcessor.forward between the q/k/v projections and to_out
 * (face_replace/models/attn_processors.py:232-264): the 3+2N head_to_batch_dim copies
 * (:232-241), adain() of every reference V (:242-246, when adain_a/adain_b are given), the
 * torch.cat of the extended K/V (:247-252), get_attention_scores = baddbmm+softmax (:257,
 * diffusers 0.24 Attention) and the bmm + batch_to_head_dim (:263-264).  With n_refs == 0 it is
 * the plain attention of AttnProcessor.forward (:76-82) and of the self_attn_idx=None branch
 * (:253-255), cross attention included (kv length = len_self).
 *
 *   O[b,i,h,:] = sum_j softmax_j( scale * <Q[b,i,h,:], K_ext[b,j,h,:]> ) * V_ext[b,j,h,:]
 *   K_ext / V_ext column order: [self tokens (iff IR_FLAG_INCLUDE_SELF)] ++ ref 0 ++ ... ++ ref N-1
 *   V_ext of reference n is  v_ref[b,n,j,h,d] * adain_a[b,n,h,d] + adain_b[b,n,h,d]  (if given).
 *
 * Layouts (strides in elements, d contiguous):
 *   q      (B, len_q,   H, 64)  strides q_sb, q_sl, q_sh
 *   k_self (B, len_self,H, 64)  strides ks_sb, ks_sl, ks_sh      v_self: vs_*
 *   k_ref  (B, N, len_ref, H, 64) strides kr_sb, kr_sn, kr_sl, kr_sh   v_ref: vr_*
 *   out    (B, len_q,   H, 64)  strides o_sb, o_sl, o_sh
 *   adain_a, adain_b : fp32 (B, N, H, 64) contiguous, or both NULL
 *   lse    : fp32 (B, H, len_q) contiguous or NULL; natural-log sum-exp of the scaled scores
 * i.e. a (B, L, C=H*64) activation is passed as is with sl = C, sh = 64, and the reference's
 * ref_keys[idx] (B, N, L, C) with sn = L*C (pix2pix_turbo.py:265-266): nothing is copied.
 * All base pointers and strides must keep every (row, head) vector 16-byte aligned.
 * Batch, reference and head strides, and the distances between table entries, may be any such int64 value: every kernel forms
 * those offsets in 64 bits.  The ROW strides of K and V (ks_sl, vs_sl with IR_FLAG_INCLUDE_SELF; kr_sl, vr_sl with n_refs > 0,
 * dense or through tables) are limited in the calls that launch or describe the forward (ir_shared_attn_fwd,
 * ir_time_shared_attn_fwd, ir_shared_attn_kernel_name, ir_shared_attn_plan, ir_shared_attn_workspace_bytes_for): its kernels walk
 * one (b, segment, head) through a buffer descriptor with signed 32-bit byte offsets, so
 *     64 * ceil(len / 64) * row_stride * 2 + 128  <=  IR_ATTN_SEG_BYTES_MAX
 * (the segment's whole 64-key tiles plus one head row; (len - 1) * row_stride * 2 + 128 is the span the descriptor covers).  A
 * longer segment is refused with IR_ERR_UNSUPPORTED and a message that names the stride and the largest one accepted.  The
 * read-out entry points (ir_attn_probs, ir_attn_probs_ex, ir_attn_segment_mass, ir_attn_rows) address K through 64-bit pointers
 * and do not have the limit.
 */
#define IR_ATTN_SEG_BYTES_MAX 2147483647LL
typedef struct ir_shared_attn_args {
  uint32_t struct_size; /* = sizeof(ir_shared_attn_args), or sizeof(ir_shared_attn_table_args) / sizeof(ir_shared_attn_bias_args) / sizeof(ir_shared_attn_ragged_args) / sizeof(ir_shared_attn_region_args) when the block is one (below) */
  int32_t dtype;        /* ir_dtype */
  uint32_t flags;       /* IR_FLAG_* */
  int32_t batch;        /* B */
  int32_t heads;        /* H */
  int32_t len_q;        /* query tokens */
  int32_t len_self;     /* tokens of k_self / v_self (0 allowed iff !INCLUDE_SELF) */
  int32_t n_refs;       /* N (0 = plain attention) */
  int32_t len_ref;      /* tokens per reference */
  float scale;          /* attn.scale = head_dim ** -0.5 */
  const void* q;
  const void* k_self;
  const void* v_self;
  const void* k_ref;
  const void* v_ref;
  const float* adain_a;
  const float* adain_b;
  void* out;
  float* lse;
  int64_t q_sb, q_sl, q_sh;
  int64_t ks_sb, ks_sl, ks_sh;
  int64_t vs_sb, vs_sl, vs_sh;
  int64_t kr_sb, kr_sn, kr_sl, kr_sh;
  int64_t vr_sb, vr_sn, vr_sl, vr_sh;
  int64_t o_sb, o_sl, o_sh;
  void* workspace;          /* optional device scratch (see ir_shared_attn_workspace_bytes), or NULL */
  uint64_t workspace_bytes;
  int32_t tuning;           /* 0 = default kernel dispatch.  Benchmarks / A-B tests only: IR_TUNE_* selects one kernel
                               for this call (an unknown or unavailable value is IR_ERR_UNSUPPORTED). */
  int32_t reserved;         /* must be 0 */
  const int32_t* valid_refs; /* ABI v8, optional: int32 (B) on the device.  References n >= valid_refs[b] of batch entry b are
                               ALL-ZERO in k_ref and v_ref (ir_zero_invalid_refs; pix2pix_turbo.py:269-273) - a promise by the
                               caller, which lets the kernel account for those segments in closed form (every score of a zero
                               key is exactly 0, every value row is 0, or the AdaIN shift b when an affine is given) instead of
                               walking their tiles.  Same result as with NULL: zeroed, not masked - the tokens keep their exp(0)
                               weight.  NULL = every reference is walked. */
  float* seg_mass;          /* ABI v9, optional output: fp32 (B, H, len_q, S) contiguous, S = (INCLUDE_SELF ? 1 : 0) + n_refs - the
                               attention mass of every K/V segment, mass[b,h,i,s] = sum over the keys j of segment s of
                               softmax_j(scale * <q_i, k_j>), as a BY-PRODUCT of this launch: the kernels hold the row sums at
                               every segment boundary anyway and store the cumulative log-sum-exp there; a row-sized finishing
                               kernel on the same stream turns them into masses (the S masses of a row sum to exactly 1).  What
                               gradio_demo.py:119-127 reduces attention_probs to, with no second pass over Q and K
                               (ir_attn_segment_mass is that second pass, for callers that only kept the LSE).  Taken as
                               differences of cumulative sums: absolute accuracy ~1e-6, not relative.  Column order: segment 0
                               is the SELF segment when INCLUDE_SELF is set, so the reference demo's blocks idx 0..3 (which start
                               at column 0) are mass[..., 0:4] - valid only when len_self == len_ref - and the per-REFERENCE
                               masses are mass[..., INCLUDE_SELF:].  NULL = off. */
} ir_shared_attn_args;

/*
 * Reference K/V through pointer tables: ir_shared_attn_args with two optional fields appended.  Every entry point that takes an
 * `const ir_shared_attn_args*` also takes a pointer to this block (cast to its first member) and tells the two apart by
 * `args.struct_size`: sizeof(ir_shared_attn_args) - the block ends behind seg_mass and there are no tables - or
 * sizeof(ir_shared_attn_table_args).  Every other size is IR_ERR_INVALID_ARG.  IR_ABI_VERSION stays 10: callers built against the
 * shorter block keep working unchanged, and struct_size carries the compatibility.
 *
 *   k_ref_table : device array of B*N device pointers, entry [b*N + n] = &K[b, n, 0, 0, 0] (the first element of reference n of batch
 *                 entry b, a (len_ref, H, 64) matrix with strides kr_sl, kr_sh); v_ref_table the same for V (vr_sl, vr_sh)
 *
 * Rules of a table call:
 *   - both tables are given or both are NULL (NULL: the call is a dense one);
 *   - with tables k_ref and v_ref must be NULL, n_refs must be > 0, and kr_sb, kr_sn, vr_sb, vr_sn must be 0;
 *   - every ENTRY is 16-byte aligned: the caller's promise (the library cannot read device memory while it validates);
 *   - with valid_refs, entries [b*N + n] with n >= valid_refs[b] are never read or dereferenced by ir_shared_attn_fwd
 *     (ir_attn_probs[_ex], ir_attn_segment_mass and ir_attn_rows walk every reference and read every entry of the K table);
 *   - the tables are read by the kernels when they RUN: a replayed hipGraph follows in-place updates of them (as row_index of
 *     ir_attn_rows does).
 * A table call runs the kernel, form and K/V-range pieces the same dense call would run (ir_shared_attn_kernel_name and
 * ir_shared_attn_plan give the same answers) and the same arithmetic: identical bytes for identical data.  ir_adain_stats keeps its
 * dense v_ref; a table caller gets its AdaIN affine from cached content statistics (ir_adain_stats_cached,
 * ir_adain_affine_from_partials).
 */
typedef struct ir_shared_attn_table_args {
  ir_shared_attn_args args;        /* args.struct_size = sizeof(ir_shared_attn_table_args) */
  const void* const* k_ref_table;
  const void* const* v_ref_table;
} ir_shared_attn_table_args;

/*
 * Additive key bias: masks and weights on keys.  A third block, ir_shared_attn_table_args with three fields appended, told apart by
 * `struct_size` as the table block is (sizeof(ir_shared_attn_bias_args) = the table block's size + 24; every size other than the
 * three is IR_ERR_INVALID_ARG; IR_ABI_VERSION stays 10).  The tables may be NULL (a dense call); key_bias may be NULL, and then the
 * call is the call of the shorter blocks in every respect (kernel, plan, bytes).
 *
 *   extended key order: [self (iff INCLUDE_SELF)] ++ ref 0 ++ ... ++ ref N-1, lengths len_self and len_ref, PACKED (no tile padding):
 *                       Lkv = INCLUDE_SELF * len_self + N * len_ref
 *   bias[b,h,j] = key_bias[b * kb_sb + h * kb_sh + j]            (fp32 on the device; kb_sh = 0: one row shared by all heads)
 *   P[b,h,i,:]  = softmax_j( scale * <q_i, k_j> + bias[b,h,j] )   (what diffusers' attention_mask is: added to the scaled scores)
 *   lse         = log sum_j exp(scale * s_j + bias_j), natural units
 *
 * A key whose bias is -inf or <= IR_KEY_BIAS_MASKED is MASKED: its probability is exactly 0 and it never moves the kernel's running
 * reference.  (diffusers' -10000.0 convention; exp(-1e4) is 0 in fp32 and fp64 anyway, so this differs from the literal arithmetic
 * only where EVERY key of a (b, h) is masked.)  A (b, h) with every key masked gives out = 0 (exact zeros), lse = -inf and all segment
 * masses 0 - never NaN.  NaN or +inf bias: undefined.  Accuracy: finite unmasked biases of magnitude <= 64 meet the tolerances of the
 * call without bias; larger finite magnitudes are legal, with an exponent error of 2^-24 * |bias| * log2(e).
 * The bias is read when the kernel RUNS: a replayed hipGraph follows in-place updates.  Alignment: key_bias, kb_sb and kb_sh are
 * 4-byte quantities (any float pointer, any element strides >= 0); segment starts need no alignment, len_self and len_ref are arbitrary.
 * Nothing outside the Lkv floats of a (b, h) row is used.
 * AdaIN is unchanged by a bias: the affine comes from the statistics over ALL reference tokens, masked or not (the reference's adain()
 * knows no mask); a masked reference merely takes no attention.  Statistics over the kept tokens alone are an opt-in of their own:
 * ir_token_stats_weighted + ir_adain_affine_from_stats make the affine, which is an input here.
 * Per-reference weights are a special case: weight w_n on reference n is the bias log(w_n) on every key of its segment (w_n = 0:
 * masked), with seg_mass as the read-back.  Masked is not zeroed: a zero-filled reference (valid_refs) keeps exp(0) per key.
 *
 * Taken by ir_shared_attn_fwd, ir_time_shared_attn_fwd, ir_shared_attn_kernel_name, ir_shared_attn_plan and
 * ir_shared_attn_workspace_bytes_for.  A call with a bias always runs the software-pipelined 32-row kernel (its BIAS form: the
 * pre-scaled-Q form with IR_FLAG_Q_PRESCALED or IR_TUNE_PIPE32_PRESCALE_Q, the early-QK form otherwise), at every len_q.
 * Accepted with it: seg_mass, lse, IR_FLAG_OUT_F32, IR_FLAG_Q_PRESCALED, AdaIN, tables, IR_FLAG_BATCH_INVARIANT, n_refs = 0.
 * Refused (IR_ERR_UNSUPPORTED): key_bias with valid_refs (the closed form assumes score 0 on the zero suffix); a tuning other than
 * IR_TUNE_DEFAULT, IR_TUNE_PIPE32_PRESCALE_Q, IR_TUNE_PIPE32_EARLYQK; and ir_attn_probs[_ex], ir_attn_segment_mass, ir_attn_rows
 * with a non-NULL key_bias (their exp(s - lse) would be wrong without it).
 */
typedef struct ir_shared_attn_bias_args {
  ir_shared_attn_table_args t;   /* t.args.struct_size = sizeof(ir_shared_attn_bias_args); tables may be NULL (dense call) */
  const float* key_bias;         /* fp32 on the device, or NULL (= a call without bias, same as the shorter blocks) */
  int64_t kb_sb, kb_sh;          /* strides in fp32 elements over batch and head; kb_sh = 0: one row shared by all heads */
} ir_shared_attn_bias_args;
#define IR_KEY_BIAS_MASKED (-1.0e4f)

/*
 * Per-reference token counts (ragged references).  A fourth block, ir_shared_attn_bias_args with two fields appended, told apart by
 * `struct_size` as the others are (sizeof(ir_shared_attn_ragged_args) = the bias block's size + 16; every size other than the four is
 * IR_ERR_INVALID_ARG; IR_ABI_VERSION stays 10).  Tables and key_bias may be NULL; ref_lens may be NULL, and then the call is the call
 * of the shorter blocks in every respect (kernel, plan, bytes).
 *
 *   c[b,n] = clamp(ref_lens[b * rl_sb + n], 0, len_ref)    the number of keys reference n of batch entry b HAS
 *
 * len_ref becomes the CAPACITY of a reference segment: its allocation, its strides and the 32-bit span rule stay as they are.  Keys
 * t >= c[b,n] do not exist: they are never used, whatever bytes lie there (NaN included), and in a table call an entry whose count is
 * 0 is never read or dereferenced.  The self segment is untouched.  The extended key order is unchanged; lse and seg_mass are over
 * the existing keys, and a reference with count 0 has mass 0: ABSENT (probability exactly 0), not zero-filled (valid_refs: exp(0)
 * per key).  A (b, h) with no key at all (no self block, every count 0) gives out = 0, lse = -inf and masses 0 - never NaN: the
 * rule of a wholly masked row of the key bias.  The AdaIN affine (adain_a, adain_b) is an input as before; which tokens its
 * statistics are taken over is the caller's business.  ref_lens is read when the kernel RUNS: a replayed hipGraph follows in-place
 * updates.  ir_compact_ref_tokens (below) packs the kept tokens of a reference to the front of a segment and writes the counts.
 *
 * Taken by ir_shared_attn_fwd, ir_time_shared_attn_fwd, ir_shared_attn_kernel_name, ir_shared_attn_plan and
 * ir_shared_attn_workspace_bytes_for.  A call with counts always runs the software-pipelined 32-row kernel (its RAGGED form: the
 * pre-scaled-Q form with IR_FLAG_Q_PRESCALED or IR_TUNE_PIPE32_PRESCALE_Q, the early-QK form otherwise), at every len_q; the cut
 * into K/V-range pieces and the workspace are planned for full references (a piece of a short entry may be empty).  With every count
 * equal to len_ref the bytes are those of the same form without counts.
 * Accepted with it: seg_mass, lse, IR_FLAG_OUT_F32, IR_FLAG_Q_PRESCALED, AdaIN, tables, IR_FLAG_BATCH_INVARIANT.
 * Refused (IR_ERR_UNSUPPORTED): ref_lens with valid_refs (a count of 0 says "absent", valid_refs says "zero-filled": pick one);
 * ref_lens with a non-NULL key_bias (the bias indexes the packed uniform key axis: a follow-up); n_refs == 0; a tuning other than
 * IR_TUNE_DEFAULT, IR_TUNE_PIPE32_PRESCALE_Q, IR_TUNE_PIPE32_EARLYQK; a ref_lens that is not 4-byte aligned; and ir_attn_probs[_ex],
 * ir_attn_segment_mass, ir_attn_rows with a non-NULL ref_lens (they would walk the tails).  rl_sb < n_refs is IR_ERR_INVALID_ARG.
 */
typedef struct ir_shared_attn_ragged_args {
  ir_shared_attn_bias_args b;    /* b.t.args.struct_size = sizeof(ir_shared_attn_ragged_args); tables and key_bias may be NULL */
  const int32_t* ref_lens;       /* device, int32 [B][N] rows rl_sb apart, or NULL (= the call of the shorter blocks in every respect) */
  int64_t rl_sb;                 /* elements between batch rows, >= N */
} ir_shared_attn_ragged_args;

/*
 * Region-restricted attention: per-query masks from region labels.  A fifth block, ir_shared_attn_ragged_args with four fields
 * appended, told apart by `struct_size` as the others are (sizeof(ir_shared_attn_region_args) = the ragged block's size + 32; every
 * size other than the five is IR_ERR_INVALID_ARG; IR_ABI_VERSION stays 10).  Tables, key_bias and ref_lens may be NULL; q_allow and
 * key_region may BOTH be NULL, and then the call is the call of the shorter blocks in every respect (kernel, plan, bytes).  Exactly
 * one of them NULL is IR_ERR_INVALID_ARG.
 *
 *   region[b,j]  = key_region[b * kg_sb + j]      one small integer per key of the PACKED extended key axis (the axis of key_bias)
 *   allow[b,i]   = q_allow[b * qa_sb + i]         one 32-bit word per query row: bit g set = the row may attend keys of region g
 *   allowed(b,i,j) = region[b,j] in [0, IR_REGION_MAX - 1]  &&  ((allow[b,i] >> region[b,j]) & 1)
 *   P[b,h,i,:]   = softmax over the allowed j of scale * <q_i, k_j>
 *
 * One rule for all heads.  A key whose region is outside [0, 31] belongs to nobody.  A pair that is not allowed has probability
 * exactly 0 and never moves the row's running reference, whatever its score (the rule of a masked key of the bias).  A row with no
 * allowed key (allow == 0, or no key of its regions present) gives out = 0 (exact zeros), lse = -inf and masses 0 - never NaN.  lse
 * and seg_mass are over the allowed keys.  AdaIN is unchanged: the affine is an input; a region rule merely takes attention away.
 * Both arrays are read when the kernel RUNS: a replayed hipGraph follows in-place updates.  Both are 4-byte aligned, and nothing
 * outside the len_q / Lkv words of an entry is used.  The mask costs what a key bias costs in bytes: a dense (len_q, Lkv) bias never
 * exists.
 *
 * Taken by ir_shared_attn_fwd, ir_time_shared_attn_fwd, ir_shared_attn_kernel_name, ir_shared_attn_plan and
 * ir_shared_attn_workspace_bytes_for.  A call with regions always runs the software-pipelined 32-row kernel (its REGION form: the
 * pre-scaled-Q form with IR_FLAG_Q_PRESCALED or IR_TUNE_PIPE32_PRESCALE_Q, the early-QK form otherwise), at every len_q.  Every tile
 * is walked: a tile no row of a 32-row block may attend contributes zeros (skipping it is a follow-up).
 * Accepted with it: seg_mass, lse, IR_FLAG_OUT_F32, IR_FLAG_Q_PRESCALED, AdaIN, tables, IR_FLAG_BATCH_INVARIANT, n_refs = 0.
 * Refused (IR_ERR_UNSUPPORTED): regions with a non-NULL key_bias and regions with a non-NULL ref_lens (regions together with a bias
 * or with counts are a follow-up); regions with valid_refs (the closed form of the zero suffix gives every row its keys); a tuning
 * other than IR_TUNE_DEFAULT, IR_TUNE_PIPE32_PRESCALE_Q, IR_TUNE_PIPE32_EARLYQK; arrays that are not 4-byte aligned; and every
 * read-out entry point (ir_attn_probs[_ex], ir_attn_segment_mass, ir_attn_rows, ir_attn_match, ir_attn_topk, ir_attn_transfer,
 * ir_attn_received, ir_attn_key_match) with non-NULL arrays (their exp(s - lse) would count the pairs the forward left out).
 * qa_sb < len_q and kg_sb < Lkv are IR_ERR_INVALID_ARG.
 */
#define IR_REGION_MAX 32
typedef struct ir_shared_attn_region_args {
  ir_shared_attn_ragged_args r;   /* r.b.t.args.struct_size = sizeof(ir_shared_attn_region_args); tables, key_bias and ref_lens may be NULL */
  const uint32_t* q_allow;        /* device, (B, Lq) rows qa_sb apart: bit g set = the row may attend keys of region g; or NULL (both) */
  int64_t qa_sb;                  /* elements between batch rows, >= len_q */
  const int32_t* key_region;      /* device, (B, Lkv) over the PACKED extended key axis (the axis of key_bias), rows kg_sb apart */
  int64_t kg_sb;                  /* >= Lkv */
} ir_shared_attn_region_args;

/* values of ir_shared_attn_args.tuning (csrc/shared_attn_fwd.hip: kAttnVariants has one row per value - kernel family, form, what
 * it takes; ir_attn_choose is the dispatch) */
#define IR_TUNE_DEFAULT 0
#define IR_TUNE_PIPE32_EXACTMAX 7
#define IR_TUNE_PIPE32 10
#define IR_TUNE_PIPE32_PRESCALE_Q 11
#define IR_TUNE_W64X4 12
#define IR_TUNE_W64X8 13
#define IR_TUNE_PIPE32_EARLYQK 14
#define IR_TUNE_W128 16            /* round 6: one wave per SIMD, 128 query rows per wave, hand-placed instruction stream; needs
                                      IR_FLAG_Q_PRESCALED and segment lengths that are multiples of 64; takes valid_refs and
                                      seg_mass (the default dispatch still keeps calls that carry either on the kernel it chose
                                      before: IR_ATTN_W128=1 in the environment sends them to this one) */
#define IR_TUNE_W64_ABL_FIRST 20 /* 20 ... : development builds (-DIR_ABLATIONS) only - energy / timing ablations of the 64-row kernel
                                    (WRONG results: one class of work removed per bit; tools/gpu_energy_probe.py).  Values 3, 4,
                                    6, 9 (round 1: experiments inside the 32-row kernel) and 17 (rounds 2-3: a three-stage
                                    experiment) are retired: every build refuses them. */
#define IR_TUNE_PIPE32_POSTCHECK 18   /* 32-row kernel, pre-scaled Q, reference checked after the exponentials (needs
                                         IR_FLAG_Q_PRESCALED; parity-green, same speed as PIPE32_PRESCALE_Q: opt-in) */

/*
 * Scratch for the remainder split: when the number of (batch, head, query-block) work items is not
 * a multiple of the resident workgroup slots, the items of the last, partially filled round are
 * cut into K/V-range pieces whose partial (O, max, sum) results are merged by a second small
 * kernel, so that round ends early instead of running at full length.  Passing NULL (or a smaller
 * buffer) only disables (or limits) the split; results are identical up to fp32 rounding.
 */
size_t ir_shared_attn_workspace_bytes(void);

/* Name of the kernel ir_shared_attn_fwd would launch for these arguments (incl. their `tuning` field)
 * (reporting only: bench.py's roofline block); "" if the arguments are invalid. Storage: one buffer per thread, overwritten by
 * the thread's next call. */
const char* ir_shared_attn_kernel_name(const ir_shared_attn_args* args);

int ir_shared_attn_fwd(const ir_shared_attn_args* args, void* stream);

/*
 * Batch-invariant plan (ABI v10, IR_FLAG_BATCH_INVARIANT; host only, no GPU touched).  Every (batch entry, head, query block)
 * work item runs `pieces_per_item` K/V-range pieces whose tile boundaries depend on that item alone, merged in piece order
 * (1: whole items, no merge pass, no workspace - always so for plain attention, n_refs == 0).  Scratch: ir_shared_attn_workspace_bytes_for(args) bytes cover one launch
 * over the whole batch; a smaller workspace runs the batch as several launches of `batch_per_launch` entries (same per-item
 * plan, same bytes); a workspace that cannot hold one entry's pieces makes ir_shared_attn_fwd fail with IR_ERR_WORKSPACE.
 * Without IR_FLAG_BATCH_INVARIANT the plan query returns IR_ERR_INVALID_ARG (the default dispatch plans inside each launch).
 */
typedef struct ir_shared_attn_plan_info {
  uint32_t struct_size;      /* = sizeof(ir_shared_attn_plan_info) */
  int32_t kernel;            /* IR_TUNE_* value of the kernel family the plan launches (W128, W64X8, PIPE32_PRESCALE_Q, PIPE32_EARLYQK) */
  int32_t rows_per_item;     /* query rows per work item */
  int32_t items_per_batch;   /* work items per batch entry: heads * ceil(len_q / rows_per_item) */
  int32_t pieces_per_item;   /* K/V-range pieces per work item */
  int32_t batch_per_launch;  /* batch entries per launch with the args' workspace (0: one entry does not fit) */
  uint64_t workspace_bytes;  /* = ir_shared_attn_workspace_bytes_for(args) */
} ir_shared_attn_plan_info;
int ir_shared_attn_plan(const ir_shared_attn_args* args, ir_shared_attn_plan_info* plan);
/* scratch bytes ir_shared_attn_fwd can use for these arguments in one launch: the batch-invariant plan's pieces with the flag,
 * ir_shared_attn_workspace_bytes() without it; 0 if the arguments are invalid or the plan needs none */
size_t ir_shared_attn_workspace_bytes_for(const ir_shared_attn_args* args);

/*
 * ir_attn_probs - materialise attention_probs (B, H, len_q, Lkv) for the dump path.
 *
 * Replaces `self.attention_probs = attention_probs.reshape(B, heads, L, Lkv)`
 * (attn_processors.py:258-261), read by test.py:108, gradio_demo.py:118, coach.py:312.
 * Uses the same args as ir_shared_attn_fwd (out / adain_* are ignored) plus the `lse` that
 * call produced:  probs[b,h,i,j] = exp(scale*<q_i,k_j> - lse[b,h,i]), stored in `dtype`,
 * contiguous, column order as above.
 * Accuracy: this fp32 probability - shared by every read-out below - is held by the tests to a relative error of 8 * 2^-23 *
 * max(1, |lse|, scale * sum_d |q_d k_d|) against float64 with the same lse, ahead of the one rounding to `dtype`
 * (tests/prob_bounds.py has the bound and the measured table).
 *
 * HBM-write bound (H*L*Lkv*2 bytes per identity).  When len_self and len_ref are multiples of 8 keys (every row of
 * probs then starts 16-byte aligned) the line kernel runs: whole 128-byte lines per store instruction (round 5); other
 * lengths take the 2-byte-store kernel.  ir_attn_probs_ex names the kernel (benchmarks / A-B tests).
 */
int ir_attn_probs(const ir_shared_attn_args* args, void* probs, void* stream);
#define IR_PROBS_AUTO 0
#define IR_PROBS_GENERIC 1   /* 2-byte stores, any length */
#define IR_PROBS_LINES64 2       /* line kernel, 64 query rows x 64 keys (128 B per row) per wave and step */
#define IR_PROBS_LINES32 3       /* 32 rows x 64 keys */
#define IR_PROBS_LINES32_K128 4  /* 32 rows x 128 keys (256 B per row and store batch) */
#define IR_PROBS_LINES64_K128 5  /* 64 rows x 128 keys */
#define IR_PROBS_LINES32_K256 6  /* 32 rows x 256 keys (512 B per row and store batch) */
int ir_attn_probs_ex(const ir_shared_attn_args* args, void* probs, int32_t kernel, void* stream);
/* IR_FLAG_BATCH_INVARIANT (ABI v10) is accepted by ir_attn_probs[_ex] and ir_attn_segment_mass: every probability and every
 * mass is computed from its own row of q and the keys of its own batch entry in an order fixed by the per-entry parameters
 * (IR_PROBS_AUTO: the line kernel when every segment length is a multiple of 8 keys, 64 rows per wave from len_q >= 256,
 * else the 2-byte-store kernel), so given an invariant lse they are batch invariant. */

/*
 * ir_attn_segment_mass (ABI v8, opt-in) - attention mass per K/V segment without the probability matrix.
 *
 *   mass[b,h,i,s] = sum over the keys j of segment s of exp(scale*<q_i,k_j> - lse[b,h,i]),  fp32 (B, H, len_q, S) contiguous,
 *   segments s in the column order above: [self (iff IR_FLAG_INCLUDE_SELF)] ++ ref 0 ++ ... ++ ref N-1, S = include_self + N.
 * What gradio_demo.py:119-127 reduces attention_probs to (`probs[..., attn_size*idx : attn_size*(idx+1)].sum(-1)` per
 * reference): the same numbers (summed in fp32 before any 16-bit rounding) without writing H*L*Lkv*2 bytes.  Same args as
 * ir_attn_probs; any segment length.
 */
int ir_attn_segment_mass(const ir_shared_attn_args* args, float* mass, void* stream);

/*
 * ir_attn_rows (opt-in) - the probability rows of a caller-chosen set of query tokens, without the probability matrix.
 *
 * Replaces `attention_probs[:, :, idx, :]` and what face_replace/training/utils/vis_utils.py:88-110
 * (get_visualization_image; coach.py:308-317, 367-377) reduces it to: the head mean of attention_probs, the rows of the
 * facial landmarks picked out of it (`img[landmark_indices]`) and their sum, reshaped to one heat map over the degraded
 * image and its references.  calc_landmark_loss (coach.py:531-560) and calc_attn_probs (inference/test.py:93-110) read rows
 * of the same tensor.  Same args as ir_attn_probs (q, the K pointers, lse; v_*, adain_*, out, valid_refs, seg_mass and workspace
 * are ignored, `tuning` must be 0) plus
 *   row_index  int32 (B, n_rows) contiguous on the device: token indices into the query axis, one list per batch entry.
 *              Duplicates are legal and produce repeated rows (IR_ROWS_MAP counts them as often as they occur, like NumPy
 *              fancy indexing); an index outside [0, len_q) yields an all-zero row and is never used as an address.  Read by
 *              the kernel when it runs: a replayed hipGraph follows in-place updates of it.
 *   n_rows     1 ... len_q
 *   reduce     IR_ROWS_NONE       out = `dtype` (B, H, n_rows, Lkv): p[b,h,r,j] = exp(scale*<q[idx[b,r]], k_j> - lse[b,h,idx[b,r]]),
 *                                 bit-identical to rows idx[b,:] of ir_attn_probs' output (IR_FLAG_Q_PRESCALED: same rule)
 *              IR_ROWS_HEAD_MEAN  out = fp32 (B, n_rows, Lkv): (sum over heads, ascending, of the fp32 p) * (1/H)
 *              IR_ROWS_MAP        out = fp32 (B, Lkv): the sum of the head-mean rows over r in a fixed order
 *   out        contiguous, 16-byte aligned, column order [self (iff INCLUDE_SELF)] ++ ref 0 ++ ... ++ ref N-1
 * Bound: K read once (B * H * Lkv * 128 bytes) + the output written; no workspace, no atomics, one launch; asynchronous and
 * capturable.  The cut of the work follows len_self, len_ref, n_refs, n_rows and reduce only: the call is batch invariant with
 * or without IR_FLAG_BATCH_INVARIANT.  Any segment length; rows are written 16 bytes at a time when every segment length is
 * a multiple of 8 keys (IR_ROWS_NONE) or 4 keys (fp32 forms).
 */
#define IR_ROWS_NONE 0
#define IR_ROWS_HEAD_MEAN 1
#define IR_ROWS_MAP 2
int ir_attn_rows(const ir_shared_attn_args* args, const int32_t* row_index, int32_t n_rows, int32_t reduce, void* out, void* stream);

/*
 * ir_attn_match (opt-in) - the best-matching key of every K/V segment for a caller-chosen set of query tokens, without the
 * probability matrix.
 *
 * Replaces `attention_probs[..., segment].max(-1)` / `.argmax(-1)` per segment s of the column order above
 * ([self (iff INCLUDE_SELF)] ++ ref 0 ++ ... ++ ref N-1, S = include_self + N): for this token of the degraded face, which token
 * of each reference it draws from, and how strongly - a dense correspondence field with a confidence, at resolutions where the
 * dump cannot be formed.  Same args as ir_attn_rows (q, the K pointers or the K table, lse; v_*, adain_*, out, valid_refs, seg_mass
 * and workspace are ignored - every reference is walked - and `tuning` must be 0) plus
 *   row_index  int32 (B, n_rows) contiguous on the device, as for ir_attn_rows: duplicates are rows like any other; an index
 *              outside [0, len_q) gives index = -1, prob = 0 and is never used as an address.  Read by the kernel when it runs:
 *              a replayed hipGraph follows in-place updates of it (and of the pointer tables).
 *   n_rows     1 ... len_q
 *   reduce     IR_MATCH_PER_HEAD   index int32 (B, H, n_rows, S), prob fp32 (B, H, n_rows, S):
 *                                  prob = max over the keys j of segment s of the fp32
 *                                  p = exp2(fma(<q[idx[b,r]], k_j>, scale*log2(e), -lse[b,h,idx[b,r]]*log2(e))) - the value ir_attn_probs and
 *                                  ir_attn_rows round to `dtype`, so prob rounded to `dtype` IS the maximum of their row segment
 *                                  (IR_FLAG_Q_PRESCALED: same rule as there)
 *              IR_MATCH_HEAD_MEAN  index int32 (B, n_rows, S), prob fp32 (B, n_rows, S): the maximum of the head mean formed as
 *                                  IR_ROWS_HEAD_MEAN forms it ((sum over heads, ascending, of the fp32 p) * (1/H)) - bit for bit
 *                                  the maximum of ir_attn_rows' head-mean row segment
 *   index      the LOWEST key j, counted from 0 inside its segment, that attains prob (ties go to the lowest key)
 *   index, prob  contiguous, 4-byte aligned
 * Bound: K read once per group of 96 rows (ceil(n_rows / 96) * B * H * Lkv * 128 bytes) and two numbers per (row, segment)
 * written; no workspace, no atomics, one launch; asynchronous and capturable.  One wave walks a whole segment for up to 96
 * rows, so every output element has one writer and one order; the cut follows len_self, len_ref, n_refs, n_rows and reduce only:
 * the call is batch invariant with or without IR_FLAG_BATCH_INVARIANT.  Any segment length.
 * Refused: a key_bias or ref_lens block (IR_ERR_UNSUPPORTED, as for the other read-outs), tuning != 0, NULL or misaligned
 * row_index / index / prob, NULL lse, n_rows outside 1 ... len_q, another reduce, more than 2^31 - 4 work items.
 */
#define IR_MATCH_PER_HEAD 0
#define IR_MATCH_HEAD_MEAN 1
int ir_attn_match(const ir_shared_attn_args* args, const int32_t* row_index, int32_t n_rows, int32_t reduce, int32_t* index, float* prob,
                  void* stream);

/*
 * ir_attn_transfer (opt-in) - attention-weighted sums of a per-key payload for a caller-chosen set of query tokens, per K/V
 * segment, without the probability matrix.
 *
 * Replaces `einsum('bhij,bjc->bhic', attention_probs[..., segment], y[:, segment])` per segment s of the column order above
 * ([self (iff INCLUDE_SELF)] ++ ref 0 ++ ... ++ ref N-1, S = include_self + N): the soft form of ir_attn_match.  With y = the
 * (y, x) of every key it is the expected position inside each reference at sub-token precision (soft-argmax correspondences,
 * the segment mass as confidence); with y = the reference pixels pooled to the token grid, the attention-warped reference;
 * with y = a parsing map or landmark heat map, label transfer - at resolutions where the dump cannot be formed.  Same args as
 * ir_attn_rows / ir_attn_match (q, the K pointers or the K table, lse; v_*, adain_*, out, valid_refs, seg_mass and workspace are
 * ignored - every reference is walked - and `tuning` must be 0; IR_FLAG_Q_PRESCALED and IR_FLAG_BATCH_INVARIANT: same rules) plus
 *   payload    fp32 on the device, 4-byte aligned, over the PACKED extended key axis (the axis of key_bias):
 *              y[b, j, c] = payload[b * pay_sb + j * pay_sj + c], strides in floats, every offset formed in 64 bits.
 *              pay_sb >= 0 (0: one payload for every batch entry), pay_sj >= channels; nothing outside the `channels` floats of
 *              a key is read.  Read by the kernel when it runs: a replayed hipGraph follows in-place updates of it (and of
 *              row_index and the pointer tables).
 *   channels   1 ... IR_TRANSFER_MAX_CHANNELS (call again for more)
 *   row_index, n_rows   exactly as for ir_attn_match
 *   reduce     IR_TRANSFER_PER_HEAD   sums fp32 (B, H, n_rows, S, channels), mass fp32 (B, H, n_rows, S)
 *              IR_TRANSFER_HEAD_MEAN  sums fp32 (B, n_rows, S, channels), mass fp32 (B, n_rows, S)
 *   sums       contiguous, 4-byte aligned: sums[.., s, c] = sum over the keys j of segment s of p_j * y[b, j, c], UNNORMALISED, with
 *              the fp32 p = exp2(fma(<q[idx[b,r]], k_j>, scale*log2(e), -lse[b,h,idx[b,r]]*log2(e))) of ir_attn_probs / ir_attn_rows
 *   mass       contiguous, 4-byte aligned, or NULL (not written): mass[.., s] = sum of p_j over the segment.  sums / mass is the
 *              expectation inside a segment, sums summed over s the expectation over all keys.
 * Bit for bit (part of the interface):
 *   - the mass and every channel of a (row, segment, head) are accumulated over the same keys in the same order, one fp32 fused
 *     multiply-add per term with the payload value as multiplicand (the mass: multiplicand 1).  A channel that is 1.0f on every key
 *     equals the mass; a channel that is 1 at a single key and 0 elsewhere equals that key's fp32 p - the value ir_attn_rows
 *     rounds to `dtype` - and is exactly 0 in every other segment;
 *   - IR_TRANSFER_HEAD_MEAN == ((S_0 + S_1) + ... + S_{H-1}) * (1.0f / (float)H) of the IR_TRANSFER_PER_HEAD outputs S_h, sums and
 *     mass alike; with a one-hot channel that is the element of ir_attn_rows' IR_ROWS_HEAD_MEAN row;
 *   - an index outside [0, len_q) gives sums 0 and mass 0 and is never used as an address.
 * Bound: K read once per group of 96 rows (ceil(n_rows / 96) * B * H * Lkv * 128 bytes) and the payload once per work item
 * (Lkv * channels * 4 bytes per row group, head and batch entry); channels + 1 numbers per (row, segment) written; no workspace,
 * no atomics, one launch; asynchronous and capturable.  One wave walks a whole segment for up to 96 rows, so every output element
 * has one writer and one order; the cut follows len_self, len_ref, n_refs, n_rows, channels and reduce only: the call is batch
 * invariant with or without IR_FLAG_BATCH_INVARIANT.  Any segment length.
 * Refused: a key_bias or ref_lens block (IR_ERR_UNSUPPORTED, as for the other read-outs), tuning != 0; IR_ERR_INVALID_ARG: NULL
 * payload / row_index / sums / lse, n_rows outside 1 ... len_q, pay_sb < 0, pay_sj < channels; IR_ERR_UNSUPPORTED: channels
 * outside its range, a misaligned payload / row_index / sums / mass, another reduce, more than 2^31 - 4 work items.
 */
#define IR_TRANSFER_PER_HEAD 0
#define IR_TRANSFER_HEAD_MEAN 1
#define IR_TRANSFER_MAX_CHANNELS 8
int ir_attn_transfer(const ir_shared_attn_args* args, const float* payload, int64_t pay_sb, int64_t pay_sj, int32_t channels,
                     const int32_t* row_index, int32_t n_rows, int32_t reduce, float* sums, float* mass, void* stream);

/*
 * ir_attn_received (opt-in) - per-key sums of the attention over ALL query rows, weighted by a per-row payload, without the
 * probability matrix: the column sums of P.
 *
 * Replaces `einsum('bhij,bic->bhjc', attention_probs, w)` (w = 1: `attention_probs.sum(dim=-2)`): how much every key - every
 * token of every reference - is looked at by the whole degraded face (w = 1), by a region of it (w = a mask) or per label (w = a
 * parsing map).  Every other read-out reduces along the key axis; this one reduces along the query axis, and it is the adjoint of
 * ir_attn_transfer: <w, P y> = <P^T w, y>.  Same args as ir_attn_rows / ir_attn_match / ir_attn_transfer (q, the K pointers or the
 * K table, lse; v_*, adain_*, out, valid_refs, seg_mass and workspace are ignored - every reference is walked - and `tuning` must
 * be 0; IR_FLAG_Q_PRESCALED: same rule; IR_FLAG_BATCH_INVARIANT: accepted, inert) plus
 *   weights    fp32 on the device, 4-byte aligned, over the query axis: w[b, i, c] = weights[b * w_sb + i * w_si + c], strides in
 *              floats, every offset formed in 64 bits.  w_sb >= 0 (0: one payload for every batch entry), w_si >= channels;
 *              nothing outside the `channels` floats of a row is read.  NULL: one channel of ones (channels must be 1).  Read by
 *              the kernel when it runs: a replayed hipGraph follows in-place updates of it (and of the pointer tables).
 *   channels   1 ... IR_RECEIVED_MAX_CHANNELS (call again for more)
 *   reduce     IR_RECEIVED_PER_HEAD   recv fp32 (B, H, Lkv, channels)
 *              IR_RECEIVED_HEAD_MEAN  recv fp32 (B, Lkv, channels)
 *   recv       contiguous, 4-byte aligned: recv[b, h, j, c] = sum over i = 0 .. len_q - 1 of p[b,h,i,j] * w[b,i,c], j on the PACKED
 *              extended key axis [self (iff INCLUDE_SELF)] ++ ref 0 ++ ... ++ ref N-1 (the axis of ir_attn_transfer's payload and of
 *              key_bias), with the fp32 p = exp2(fma(<q_i, k_j>, scale*log2(e), -lse[b,h,i]*log2(e))) of ir_attn_probs / ir_attn_rows
 * Bit for bit (part of the interface):
 *   - every (row, key, channel) term is one fp32 fused multiply-add with the weight as multiplicand (no weights: multiplicand
 *     1.0f); all channels of a key are accumulated over the same rows in the same order.  weights == NULL equals a channel of ones;
 *     two equal channels give equal outputs; a channel that is 1 at one row i and 0 elsewhere equals that row's fp32 p[i, j] at every
 *     key j - the value ir_attn_rows rounds to `dtype`;
 *   - the order is a function of len_q and reduce only - not of batch, the grid, the stream or the device's CU count.  With
 *     l = i mod 32: the partial sum s_l starts at 0 and takes the rows l, l + 32, l + 64, ... in ascending order (lane l of a
 *     half-wave, one row per 32-row block).  The 32 partial sums then meet in a butterfly over the lane bits 1, 2, 4, 8, 16 in that
 *     order - at step m lane l replaces its value by (its own + lane l ^ m's) - which is the balanced tree
 *       ((((s0+s1) + (s2+s3)) + ((s4+s5) + (s6+s7))) + (the same over s8..s15)) + (the same over s16..s31);
 *   - IR_RECEIVED_HEAD_MEAN == ((R_0 + R_1) + ... + R_{H-1}) * (1.0f / (float)H) of the IR_RECEIVED_PER_HEAD outputs R_h (the fold
 *     starts at 0 + R_0); with a one-hot channel that is the element of ir_attn_rows' IR_ROWS_HEAD_MEAN row;
 *   - rows of the padding to a whole 32-row block contribute exactly nothing (probability and weight replaced by 0; a padded
 *     row's own weight is never addressed - nothing behind row len_q - 1 of `weights` is read); keys past the end of a segment
 *     are never written.
 * Bound: Q, lse and the weights read once per group of 96 / 96 / 64 / 32 keys (channels padded to 1 / 2 / 4 / 8), K once;
 * Lkv * channels floats written per (head,) batch entry; no workspace, no atomics, one launch; asynchronous and capturable.  One
 * wave walks the whole query axis for its keys, so every output element has one writer; the cut follows len_self, len_ref,
 * n_refs, channels and reduce only.  Any segment length, any len_q.
 * Checked in this order, after the checks of the args block: IR_ERR_INVALID_ARG: NULL recv, NULL lse; IR_ERR_UNSUPPORTED: channels
 * outside its range; IR_ERR_INVALID_ARG: NULL weights with channels != 1, w_sb < 0, w_si < channels; IR_ERR_UNSUPPORTED: another
 * reduce, a misaligned weights / recv, more than 2^31 - 4 work items.  Refused with the args block: a key_bias or ref_lens block
 * (IR_ERR_UNSUPPORTED, as for the other read-outs), tuning != 0.
 */
#define IR_RECEIVED_PER_HEAD 0
#define IR_RECEIVED_HEAD_MEAN 1
#define IR_RECEIVED_MAX_CHANNELS 8
int ir_attn_received(const ir_shared_attn_args* args, const float* weights, int64_t w_sb, int64_t w_si, int32_t channels,
                     int32_t reduce, float* recv, void* stream);

/*
 * ir_attn_topk (opt-in) - the k best keys of every K/V segment for a caller-chosen set of query tokens, without the probability
 * matrix: ir_attn_match with ranks.
 *
 * Replaces `torch.topk(attention_probs[..., segment], k)` per segment s of the column order above ([self (iff INCLUDE_SELF)] ++
 * ref 0 ++ ... ++ ref N-1, S = include_self + N): the runner-up of a match (the ratio test - a face repeats its structure, and
 * one probability cannot tell one sharp peak from two equal ones), the few best hypotheses of a token, the share of a segment's
 * attention that its k best keys carry - at resolutions where the dump cannot be formed.  Same args as ir_attn_rows /
 * ir_attn_match (q, the K pointers or the K table, lse; v_*, adain_*, out, valid_refs, seg_mass and workspace are ignored - every
 * reference is walked - and `tuning` must be 0; IR_FLAG_Q_PRESCALED: same rule; IR_FLAG_BATCH_INVARIANT: accepted, inert) plus
 *   row_index, n_rows   exactly as for ir_attn_match: duplicates are rows like any other; an index outside [0, len_q) gives
 *              index = -1, prob = 0 in every rank and is never used as an address.  Read by the kernel when it runs: a replayed
 *              hipGraph follows in-place updates of it (and of the pointer tables).
 *   k          1 ... IR_TOPK_MAX
 *   reduce     IR_MATCH_PER_HEAD   index int32 (B, H, n_rows, S, k), prob fp32 (B, H, n_rows, S, k), over the fp32
 *                                  p = exp2(fma(<q[idx[b,r]], k_j>, scale*log2(e), -lse[b,h,idx[b,r]]*log2(e))) - the value ir_attn_probs and
 *                                  ir_attn_rows round to `dtype`, so prob rounded to `dtype` holds the k largest values of their row segment
 *              IR_MATCH_HEAD_MEAN  index int32 (B, n_rows, S, k), prob fp32 (B, n_rows, S, k), over the head mean formed as
 *                                  IR_ROWS_HEAD_MEAN forms it ((sum over heads, ascending, of the fp32 p) * (1/H)) - bit for bit a
 *                                  stable descending sort of ir_attn_rows' head-mean row segment
 *   index, prob  contiguous, 4-byte aligned.  Rank t of a (row, segment) holds the t-th key of the segment under the TOTAL order
 *              (p descending, key ascending): among equal p the lower key comes first.  index counts from 0 inside its segment.
 *              A segment with fewer than k keys fills the ranks len ... k - 1 with index = -1, prob = 0.
 * Bit for bit (part of the interface): rank 0 IS ir_attn_match of the same call, index and prob, in both forms.
 * Bound: K read once per group of 96 rows (ceil(n_rows / 96) * B * H * Lkv * 128 bytes) and 2 k numbers per (row, segment)
 * written; no workspace, no atomics, one launch; asynchronous and capturable.  One wave walks a whole segment for up to 96
 * rows, so every output element has one writer and one order; the cut follows len_self, len_ref, n_refs, n_rows, k and reduce
 * only: the call is batch invariant with or without IR_FLAG_BATCH_INVARIANT.  Any segment length.
 * Refused: a key_bias or ref_lens block (IR_ERR_UNSUPPORTED, as for the other read-outs), tuning != 0; IR_ERR_INVALID_ARG: NULL
 * args / row_index / index / prob / lse, n_rows outside 1 ... len_q; IR_ERR_UNSUPPORTED: another reduce, a misaligned row_index /
 * index / prob, k outside 1 ... IR_TOPK_MAX, more work items than ir_attn_match accepts (2^31 - 4).
 */
#define IR_TOPK_MAX 8
int ir_attn_topk(const ir_shared_attn_args* args, const int32_t* row_index, int32_t n_rows, int32_t k, int32_t reduce,
                 int32_t* index, float* prob, void* stream);

/*
 * ir_attn_key_match (opt-in) - per key, the largest attention probability over ALL query rows and the query row that attains it,
 * without the probability matrix: the column maximum of P.
 *
 * Replaces `attention_probs.max(dim=-2)` / `.argmax(dim=-2)`: which token of the degraded face looks hardest at every token of
 * every reference.  ir_attn_match answers for every query row - occluded skin, hair and background included - and its answer there
 * is the best of a bad lot; correspondence pipelines filter it with the MUTUAL (cycle) check: keep the pair (i, j) only if j is the
 * best key of row i (ir_attn_match) AND i is the best row of key j (this call).  The column maximum is also a keep rule for
 * reference tokens: a token that at least one query token looks at strongly.  Same args as ir_attn_received (q, the K pointers or
 * the K table, lse; v_*, adain_*, out, valid_refs, seg_mass and workspace are ignored - every reference is walked - and `tuning`
 * must be 0; IR_FLAG_Q_PRESCALED: same rule; IR_FLAG_BATCH_INVARIANT: accepted, inert) plus
 *   reduce     IR_MATCH_PER_HEAD   index int32 (B, H, Lkv), prob fp32 (B, H, Lkv): prob[b,h,j] = max over i = 0 .. len_q - 1 of
 *                                  the fp32 p[b,h,i,j] = exp2(fma(<q_i, k_j>, scale*log2(e), -lse[b,h,i]*log2(e))) - the value
 *                                  ir_attn_probs and ir_attn_rows round to `dtype`
 *              IR_MATCH_HEAD_MEAN  index int32 (B, Lkv), prob fp32 (B, Lkv): the maximum over i of the head mean formed as
 *                                  IR_ROWS_HEAD_MEAN forms it ((sum over heads, ascending, of the fp32 p) * (1.0f / (float)H))
 *   index, prob  contiguous, 4-byte aligned; j on the PACKED extended key axis [self (iff INCLUDE_SELF)] ++ ref 0 ++ ... ++ ref N-1
 *              (the axis of ir_attn_received's recv).  index is the LOWEST query row that attains prob: the order is TOTAL (p
 *              descending, then row ascending).  A column whose probabilities are all 0 gives index 0, prob 0.
 * Bit for bit (part of the interface):
 *   - prob IS the maximum of the fp32 values named above and index its first row.  The order is total, so the result does not
 *     depend on the order in which the rows meet: unlike its siblings, which have to state their summation order, this call has
 *     none to state;
 *   - IR_MATCH_HEAD_MEAN: prob is the column maximum of ir_attn_rows' IR_ROWS_HEAD_MEAN rows (all rows), index the first row of it;
 *   - rows of the padding to a whole 32-row block never take part: they are not compared, index is always in [0, len_q), and
 *     nothing behind row len_q - 1 of q or lse is read; keys past the end of a segment are never written.
 * Bound: K read once per head (head mean: once per 32-row block, from L2); Q and lse once per group of 64 keys; 2 * Lkv numbers
 * written per (head,) batch entry; no workspace, no atomics, one launch; asynchronous and capturable.  One wave walks the whole
 * query axis for its keys, so every output element has one writer; the cut follows len_self, len_ref, n_refs and reduce only.
 * Every offset is formed in 64 bits; the pointer tables are read by the kernel when it runs: a replayed hipGraph follows in-place
 * updates of them.  Any segment length, any len_q.
 * Checked in this order, after the checks of the args block: IR_ERR_INVALID_ARG: NULL index, NULL prob, NULL lse;
 * IR_ERR_UNSUPPORTED: another reduce, a misaligned index / prob, more than 2^31 - 4 work items.  Refused with the args block: a
 * key_bias or ref_lens block (IR_ERR_UNSUPPORTED, as for the other read-outs), tuning != 0.
 */
int ir_attn_key_match(const ir_shared_attn_args* args, int32_t reduce, int32_t* index, float* prob, void* stream);

/*
 * ir_adain_stats - per-(b, n, channel) AdaIN affine from token statistics.
 *
 * Replaces the statistics half of adain() (attn_processors.py:9-10) and of its call site
 * (:244-245): mean and UNBIASED standard deviation over the token axis of the degraded
 * image's V (style) and of every reference V (content), eps = 1e-5 added to both deviations:
 *      a = (std(v_self)+eps) / (std(v_ref_n)+eps),   b = mean(v_self) - mean(v_ref_n) * a
 * so that adain(v_ref_n) == v_ref_n * a + b.  One pass over the data, fp32 Chan/Welford merge.
 *   v_self (B, len_self, H, 64) strides vs_*;  v_ref (B, N, len_ref, H, 64) strides vr_*
 *   a, b : fp32 (B, N, H, 64) contiguous
 *   workspace: >= ir_adain_stats_workspace_bytes(...) bytes of device memory
 */
size_t ir_adain_stats_workspace_bytes(int32_t batch, int32_t heads, int32_t len_self, int32_t n_refs,
                                      int32_t len_ref);
int ir_adain_stats(int32_t dtype, int32_t batch, int32_t heads, int32_t len_self, int32_t n_refs,
                   int32_t len_ref, const void* v_self, int64_t vs_sb, int64_t vs_sl, int64_t vs_sh,
                   const void* v_ref, int64_t vr_sb, int64_t vr_sn, int64_t vr_sl, int64_t vr_sh,
                   float eps, float* a, float* b, void* workspace, size_t workspace_bytes, void* stream);
/*
 * ir_adain_stats_cached - the same affine when the CONTENT statistics are already known.
 *
 * mean(v_ref_n) and std(v_ref_n) of a reference V do not change while the identity's references do not
 * (pix2pix_turbo.py:255-266 recomputes them every frame): the K/V-capture layer emits them once with ir_token_stats
 * (content_mean, content_std: fp32 (B, N, H, 64) contiguous, std WITHOUT the eps) and every frame reads only v_self,
 * 1/(N+1) of the bytes.  Bit-identical (a, b) to ir_adain_stats on the same tensors: both run the same partial kernel
 * and the same merge order.  A reference zero-filled by ir_zero_invalid_refs has statistics (0, 0): the caller zeroes
 * its cached entries (instantrestore_amd/kv_harvest.py does).
 *   workspace: >= ir_adain_stats_workspace_bytes(batch, heads, len_self, 0, len_self)
 */
int ir_adain_stats_cached(int32_t dtype, int32_t batch, int32_t heads, int32_t len_self, int32_t n_refs,
                          const void* v_self, int64_t vs_sb, int64_t vs_sl, int64_t vs_sh,
                          const float* content_mean, const float* content_std,
                          float eps, float* a, float* b, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ir_token_stats - mean and UNBIASED standard deviation over the token axis.
 *
 * The content-statistics lines of adain() on their own (attn_processors.py:9-10, without the
 * +1e-5): used by the exported adain(content, style_mean, style_std), whose style statistics
 * arrive precomputed.   x (B, M, len, H, 64) strides x_*;  mean, std: fp32 (B, M, H, 64).
 * workspace >= ir_adain_stats_workspace_bytes(batch, heads, len, n_mats - 1, len).
 */
int ir_token_stats(int32_t dtype, int32_t batch, int32_t heads, int32_t n_mats, int32_t len,
                   const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                   float* mean, float* std, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ir_token_stats_weighted - ir_token_stats over WEIGHTED or COUNTED tokens (mask-aware AdaIN statistics).
 *
 * Per (b, m, head, channel), with the effective weight of token t   w_t = (t < c[b,m]) ? w[b,m,t] : 0:
 *      W = sum w_t,   W2 = sum w_t^2,   mean = sum w_t x_t / W,   M2 = sum w_t (x_t - mean)^2,   std = sqrt(M2 / (W - W2 / W))
 * - the unbiased estimator under reliability weights.  For 0/1 weights the divisor is count - 1: mean(dim=1) / std(dim=1)
 * (attn_processors.py:9-10) over the kept tokens alone.
 *   x (B, M, len, H, 64) strides x_* (the 16-byte rule of ir_token_stats);  mean, std: fp32 (B, M, H, 64), std WITHOUT eps
 *   weights: fp32, w[b,m,t] = weights[b * w_sb + m * w_sn + t] >= 0 (w_sb = 0: one set shared by the batch), or NULL (= 1).
 *            Negative, NaN or Inf weights: undefined.
 *   lens:    int32, c[b,m] = clamp(lens[b * ln_sb + m], 0, len), or NULL (= len)
 *   wsum:    optional fp32 (B, M): W, the effective token count; NULL = off
 *   workspace >= ir_token_stats_weighted_workspace_bytes(batch, heads, n_mats, len)  (chunks x heads x matrices; > 0 for len >= 1)
 * Zero-weight tokens: a token with w_t == 0 contributes nothing whatever its bytes, NaN and Inf included - it is selected
 * away, never multiplied by 0; rows at or behind a count are never used; nothing outside the `len` floats of a weights row or the
 * n_mats ints of a lens row is read.
 * Never NaN: W == 0 gives mean 0, std 0 (the statistics of a zero-filled reference); W - W2 / W <= 0 (one effective token)
 * gives that token's value as the mean and std 0 (so len == 1 gives (x, 0) where ir_token_stats gives NaN).
 * Bit for bit: for 2 <= len < 2^24, weights == NULL && lens == NULL, weights of all 1.0f, and lens == len each produce the bytes
 * of ir_token_stats on the same tensor (same row slots, same shifted sums, same Chan merge over ascending 256-row chunks).
 * Order: the order of evaluation is a function of len only - a (b, m) result does not depend on the batch, its position, its
 * neighbours, the grid or the stream.  No atomics, one writer per output, two launches, asynchronous and capturable; weights
 * and lens are read when the kernel RUNS: a replayed hipGraph follows in-place updates of them.
 * Checked in this order, before any launch, no device pointer dereferenced: IR_ERR_UNSUPPORTED: dtype; IR_ERR_INVALID_ARG:
 * a size <= 0, NULL x, NULL mean, NULL std, NULL workspace; IR_ERR_UNSUPPORTED: x not 16-byte aligned or an x stride that is
 * negative or no multiple of 8; IR_ERR_INVALID_ARG (with weights): w_sn < len, w_sb < 0; (with lens): ln_sb < n_mats;
 * IR_ERR_UNSUPPORTED: weights, lens, mean, std, wsum not 4-byte aligned, batch * n_mats or heads > 65535; IR_ERR_WORKSPACE: a
 * workspace that is too small.
 */
size_t ir_token_stats_weighted_workspace_bytes(int32_t batch, int32_t heads, int32_t n_mats, int32_t len);
int ir_token_stats_weighted(int32_t dtype, int32_t batch, int32_t heads, int32_t n_mats, int32_t len,
                            const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                            const float* weights, int64_t w_sb, int64_t w_sn, const int32_t* lens, int64_t ln_sb,
                            float* mean, float* std, float* wsum, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ir_adain_affine_from_stats - the AdaIN affine from FINISHED statistics (whoever made them, with whatever weights).
 *
 *   style_mean, style_std: fp32 (B, H, 64);  content_mean, content_std: fp32 (B, N, H, 64);  a, b: fp32 (B, N, H, 64); std WITHOUT eps
 *      sd_v = style_std + eps,   a = sd_v / (content_std + eps),   b = style_mean - content_mean * a
 * with the constant-content rule of the other AdaIN entry points (content_std == 0: a = 2^-24 sd_v).  The expression of
 * ir_adain_stats_cached: ir_token_stats(v_self) followed by this call gives its (a, b) bit for bit.  One launch, asynchronous,
 * capturable.  IR_ERR_INVALID_ARG: a size <= 0, a NULL pointer; IR_ERR_UNSUPPORTED: a pointer that is not 4-byte aligned.
 */
int ir_adain_affine_from_stats(int32_t batch, int32_t heads, int32_t n_refs,
                               const float* style_mean, const float* style_std, const float* content_mean, const float* content_std,
                               float eps, float* a, float* b, void* stream);

/*
 * ir_adain_apply - standalone AdaIN application  y = x * a + b  (fp32 math, stored in dtype).
 *
 * Replaces the normalise/scale/shift half of adain() (attn_processors.py:12-16) for callers
 * that need the renormalised V materialised (op-level parity, the exported adain()).  The fused
 * attention folds the same affine into its V staging and never writes this tensor.
 *   x, y (B, N, len, H, 64) with strides x_* / y_*;  a, b fp32 (B, N, H, 64) contiguous
 */
int ir_adain_apply(int32_t dtype, int32_t batch, int32_t heads, int32_t n_refs, int32_t len,
                   const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                   const float* a, const float* b,
                   void* y, int64_t y_sb, int64_t y_sn, int64_t y_sl, int64_t y_sh, void* stream);

/*
 * ir_token_stats_labelled - ir_token_stats per REGION label, every region in one pass over x (per-region AdaIN statistics).
 *
 * Token t of matrix (b, m) carries the label  l = labels[b * lb_sb + m * lb_sn + t].  Per (b, region r, m, head, channel) the
 * outputs are the mean and the UNBIASED std over the tokens with l == r: mean(dim=1) / std(dim=1) (attn_processors.py:9-10)
 * over x[:, labels == r] - what ir_token_stats_weighted gives with the weights (l == r), for every r < n_regions, while x is
 * read once.
 *   x (B, M, len, H, 64) strides x_* (the 16-byte rule of ir_token_stats)
 *   labels: int32; lb_sb = 0 shares one set across the batch; lb_sn >= len
 *   n_regions: 1 ... IR_ADAIN_REGIONS_MAX (the range of IR_REGION_MAX: one parsing map serves the region masks and these)
 *   mean, std: fp32 (B, n_regions, M, H, 64) contiguous, std WITHOUT eps.  Region-major: (B * n_regions) is then the batch of
 *              ir_adain_affine_from_stats as it stands
 *   count:   optional fp32 (B, n_regions, M): the tokens of the region, an exact integer; NULL = off
 *   workspace >= ir_token_stats_labelled_workspace_bytes(batch, heads, n_mats, len, n_regions)
 * A token whose label lies outside [0, n_regions) belongs to no region: it is selected away whatever its bytes, NaN and Inf
 * included.  Nothing outside the `len` rows of x and the `len` ints of a label row is read.
 * Never NaN: a region with no token gives mean 0, std 0, count 0; a region with one token gives (x, 0), count 1.
 * Bit for bit: for every r the outputs are the bytes of ir_token_stats_weighted on the same x with the fp32 weights (l == r)
 * (same row slots, same shifted sums, same Chan merge over the row slots and over ascending 256-row chunks; count == its wsum).
 * Order: the order of evaluation is a function of len and n_regions only - a (b, m) result does not depend on the batch, its
 * position, its neighbours, the grid or the stream.  No atomics, one writer per output, two launches, asynchronous and
 * capturable; labels are read when the kernel RUNS: a replayed hipGraph follows in-place updates of them.
 * Checked in this order, before any launch, no device pointer dereferenced: IR_ERR_UNSUPPORTED: dtype; IR_ERR_INVALID_ARG:
 * a size <= 0, n_regions outside [1, IR_ADAIN_REGIONS_MAX], NULL x, NULL labels, NULL mean, NULL std, NULL workspace;
 * IR_ERR_UNSUPPORTED: x not 16-byte aligned or an x stride that is negative or no multiple of 8; IR_ERR_INVALID_ARG:
 * lb_sn < len, lb_sb < 0; IR_ERR_UNSUPPORTED: labels, mean, std, count not 4-byte aligned, batch * n_mats or heads > 65535 (or
 * batch * n_mats * n_regions * heads >= 2^31); IR_ERR_WORKSPACE: a workspace that is too small.
 */
#define IR_ADAIN_REGIONS_MAX 32
size_t ir_token_stats_labelled_workspace_bytes(int32_t batch, int32_t heads, int32_t n_mats, int32_t len, int32_t n_regions);
int ir_token_stats_labelled(int32_t dtype, int32_t batch, int32_t heads, int32_t n_mats, int32_t len, int32_t n_regions,
                           const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                           const int32_t* labels, int64_t lb_sb, int64_t lb_sn,
                           float* mean, float* std, float* count, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ir_adain_apply_labelled - ir_adain_apply with the affine chosen PER TOKEN by its region label.
 *
 *   y[b,n,t,h,:] = fma(x[b,n,t,h,:], a[b,n,s,h,:], b[b,n,s,h,:]),   s = (unsigned)label[b,n,t] < n_regions ? label[b,n,t] : n_regions
 * fp32 math, one rounding to dtype: the expression of ir_adain_apply, so a token of region r gets the bytes ir_adain_apply gives
 * it with slot r's affine.
 *   x, y (B, N, len, H, 64) with strides x_* / y_* (16-byte aligned, strides non-negative multiples of 8); y may be a view into
 *        a wider buffer: only the 64-element head rows of y are written
 *   a, b: fp32 (B, N, n_regions + 1, H, 64) contiguous; the LAST slot is the affine of the tokens without a region
 *   labels: int32, label[b,n,t] = labels[b * lb_sb + n * lb_sn + t]  (lb_sb = 0: shared by the batch; lb_sn >= len), read when
 *        the kernel RUNS, once per token and group of four heads (shared by the 8 sixteen-byte pieces of each of its head rows)
 * y == x with identical strides (in place) is allowed: every 16-byte piece is read and then written by one thread.  Any other
 * overlap of x and y is undefined.  One launch, asynchronous, capturable, batch-invariant.
 * Checked in this order, before any launch: IR_ERR_UNSUPPORTED: dtype; IR_ERR_INVALID_ARG: a size <= 0, n_regions outside
 * [1, IR_ADAIN_REGIONS_MAX], NULL x, NULL y, NULL a / b, NULL labels; IR_ERR_UNSUPPORTED: x / y not 16-byte aligned, a stride
 * that is negative or no multiple of 8; IR_ERR_INVALID_ARG: lb_sn < len, lb_sb < 0; IR_ERR_UNSUPPORTED: labels, a, b not
 * 4-byte aligned.
 */
int ir_adain_apply_labelled(int32_t dtype, int32_t batch, int32_t heads, int32_t n_refs, int32_t len, int32_t n_regions,
                           const void* x, int64_t x_sb, int64_t x_sn, int64_t x_sl, int64_t x_sh,
                           const int32_t* labels, int64_t lb_sb, int64_t lb_sn, const float* a, const float* b,
                           void* y, int64_t y_sb, int64_t y_sn, int64_t y_sl, int64_t y_sh, void* stream);

/*
 * ir_zero_invalid_refs - zero the K and V of references n >= valid[b] in place.
 *
 * Replaces the Python double loop of Pix2Pix_Turbo.get_conditioning_keys_values
 * (face_replace/models/pix2pix_turbo.py:269-273).  Zeroed, not masked: the tokens keep their
 * exp(0) softmax weight, exactly like the reference.  valid: int32 (B) on the device.
 *   k, v (B, N, len, H*64) described as (B, N, len, H, 64) with strides *_sb,_sn,_sl,_sh
 */
int ir_zero_invalid_refs(int32_t batch, int32_t heads, int32_t n_refs, int32_t len, const int32_t* valid,
                         void* k, int64_t k_sb, int64_t k_sn, int64_t k_sl, int64_t k_sh,
                         void* v, int64_t v_sb, int64_t v_sn, int64_t v_sl, int64_t v_sh, void* stream);

/*
 * ir_compact_ref_tokens - pack the kept tokens of every reference to the front of its segment (stable stream compaction).
 *
 * For every (b, n): the rows t of k_in / v_in with keep[b, n, t] != 0 are copied, in their order, to rows 0 .. c-1 of k_out / v_out,
 * and ref_lens[b * rl_sb + n] = c - the counts a call with ir_shared_attn_ragged_args then walks instead of a masked full reference.
 * Rows of the outputs behind the count are NOT written.  keep: uint8 (B, N, len_ref) contiguous on the device.
 *   k_in, v_in, k_out, v_out (B, N, len_ref, H, 64) with strides *_sb, *_sn, *_sl, *_sh (elements, multiples of 8; 16-byte aligned
 *   bases); the byte span of each output (base to the last element its strides reach) must not overlap the span of an input or of
 *   the other output (aliasing, at any offset, is IR_ERR_INVALID_ARG).
 * One launch, no host synchronisation, no atomics, deterministic, capturable; runs once per identity.
 */
int ir_compact_ref_tokens(int32_t dtype, int32_t batch, int32_t heads, int32_t n_refs, int32_t len_ref,
                          const void* k_in, int64_t ki_sb, int64_t ki_sn, int64_t ki_sl, int64_t ki_sh,
                          const void* v_in, int64_t vi_sb, int64_t vi_sn, int64_t vi_sl, int64_t vi_sh,
                          const uint8_t* keep,
                          void* k_out, int64_t ko_sb, int64_t ko_sn, int64_t ko_sl, int64_t ko_sh,
                          void* v_out, int64_t vo_sb, int64_t vo_sn, int64_t vo_sl, int64_t vo_sh,
                          int32_t* ref_lens, int64_t rl_sb, void* stream);

/*
 * ir_tensor2im_u8 - the caller's output path on the device.
 *
 * Replaces tensor2im(var, unnorm=True) (face_replace/training/utils/vis_utils.py:14-23, called at
 * face_replace/inference/test.py:139): x*0.5+0.5 in the tensor's dtype, clamp [0,1], *255 in that
 * dtype, truncation to uint8, CHW -> HWC.  Bit-identical bytes; only H*W*C bytes cross PCIe.
 *   x (B, C, H, W) strides x_sb, x_sc, x_sh, x_sw (elements); dtype 0 = fp16, 1 = bf16, 2 = fp32
 *   out_u8 (B, H, W, C) contiguous uint8
 */
int ir_tensor2im_u8(int32_t dtype, int32_t batch, int32_t channels, int32_t height, int32_t width, const void* x,
                    int64_t x_sb, int64_t x_sc, int64_t x_sh, int64_t x_sw, void* out_u8, void* stream);

/*
 * ir_preprocess_lanczos_u8 - the caller's input transform on the device.
 *
 * Replaces, for a batch of differently sized RGB images, the per-image CPU pipeline of
 * face_replace/inference/test.py:54-59 (applied at :76, :127, :150):
 *     Resize(size, LANCZOS) -> CenterCrop(size) -> ToTensor() -> Normalize(0.5, 0.5)
 * i.e. Pillow's 8-bit two-pass resampler (pillow==10.4.0 Resample.c; horizontal pass rounded to
 * uint8, then vertical, 22-bit fixed-point taps) and (v/255 - 0.5)/0.5 in float32, cast to
 * out_dtype.  The resampled bytes are bit-identical to Pillow's; only the crop is computed.
 *
 * The tap tables are Pillow's precompute_coeffs + normalize_coeffs_8bpc, produced on the HOST by
 * ir_lanczos_ksize / ir_lanczos_coeffs (no GPU involved; same libm and operation order) and uploaded
 * by the caller once per (in_size, out_size); out sizes and crop offsets follow torchvision 0.15.2
 * (instantrestore_amd/preprocess.py).
 *   images: HOST array of n descriptors; every pointer inside is a DEVICE pointer
 *   out   : (n, 3, size, size) contiguous, dtype 0 = fp16, 1 = bf16, 2 = fp32
 */
typedef struct ir_image_desc {
  const void* src;          /* (in_h, in_w, 3) uint8, rows src_row_bytes apart */
  int64_t src_row_bytes;
  int32_t in_h, in_w;
  int32_t out_h, out_w;     /* resized size (before the crop) */
  int32_t crop_top, crop_left;
  const int32_t* bounds_h;  /* (out_w, 2) */
  const int32_t* kk_h;      /* (ksize_h, out_w): TAP-MAJOR, the transpose of ir_lanczos_coeffs' table */
  const int32_t* bounds_v;  /* (out_h, 2) */
  const int32_t* kk_v;      /* (out_h, ksize_v) */
  int32_t ksize_h, ksize_v;
  int32_t row_first, row_count; /* source rows touched by the vertical taps of the crop's rows */
  int32_t col_first, col_count; /* source columns touched by the horizontal taps of the crop's columns */
  void* tmp;                /* 4-byte aligned scratch, >= row_count * ((size*3 + 3) & ~3) bytes */
} ir_image_desc;

int ir_lanczos_ksize(int32_t in_size, int32_t out_size);            /* taps per output sample; < 0 on error */
int ir_lanczos_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds /* host (out,2) */,
                      int32_t* kk /* host (out, ksize) */);
int ir_preprocess_lanczos_u8(const ir_image_desc* images, int32_t n_images, int32_t size, int32_t out_dtype,
                             void* out, void* stream);

/*
 * ir_freeu_fourier_filter - FreeU's skip-feature filter.
 *
 * Replaces fourier_filter(res_hidden_states.float(), threshold, scale).to(dtype)
 * (face_replace/models/unet_2d_condition/block.py:3514,3518 -> diffusers==0.24.0
 * utils/torch_utils.py): fftn -> fftshift -> multiply the (2*threshold)^2 centre bins by `scale`
 * -> ifftshift -> ifftn -> real.  Computed in closed form (only those bins change): one read of x,
 * one write of out, fp32 arithmetic, no intermediate tensors.  In place (out == x) is allowed.
 *   x, out: `planes` = B*C planes of height*width contiguous elements, plane strides in elements
 *   dtype 0 = fp16, 1 = bf16, 2 = fp32; height*width <= 4096; 1 <= threshold <= min(H,W)/2
 */
int ir_freeu_fourier_filter(int32_t dtype, int64_t planes, int32_t height, int32_t width, const void* x,
                            int64_t x_plane_stride, void* out, int64_t out_plane_stride, int32_t threshold,
                            float scale, void* stream);

/*
 * ir_linear_fwd - y = x W^T (+ bias): the q/k/v (fused, N = 3C) and out projections of every layer class
 * (SURVEY.md section 8f rank 4).
 *
 * Replaces attn.to_q/to_k/to_v and attn.to_out[0] (nn.Linear; attn_processors.py:222-230,267).  Two kernel families,
 * both fp32 accumulation with ONE rounding to the 16-bit dtype (bias added in fp32 before it), both deterministic
 * (no atomics, no split-K reduction through memory):
 *   - X-stationary (K in {64, 128, ..., 320}, and K = 640 with the contraction split over two waves whose fp32
 *     partial tiles meet in LDS): X is read once and kept in registers, W streams through LDS; N % 32 == 0,
 *     N <= 4096 with bias.  Chosen for large M (M >= 65536 rows).
 *   - LDS-tiled (any K % 64 == 0, N % 64 == 0): 256x256 ... 64x128 tiles of Y, both operands through swizzled LDS
 *     stages; K = 1280 and the small-M shapes of every class.
 * Other shapes return IR_ERR_UNSUPPORTED.
 *   x (M, K) rows x_ld elements apart; w (N, K) rows w_ld apart (torch Linear weight layout);
 *   bias (N) or NULL; y (M, N) rows y_ld apart; all ld % 8 == 0, pointers 16-B aligned
 */
int ir_linear_fwd(int32_t dtype, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                  int64_t w_ld, const void* bias, void* y, int64_t y_ld, void* stream);
/* The same with (a) output columns [0, scale_cols) multiplied by col_scale in the fp32 accumulator, before the one rounding
 * (y = acc * col_scale + bias there): the fused q/k/v projection hands the attention kernel Q * scale * log2(e)
 * (IR_FLAG_Q_PRESCALED) at no extra rounding; scale_cols % 32 == 0; (b) x_is_f32 != 0: x is fp32 (x_ld in fp32
 * elements) and is rounded to `dtype` while it is loaded - the `.to(fp16)` the reference's autocast performs on the
 * LayerNorm output ahead of every projection (inference/test.py:83), without its pass over memory. */
int ir_linear_fwd_scaled(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                         int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                         void* stream);
/* The same with the kernel named by the caller (benchmarks, A/B, tests of every tile shape): */
#define IR_LIN_AUTO 0           /* what ir_linear_fwd / ir_linear_fwd_scaled pick (ir_linear_kernel_for) */
#define IR_LIN_X_STATIONARY 1
#define IR_LIN_TILED_FIRST 2    /* 2: 256x128, 3: 128x128, 4: 128x64, 5: 256x64, 6: 64x128, 7: 128x256, 8: 256x256 (rows x columns of Y per
                                   workgroup; 7 and 8 with 64 x 128 per wave), 9: 128x128 with the contraction split over two wave
                                   groups of the workgroup (K / 64 even; partial sums meet in LDS in a fixed order: deterministic, but
                                   not the same fp32 rounding as the single-pass tiles) */
#define IR_LIN_BATCH_INVARIANT 16 /* ABI v10: ONE kernel per (N, K, bias) for every M, never a split of the contraction - row r of y
                                     depends on row r of x, on w and on the bias only, whatever the number of rows (batch-invariant
                                     mode): the 256x256 tile where N % 64 == 0 and K % 64 == 0, the X-stationary kernel elsewhere */
int ir_linear_fwd_ex(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                     int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                     int32_t kernel, void* stream);
/* kernel id (IR_LIN_*) the automatic choice makes for a shape, or -1 when no kernel covers it */
int ir_linear_kernel_for(int64_t m, int32_t n, int32_t k, int32_t has_bias);
/* ABI v10: the kernel a selector (IR_LIN_AUTO or IR_LIN_BATCH_INVARIANT) resolves to for a shape, or -1 */
int ir_linear_kernel_for_ex(int64_t m, int32_t n, int32_t k, int32_t has_bias, int32_t selector);

/*
 * ir_linear_fwd_stats - ir_linear_fwd_scaled that ALSO leaves the token statistics of output columns
 * [stats_col0, stats_col0 + stats_cols) behind: the AdaIN statistics pass (attn_processors.py:9-10, :244-245) fused into
 * the projection that produces V (ABI 6, round 4).
 *
 * The workgroup that has stored a (rows x 64-column) block of those columns re-reads it from its L2 and writes the block's
 * partial statistics - mean[64] | M2[64], fp32, of the ROUNDED 16-bit outputs, the values the attention kernel will read -
 * to stats_ws[(row_block * (stats_cols / 64) + head) * 128 ...], row blocks of ir_linear_stats_rows(m, n, k, has_bias)
 * rows in row order.  For the V third of a fused q/k/v projection (stats_col0 = 2C, stats_cols = C) over token sets of
 * L rows each (L % rows == 0) the partials of set s are blocks [s L / rows, (s + 1) L / rows): what
 * ir_adain_affine_from_partials / ir_token_stats_from_partials merge.  Same arithmetic as ir_adain_stats' own partial pass
 * (shifted single-pass sums, Chan merge); no pass over V, no extra launch.
 *   stats_col0, stats_cols, n: multiples of 64; m % rows == 0, rows = ir_linear_stats_rows(...) > 0 (0: this shape's kernel
 *   cannot emit them - use ir_adain_stats / ir_token_stats);  stats_ws: >= (m / rows) * (stats_cols / 64) * 512 bytes
 */
int ir_linear_stats_rows(int64_t m, int32_t n, int32_t k, int32_t has_bias);
int ir_linear_fwd_stats(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                        int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                        int32_t stats_col0, int32_t stats_cols, float* stats_ws, size_t stats_ws_bytes, void* stream);
/* ABI v10: the same with a kernel selector - IR_LIN_AUTO (= ir_linear_fwd_stats) or IR_LIN_BATCH_INVARIANT; every kernel's
 * statistics blocks are 64 rows of one wave, so a block's partials depend on its own rows only */
int ir_linear_fwd_stats_ex(int32_t dtype, int32_t x_is_f32, int64_t m, int32_t n, int32_t k, const void* x, int64_t x_ld, const void* w,
                           int64_t w_ld, const void* bias, void* y, int64_t y_ld, int32_t scale_cols, float col_scale,
                           int32_t stats_col0, int32_t stats_cols, float* stats_ws, size_t stats_ws_bytes, int32_t kernel, void* stream);
/*
 * ir_adain_affine_from_partials - the (a, b) of ir_adain_stats from those partials: one small launch per shared layer.
 *   style_ws: partials of V_self from the shared layer's own q/k/v projection (B sets of len_self rows, style_rows per block);
 *   content: EITHER content_ws / content_rows - partials of the reference V's from the K/V-capture layer's projection
 *   (B * N sets of len_ref rows, set index b * N + n) - OR content_mean / content_std, fp32 (B, N, H, 64), std without eps
 *   (ir_token_stats_from_partials, ir_token_stats: a per-identity cache); valid: optional int32 (B) on the device -
 *   references n >= valid[b] were zero-filled (ir_zero_invalid_refs) and count with statistics (0, 0).
 */
int ir_adain_affine_from_partials(int32_t batch, int32_t heads, int32_t n_refs, int32_t len_self, int32_t len_ref,
                                  const float* style_ws, int32_t style_rows, const float* content_ws, int32_t content_rows,
                                  const float* content_mean, const float* content_std, const int32_t* valid, float eps,
                                  float* a, float* b, void* stream);
/* mean and unbiased std (no eps) of n_sets matrices of `len` rows from their partials: fp32 (n_sets, H, 64) each.
 * Batch invariance (ABI v10): this merge, ir_adain_affine_from_partials, ir_token_stats and ir_adain_stats[_cached] pick their
 * kernels from per-set sizes (token counts, rows per block, N, H) and merge every set's partials in a fixed order inside one
 * workgroup: the statistics of a set never depend on how many other sets share the call. */
int ir_token_stats_from_partials(int32_t n_sets, int32_t heads, int32_t len, const float* ws, int32_t rows, float* mean, float* std,
                                 void* stream);

/* library identity / diagnostics */
int ir_abi_version(void);                  /* == IR_ABI_VERSION */
const char* ir_build_info(void);           /* "gfx950 hipcc ... <date>" */
const char* ir_last_error_string(void);    /* thread-local, never NULL */

/*
 * ir_time_shared_attn_fwd - launch ir_shared_attn_fwd `iters` times on `stream` bracketed by
 * HIP events recorded on that same stream and return the average milliseconds per launch in
 * *ms_per_launch (bench.py's live roofline measurement; synchronises the stream).
 */
int ir_time_shared_attn_fwd(const ir_shared_attn_args* args, int32_t iters, void* stream, float* ms_per_launch);

/*
 * ir_bench_mfma_stream (ABI v7) - what the matrix pipe SUSTAINS on this device: `launches` back-to-back launches of an
 * MFMA-only stream of the attention kernels' instruction (v_mfma_f32_32x32x16 of `dtype`; two waves per SIMD on every CU,
 * iters x 16 MFMAs per wave, pseudo-random operands or - zero_operands != 0 - all zeros), bracketed by HIP events on
 * `stream`; returns the TFLOP/s of the bracketed launches in *tflops (synchronises the stream).  `scratch`: device memory,
 * >= ir_bench_mfma_stream_scratch_bytes().  Give it >= 0.1 s in all (e.g. iters 40000, launches 5) so that the board's
 * power controller settles: on random operands the 1400 W cap, not the 2.4 GHz of the datasheet peak, sets the result
 * (bench.py `roofline.at_power_cap`).  No reference counterpart: measurement only.
 */
size_t ir_bench_mfma_stream_scratch_bytes(void);
int ir_bench_mfma_stream(int32_t dtype, int32_t zero_operands, int32_t iters, int32_t launches, void* scratch, size_t scratch_bytes,
                         void* stream, float* tflops);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTRESTORE_HIP_H */
