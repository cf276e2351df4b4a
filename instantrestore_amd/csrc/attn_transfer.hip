// attn_transfer.hip - attention-weighted sums of a per-key payload for a caller-chosen set of query tokens: per K/V segment,
// sum_j p[b,h,r,j] * y[b,j,:] and the segment's mass sum_j p[b,h,r,j], without the (B, H, Lq, Lkv) dump (gfx950).
//
// "Where in each reference does this token of the degraded face look, to a fraction of a token" (y = the (y, x) of every key),
// "what does the reference look like through the attention" (y = its pixels pooled to the token grid) and "which label does
// the token inherit" (y = a parsing map) are all einsum('bhij,bjc->bhic') over the columns of one segment.  The dump is 6.7 GB
// at cfg 2's top shared layer and cannot be formed at the 1024-px layer; ir_attn_rows reaches all rows only by writing every
// one of them.  This kernel issues the contraction of the dump kernels and keeps channels + 1 running sums per row:
//
//   p[b,h,r,j] = exp2(fma(<q[b, idx[b,r], h, :], k_seg[b, j, h, :]>, scale*log2(e), -lse[b,h,idx[b,r]]*log2(e)))
//
// the expression and the contraction of ir_readout.h, which attn_probs.hip, attn_rows.hip and attn_match.hip share.
//
//   IR_TRANSFER_PER_HEAD   sums fp32 (B, H, R, S, C), mass fp32 (B, H, R, S)
//   IR_TRANSFER_HEAD_MEAN  sums fp32 (B, R, S, C),    mass fp32 (B, R, S): ((S_0 + S_1) + ... + S_{H-1}) * (1/H) of the per-head
//                                                     outputs S_h, bit for bit
//
// The summation contract (the tests hold it with torch.equal):
//   * the mass and every channel of a (row, segment, head) are accumulated over the SAME keys in the SAME order, one fp32 fused
//     multiply-add per term with the payload value as multiplicand (the mass: multiplicand 1.0f).  A lane holds 16 consecutive
//     keys of a row per 32-key block (the layout of ir_readout.h); it adds them in ascending order, block after block, and the
//     two half-waves - keys 0-15 and 16-31 of every block - meet once at the end of the walk: lower half + upper half.
//     So a channel that is 1.0f on every key IS the mass, and a channel that is 1 at one key and 0 elsewhere IS that key's
//     fp32 prob(): adding exact zeros changes nothing, whatever the order;
//   * the head-mean form walks the heads in ascending order, forms each head's sums exactly as the per-head form does (half-wave
//     combine included), adds them into a running total and multiplies by 1.0f / (float)H once at the end.  Only NQ * (C + 1)
//     totals live across heads; Q is gathered again per head;
//   * an index outside [0, len_q) reads row 0 of q and lse (always a valid address) and writes sums 0, mass 0; rows of the padding
//     to 32 are not written.  Keys past the end of a segment are clamped to its last key as addresses by load_k; their
//     probabilities are replaced by 0 before anything is added (a clamped key would count the last key twice), and their
//     payload is staged as 0 without being read.  Whole blocks skip the replacement on a wave-uniform branch.
// Shape of the work, as in attn_match.hip: a wave owns one segment and up to 96 rows (NQ <= 3 blocks of 32; more rows are
// further row groups) and walks the WHOLE segment: every output element has one writer and one order.  Items are (row group,
// segment, head in the per-head form, batch entry), four to a workgroup whose waves never exchange data: no barrier, no
// atomics, no workspace.  The cut follows len_self, len_ref, n_refs, R, channels and the form only: batch invariant by construction.
// The payload: the 32 lanes of a half-wave need the same 16 x C floats per block.  The wave reads the block's 32 x C floats
// once, one or a few dwords per lane (64-bit offsets, any row stride; the next block's are in flight during this block's
// arithmetic), stages them in 1 KB of wave-private LDS (ir_wave_lds_fence, no barrier) and every lane reads its half's keys
// back as broadcast 8- / 16-byte pieces.  C is padded to CH = 2 / 4 / 8 registers; channels past C are never read or written.
#include "ir_readout.h"

namespace {
using namespace ir_readout;

constexpr int RW = 4;   // waves per workgroup (independent of each other: one item each)

struct TransferPlan {
  const int32_t* idx;    // (B, R) on the device
  const float* payload;  // y[b, j, c] = payload[b * pay_sb + j * pay_sj + c], j on the packed extended key axis
  int64_t pay_sb, pay_sj;
  float* sums;
  float* mass;           // or nullptr
  int channels;
  int R;        // rows per batch entry
  int ngroups;  // row groups of 32 * NQ rows
  int nseg;     // include_self + N
  int items;    // ngroups * nseg * (H in the per-head form) * B
  float inv_h;  // 1 / H
};

typedef f32x2 __attribute__((may_alias)) f32x2_alias;

// this lane's share of the 32 x CH payload floats of the block that starts at key j of the segment: float f = lane + 64 i is
// channel f % CH of key f / CH.  Keys past the segment and channels past `channels` are 0 and are not read
template <int CH>
static __device__ __forceinline__ void load_payload(const float* pseg, int64_t pay_sj, int channels, int j, int len, int lane, float (&pv)[CH / 2]) {
  const __attribute__((address_space(1))) float* gseg = (const __attribute__((address_space(1))) float*)pseg;   // device memory: global loads, not flat ones
#pragma unroll
  for (int i = 0; i < CH / 2; ++i) {
    const int f = lane + 64 * i, key = j + f / CH, c = f % CH;
    pv[i] = (key < len && c < channels) ? gseg[(int64_t)key * pay_sj + c] : 0.f;
  }
}

// the CH payload values of key `k` (0..31) of the staged block, in channel pairs
template <int CH>
static __device__ __forceinline__ void read_payload(const float* stage, int k, f32x2 (&y)[CH / 2]) {
  if constexpr (CH == 2) {
    y[0] = *(const f32x2_alias*)(stage + k * 2);
  } else {
#pragma unroll
    for (int c4 = 0; c4 < CH / 4; ++c4) {
      const f32x4 v = *(const f32x4_alias*)(stage + k * CH + 4 * c4);
      y[2 * c4] = f32x2{v[0], v[1]};
      y[2 * c4 + 1] = f32x2{v[2], v[3]};
    }
  }
}

// The sums of head h over the whole segment for this lane's NQ rows, both half-waves combined: a[qi][c] for c < CH, the mass in
// a[qi][CH].  `pseg`: the payload of key 0 of the segment; `stage`: the wave's 32 * CH floats of LDS
template <typename T, int NQ, int CH>
static __device__ __forceinline__ void head_sums(const AttnKParams& p, const TransferPlan& pl, const KeySeg<T>& ks, const float* pseg, int b, int h,
                                                 const int (&qrow)[NQ], float* stage, float (&a)[NQ][CH + 1]) {
  using v8 = typename ElemTraits<T>::v8;
  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5, lq = lane & 31;
  const int len = ks.len;
  const int km = keymap(lq);
  f32x2 a2[NQ][CH / 2];   // channels 2 c2, 2 c2 + 1 of row qi: one fused multiply-add per term and element, issued in pairs
  float m[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
    for (int c2 = 0; c2 < CH / 2; ++c2) a2[qi][c2] = f32x2{0.f, 0.f};
    m[qi] = 0.f;
  }

  v8 qf[NQ][4];
  float lse2[NQ];
  load_q<T, NQ>(p, b, h, hi, qrow, qf, lse2);
  v8 kf[4];
  load_k(ks, h, km, hi, kf);
  float pv[CH / 2];
  load_payload<CH>(pseg, pl.pay_sj, pl.channels, 0, len, lane, pv);
  for (int j = 0; j < len; j += 32) {
    // the reads of the last block are behind us (a wave's LDS operations execute in order): stage this block's payload
    ir_wave_lds_fence();
#pragma unroll
    for (int i = 0; i < CH / 2; ++i) stage[lane + 64 * i] = pv[i];
    ir_wave_lds_fence();
    f32x16 sc[NQ];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) sc[qi] = scores<T>(kf, qf[qi]);
    // the next block's keys and payload arrive while this block's exponentials run (keys clamped: a valid address; payload past
    // the segment: not read)
    load_k(ks, h, j + 32 + km, hi, kf);
    load_payload<CH>(pseg, pl.pay_sj, pl.channels, j + 32, len, lane, pv);
    const int key0 = j + 16 * hi;
    const bool whole = j + 32 <= len;   // wave-uniform: every key of the block exists
    // the probabilities in pairs, as the packed multiply-adds take them: a pair is one 64-bit operand and either half is
    // broadcast by the instruction (a scalar e[t] would take a register pair of its own)
    f32x2 e2[NQ][8];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
      for (int t = 0; t < 16; ++t) e2[qi][t >> 1][t & 1] = prob(sc[qi][t], p.scale_log2, lse2[qi]);
      if (!whole) {
#pragma unroll
        for (int t = 0; t < 16; ++t) e2[qi][t >> 1][t & 1] = key0 + t < len ? e2[qi][t >> 1][t & 1] : 0.f;
      }
    }
    // the staged keys come back GK at a time, the next group in flight during this group's multiply-adds; the fences keep the
    // compiler from hoisting every read of the block to its top (16 * CH registers)
    constexpr int GK = 16 / CH;
    f32x2 y[2][GK][CH / 2];
#pragma unroll
    for (int k = 0; k < GK; ++k) read_payload<CH>(stage, 16 * hi + k, y[0][k]);
#pragma unroll
    for (int g = 0; g < 16 / GK; ++g) {
      if (g + 1 < 16 / GK) {
#pragma unroll
        for (int k = 0; k < GK; ++k) read_payload<CH>(stage, 16 * hi + (g + 1) * GK + k, y[(g + 1) & 1][k]);
      }
      ir_wave_lds_fence();
#pragma unroll
      for (int k = 0; k < GK; ++k) {
        const int t = g * GK + k;
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
          const f32x2 ep = e2[qi][t >> 1];
          const f32x2 es = (t & 1) ? __builtin_shufflevector(ep, ep, 1, 1) : __builtin_shufflevector(ep, ep, 0, 0);
#pragma unroll
          for (int c2 = 0; c2 < CH / 2; ++c2) a2[qi][c2] = __builtin_elementwise_fma(es, y[g & 1][k][c2], a2[qi][c2]);
          m[qi] = __builtin_fmaf(ep[t & 1], 1.0f, m[qi]);
        }
      }
    }
  }
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
    for (int c = 0; c < CH; ++c) a[qi][c] = a2[qi][c >> 1][c & 1];
    a[qi][CH] = m[qi];
  }
  // the two half-waves hold disjoint keys of the same rows: lower half + upper half (both halves arrive at the same sum)
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
    for (int c = 0; c <= CH; ++c) a[qi][c] = a[qi][c] + __shfl_xor(a[qi][c], 32);
}

template <typename T, int NQ, int RED, int CH>
__global__ void __launch_bounds__(RW * 64) attn_transfer_kernel(const AttnKParams p, const TransferPlan pl) {
  __shared__ __attribute__((aligned(16))) float stage_all[RW][32 * CH];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane >> 5, lq = lane & 31;

  // work item of this wave: row group fastest (the waves of a workgroup read the same keys), then segment, then head
  // (per-head form), then batch entry
  int id = blockIdx.x * RW + wid;
  if (id >= pl.items) return;
  const int g0 = id % pl.ngroups;
  id /= pl.ngroups;
  const int seg = id % pl.nseg;
  id /= pl.nseg;
  int h0 = 0;
  if constexpr (RED == kTransferPerHead) { h0 = id % p.H; id /= p.H; }
  const int b = id;

  const KeySeg<T> ks = key_segment<T>(p, b, seg);
  // the segment's first key on the packed extended key axis
  const int col0 = (p.include_self && seg == 0) ? 0 : p.include_self * p.Ls + (seg - p.include_self) * p.Lr;
  const float* pseg = pl.payload + (int64_t)b * pl.pay_sb + (int64_t)col0 * pl.pay_sj;
  float* stage = stage_all[wid];

  int qrow[NQ];
  bool ok[NQ];
  gather_rows<NQ>(pl.idx + (int64_t)b * pl.R, pl.R, p.Lq, g0, lq, qrow, ok);

  float out[NQ][CH + 1];
  if constexpr (RED == kTransferPerHead) {
    head_sums<T, NQ, CH>(p, pl, ks, pseg, b, h0, qrow, stage, out);
  } else {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
      for (int c = 0; c <= CH; ++c) out[qi][c] = 0.f;
    for (int h = 0; h < p.H; ++h) {
      float a[NQ][CH + 1];
      head_sums<T, NQ, CH>(p, pl, ks, pseg, b, h, qrow, stage, a);
#pragma unroll
      for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
        for (int c = 0; c <= CH; ++c) out[qi][c] = out[qi][c] + a[qi][c];
    }
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
      for (int c = 0; c <= CH; ++c) out[qi][c] = out[qi][c] * pl.inv_h;
  }

  const int64_t obase = RED == kTransferPerHead ? ((int64_t)b * p.H + h0) * pl.R : (int64_t)b * pl.R;
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const int r = (g0 * NQ + qi) * 32 + lq;
    if (hi == 0 && r < pl.R) {
      const int64_t o = (obase + r) * pl.nseg + seg;
      float* sp = pl.sums + o * pl.channels;
#pragma unroll
      for (int c = 0; c < CH; ++c)
        if (c < pl.channels) sp[c] = ok[qi] ? out[qi][c] : 0.f;
      if (pl.mass != nullptr) pl.mass[o] = ok[qi] ? out[qi][CH] : 0.f;
    }
  }
}

}  // namespace

int64_t ir_attn_transfer_items(const AttnKParams& p, int n_rows, int reduce) {
  return (int64_t)rows_ngroups(n_rows) * (p.include_self + p.N) * (reduce == kTransferPerHead ? p.H : 1) * p.B;
}

hipError_t ir_launch_attn_transfer(const AttnKParams& p, int dtype, const float* payload, int64_t pay_sb, int64_t pay_sj, int channels,
                                   const int32_t* row_index, int n_rows, int reduce, float* sums, float* mass, hipStream_t s) {
  const int64_t items = ir_attn_transfer_items(p, n_rows, reduce);
  if (items <= 0 || items > kTransferMaxItems) return hipErrorInvalidValue;
  if (channels < 1 || channels > kTransferMaxChannels) return hipErrorInvalidValue;
  TransferPlan pl;
  pl.idx = row_index;
  pl.payload = payload;
  pl.pay_sb = pay_sb;
  pl.pay_sj = pay_sj;
  pl.sums = sums;
  pl.mass = mass;
  pl.channels = channels;
  pl.R = n_rows;
  pl.ngroups = rows_ngroups(n_rows);
  pl.nseg = p.include_self + p.N;
  pl.items = (int)items;
  pl.inv_h = 1.0f / (float)p.H;
  return dispatch_rows(dtype, n_rows, [&](auto t, auto nq) {
    using T = typename decltype(t)::type;
    constexpr int NQ = decltype(nq)::value;
    const dim3 grid((pl.items + RW - 1) / RW), block(RW * 64);
    auto by_ch = [&](auto ch) {
      constexpr int CH = decltype(ch)::value;
      switch (reduce) {
        case kTransferPerHead: hipLaunchKernelGGL((attn_transfer_kernel<T, NQ, kTransferPerHead, CH>), grid, block, 0, s, p, pl); break;
        case kTransferHeadMean: hipLaunchKernelGGL((attn_transfer_kernel<T, NQ, kTransferHeadMean, CH>), grid, block, 0, s, p, pl); break;
        default: return hipErrorInvalidValue;
      }
      return hipGetLastError();
    };
    // the channel count padded to the accumulators a lane keeps: 2, 4 or 8 (+ the mass)
    return channels <= 2 ? by_ch(Int<2>{}) : channels <= 4 ? by_ch(Int<4>{}) : by_ch(Int<8>{});
  });
}
