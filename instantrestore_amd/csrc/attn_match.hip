// attn_match.hip - the best-matching key of every K/V segment for a caller-chosen set of query tokens: the per-segment maximum of
// the attention probabilities and the key that attains it, without the (B, H, Lq, Lkv) dump (gfx950).
//
// "Which token of each reference does this token of the degraded face draw from, and how strongly?" is
// attention_probs[..., segment].max(-1) / .argmax(-1).  The dump is 6.7 GB at cfg 2's top shared layer and cannot be formed at
// the 1024-px layer; ir_attn_rows reaches all rows only by writing every one of them.  This kernel issues the contraction of
// the dump kernels and keeps a running (value, key) pair per row instead of storing anything:
//
//   p[b,h,r,j] = exp2(fma(<q[b, idx[b,r], h, :], k_seg[b, j, h, :]>, scale*log2(e), -lse[b,h,idx[b,r]]*log2(e)))
//
// the expression and the contraction of ir_readout.h, which attn_probs.hip and attn_rows.hip share.
//
//   IR_MATCH_PER_HEAD   index int32 / prob fp32 (B, H, R, S)   prob = max_j p,  index = the lowest j (inside the segment) attaining it
//   IR_MATCH_HEAD_MEAN  index int32 / prob fp32 (B, R, S)      the same of the head mean, formed as IR_ROWS_HEAD_MEAN forms it:
//                                                              the fp32 p summed over the heads in ascending order, then * (1/H)
//
// so prob rounded to the 16-bit format is the maximum of the dump's row segment, and the head-mean prob is the maximum of
// ir_attn_rows' head-mean row segment bit for bit.  Shape of the work:
//   * the lane layout of ir_readout.h: a lane holds 16 CONSECUTIVE keys of ONE gathered row per 32 x 32 block;
//   * a wave owns one segment and up to 96 rows (NQ <= 3 blocks of 32; more rows are further row groups) and walks the WHOLE
//     segment: every output element has one writer and one order, nothing is combined across waves or through memory.  The
//     per-head form keeps the Q fragments of its head in registers for the walk; the head-mean form walks the heads in
//     ascending order over every 128 keys and gathers Q again for each (the sums of 128 keys x 96 rows fill the registers);
//   * the running (value, key) pair of a row lives in the lane that holds the row: the lane takes the maximum of its 16 new
//     values and looks for its position only when it beats the running value (strictly: an equal value later in the walk never
//     replaces an earlier key; inside the 16, the lowest position is taken).  The two half-waves, which hold keys 0-15 and
//     16-31 of every block, meet once at the end: larger value wins, then lower key;
//   * items are (row group, segment, head in the per-head form, batch entry), four to a workgroup whose waves never exchange
//     data: no LDS, no barrier, no atomics, no workspace.  The cut follows len_self, len_ref, n_refs, R and the form only:
//     the call is batch invariant by construction;
//   * an index outside [0, len_q) reads row 0 of q and lse (always a valid address) and gives index -1, prob 0; rows of the
//     padding to 32 are not written.  Duplicated indices are rows like any other.  Keys past the end of a segment are clamped
//     to its last key as addresses and never compared.
#include "ir_readout.h"

namespace {
using namespace ir_readout;

constexpr int RW = 4;   // waves per workgroup (independent of each other: one item each)
constexpr int KB = 2;   // 32-key blocks per step of the per-head walk (the next step's are in flight meanwhile)
// 32-key blocks per step of the head-mean walk: their sums over the heads stay in registers (48 per block at 96 rows) and Q is
// gathered once per head and step, so the step is as long as the registers allow.  Same box, all rows, bf16, 1 / 2 / 4 blocks
// (alternative builds, equal bytes out): 2816 / 1465 / 1163 us at cfg 2's top layer, 406 / 213 / 147 us at its 256-token class,
// 7146 / 2968 / 2240 us at the 1024-px layer - the time follows the number of (head, step) rounds, not the keys in one
// (profiles/attn_match_ab.txt).  Not tried beyond 4: the sums of 8 blocks alone are 384 registers
constexpr int KBM = 4;

struct MatchPlan {
  const int32_t* idx;  // (B, R) on the device
  int32_t* index;
  float* prob;
  int R;        // rows per batch entry
  int ngroups;  // row groups of 32 * NQ rows
  int nseg;     // include_self + N
  int items;    // ngroups * nseg * (H in the per-head form) * B
  float inv_h;  // 1 / H
};

// the 16 values of one row and block against the row's running pair; `key0`: the key of e[0] inside the segment
static __device__ __forceinline__ void take_best(const float (&e)[16], int key0, float& bv, int& bk) {
  float m = e[0];
#pragma unroll
  for (int t = 1; t < 16; ++t) m = __builtin_fmaxf(m, e[t]);
  if (m > bv) {
    int t0 = 15;
#pragma unroll
    for (int t = 14; t >= 0; --t) t0 = e[t] == m ? t : t0;
    bv = m;
    bk = key0 + t0;
  }
}

template <typename T, int NQ, int RED>
__global__ void __launch_bounds__(RW * 64) attn_match_kernel(const AttnKParams p, const MatchPlan pl) {
  using v8 = typename ElemTraits<T>::v8;
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
  if constexpr (RED == kMatchPerHead) { h0 = id % p.H; id /= p.H; }
  const int b = id;

  const KeySeg<T> ks = key_segment<T>(p, b, seg);   // keys past its end are clamped as addresses and never compared
  const int len = ks.len;
  const int km = keymap(lq);

  int qrow[NQ];
  bool ok[NQ];
  gather_rows<NQ>(pl.idx + (int64_t)b * pl.R, pl.R, p.Lq, g0, lq, qrow, ok);

  // the running pair of each row: every probability is >= 0, so the first compared key replaces the start value
  float bv[NQ];
  int bk[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) { bv[qi] = -1.f; bk[qi] = 0; }

  if constexpr (RED == kMatchPerHead) {
    v8 qf[NQ][4];
    float lse2[NQ];
    load_q<T, NQ>(p, b, h0, hi, qrow, qf, lse2);
    v8 kf[KB][4];
#pragma unroll
    for (int kblk = 0; kblk < KB; ++kblk) load_k(ks, h0, 32 * kblk + km, hi, kf[kblk]);
    for (int j = 0; j < len; j += 32 * KB) {
#pragma unroll
      for (int kblk = 0; kblk < KB; ++kblk) {
        f32x16 sc[NQ];
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) sc[qi] = scores<T>(kf[kblk], qf[qi]);
        load_k(ks, h0, j + 32 * (KB + kblk) + km, hi, kf[kblk]);   // the next step's fragments arrive while this step's exponentials run (clamped: a valid address)
        const int key0 = j + 32 * kblk + 16 * hi;
        const bool whole = j + 32 * kblk + 32 <= len;   // wave-uniform: every key of the block exists
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
          float e[16];
#pragma unroll
          for (int t = 0; t < 16; ++t) e[t] = prob(sc[qi][t], p.scale_log2, lse2[qi]);
          if (!whole) {
#pragma unroll
            for (int t = 0; t < 16; ++t) e[t] = key0 + t < len ? e[t] : -1.f;
          }
          take_best(e, key0, bv[qi], bk[qi]);
        }
      }
    }
  } else {
    for (int j = 0; j < len; j += 32 * KBM) {
      // the 32 * KBM keys of this step, every head in ascending order (the order of attn_rows.hip's head mean)
      f32x16 acc[KBM][NQ];
#pragma unroll
      for (int kblk = 0; kblk < KBM; ++kblk)
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
          for (int t = 0; t < 16; ++t) acc[kblk][qi][t] = 0.f;
      for (int h = 0; h < p.H; ++h) {
        v8 qf[NQ][4];
        float lse2[NQ];
        v8 kf[KBM][4];
#pragma unroll
        for (int kblk = 0; kblk < KBM; ++kblk) load_k(ks, h, j + 32 * kblk + km, hi, kf[kblk]);
        load_q<T, NQ>(p, b, h, hi, qrow, qf, lse2);
#pragma unroll
        for (int kblk = 0; kblk < KBM; ++kblk) {
#pragma unroll
          for (int qi = 0; qi < NQ; ++qi) {
            const f32x16 sc = scores<T>(kf[kblk], qf[qi]);
#pragma unroll
            for (int t = 0; t < 16; ++t) acc[kblk][qi][t] += prob(sc[t], p.scale_log2, lse2[qi]);
          }
        }
      }
#pragma unroll
      for (int kblk = 0; kblk < KBM; ++kblk) {
        const int key0 = j + 32 * kblk + 16 * hi;
        const bool whole = j + 32 * kblk + 32 <= len;
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
          float e[16];
#pragma unroll
          for (int t = 0; t < 16; ++t) e[t] = acc[kblk][qi][t] * pl.inv_h;
          if (!whole) {
#pragma unroll
            for (int t = 0; t < 16; ++t) e[t] = key0 + t < len ? e[t] : -1.f;
          }
          take_best(e, key0, bv[qi], bk[qi]);
        }
      }
    }
  }

  // the two half-waves hold disjoint keys of the same rows: larger value wins, then lower key (both halves arrive at the same pair)
  const int64_t obase = RED == kMatchPerHead ? ((int64_t)b * p.H + h0) * pl.R : (int64_t)b * pl.R;
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const float ov = __shfl_xor(bv[qi], 32);
    const int okey = __shfl_xor(bk[qi], 32);
    if (ov > bv[qi] || (ov == bv[qi] && okey < bk[qi])) { bv[qi] = ov; bk[qi] = okey; }
    const int r = (g0 * NQ + qi) * 32 + lq;
    if (hi == 0 && r < pl.R) {
      const int64_t o = (obase + r) * pl.nseg + seg;
      pl.index[o] = ok[qi] ? bk[qi] : -1;
      pl.prob[o] = ok[qi] ? bv[qi] : 0.f;
    }
  }
}

}  // namespace

int64_t ir_attn_match_items(const AttnKParams& p, int n_rows, int reduce) {
  return (int64_t)rows_ngroups(n_rows) * (p.include_self + p.N) * (reduce == kMatchPerHead ? p.H : 1) * p.B;
}

hipError_t ir_launch_attn_match(const AttnKParams& p, int dtype, const int32_t* row_index, int n_rows, int reduce, int32_t* index, float* prob,
                                hipStream_t s) {
  const int64_t items = ir_attn_match_items(p, n_rows, reduce);
  if (items <= 0 || items > kMatchMaxItems) return hipErrorInvalidValue;
  MatchPlan pl;
  pl.idx = row_index;
  pl.index = index;
  pl.prob = prob;
  pl.R = n_rows;
  pl.ngroups = rows_ngroups(n_rows);
  pl.nseg = p.include_self + p.N;
  pl.items = (int)items;
  pl.inv_h = 1.0f / (float)p.H;
  return dispatch_rows(dtype, n_rows, [&](auto t, auto nq) {
    using T = typename decltype(t)::type;
    constexpr int NQ = decltype(nq)::value;
    const dim3 grid((pl.items + RW - 1) / RW), block(RW * 64);
    switch (reduce) {
      case kMatchPerHead: hipLaunchKernelGGL((attn_match_kernel<T, NQ, kMatchPerHead>), grid, block, 0, s, p, pl); break;
      case kMatchHeadMean: hipLaunchKernelGGL((attn_match_kernel<T, NQ, kMatchHeadMean>), grid, block, 0, s, p, pl); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  });
}
