// attn_topk.hip - the k best keys of every K/V segment for a caller-chosen set of query tokens: the k largest attention
// probabilities of each segment and the keys that attain them, without the (B, H, Lq, Lkv) dump (gfx950).
//
// One best key per segment (attn_match.hip) cannot tell one sharp peak from two equal ones - a face repeats its structure - and
// what correspondence code uses to tell them apart is an order statistic: the runner-up (the ratio test), the few best
// hypotheses of a token, the share of a segment's attention that its k best keys carry.  torch.topk over the dump needs the dump.
// This kernel is attn_match.hip with a sorted list of K_T (value, key) pairs per row where that one keeps one running pair:
//
//   p[b,h,r,j] = exp2(fma(<q[b, idx[b,r], h, :], k_seg[b, j, h, :]>, scale*log2(e), -lse[b,h,idx[b,r]]*log2(e)))
//
// the expression and the contraction of ir_readout.h, which every read-out shares.
//
//   IR_MATCH_PER_HEAD   index int32 / prob fp32 (B, H, R, S, k)   rank t: the t-th key of the segment under (p descending, key ascending)
//   IR_MATCH_HEAD_MEAN  index int32 / prob fp32 (B, R, S, k)      the same of the head mean, formed as IR_ROWS_HEAD_MEAN forms it:
//                                                                 the fp32 p summed over the heads in ascending order, then * (1/H)
//
// so rank 0 IS ir_attn_match bit for bit, and the head-mean ranks are a stable descending sort of ir_attn_rows' head-mean row
// segment.  Shape of the work - that of attn_match_kernel:
//   * the lane layout of ir_readout.h: a lane holds 16 CONSECUTIVE keys of ONE gathered row per 32 x 32 block;
//   * a wave owns one segment and up to 96 rows (NQ <= 3 blocks of 32; more rows are further row groups) and walks the WHOLE
//     segment: every output element has one writer and one order.  The per-head form keeps the Q fragments of its head in
//     registers for the walk and has the next step's K in flight; the head-mean form walks the heads in ascending order over
//     every 128 keys and owns the same 96 rows (KBM below);
//   * the list of a row lives in the lane that holds the row, K_T pairs sorted by (value descending, key ascending), K_T the
//     compiled capacity at or above k (2, 4 or 8).  A lane sees its keys in ascending order: the maximum of its 16 new values is
//     tested against the list's LAST value, and only when it beats it strictly does the lane insert - each new value behind
//     every entry greater than or equal to it, so a later equal value never displaces an earlier key.  Every list access has a
//     compile-time index (unrolled compare-and-swap chains): the lists are registers, never scratch;
//   * the two half-waves, which hold keys 0-15 and 16-31 of every block, meet once at the end: a lane reads its partner's list
//     through __shfl_xor(., 32) and merges it into its own under the same order, keeping the first K_T;
//   * a list starts at value -1, key -1; values past the end of a segment become -1 before any compare (their addresses stay
//     clamped to the last key), so neither is ever inserted and a segment shorter than k leaves key -1 in its last ranks,
//     written as index -1, prob 0;
//   * items are (row group, segment, head in the per-head form, batch entry), four to a workgroup whose waves never exchange
//     data: no LDS, no barrier, no atomics, no workspace, one launch.  The cut follows len_self, len_ref, n_refs, R, k and the
//     form only: the call is batch invariant by construction;
//   * an index outside [0, len_q) reads row 0 of q and lse (always a valid address) and gives index -1, prob 0 in every rank;
//     rows of the padding to 32 are not written.  Duplicated indices are rows like any other.
// Instantiations: 2 element types x 3 row-block counts x 2 forms x 3 capacities = 36.
#include "ir_readout.h"

namespace {
using namespace ir_readout;

constexpr int RW = 4;    // waves per workgroup (independent of each other: one item each)
constexpr int KB = 2;    // 32-key blocks per step of the per-head walk (the next step's are in flight meanwhile)
constexpr int KBM = 4;   // 32-key blocks per step of the head-mean walk, as in attn_match.hip: 96 rows and lists of 8 fit beside their sums

struct TopkPlan {
  const int32_t* idx;  // (B, R) on the device
  int32_t* index;
  float* prob;
  int R;        // rows per batch entry
  int k;        // ranks written, <= the compiled capacity
  int ngroups;  // row groups of 32 * NQ rows
  int nseg;     // include_self + N
  int items;    // ngroups * nseg * (H in the per-head form) * B
  float inv_h;  // 1 / H
};

// (v, k) goes to the end of the sorted list and moves up past every entry it beats: `before(a, ak, b, bk)` says that pair a
// stands before pair b.  Compile-time indices only
template <int KT, typename Before>
static __device__ __forceinline__ void list_insert(float v, int k, float (&lv)[KT], int (&lk)[KT], Before before) {
  lv[KT - 1] = v;
  lk[KT - 1] = k;
#pragma unroll
  for (int i = KT - 1; i >= 1; --i) {
    const bool up = before(lv[i], lk[i], lv[i - 1], lk[i - 1]);
    const float hv = up ? lv[i] : lv[i - 1], lo_v = up ? lv[i - 1] : lv[i];
    const int hk = up ? lk[i] : lk[i - 1], lo_k = up ? lk[i - 1] : lk[i];
    lv[i - 1] = hv;
    lk[i - 1] = hk;
    lv[i] = lo_v;
    lk[i] = lo_k;
  }
}

// the 16 values of one row and block against the row's list; `key0`: the key of e[0] inside the segment.  The keys ascend, so
// "strictly greater" is the whole order here: an equal value stays behind the earlier key
template <int KT>
static __device__ __forceinline__ void take_topk(const float (&e)[16], int key0, float (&lv)[KT], int (&lk)[KT]) {
  float m = e[0];
#pragma unroll
  for (int t = 1; t < 16; ++t) m = __builtin_fmaxf(m, e[t]);
  if (m > lv[KT - 1]) {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      auto gt = [](float a, int, float b, int) { return a > b; };
      if constexpr (KT <= 2) {
        // a short list takes every value through selects (a value that does not enter replaces the last pair by itself): a
        // branch per value costs more than the chain it skips
        const bool in = e[t] > lv[KT - 1];
        list_insert<KT>(in ? e[t] : lv[KT - 1], in ? key0 + t : lk[KT - 1], lv, lk, gt);
      } else {
        if (e[t] > lv[KT - 1]) list_insert<KT>(e[t], key0 + t, lv, lk, gt);
      }
    }
  }
}

template <typename T, int NQ, int RED, int KT>
__global__ void __launch_bounds__(RW * 64) attn_topk_kernel(const AttnKParams p, const TopkPlan pl) {
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

  // the list of each row: every probability is >= 0, so the first KT compared keys replace the start pairs
  float lv[NQ][KT];
  int lk[NQ][KT];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
    for (int i = 0; i < KT; ++i) { lv[qi][i] = -1.f; lk[qi][i] = -1; }

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
          take_topk<KT>(e, key0, lv[qi], lk[qi]);
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
          take_topk<KT>(e, key0, lv[qi], lk[qi]);
        }
      }
    }
  }

  // the two half-waves hold disjoint keys of the same rows: each merges its partner's sorted list into its own - larger value
  // first, then lower key - and keeps the first KT (both halves arrive at the same list; the start pairs are equal and stay last)
  const int64_t obase = RED == kMatchPerHead ? ((int64_t)b * p.H + h0) * pl.R : (int64_t)b * pl.R;
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    float ov[KT];
    int okey[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      ov[i] = __shfl_xor(lv[qi][i], 32);
      okey[i] = __shfl_xor(lk[qi][i], 32);
    }
    auto before = [](float a, int ak, float b2, int bk) { return a > b2 || (a == b2 && ak < bk); };
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      // the partner's list is sorted: once an entry does not enter, none behind it does (the test then fails for each of them)
      if (before(ov[i], okey[i], lv[qi][KT - 1], lk[qi][KT - 1])) list_insert<KT>(ov[i], okey[i], lv[qi], lk[qi], before);
    }
    const int r = (g0 * NQ + qi) * 32 + lq;
    if (hi == 0 && r < pl.R) {
      const int64_t o = ((obase + r) * pl.nseg + seg) * pl.k;
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        if (i < pl.k) {
          const bool have = ok[qi] && lk[qi][i] >= 0;   // key -1: the segment has fewer keys than ranks
          pl.index[o + i] = have ? lk[qi][i] : -1;
          pl.prob[o + i] = have ? lv[qi][i] : 0.f;
        }
      }
    }
  }
}

}  // namespace

int64_t ir_attn_topk_items(const AttnKParams& p, int n_rows, int reduce) {
  return (int64_t)rows_ngroups(n_rows) * (p.include_self + p.N) * (reduce == kMatchPerHead ? p.H : 1) * p.B;
}

hipError_t ir_launch_attn_topk(const AttnKParams& p, int dtype, const int32_t* row_index, int n_rows, int k, int reduce, int32_t* index, float* prob,
                               hipStream_t s) {
  const int64_t items = ir_attn_topk_items(p, n_rows, reduce);
  if (items <= 0 || items > kTopkMaxItems || k < 1 || k > kTopkMax) return hipErrorInvalidValue;
  TopkPlan pl;
  pl.idx = row_index;
  pl.index = index;
  pl.prob = prob;
  pl.R = n_rows;
  pl.k = k;
  pl.ngroups = rows_ngroups(n_rows);
  pl.nseg = p.include_self + p.N;
  pl.items = (int)items;
  pl.inv_h = 1.0f / (float)p.H;
  return dispatch_rows(dtype, n_rows, [&](auto t, auto nq) {
    using T = typename decltype(t)::type;
    constexpr int NQ = decltype(nq)::value;
    const dim3 grid((pl.items + RW - 1) / RW), block(RW * 64);
    auto by_cap = [&](auto kt) {
      constexpr int KT = decltype(kt)::value;
      switch (reduce) {
        case kMatchPerHead: hipLaunchKernelGGL((attn_topk_kernel<T, NQ, kMatchPerHead, KT>), grid, block, 0, s, p, pl); break;
        case kMatchHeadMean: hipLaunchKernelGGL((attn_topk_kernel<T, NQ, kMatchHeadMean, KT>), grid, block, 0, s, p, pl); break;
        default: return hipErrorInvalidValue;
      }
      return hipGetLastError();
    };
    // the compiled capacity at or above k
    if (k <= 2) return by_cap(Int<2>{});
    if (k <= 4) return by_cap(Int<4>{});
    return by_cap(Int<8>{});
  });
}
