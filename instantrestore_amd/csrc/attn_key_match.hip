// attn_key_match.hip - per key of the packed extended key axis, the largest attention probability over ALL query rows and the
// query row that attains it: the column maximum and argmax of P without the (B, H, Lq, Lkv) dump (gfx950).
//
//   prob[b,h,j]  = max over i = 0 .. len_q - 1 of p[b,h,i,j]        index[b,h,j] = the LOWEST i with p[b,h,i,j] == prob[b,h,j]
//   p[b,h,i,j]   = exp2(fma(<q[b,i,h,:], k[b,j,h,:]>, scale*log2(e), -lse[b,h,i]*log2(e)))
//
// the expression and the contraction of ir_readout.h.  It is the query-axis counterpart of attn_match.hip (which takes the maximum
// along the keys of a segment), and together the two give the mutual (cycle) check of a correspondence: keep (i, j) only if j is
// the best key of row i and i is the best row of key j.
//
//   IR_MATCH_PER_HEAD   index int32 (B, H, Lkv), prob fp32 (B, H, Lkv)
//   IR_MATCH_HEAD_MEAN  index int32 (B, Lkv),    prob fp32 (B, Lkv): over m[i,j] = ((p_0 + p_1) + ... + p_{H-1}) * (1/H), the head
//                       mean formed as attn_rows.hip forms it (the sum starts at 0, heads ascending)
//
// The walk is attn_received.hip's - K-STATIONARY.  A wave owns NK = 2 blocks of 32 consecutive keys of ONE segment and walks the
// whole query axis in 32-row blocks, the next block's Q fragments and LSE in flight during this block's exponentials (every load
// of the loop is unconditional).  Lane (lq, hi) holds, per key block, the 16 consecutive keys 16*hi + r of query row i0 + lq and
// keeps a running (max, row) per key, where attn_received.hip has a fused multiply-add.
//
// The order is TOTAL - p descending, then row ascending - so the result does not depend on the order in which the rows meet:
//   * a lane's rows lq, lq + 32, ... arrive in ascending order, and it replaces its pair only on a strict >: the lowest row of
//     the lane's largest value stays;
//   * the start value is -1, below every probability (p >= 0): a row that exists always wins over it, and the row that goes with
//     it is 0 - a lane without any row (len_q < 32) loses to every lane that has one;
//   * at the end the 32 lanes of a half-wave meet in a butterfly over (value, row): a lane takes its partner's pair if the value is
//     larger, or equal with a lower row.  Both partners make the same choice, and a maximum under a total order is the same
//     whatever the tree;
//   * a column of zeros therefore gives row 0, prob 0;
//   * rows of the padding to a whole 32-row block read row len_q - 1 of q and lse again (addresses that exist); their values are
//     replaced by -1 before the comparison, so they never win: index is always in [0, len_q).  Keys past the end of a segment are
//     clamped as addresses by load_k; their pairs are dropped: never written.
// Per head the K fragments of the item's 64 keys stay in registers.  The head mean is not linear under the maximum: the head sum
// of every (row, key) has to exist before the comparison, so the heads are walked INNERMOST per 32-row block, in ascending order,
// into a per-lane accumulator that starts at 0; it is multiplied by 1 / H, then compared.  K of all heads cannot stay in
// registers (H = 20: 80 VGPRs per key block), so the K fragments of the (block, head) step are read again with its Q fragments -
// 16 KB per item, resident in L2 for the whole walk - and the next step's K and Q are in flight during this step's exponentials.
// No LDS, no barrier in either form: a workgroup is four waves that never exchange data.
// Shape of the work: items are (key group of 64 keys, segment, head in the per-head form, batch entry), one wave each, key groups
// of one (segment, head) neighbours in the grid (they read the same Q: L2).  No atomics, no workspace, one launch, one writer per
// output element.  The cut into items follows len_self, len_ref, n_refs and the form only.
#include "ir_readout.h"

namespace {
using namespace ir_readout;

constexpr int KW = 4;   // waves per workgroup (independent of each other: one item each)
constexpr int NK = 2;   // key blocks of 32 keys per wave: 32 * NK (value, row) pairs per lane

struct KeyMatchPlan {
  int32_t* index;
  float* prob;
  int ng_self, ng_ref;   // key groups (32 * NK keys) of the self segment (0 without it) and of one reference
  int per_bh;            // ng_self + N * ng_ref
  int items;             // per_bh * (H in the per-head form) * B
  float inv_h;           // 1 / H
};

typedef float f32x4_dw __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte piece at a 4-byte aligned address
typedef int i32x4_dw __attribute__((ext_vector_type(4), aligned(4)));

// One 32-row block's operands at head h: Q fragments and LSE of row min(i0 + lq, Lq - 1).  Every load is unconditional at an
// address that exists - a padded row reads row Lq - 1 again and is dropped
template <typename T>
struct RowBlock {
  typename ElemTraits<T>::v8 qf[1][4];
  float lse2[1];
};
template <typename T>
static __device__ __forceinline__ void load_rows(const AttnKParams& p, int b, int h, int i0, int lq, int hi, RowBlock<T>& rb) {
  const int row = i0 + lq < p.Lq ? i0 + lq : p.Lq - 1;
  const int qrow[1] = {row};
  load_q<T, 1>(p, b, h, hi, qrow, rb.qf, rb.lse2);
}

// the running pairs of a lane: bv[kb][r], br[kb][r] for key j0 + 32 kb + 16 hi + r
struct Best {
  float v[NK][16];
  int r[NK][16];
};

// values e[0 .. 15] of row `row` meet the lane's pairs of key block kb: strict >, so the earlier (lower) row stays
static __device__ __forceinline__ void take(Best& bs, int kb, const float (&e)[16], int row) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const bool win = e[r] > bs.v[kb][r];
    bs.v[kb][r] = win ? e[r] : bs.v[kb][r];
    bs.r[kb][r] = win ? row : bs.r[kb][r];
  }
}

template <typename T, int RED>
__global__ void __launch_bounds__(KW * 64) attn_key_match_kernel(const AttnKParams p, const KeyMatchPlan pl) {
  using v8 = typename ElemTraits<T>::v8;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane >> 5, lq = lane & 31;
  const int km = keymap(lq);

  // work item: key group fastest (neighbours in the grid read the same Q), then segment, then head (per-head form), then batch entry
  int id = blockIdx.x * KW + wid;
  if (id >= pl.items) return;   // (whole waves; no barrier)
  const int c = id % pl.per_bh;
  id /= pl.per_bh;
  int h0 = 0;
  if constexpr (RED == kKeyMatchPerHead) { h0 = id % p.H; id /= p.H; }
  const int b = id;
  int seg, g;
  if (c < pl.ng_self) {
    seg = 0;
    g = c;
  } else {
    const int cr = c - pl.ng_self, n = cr / pl.ng_ref;
    seg = p.include_self + n;
    g = cr - n * pl.ng_ref;
  }
  const KeySeg<T> ks = key_segment<T>(p, b, seg);
  // the segment's first key on the packed extended key axis
  const int col0 = (p.include_self && seg == 0) ? 0 : p.include_self * p.Ls + (seg - p.include_self) * p.Lr;
  const int j0 = g * 32 * NK;                                  // < ks.len: a group holds at least one key
  const int left = (ks.len - j0 + 31) / 32;
  const int nkb = left < NK ? left : NK;                       // the blocks that hold a key of the segment (wave-uniform)

  Best bs;
#pragma unroll
  for (int kb = 0; kb < NK; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      bs.v[kb][r] = -1.0f;
      bs.r[kb][r] = 0;
    }

  if constexpr (RED == kKeyMatchPerHead) {
    v8 kf[NK][4];
#pragma unroll
    for (int kb = 0; kb < NK; ++kb) load_k(ks, h0, j0 + 32 * kb + km, hi, kf[kb]);   // (blocks past the segment: clamped, never used)
    RowBlock<T> cur, nxt;
    load_rows<T>(p, b, h0, 0, lq, hi, cur);
    for (int i0 = 0; i0 < p.Lq; i0 += 32) {
      // the next block's rows arrive while this block's exponentials run (past the last row: row Lq - 1 again, unused)
      load_rows<T>(p, b, h0, i0 + 32, lq, hi, nxt);
      const bool whole = i0 + 32 <= p.Lq;   // wave-uniform: every row of the block exists
      const bool ok = i0 + lq < p.Lq;
#pragma unroll
      for (int kb = 0; kb < NK; ++kb) {
        if (kb < nkb) {
          const f32x16 sc = scores<T>(kf[kb], cur.qf[0]);
          float e[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) e[r] = prob(sc[r], p.scale_log2, cur.lse2[0]);
          if (!whole) {
#pragma unroll
            for (int r = 0; r < 16; ++r) e[r] = ok ? e[r] : -1.0f;
          }
          take(bs, kb, e, i0 + lq);
        }
      }
      cur = nxt;
    }
  } else {
    // one step is (32-row block, head): its Q fragments, LSE and the K fragments of the item's keys at that head
    struct Step {
      RowBlock<T> rb;
      v8 kf[NK][4];
    };
    auto load_step = [&](int i0, int h, Step& st) {
      load_rows<T>(p, b, h, i0, lq, hi, st.rb);
#pragma unroll
      for (int kb = 0; kb < NK; ++kb) load_k(ks, h, j0 + 32 * kb + km, hi, st.kf[kb]);
    };
    Step cur, nxt;
    load_step(0, 0, cur);
    for (int i0 = 0; i0 < p.Lq; i0 += 32) {
      float acc[NK][16];
#pragma unroll
      for (int kb = 0; kb < NK; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kb][r] = 0.f;
      for (int h = 0; h < p.H; ++h) {
        // the next step arrives while this one's exponentials run (past the last block: row Lq - 1 of head 0 again, unused)
        const bool last = h + 1 == p.H;
        load_step(last ? i0 + 32 : i0, last ? 0 : h + 1, nxt);
#pragma unroll
        for (int kb = 0; kb < NK; ++kb) {
          if (kb < nkb) {
            const f32x16 sc = scores<T>(cur.kf[kb], cur.rb.qf[0]);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kb][r] += prob(sc[r], p.scale_log2, cur.rb.lse2[0]);
          }
        }
        cur = nxt;
      }
      const bool ok = i0 + lq < p.Lq;
#pragma unroll
      for (int kb = 0; kb < NK; ++kb) {
        if (kb < nkb) {
          float e[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) e[r] = ok ? acc[kb][r] * pl.inv_h : -1.0f;
          take(bs, kb, e, i0 + lq);
        }
      }
    }
  }

  // the 32 lanes of a half-wave hold pairs of the same keys over disjoint rows: a butterfly under the total order (value
  // descending, row ascending).  Both partners choose the same pair
#pragma unroll
  for (int kb = 0; kb < NK; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = bs.v[kb][r];
      int w = bs.r[kb][r];
#pragma unroll
      for (int m = 1; m < 32; m <<= 1) {
        const float ov = __shfl_xor(v, m);
        const int ow = __shfl_xor(w, m);
        const bool other = ov > v || (ov == v && ow < w);
        v = other ? ov : v;
        w = other ? ow : w;
      }
      bs.v[kb][r] = v;
      bs.r[kb][r] = w;
    }

  // every lane of a half-wave holds the half's 16 keys of each block: lane lq == 0 writes them, 16 contiguous numbers per output
  if (lq != 0) return;
  const int64_t obase = (RED == kKeyMatchPerHead ? ((int64_t)b * p.H + h0) : (int64_t)b) * p.lkv + col0;
  __attribute__((address_space(1))) float* gprob = (__attribute__((address_space(1))) float*)pl.prob;
  __attribute__((address_space(1))) int* gindex = (__attribute__((address_space(1))) int*)pl.index;
#pragma unroll
  for (int kb = 0; kb < NK; ++kb) {
    if (kb < nkb) {
      const int key0 = j0 + 32 * kb + 16 * hi;
      const int nkeys = ks.len - key0;   // keys of this half that exist: 16 or more - all of them
      __attribute__((address_space(1))) float* pp = gprob + (obase + key0);
      __attribute__((address_space(1))) int* ip = gindex + (obase + key0);
      if (nkeys >= 16) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          *(__attribute__((address_space(1))) f32x4_dw*)(pp + 4 * t) = f32x4{bs.v[kb][4 * t], bs.v[kb][4 * t + 1], bs.v[kb][4 * t + 2], bs.v[kb][4 * t + 3]};
          i32x4_dw iv;
          iv[0] = bs.r[kb][4 * t]; iv[1] = bs.r[kb][4 * t + 1]; iv[2] = bs.r[kb][4 * t + 2]; iv[3] = bs.r[kb][4 * t + 3];
          *(__attribute__((address_space(1))) i32x4_dw*)(ip + 4 * t) = iv;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (r < nkeys) {
            pp[r] = bs.v[kb][r];
            ip[r] = bs.r[kb][r];
          }
      }
    }
  }
}

}  // namespace

int64_t ir_attn_key_match_items(const AttnKParams& p, int reduce) {
  const int keys = 32 * NK;
  const int64_t ng_self = p.include_self ? (p.Ls + keys - 1) / keys : 0;
  const int64_t ng_ref = p.N > 0 ? (p.Lr + keys - 1) / keys : 0;
  return (ng_self + p.N * ng_ref) * (reduce == kKeyMatchPerHead ? p.H : 1) * p.B;
}

hipError_t ir_launch_attn_key_match(const AttnKParams& p, int dtype, int reduce, int32_t* index, float* prob, hipStream_t s) {
  const int64_t items = ir_attn_key_match_items(p, reduce);
  if (items <= 0 || items > kKeyMatchMaxItems) return hipErrorInvalidValue;
  const int keys = 32 * NK;
  KeyMatchPlan pl;
  pl.index = index;
  pl.prob = prob;
  pl.ng_self = p.include_self ? (p.Ls + keys - 1) / keys : 0;
  pl.ng_ref = p.N > 0 ? (p.Lr + keys - 1) / keys : 0;
  pl.per_bh = pl.ng_self + p.N * pl.ng_ref;
  pl.items = (int)items;
  pl.inv_h = 1.0f / (float)p.H;
  const dim3 grid((pl.items + KW - 1) / KW), block(KW * 64);
  auto by_t = [&](auto t) {
    using T = typename decltype(t)::type;
    switch (reduce) {
      case kKeyMatchPerHead: hipLaunchKernelGGL((attn_key_match_kernel<T, kKeyMatchPerHead>), grid, block, 0, s, p, pl); break;
      case kKeyMatchHeadMean: hipLaunchKernelGGL((attn_key_match_kernel<T, kKeyMatchHeadMean>), grid, block, 0, s, p, pl); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  };
  return dtype == 1 ? by_t(Elem<__bf16>{}) : by_t(Elem<_Float16>{});
}
