// attn_received.hip - per-key sums of the attention over the query rows, weighted by a per-row payload: the column sums of P
// without the (B, H, Lq, Lkv) dump (gfx950).
//
//   recv[b,h,j,c] = sum_i p[b,h,i,j] * w[b,i,c]        i over ALL len_q rows, j on the packed extended key axis
//   p[b,h,i,j]    = exp2(fma(<q[b,i,h,:], k[b,j,h,:]>, scale*log2(e), -lse[b,h,i]*log2(e)))
//
// the expression and the contraction of ir_readout.h, which attn_probs.hip, attn_rows.hip, attn_match.hip and attn_transfer.hip
// share.  "Which tokens of each reference does the restored face use, and how much" is w = 1; a region mask or a parsing map of
// the degraded face is a w with several channels.  It is the adjoint of ir_attn_transfer: <w, P y> = <P^T w, y>.
//
//   IR_RECEIVED_PER_HEAD   recv fp32 (B, H, Lkv, C)
//   IR_RECEIVED_HEAD_MEAN  recv fp32 (B, Lkv, C): ((R_0 + R_1) + ... + R_{H-1}) * (1/H) of the per-head outputs, bit for bit
//
// The walk is the transpose of attn_transfer.hip's - K-STATIONARY.  A wave owns NK blocks of 32 consecutive keys of ONE segment;
// their K fragments stay in registers.  It walks the whole query axis in 32-row blocks, the next block's Q fragments, LSE and
// weights in flight during this block's exponentials (every load of the loop is unconditional).  Lane (lq, hi) holds, per key
// block, the 16 consecutive keys 16*hi + r of query row i0 + lq (the layout of ir_readout.h), so the row's LSE and its C weights
// are lane-local: no staging, no broadcast.
//
// The summation contract (the tests hold it with torch.equal):
//   * every (row, key, channel) term is ONE fp32 fused multiply-add acc = fma(p, w, acc) with the weight as multiplicand (no
//     weights: multiplicand 1.0f).  All channels of a key are accumulated over the same rows in the same order.  So no weights
//     IS a channel of ones, equal channels give equal outputs, and a channel that is 1 at one row and 0 elsewhere IS that row's
//     fp32 prob() at every key: adding exact zeros changes nothing, whatever the order;
//   * THE ORDER, a function of len_q and the form only.  Lane (lq, hi) starts from 0 and adds the rows lq, lq + 32, lq + 64, ...
//     in ASCENDING order, one per 32-row block.  At the end of the walk the 32 lanes of a half-wave hold partial sums of the same
//     (key, channel) pairs over the residue classes lq = 0 .. 31 of the rows.  They meet in a butterfly of five steps over the
//     lane bits 1, 2, 4, 8, 16 in THAT order: at step m every lane replaces its value by (its own + the value of lane lq ^ m).
//     Both partners form the same sum (a + b == b + a), so after the fifth step every lane of the half-wave holds
//       ((((s0+s1) + (s2+s3)) + ((s4+s5) + (s6+s7))) + ...) + (... the same tree over s16 .. s31)
//     with s_l the partial sum of residue class l: a balanced tree, leaves in ascending lq.  Nothing depends on B, the grid, the
//     stream or the CU count; IR_FLAG_BATCH_INVARIANT is inert;
//   * the head-mean form gives one item to a workgroup whose waves share the heads: in round n wave w walks head n * nw + w,
//     forms its sums exactly as the per-head form does (butterfly included) and leaves them in LDS.  After the round's barrier
//     ONE lane per output element (in wave 0) adds the round's heads in ASCENDING order into a running total that starts at 0,
//     and multiplies by 1.0f / (float)H once at the end: ((R_0 + R_1) + ... + R_{H-1}) * (1/H) whatever the number of waves.
//     K is fetched again per head;
//   * rows of the padding to a whole 32-row block read row len_q - 1 of q, lse and the weights again (addresses that exist);
//     their probabilities are replaced by 0 before the multiply-add and their weights by 0 - a padded row's own weight is never
//     addressed.  Keys past the end of a segment are clamped as addresses by load_k; their sums are dropped: never written.
//     Whole row blocks skip the replacement and whole key blocks take the 16-byte stores, both on wave-uniform branches.
// Shape of the work: items are (key group of 32 * NK keys, segment, head in the per-head form, batch entry), key groups of one
// (segment, head) neighbours in the grid (they read the same Q: L2).  Per head: one wave per item, four to a workgroup whose
// waves never exchange data - no barrier, no LDS.  Head mean: one workgroup per item, ceil(H / ceil(H / 8)) waves (H 5 / 10 /
// 20: 5 / 5 / 7), one barrier per round of heads.  No atomics, no workspace, one launch, one writer per output element.  C is
// padded to CH = 1 / 2 / 4 / 8 accumulators per key; NK = 3 / 3 / 2 / 1.  The cut into items follows len_self, len_ref, n_refs,
// channels and the form only.  (ir_readout.h's first line lists the files that shared it before this one; it is left as it is,
// so that the objects built from it stay byte for byte what they were.)
#include "ir_readout.h"

namespace {
using namespace ir_readout;

constexpr int RW = 4;   // per-head form: waves per workgroup (independent of each other: one item each)
constexpr int HW = 8;   // head-mean form: at most this many waves per workgroup (one item; the waves share its heads)

constexpr int received_ch(int channels) { return channels <= 1 ? 1 : channels <= 2 ? 2 : channels <= 4 ? 4 : 8; }
constexpr int received_nk(int ch) { return ch <= 2 ? 3 : ch == 4 ? 2 : 1; }   // key blocks per wave: 16 * NK * CH accumulators per lane

struct ReceivedPlan {
  const float* weights;   // w[b, i, c] = weights[b * w_sb + i * w_si + c], or nullptr: one channel of ones
  int64_t w_sb, w_si;
  float* recv;
  int channels;
  int ng_self, ng_ref;    // key groups (32 * NK keys) of the self segment (0 without it) and of one reference
  int per_bh;             // ng_self + N * ng_ref
  int items;              // per_bh * (H in the per-head form) * B
  float inv_h;            // 1 / H
};

typedef float f32x4_dw __attribute__((ext_vector_type(4), aligned(4)));   // a 16-byte piece at a 4-byte aligned address

// One 32-row block's operands: Q fragments, LSE and weights of row min(i0 + lq, Lq - 1), the weights of a padded row replaced by 0
template <typename T, int CH>
struct RowBlock {
  typename ElemTraits<T>::v8 qf[1][4];
  float lse2[1];
  float w[CH];
};

// WM: how the weights come - kOnes (none: 1.0f), kFull (channels == CH: whole pieces), kPart (channels < CH: the padding is 0,
// unread).  Every load is unconditional at an address that exists - a padded row reads row Lq - 1 again and drops it - so that
// nothing in the walk's loop waits on a branch
constexpr int kOnes = 0, kFull = 1, kPart = 2;
template <typename T, int CH, int WM>
static __device__ __forceinline__ void load_rows(const AttnKParams& p, const ReceivedPlan& pl, const float* wb, int b, int h, int i0, int lq, int hi,
                                                 RowBlock<T, CH>& rb) {
  const bool ok = i0 + lq < p.Lq;
  const int row = ok ? i0 + lq : p.Lq - 1;
  const int qrow[1] = {row};
  load_q<T, 1>(p, b, h, hi, qrow, rb.qf, rb.lse2);
  if constexpr (WM == kOnes) {
#pragma unroll
    for (int c = 0; c < CH; ++c) rb.w[c] = (ok && c == 0) ? 1.0f : 0.f;
  } else {
    const __attribute__((address_space(1))) float* gw = (const __attribute__((address_space(1))) float*)wb + (int64_t)row * pl.w_si;   // device memory: global loads, not flat ones
    if constexpr (WM == kFull && CH >= 4) {   // whole 16-byte pieces (4-byte aligned)
#pragma unroll
      for (int c4 = 0; c4 < CH / 4; ++c4) {
        const f32x4 v = *(const __attribute__((address_space(1))) f32x4_dw*)(gw + 4 * c4);
#pragma unroll
        for (int c = 0; c < 4; ++c) rb.w[4 * c4 + c] = ok ? v[c] : 0.f;
      }
    } else {
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const bool have = WM == kFull || c < pl.channels;
        const float v = gw[have ? c : 0];
        rb.w[c] = (ok && have) ? v : 0.f;
      }
    }
  }
}

// The sums of head h over ALL query rows for the wave's key blocks, the 32 lanes of each half-wave combined: a[kb][r * CH + c] is
// key j0 + 32 kb + 16 hi + r, channel c - the order of `recv`.  `nkb`: the blocks that hold a key of the segment (wave-uniform)
template <typename T, int NK, int CH, int WM>
static __device__ __forceinline__ void head_sums_as(const AttnKParams& p, const ReceivedPlan& pl, const KeySeg<T>& ks, const float* wb, int b, int h, int j0,
                                                 int nkb, float (&a)[NK][16 * CH]) {
  using v8 = typename ElemTraits<T>::v8;
  int lane = threadIdx.x & 63;
  // (opaque per call: what the walk derives from the lane is formed again for every head of the head-mean form, not kept in
  // registers across its head loop; with 8 channels the same for the batch entry, whose offsets would not fit the SGPRs)
  if constexpr (CH == 8) asm volatile("" : "+v"(lane), "+s"(b));
  else asm volatile("" : "+v"(lane));
  const int hi = lane >> 5, lq = lane & 31;
  const int km = keymap(lq);
  // two accumulators to a register pair, in the order of `recv`: CH >= 2 - channels c, c + 1 of one key; CH == 1 - keys r, r + 1
  f32x2 a2[NK][8 * CH];
#pragma unroll
  for (int kb = 0; kb < NK; ++kb)
#pragma unroll
    for (int t = 0; t < 8 * CH; ++t) a2[kb][t] = f32x2{0.f, 0.f};

  v8 kf[NK][4];
#pragma unroll
  for (int kb = 0; kb < NK; ++kb) load_k(ks, h, j0 + 32 * kb + km, hi, kf[kb]);   // (blocks past the segment: clamped, never used)

  RowBlock<T, CH> cur, nxt;
  load_rows<T, CH, WM>(p, pl, wb, b, h, 0, lq, hi, cur);
  for (int i0 = 0; i0 < p.Lq; i0 += 32) {
    // the next block's rows arrive while this block's exponentials run (past the last row: row Lq - 1 again, unused)
    load_rows<T, CH, WM>(p, pl, wb, b, h, i0 + 32, lq, hi, nxt);
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
          for (int r = 0; r < 16; ++r) e[r] = ok ? e[r] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 8 * CH; ++t) {
          f32x2 pp, ww;
          if constexpr (CH == 1) {
            pp = f32x2{e[2 * t], e[2 * t + 1]};
            ww = f32x2{cur.w[0], cur.w[0]};
          } else {
            constexpr int HC = CH / 2;
            pp = f32x2{e[t / HC], e[t / HC]};
            ww = f32x2{cur.w[2 * (t % HC)], cur.w[2 * (t % HC) + 1]};
          }
          a2[kb][t] = __builtin_elementwise_fma(pp, ww, a2[kb][t]);
        }
      }
    }
    cur = nxt;
  }
  // the 32 lanes of a half-wave hold the same (key, channel) pairs over disjoint rows: the butterfly over lane bits 1, 2, 4, 8, 16
#pragma unroll
  for (int kb = 0; kb < NK; ++kb)
#pragma unroll
    for (int t = 0; t < 16 * CH; ++t) {
      float v = a2[kb][t >> 1][t & 1];
#pragma unroll
      for (int m = 1; m < 32; m <<= 1) v = v + __shfl_xor(v, m);
      a[kb][t] = v;
    }
}

// (the form of the weights is wave-uniform and fixed for the call: chosen once, outside the walk)
template <typename T, int NK, int CH>
static __device__ __forceinline__ void head_sums(const AttnKParams& p, const ReceivedPlan& pl, const KeySeg<T>& ks, const float* wb, int b, int h, int j0,
                                                 int nkb, float (&a)[NK][16 * CH]) {
  if (wb == nullptr) head_sums_as<T, NK, CH, kOnes>(p, pl, ks, wb, b, h, j0, nkb, a);
  else if (pl.channels == CH) head_sums_as<T, NK, CH, kFull>(p, pl, ks, wb, b, h, j0, nkb, a);
  else head_sums_as<T, NK, CH, kPart>(p, pl, ks, wb, b, h, j0, nkb, a);
}

template <typename T, int RED, int CH>
__global__ void __launch_bounds__((RED == kReceivedPerHead ? RW : HW) * 64) attn_received_kernel(const AttnKParams p, const ReceivedPlan pl) {
  constexpr int NK = received_nk(CH);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane >> 5, lq = lane & 31;

  // work item: key group fastest (neighbours in the grid read the same Q), then segment, then head (per-head form), then batch
  // entry.  Per head: one item per wave; head mean: one item per workgroup, its waves share the heads
  int id = RED == kReceivedPerHead ? blockIdx.x * RW + wid : blockIdx.x;
  if constexpr (RED == kReceivedPerHead) {
    if (id >= pl.items) return;   // (whole waves; the form has no barrier)
  }
  const int c = id % pl.per_bh;
  id /= pl.per_bh;
  int h0 = 0;
  if constexpr (RED == kReceivedPerHead) { h0 = id % p.H; id /= p.H; }
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
  const int nkb = left < NK ? left : NK;
  const float* wb = pl.weights == nullptr ? nullptr : pl.weights + (int64_t)b * pl.w_sb;
  __attribute__((address_space(1))) float* grecv = (__attribute__((address_space(1))) float*)pl.recv;

  if constexpr (RED == kReceivedPerHead) {
    float out[NK][16 * CH];
    head_sums<T, NK, CH>(p, pl, ks, wb, b, h0, j0, nkb, out);
    // every lane of a half-wave holds the half's 16 keys x CH channels of each block: lane lq == 0 writes them, 16 * channels
    // contiguous floats per block
    if (lq != 0) return;
    const int64_t obase = ((int64_t)b * p.H + h0) * p.lkv + col0;
#pragma unroll
    for (int kb = 0; kb < NK; ++kb) {
      if (kb < nkb) {
        const int key0 = j0 + 32 * kb + 16 * hi;
        const int nkeys = ks.len - key0;   // keys of this half that exist: 16 or more - all of them
        __attribute__((address_space(1))) float* op = grecv + (obase + key0) * pl.channels;
        if (nkeys >= 16 && pl.channels == CH) {   // wave-uniform but for the segment's last block
#pragma unroll
          for (int t = 0; t < 4 * CH; ++t)
            *(__attribute__((address_space(1))) f32x4_dw*)(op + 4 * t) = f32x4{out[kb][4 * t], out[kb][4 * t + 1], out[kb][4 * t + 2], out[kb][4 * t + 3]};
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int cc = 0; cc < CH; ++cc)
              if (r < nkeys && cc < pl.channels) op[r * pl.channels + cc] = out[kb][r * CH + cc];
        }
      }
    }
  } else {
    // Head mean: round n of the walk gives head n * nw + w to wave w of the nw waves.  A wave forms its head's sums as the
    // per-head form does and lane lq == 0 of each half leaves them in LDS in the order of `recv`: element
    // e = ((kb * 2 + hi) * 16 + r) * CH + c is key j0 + e / CH, channel e % CH.  After the barrier, lane l < E / 4 of wave 0
    // adds elements 4 l .. 4 l + 3 of waves 0, 1, ... in that order - heads ascending - into its running totals, while the
    // other waves walk their next heads.  Two buffers, so one barrier per round: a wave writes round n + 1 only after wave 0
    // has reached barrier n, that is after its additions of round n - 1, the last reader of that buffer
    constexpr int E = 2 * NK * 16 * CH;
    __shared__ __attribute__((aligned(16))) float part[2][HW][E];
    const int nw = blockDim.x >> 6;
    __shared__ __attribute__((aligned(16))) float total[E];   // wave 0's alone: lane l owns elements 4 l .. 4 l + 3 (no register held across the walks)
    if (wid == 0 && lane < E / 4) *(f32x4*)&total[4 * lane] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int hb = 0, buf = 0; hb < p.H; hb += nw, buf ^= 1) {
      const int h = hb + wid;
      if (h < p.H) {   // wave-uniform
        float a[NK][16 * CH];
        head_sums<T, NK, CH>(p, pl, ks, wb, b, h, j0, nkb, a);
        if (lq == 0) {
#pragma unroll
          for (int kb = 0; kb < NK; ++kb)
#pragma unroll
            for (int t = 0; t < 4 * CH; ++t)
              *(f32x4*)&part[buf][wid][(kb * 2 + hi) * 16 * CH + 4 * t] = f32x4{a[kb][4 * t], a[kb][4 * t + 1], a[kb][4 * t + 2], a[kb][4 * t + 3]};
        }
      }
      __syncthreads();
      if (wid == 0 && lane < E / 4) {
        const int n = p.H - hb < nw ? p.H - hb : nw;
        f32x4 tot = *(const f32x4*)&total[4 * lane];
        for (int w = 0; w < n; ++w) tot = tot + *(const f32x4*)&part[buf][w][4 * lane];
        *(f32x4*)&total[4 * lane] = tot;
      }
    }
    if (wid != 0 || lane >= E / 4) return;
    const f32x4 tot = *(const f32x4*)&total[4 * lane] * pl.inv_h;
    // one writer per element: 4 consecutive floats of `recv` per lane, a 16-byte piece where all of them exist
    const int e0 = 4 * lane;
    const int64_t obase = (int64_t)b * p.lkv + col0 + j0;
    if (pl.channels == CH && j0 + (e0 + 3) / CH < ks.len) {
      *(__attribute__((address_space(1))) f32x4_dw*)(grecv + obase * CH + e0) = tot;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int key = (e0 + u) / CH, cc = (e0 + u) % CH;
        if (j0 + key < ks.len && cc < pl.channels) grecv[(obase + key) * pl.channels + cc] = tot[u];
      }
    }
  }
}

}  // namespace

int64_t ir_attn_received_items(const AttnKParams& p, int channels, int reduce) {
  const int keys = 32 * received_nk(received_ch(channels));
  const int64_t ng_self = p.include_self ? (p.Ls + keys - 1) / keys : 0;
  const int64_t ng_ref = p.N > 0 ? (p.Lr + keys - 1) / keys : 0;
  return (ng_self + p.N * ng_ref) * (reduce == kReceivedPerHead ? p.H : 1) * p.B;
}

hipError_t ir_launch_attn_received(const AttnKParams& p, int dtype, const float* weights, int64_t w_sb, int64_t w_si, int channels, int reduce,
                                   float* recv, hipStream_t s) {
  const int64_t items = ir_attn_received_items(p, channels, reduce);
  if (items <= 0 || items > kReceivedMaxItems) return hipErrorInvalidValue;
  if (channels < 1 || channels > kReceivedMaxChannels) return hipErrorInvalidValue;
  if (weights == nullptr && channels != 1) return hipErrorInvalidValue;
  const int keys = 32 * received_nk(received_ch(channels));
  ReceivedPlan pl;
  pl.weights = weights;
  pl.w_sb = w_sb;
  pl.w_si = w_si;
  pl.recv = recv;
  pl.channels = channels;
  pl.ng_self = p.include_self ? (p.Ls + keys - 1) / keys : 0;
  pl.ng_ref = p.N > 0 ? (p.Lr + keys - 1) / keys : 0;
  pl.per_bh = pl.ng_self + p.N * pl.ng_ref;
  pl.items = (int)items;
  pl.inv_h = 1.0f / (float)p.H;
  // head mean: the fewest rounds that HW waves allow, and then the fewest waves for that many rounds (H 20: 3 rounds of 7)
  const int rounds = (p.H + HW - 1) / HW, hwaves = (p.H + rounds - 1) / rounds;
  const dim3 grid(reduce == kReceivedPerHead ? (pl.items + RW - 1) / RW : pl.items), block((reduce == kReceivedPerHead ? RW : hwaves) * 64);
  auto by_ch = [&](auto t, auto ch) {
    using T = typename decltype(t)::type;
    constexpr int CH = decltype(ch)::value;
    switch (reduce) {
      case kReceivedPerHead: hipLaunchKernelGGL((attn_received_kernel<T, kReceivedPerHead, CH>), grid, block, 0, s, p, pl); break;
      case kReceivedHeadMean: hipLaunchKernelGGL((attn_received_kernel<T, kReceivedHeadMean, CH>), grid, block, 0, s, p, pl); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  };
  auto by_t = [&](auto t) {
    switch (received_ch(channels)) {
      case 1: return by_ch(t, Int<1>{});
      case 2: return by_ch(t, Int<2>{});
      case 4: return by_ch(t, Int<4>{});
      default: return by_ch(t, Int<8>{});
    }
  };
  return dtype == 1 ? by_t(Elem<__bf16>{}) : by_t(Elem<_Float16>{});
}
