// attn_rows.hip - the probability rows of a caller-chosen set of query tokens, and the reference's reductions of them, without
// the (B, H, Lq, Lkv) dump (gfx950).
//
// face_replace/training/utils/vis_utils.py:88-110 (get_visualization_image, behind coach.py's vis_attn_probs) takes the head
// mean of attention_probs, picks the rows of the ~68 facial landmarks, sums them and reshapes the result to one heat map over
// the degraded image and its references; calc_landmark_loss (coach.py:531-560) and calc_attn_probs (inference/test.py:93-110)
// read rows of the same tensor.  68 of 4096 rows are 1.7 % of what ir_attn_probs writes, and at the 1024-px configuration the
// tensor cannot be formed at all.  This kernel recomputes exactly those rows from Q, K and the LSE of the fused forward:
//
//   p[b,h,r,j] = exp2(fma(<q[b, idx[b,r], h, :], k_ext[b, j, h, :]>, scale*log2(e), -lse[b,h,idx[b,r]]*log2(e)))
//
// the expression and the contraction of ir_readout.h, which attn_probs.hip shares: form 0 below is the dump's rows bit for bit.
//
//   IR_ROWS_NONE       `dtype` (B, H, R, Lkv)   attention_probs[:, :, idx, :]
//   IR_ROWS_HEAD_MEAN  fp32    (B, R, Lkv)      attn.mean(dim=1)[b][idx]            (vis_utils.py:92, 104)
//   IR_ROWS_MAP        fp32    (B, Lkv)         the sum of those rows over r        (vis_utils.py:106)
//
// Bound: K is read once (B * H * Lkv * 128 bytes) plus the output; the gathered Q rows (R * H * 128 bytes per batch entry)
// come from L2.  Shape of the work:
//   * the lane layout of ir_readout.h: a lane holds 16 CONSECUTIVE keys of ONE gathered row per 32 x 32 block and stores them
//     16 bytes at a time (32 B of a 16-bit row, 64 B of an fp32 row per lane, the two half-waves side by side);
//   * a wave owns a key range of one segment and up to 96 rows (NQ <= 3 blocks of 32; more rows are further row groups) whose
//     Q fragments stay in registers for the walk of that range.  Waves never exchange data: no LDS, no barrier, no atomics;
//   * form 0: a wave walks 256 keys of one head.  Forms 1 / 2: a wave owns 64 keys and walks the HEADS in ascending order
//     over them, summing the fp32 probabilities per (row, key) in registers; the head mean is sum * (1/H) after the sum.
//     Form 2 also walks the row groups (ascending) and adds the head means per key: a lane adds its rows lq, lq + 32, ... in
//     ascending order, then the 32 lanes of a half-wave are folded by a fixed butterfly (strides 1, 2, 4, 8, 16).  Every
//     output element has exactly one writer and one summation order;
//   * the cut of the key axis (256-key chunks of a segment per 4-wave workgroup in forms 1 / 2, 1024-key chunks in form 0)
//     and of the rows follows len_self, len_ref, n_refs, R and `reduce` only - never the batch size, the entry's position or
//     the device: the call is batch invariant by construction;
//   * an index outside [0, len_q) reads row 0 of q and lse (always a valid address) and its probabilities are replaced by
//     zeros; rows of the padding to 32 are neither stored nor summed.  Duplicated indices are rows like any other;
//   * 16-byte stores need every row segment 16-byte aligned (segment lengths multiples of 8 keys for 16-bit rows, of 4 for
//     fp32 rows); other lengths take element stores in the same kernel (a wave-uniform branch).
#include "ir_readout.h"

namespace {
using namespace ir_readout;

constexpr int RW = 4;            // waves per workgroup (independent of each other)
constexpr int KEYS_FORM0 = 256;  // keys a wave walks in form 0
// A/B hooks (alternative builds loaded through IR_LIB_PATH under tools/gpu_attn_rows_ab.py; profiles/attn_rows_ab.txt):
// -DROWS_SUM_KB=<32-key blocks a wave owns in forms 1 / 2>: 1 instead of 2 halves the sums in registers (occupancy 3 instead of
//   1-2) and doubles the gathers of Q: 86.6 / 50.6 us against 98.6 / 45.9 us (head mean / map, cfg 2's top layer) - not taken;
// -DROWS_STORE_NT=1: non-temporal stores, as the line kernel of attn_probs.hip uses for whole 128-byte lines.  Here a store
//   instruction writes 16-byte pieces of 32 different rows, and the pieces of one line arrive over four instructions: with the
//   streaming hint they measured 101.7 / 98.6 us against 71.2 / 67.1 us plain (form 0 / head mean, same layer) - plain it is.
#ifndef ROWS_SUM_KB
#define ROWS_SUM_KB 2
#endif
#ifndef ROWS_STORE_NT
#define ROWS_STORE_NT 0
#endif
constexpr int KB = ROWS_SUM_KB;
constexpr int KEYS_SUM = 32 * KB;  // keys a wave owns in forms 1 / 2 (their per-head sums stay in registers)

template <typename V>
static __device__ __forceinline__ void store16(V v, V* p) {
#if ROWS_STORE_NT
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

struct RowsPlan {
  const int32_t* idx;  // (B, R) on the device
  void* out;
  int R;          // rows per batch entry
  int ngroups;    // row groups of 32 * NQ rows
  int kpw;        // keys per wave
  int nch_self;   // chunks (RW * kpw keys) of the self segment (0 without it)
  int nch_ref;    // chunks per reference segment
  int nch_total;  // nch_self + N * nch_ref
  int wide;       // every row segment of the output is 16-byte aligned
  float inv_h;    // 1 / H
};

template <typename T, int NQ, int RED>
__global__ void __launch_bounds__(RW * 64) attn_rows_kernel(const AttnKParams p, const RowsPlan pl) {
  using v8 = typename ElemTraits<T>::v8;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hi = lane >> 5, lq = lane & 31;

  // work item: row group fastest (forms 0 / 1), then key chunk, then head (form 0), then batch entry
  int id = blockIdx.x;
  int g0 = 0, h0 = 0;
  if constexpr (RED != kRowsMap) { g0 = id % pl.ngroups; id /= pl.ngroups; }
  const int c = id % pl.nch_total;
  id /= pl.nch_total;
  if constexpr (RED == kRowsNone) { h0 = id % p.H; id /= p.H; }
  const int b = id;

  const KeyChunk<T> kc = key_chunk<T>(p, b, c, pl.nch_self, pl.nch_ref);
  const KeySeg<T> ks = kc.ks;   // keys past its end are clamped as addresses; their columns are not stored
  const int len = ks.len, col0 = kc.col0;
  const int j_begin = (kc.chunk * RW + wid) * pl.kpw;
  if (j_begin >= len) return;
  const int j_end = (j_begin + pl.kpw < len) ? j_begin + pl.kpw : len;

  const int km = keymap(lq);
  const int32_t* idx = pl.idx + (int64_t)b * pl.R;

  if constexpr (RED == kRowsNone) {
    int qrow[NQ];
    bool ok[NQ];
    v8 qf[NQ][4];
    float lse2[NQ];
    gather_rows<NQ>(idx, pl.R, p.Lq, g0, lq, qrow, ok);
    load_q<T, NQ>(p, b, h0, hi, qrow, qf, lse2);
    v8 kf[2][4];
    load_k(ks, h0, j_begin + km, hi, kf[0]);
    load_k(ks, h0, j_begin + 32 + km, hi, kf[1]);
    T* const obase = (T*)pl.out + (((int64_t)b * p.H + h0) * pl.R) * (int64_t)p.lkv + col0;
    for (int j = j_begin; j < j_end; j += 64) {
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        f32x16 sc[NQ];
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) sc[qi] = scores<T>(kf[kblk], qf[qi]);
        load_k(ks, h0, j + 64 + 32 * kblk + km, hi, kf[kblk]);   // the next step's fragments arrive while this step's exponentials run (clamped: a valid address)
        const int key0 = j + 32 * kblk + 16 * hi;
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
          const int r = (g0 * NQ + qi) * 32 + lq;
          float e[16];
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const float x = prob(sc[qi][t], p.scale_log2, lse2[qi]);
            e[t] = ok[qi] ? x : 0.f;
          }
          if (r < pl.R) {
            T* op = obase + (int64_t)r * p.lkv + key0;
            if (pl.wide) {   // segment lengths are multiples of 8 keys: an 8-key piece lies wholly inside or outside
              if (key0 < len)
                store16(u32x4{pack2<T>(e[0], e[1]), pack2<T>(e[2], e[3]), pack2<T>(e[4], e[5]), pack2<T>(e[6], e[7])}, (u32x4*)op);
              if (key0 + 8 < len)
                store16(u32x4{pack2<T>(e[8], e[9]), pack2<T>(e[10], e[11]), pack2<T>(e[12], e[13]), pack2<T>(e[14], e[15])}, (u32x4*)(op + 8));
            } else {
#pragma unroll
              for (int t = 0; t < 16; ++t)
                if (key0 + t < len) op[t] = (T)e[t];
            }
          }
        }
      }
    }
  } else {
    // forms 1 / 2: 32 * KB keys of this wave, every head in ascending order
    f32x16 colsum[KB];
#pragma unroll
    for (int kblk = 0; kblk < KB; ++kblk)
#pragma unroll
      for (int t = 0; t < 16; ++t) colsum[kblk][t] = 0.f;
    const int g_first = RED == kRowsMap ? 0 : g0;
    const int g_last = RED == kRowsMap ? pl.ngroups : g0 + 1;
    for (int g = g_first; g < g_last; ++g) {
      int qrow[NQ];
      bool ok[NQ];
      gather_rows<NQ>(idx, pl.R, p.Lq, g, lq, qrow, ok);
      f32x16 acc[KB][NQ];
#pragma unroll
      for (int kblk = 0; kblk < KB; ++kblk)
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
          for (int t = 0; t < 16; ++t) acc[kblk][qi][t] = 0.f;
      for (int h = 0; h < p.H; ++h) {
        v8 qf[NQ][4];
        float lse2[NQ];
        v8 kf[KB][4];
#pragma unroll
        for (int kblk = 0; kblk < KB; ++kblk) load_k(ks, h, j_begin + 32 * kblk + km, hi, kf[kblk]);
        load_q<T, NQ>(p, b, h, hi, qrow, qf, lse2);
#pragma unroll
        for (int kblk = 0; kblk < KB; ++kblk) {
#pragma unroll
          for (int qi = 0; qi < NQ; ++qi) {
            const f32x16 sc = scores<T>(kf[kblk], qf[qi]);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
              const float x = prob(sc[t], p.scale_log2, lse2[qi]);
              acc[kblk][qi][t] += ok[qi] ? x : 0.f;
            }
          }
        }
      }
      if constexpr (RED == kRowsHeadMean) {
#pragma unroll
        for (int kblk = 0; kblk < KB; ++kblk) {
          const int key0 = j_begin + 32 * kblk + 16 * hi;
#pragma unroll
          for (int qi = 0; qi < NQ; ++qi) {
            const int r = (g * NQ + qi) * 32 + lq;
            if (r >= pl.R) continue;
            float* op = (float*)pl.out + ((int64_t)b * pl.R + r) * (int64_t)p.lkv + col0 + key0;
            if (pl.wide) {   // segment lengths are multiples of 4 keys
#pragma unroll
              for (int t = 0; t < 16; t += 4)
                if (key0 + t < len)
                  store16(f32x4{acc[kblk][qi][t] * pl.inv_h, acc[kblk][qi][t + 1] * pl.inv_h, acc[kblk][qi][t + 2] * pl.inv_h,
                                                    acc[kblk][qi][t + 3] * pl.inv_h}, (f32x4*)(op + t));
            } else {
#pragma unroll
              for (int t = 0; t < 16; ++t)
                if (key0 + t < len) op[t] = acc[kblk][qi][t] * pl.inv_h;
            }
          }
        }
      } else {
        // the head means of this lane's rows, added in ascending row order (padding and out-of-range rows hold exact zeros)
#pragma unroll
        for (int kblk = 0; kblk < KB; ++kblk)
#pragma unroll
          for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
            for (int t = 0; t < 16; ++t) {
              const float hm = acc[kblk][qi][t] * pl.inv_h;
              colsum[kblk][t] = __fadd_rn(colsum[kblk][t], hm);
            }
      }
    }
    if constexpr (RED == kRowsMap) {
#pragma unroll
      for (int kblk = 0; kblk < KB; ++kblk) {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          float s = colsum[kblk][t];
#pragma unroll
          for (int m = 1; m < 32; m <<= 1) s += __shfl_xor(s, m);   // within the half-wave: the same tree on every lane
          colsum[kblk][t] = s;
        }
        const int key0 = j_begin + 32 * kblk + 16 * hi;
        if (lq == 0) {
          float* op = (float*)pl.out + (int64_t)b * p.lkv + col0 + key0;
#pragma unroll
          for (int t = 0; t < 16; ++t)
            if (key0 + t < len) op[t] = colsum[kblk][t];
        }
      }
    }
  }
}

}  // namespace

hipError_t ir_launch_attn_rows(const AttnKParams& p, int dtype, const int32_t* row_index, int n_rows, int reduce, void* out, hipStream_t s) {
  RowsPlan pl;
  pl.idx = row_index;
  pl.out = out;
  pl.R = n_rows;
  pl.ngroups = rows_ngroups(n_rows);
  pl.kpw = reduce == kRowsNone ? KEYS_FORM0 : KEYS_SUM;
  const int kc = RW * pl.kpw;
  pl.nch_self = p.include_self ? (p.Ls + kc - 1) / kc : 0;
  pl.nch_ref = p.N > 0 ? (p.Lr + kc - 1) / kc : 0;
  pl.nch_total = pl.nch_self + p.N * pl.nch_ref;
  const int unit = reduce == kRowsNone ? 8 : 4;   // elements per 16 bytes of an output row
  pl.wide = p.lkv % unit == 0 && (!p.include_self || p.Ls % unit == 0) && (p.N == 0 || p.Lr % unit == 0) && ((uintptr_t)out & 15) == 0;
  pl.inv_h = 1.0f / (float)p.H;
  const int64_t items = (int64_t)p.B * (reduce == kRowsNone ? p.H : 1) * pl.nch_total * (reduce == kRowsMap ? 1 : pl.ngroups);
  if (items <= 0 || items > 0x7fffffffLL) return hipErrorInvalidValue;
  return dispatch_rows(dtype, n_rows, [&](auto t, auto nq) {
    using T = typename decltype(t)::type;
    constexpr int NQ = decltype(nq)::value;
    const dim3 grid((int)items), block(RW * 64);
    switch (reduce) {
      case kRowsNone: hipLaunchKernelGGL((attn_rows_kernel<T, NQ, kRowsNone>), grid, block, 0, s, p, pl); break;
      case kRowsHeadMean: hipLaunchKernelGGL((attn_rows_kernel<T, NQ, kRowsHeadMean>), grid, block, 0, s, p, pl); break;
      case kRowsMap: hipLaunchKernelGGL((attn_rows_kernel<T, NQ, kRowsMap>), grid, block, 0, s, p, pl); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  });
}
