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
// the expression of attn_probs.hip on the same fp32 MFMA result (v_mfma_f32_32x32x16, the four 16-wide steps over d in
// ascending order), so form 0 below is the dump's rows bit for bit.
//
//   IR_ROWS_NONE       `dtype` (B, H, R, Lkv)   attention_probs[:, :, idx, :]
//   IR_ROWS_HEAD_MEAN  fp32    (B, R, Lkv)      attn.mean(dim=1)[b][idx]            (vis_utils.py:92, 104)
//   IR_ROWS_MAP        fp32    (B, Lkv)         the sum of those rows over r        (vis_utils.py:106)
//
// Bound: K is read once (B * H * Lkv * 128 bytes) plus the output; the gathered Q rows (R * H * 128 bytes per batch entry)
// come from L2.  Shape of the work:
//   * the contraction is issued SWAPPED as in attn_probs.hip (keys on the MFMA rows through keymap, the gathered rows on its
//     columns): a lane then holds 16 CONSECUTIVE keys of ONE row per 32 x 32 block and stores them 16 bytes at a time (32 B
//     of a 16-bit row, 64 B of an fp32 row per lane, the two half-waves side by side);
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
#include "ir_common.h"
#include "ir_kernels.h"

namespace {

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

// MFMA row i of a swapped 32 x 32 block carries key keymap(i) of the block (attn_probs.hip): lane (lq, hi) then holds
// keys 16*hi + r, r = 0..15, of row lq
static __device__ __forceinline__ int keymap(int i) { return (i & 3) + 4 * (i >> 3) + 16 * ((i >> 2) & 1); }

template <typename T>
static __device__ __forceinline__ unsigned pack2(float a, float b) {
  typedef T T2 __attribute__((ext_vector_type(2)));
  T2 v;
  v[0] = (T)a;
  v[1] = (T)b;
  return __builtin_bit_cast(unsigned, v);
}

template <typename T, int NQ, int RED>
__global__ void __launch_bounds__(RW * 64) attn_rows_kernel(const AttnKParams p, const RowsPlan pl) {
  using Tr = ElemTraits<T>;
  using v8 = typename Tr::v8;
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

  const T* kb;   // head 0 of the segment's keys
  int64_t ksl, ksh;
  int len, col0, chunk;
  if (c < pl.nch_self) {
    kb = (const T*)p.k_self + (int64_t)b * p.ks_sb; ksl = p.ks_sl; ksh = p.ks_sh; len = p.Ls; col0 = 0; chunk = c;
  } else {
    const int cr = c - pl.nch_self;
    const int n = cr / pl.nch_ref;
    chunk = cr - n * pl.nch_ref;
    kb = ir_ref_entry((const T*)p.k_ref + (int64_t)b * p.kr_sb + (int64_t)n * p.kr_sn, p.ref_tables); ksl = p.kr_sl; ksh = p.kr_sh; len = p.Lr;
    col0 = p.include_self * p.Ls + n * p.Lr;
  }
  const int j_begin = (chunk * RW + wid) * pl.kpw;
  if (j_begin >= len) return;
  const int j_end = (j_begin + pl.kpw < len) ? j_begin + pl.kpw : len;

  const float LOG2E = 1.4426950408889634f;
  const int km = keymap(lq);
  const int32_t* idx = pl.idx + (int64_t)b * pl.R;

  // rows of group g held by this lane: r = (g * NQ + qi) * 32 + lq; their token index (row 0 for padding and indices out of range)
  auto load_idx = [&](int g, int (&qrow)[NQ], bool (&ok)[NQ]) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
      const int r = (g * NQ + qi) * 32 + lq;
      const int ix = r < pl.R ? idx[r] : -1;
      ok[qi] = (unsigned)ix < (unsigned)p.Lq;
      qrow[qi] = ok[qi] ? ix : 0;
    }
  };
  // B operand: Q[row][d = 16ks + 8hi ..] of head h; the LSE of that row in the exp2 domain
  auto load_q = [&](int h, const int (&qrow)[NQ], v8 (&qf)[NQ][4], float (&lse2)[NQ]) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
      const T* qp = (const T*)p.q + (int64_t)b * p.q_sb + (int64_t)qrow[qi] * p.q_sl + (int64_t)h * p.q_sh + hi * 8;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qf[qi][ks] = *(const v8*)(qp + ks * 16);
      lse2[qi] = p.lse[((int64_t)b * p.H + h) * p.Lq + qrow[qi]] * LOG2E;
    }
  };
  // A operand: K[key j + keymap(lq)][d = 16ks + 8hi ..] of head h, keys past the segment clamped (their columns are not stored)
  auto load_k = [&](int h, int j, v8 (&kf)[4]) {
    const int key = j + km;
    const T* kp = kb + (int64_t)h * ksh + (int64_t)(key < len ? key : len - 1) * ksl + hi * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const v8*)(kp + ks * 16);
  };
  // sc[r] = <K[j + 16 hi + r], Q[row of qi]>
  auto scores = [&](const v8 (&kf)[4], const v8 (&qf)[4]) {
    f32x16 sc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) sc = Tr::mfma(kf[ks], qf[ks], sc);
    return sc;
  };

  if constexpr (RED == kRowsNone) {
    int qrow[NQ];
    bool ok[NQ];
    v8 qf[NQ][4];
    float lse2[NQ];
    load_idx(g0, qrow, ok);
    load_q(h0, qrow, qf, lse2);
    v8 kf[2][4];
    load_k(h0, j_begin, kf[0]);
    load_k(h0, j_begin + 32, kf[1]);
    T* const obase = (T*)pl.out + (((int64_t)b * p.H + h0) * pl.R) * (int64_t)p.lkv + col0;
    for (int j = j_begin; j < j_end; j += 64) {
#pragma unroll
      for (int kblk = 0; kblk < 2; ++kblk) {
        f32x16 sc[NQ];
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) sc[qi] = scores(kf[kblk], qf[qi]);
        load_k(h0, j + 64 + 32 * kblk, kf[kblk]);   // the next step's fragments arrive while this step's exponentials run (clamped: a valid address)
        const int key0 = j + 32 * kblk + 16 * hi;
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
          const int r = (g0 * NQ + qi) * 32 + lq;
          float e[16];
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const float x = fast_exp2(__builtin_fmaf(sc[qi][t], p.scale_log2, -lse2[qi]));
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
      load_idx(g, qrow, ok);
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
        for (int kblk = 0; kblk < KB; ++kblk) load_k(h, j_begin + 32 * kblk, kf[kblk]);
        load_q(h, qrow, qf, lse2);
#pragma unroll
        for (int kblk = 0; kblk < KB; ++kblk) {
#pragma unroll
          for (int qi = 0; qi < NQ; ++qi) {
            const f32x16 sc = scores(kf[kblk], qf[qi]);
#pragma unroll
            for (int t = 0; t < 16; ++t) {
              const float x = fast_exp2(__builtin_fmaf(sc[t], p.scale_log2, -lse2[qi]));
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

template <typename T, int NQ>
hipError_t launch_nq(const AttnKParams& p, const RowsPlan& pl, int reduce, int items, hipStream_t s) {
  const dim3 grid(items), block(RW * 64);
  switch (reduce) {
    case kRowsNone: hipLaunchKernelGGL((attn_rows_kernel<T, NQ, kRowsNone>), grid, block, 0, s, p, pl); break;
    case kRowsHeadMean: hipLaunchKernelGGL((attn_rows_kernel<T, NQ, kRowsHeadMean>), grid, block, 0, s, p, pl); break;
    case kRowsMap: hipLaunchKernelGGL((attn_rows_kernel<T, NQ, kRowsMap>), grid, block, 0, s, p, pl); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <typename T>
hipError_t launch_t(const AttnKParams& p, const RowsPlan& pl, int nq, int reduce, int items, hipStream_t s) {
  switch (nq) {
    case 1: return launch_nq<T, 1>(p, pl, reduce, items, s);
    case 2: return launch_nq<T, 2>(p, pl, reduce, items, s);
    default: return launch_nq<T, 3>(p, pl, reduce, items, s);
  }
}

}  // namespace

hipError_t ir_launch_attn_rows(const AttnKParams& p, int dtype, const int32_t* row_index, int n_rows, int reduce, void* out, hipStream_t s) {
  RowsPlan pl;
  pl.idx = row_index;
  pl.out = out;
  pl.R = n_rows;
  const int nblk = (n_rows + 31) / 32;
  const int nq = nblk < 3 ? nblk : 3;   // 32-row blocks a wave holds: the padded row count up to 96, three beyond
  pl.ngroups = (nblk + nq - 1) / nq;
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
  return dtype == 1 ? launch_t<__bf16>(p, pl, nq, reduce, (int)items, s) : launch_t<_Float16>(p, pl, nq, reduce, (int)items, s);
}
