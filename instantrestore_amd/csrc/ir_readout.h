// ir_readout.h - the QK block that the read-out kernels share (attn_probs.hip, attn_rows.hip, attn_match.hip, attn_transfer.hip; gfx950).
// For this family only: the forward kernels have their own operand paths and never include it.
//
// Every read-out recomputes P = exp2(fma(<q, k>, scale*log2(e), -lse*log2(e))) from the LSE of the fused forward, and the tests
// hold the results of these files to each other bit for bit.  What that rests on is here, once:
//   * the contraction of a 32 x 32 block is issued SWAPPED (S^T = K Q^T: keys on the MFMA rows, query rows on its columns), and
//     the key a lane supplies for MFMA row i is keymap(i).  Lane (lq, hi) - lq = lane & 31, hi = lane >> 5 - then holds C rows
//     (r&3) + 8(r>>2) + 4hi, r = 0..15  ==  the 16 CONSECUTIVE keys 16*hi + r of ONE query row lq: whole 16-byte pieces of a
//     row of P, where the un-swapped form leaves a lane one key of 16 different rows;
//   * a lane's operands are 8 elements d = 16ks + 8hi .. of its row (load_q: B operand, with the row's LSE in the exp2 domain)
//     and of its key (load_k: A operand, keys past the segment clamped to its last key - a valid address; the caller drops them);
//   * scores() starts from a ZEROED accumulator and issues the four v_mfma_f32_32x32x16 steps over d in ASCENDING order, and
//     prob() is the one exponential of the family.  That order and that expression are the bit-for-bit contract;
//   * the keys are the segments [self iff include_self] ++ ref 0 ++ ... (key_segment, through ir_ref_entry for pointer tables).
// attn_probs_generic_kernel issues the contraction un-swapped (Q on A): it shares key_segment and prob only.
#pragma once
#include "ir_common.h"
#include "ir_kernels.h"

namespace ir_readout {

constexpr float LOG2E = 1.4426950408889634f;

static __device__ __forceinline__ int keymap(int i) { return (i & 3) + 4 * (i >> 3) + 16 * ((i >> 2) & 1); }

template <typename T>
static __device__ __forceinline__ unsigned pack2(float a, float b) {
  typedef T T2 __attribute__((ext_vector_type(2)));
  T2 v;
  v[0] = (T)a;
  v[1] = (T)b;
  return __builtin_bit_cast(unsigned, v);
}

template <typename T>
struct KeySeg {
  const T* kb;       // key 0 of the segment at head h0: 0 for the kernels that walk the heads, the item's head for the others
  int64_t ksl, ksh;  // strides of a key and of a head, in elements
  int len;
};

// The self segment, reference n, segment `seg` of entry b.  The parameter block goes BY VALUE here and in key_chunk: inlined, its
// fields are read straight from the kernel's arguments, where a reference would take the block's address - the kernels of
// attn_probs.hip never do, and their code moves when they start to
template <typename T>
static __device__ __forceinline__ KeySeg<T> self_segment(const AttnKParams p, int b, int h0) {
  return {(const T*)p.k_self + (int64_t)b * p.ks_sb + (int64_t)h0 * p.ks_sh, p.ks_sl, p.ks_sh, p.Ls};
}
template <typename T>
static __device__ __forceinline__ KeySeg<T> ref_segment(const AttnKParams p, int b, int n, int h0) {
  return {ir_ref_entry((const T*)p.k_ref + (int64_t)b * p.kr_sb + (int64_t)n * p.kr_sn, p.ref_tables) + (int64_t)h0 * p.kr_sh, p.kr_sl, p.kr_sh, p.Lr};
}
template <typename T>
static __device__ __forceinline__ KeySeg<T> key_segment(const AttnKParams p, int b, int seg, int h0 = 0) {
  if (p.include_self && seg == 0) return self_segment<T>(p, b, h0);
  return ref_segment<T>(p, b, seg - p.include_self, h0);
}

// chunk c of a key axis cut into nch_self chunks of the self segment, then nch_ref of every reference: its segment, its place
// inside the segment and the segment's first column of P
template <typename T>
struct KeyChunk {
  KeySeg<T> ks;
  int seg, chunk, col0;
};
template <typename T>
static __device__ __forceinline__ KeyChunk<T> key_chunk(const AttnKParams p, int b, int c, int nch_self, int nch_ref, int h0 = 0) {
  if (c < nch_self) return {self_segment<T>(p, b, h0), 0, c, 0};
  const int cr = c - nch_self, n = cr / nch_ref;
  return {ref_segment<T>(p, b, n, h0), p.include_self + n, cr - n * nch_ref, p.include_self * p.Ls + n * p.Lr};
}

// (the block by reference, as the lambdas of attn_rows.hip and attn_match.hip captured it; attn_probs_lines_kernel keeps its own copy)
template <typename T, int NQ>
static __device__ __forceinline__ void load_q(const AttnKParams& p, int b, int h, int hi, const int (&qrow)[NQ], typename ElemTraits<T>::v8 (&qf)[NQ][4],
                                              float (&lse2)[NQ]) {
  using v8 = typename ElemTraits<T>::v8;
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const T* qp = (const T*)p.q + (int64_t)b * p.q_sb + (int64_t)qrow[qi] * p.q_sl + (int64_t)h * p.q_sh + hi * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[qi][ks] = *(const v8*)(qp + ks * 16);
    lse2[qi] = p.lse[((int64_t)b * p.H + h) * p.Lq + qrow[qi]] * LOG2E;
  }
}

// `key`: the key of this lane inside the segment, j + keymap(lq) for the block that starts at key j
template <typename T>
static __device__ __forceinline__ void load_k(const KeySeg<T>& seg, int h, int key, int hi, typename ElemTraits<T>::v8 (&kf)[4]) {
  using v8 = typename ElemTraits<T>::v8;
  const T* kp = seg.kb + (int64_t)h * seg.ksh + (int64_t)(key < seg.len ? key : seg.len - 1) * seg.ksl + hi * 8;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const v8*)(kp + ks * 16);
}

// sc[r] = <K[j + 16 hi + r], Q[row lq]>
template <typename T>
static __device__ __forceinline__ f32x16 scores(const typename ElemTraits<T>::v8 (&kf)[4], const typename ElemTraits<T>::v8 (&qf)[4]) {
  f32x16 sc;
#pragma unroll
  for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) sc = ElemTraits<T>::mfma(kf[ks], qf[ks], sc);
  return sc;
}

static __device__ __forceinline__ float prob(float s, float scale_log2, float lse2) { return fast_exp2(__builtin_fmaf(s, scale_log2, -lse2)); }

// the rows of group g that this lane holds, r = (g * NQ + qi) * 32 + lq, as token indices: padding (r >= R) and indices outside
// [0, Lq) go to row 0 - always a valid address - with ok = false
template <int NQ>
static __device__ __forceinline__ void gather_rows(const int32_t* idx, int R, int Lq, int g, int lq, int (&qrow)[NQ], bool (&ok)[NQ]) {
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const int r = (g * NQ + qi) * 32 + lq;
    const int ix = r < R ? idx[r] : -1;
    ok[qi] = (unsigned)ix < (unsigned)Lq;
    qrow[qi] = ok[qi] ? ix : 0;
  }
}

// ---- host side: the row groups of ir_attn_rows / ir_attn_match / ir_attn_transfer ----
// 32-row blocks a wave holds: the padded row count up to 96, three beyond; further rows are further groups
static inline int rows_nq(int n_rows) {
  const int nblk = (n_rows + 31) / 32;
  return nblk < 3 ? nblk : 3;
}
static inline int rows_ngroups(int n_rows) {
  const int nq = rows_nq(n_rows);
  return ((n_rows + 31) / 32 + nq - 1) / nq;
}

template <typename T>
struct Elem {
  using type = T;
};
template <int N>
struct Int {
  static constexpr int value = N;
};
// launch(Elem<T>, Int<NQ>) for the call's element type (1: bf16, else fp16) and NQ = rows_nq(n_rows)
template <typename F>
static inline hipError_t dispatch_rows(int dtype, int n_rows, F&& launch) {
  auto by_nq = [&](auto t) {
    switch (rows_nq(n_rows)) {
      case 1: return launch(t, Int<1>{});
      case 2: return launch(t, Int<2>{});
      default: return launch(t, Int<3>{});
    }
  };
  return dtype == 1 ? by_nq(Elem<__bf16>{}) : by_nq(Elem<_Float16>{});
}

}  // namespace ir_readout
