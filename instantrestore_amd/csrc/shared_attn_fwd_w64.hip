// shared_attn_fwd_w64.hip - 64-query-rows-per-wave variant of the fused extended self-attention
// forward (gfx950).  Same math, layouts and C-ABI contract as the other kernels.
//
// Why: ablation of the pipelined kernel attributes ~20 % of its time to LDS fragment reads and
// ~10 % to staging + barriers - costs that are paid per wave per K/V tile.  Here every wave owns
// TWO 32-row blocks (A, B): each K fragment fetched from LDS feeds the QK^T MFMAs of both blocks,
// each V^T fragment feeds both PV MFMAs, and a 4-wave workgroup covers 256 rows, so fragment
// reads, DMA traffic and barriers per flop are all halved.  Straight schedule (no S double
// buffer - the registers go to the second block), asm-issued LDS-DMA one tile ahead, K/V rings of 2.
#include <type_traits>

#include "ir_common.h"
#include "ir_kernels.h"

namespace {

constexpr int KVB = IR_KV_TILE;
constexpr int TILE_BYTES = KVB * 64 * 2;  // 8 KiB

struct RowBlock {
  f32x16 nm;         // QS: minus the running reference in all 16 registers - the C operand of a tile's first QK^T MFMAs
  f32x16 o0, o1;     // O^T accumulators (d = 32*db + crow(r,hi), column = query row)
  f32x2 la, lb;      // partial row sums
  float m_run;       // running (lazy) max of the raw scores
  float l_done;      // FOLD: full row sum of the finished segments (la/lb then cover the current one)
};

// FOLD (AdaIN): no second accumulator set and no LDS totals - the accumulators live in a RATIO FRAME,
//   acc' = (sum over finished segments of (a_s o O_s + b_s l_s) + a_cur o O_cur) / a_cur,
// so the PV MFMAs of the current segment add straight into them; at a segment boundary
//   acc' <- acc' * (a_cur / a_next) + l_cur * (b_cur / a_next)        (a = 1, b = 0 for the self segment)
// and at the end a_next = 1 turns the frame into the true total.  a = (sigma_style + eps) /
// (sigma_content + eps) is strictly positive; the lazy-max rescale is linear and touches acc' as before.
// QS (IR_FLAG_Q_PRESCALED, 8 waves): Q arrives as Q * scale * log2(e) (the fused q/k/v projection folds the factor into
// its weights), so the scores leave the matrix pipe as exponents; the running reference enters through the C operand of
// the first QK^T MFMAs of a tile (a 16-register block per row block, rewritten only when the lazy rule moves the
// reference) and the scale-and-subtract multiply-add per score disappears (64 of ~236 VALU instructions per wave and
// tile).  The two reference blocks take the registers of the Q fragments, which move to a wave-private LDS copy and
// are read per tile next to the K fragments.
// ABL (development builds, -DIR_ABLATIONS, tuning values 20-28; always 0 in the product library): ENERGY / TIMING ablations of
// the QS form - each bit removes one class of work and leaves a kernel with WRONG results but the same matrix skeleton, so
// that joules per launch can be attributed class by class (tools/gpu_energy_probe.py, profiles/r5_energy_budget.txt):
//   1 no LDS-DMA after the prologue (both ring slots filled once, the tiles alternate)   2 no per-tile barrier
//   4 Q fragments read from LDS once per tile instead of four times                      8 no exponentials
//  16 no row sums (and no outgrown-reference check)                                      32 no fp32 -> 16-bit conversions
constexpr int W64_ABL_NODMA = 1, W64_ABL_NOBAR = 2, W64_ABL_QREUSE = 4, W64_ABL_NOEXP = 8, W64_ABL_NOSUM = 16, W64_ABL_NOPACK = 32;
// MASS (ABI v9 seg_mass): also store the cumulative log-sum-exp at every segment boundary (a separate instantiation, launched
// only when the caller asks for the masses: the default kernels' code is untouched by it).
template <typename T, bool FOLD, int NW = 4, bool QS = false, int ABL = 0, bool MASS = false>
__global__ void __launch_bounds__(NW * 64, 2) shared_attn_fwd_w64_kernel(const AttnKParams p) {
  using Tr = ElemTraits<T>;
  using v8 = typename Tr::v8;
  using v4 = typename Tr::v4;
  constexpr int NT = NW * 64, QB = NW * 64, CH = 512 / NT;
  // K/V rings of RING tiles each: pair t+RING-1 is in flight while tile t is computed.  RING = 3 (two tile
  // times for a transfer to land) measured equal on plain attention and 5 % slower with the fold (same box):
  // the transfers are not what the waves wait for.  Kept as a build-time switch (-DW64_RING=3).
#ifndef W64_RING
#define W64_RING 2
#endif
  constexpr int RING = W64_RING;
  constexpr int K_OFF = 0, V_OFF = RING * TILE_BYTES;
  constexpr bool QLDS = QS;   // Q fragments live in a wave-private LDS copy: ring + NW * 8 KiB exceed the static limit
  __shared__ __attribute__((aligned(16))) unsigned char smem_static[QLDS ? 16 : 2 * RING * TILE_BYTES];
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
  unsigned char* const smem = QLDS ? smem_dyn : smem_static;
  constexpr int Q_OFF = 2 * RING * TILE_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, lq = lane & 31;
  // Parameters that only the segment changes and the epilogue need are read from the kernel-argument segment THERE,
  // through a pointer the compiler cannot see through: held in SGPRs across the tile loop (hipcc's choice otherwise) they
  // pushed the loop's own scalars out into VGPR lanes - v_readlane on every tile
  typedef const __attribute__((address_space(4))) AttnKParams* KArgs;
  const KArgs kargs = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  auto cold = [&]() -> KArgs { KArgs q = kargs; asm volatile("" : "+s"(q)); return q; };

  // ---- work decode (whole items, then K/V-range pieces of the remainder items) -------------------
  const int xcd = blockIdx.x & 7, xslot = blockIdx.x >> 3;
  int item_local, piece = 0, npiece = 1;
  if (xslot < p.sk_full) {
    item_local = xslot;
  } else {
    npiece = p.sk_k;
    const int r = xslot - p.sk_full;
    item_local = p.sk_full + r / npiece;
    piece = r - (r / npiece) * npiece;
  }
  const int lin = xcd * p.sk_ix + item_local;
  if (item_local >= p.sk_ix || lin >= p.sk_items) return;
  const int bh = lin / p.nqb, qb = lin - bh * p.nqb;
  const int b = bh / p.H, h = bh - b * p.H;
  // ABI v8 (valid_refs): references n >= valid[b] are all-zero (ir_zero_invalid_refs; pix2pix_turbo.py:269-273).  Every score
  // of a zero key is exactly 0 and every value row is 0 (or the AdaIN shift), so that SUFFIX of the segment list is not
  // walked: this item's K/V range ends after reference nref - 1 and the piece that owns the end of the range adds the
  // suffix in closed form before the epilogue (zero_suffix below).  Same result as walking it: zeroed, not masked.
  int nref = p.N;
  if (p.valid != nullptr) {
    const int vb = p.valid[b];
    nref = vb < 0 ? 0 : (vb < p.N ? vb : p.N);
  }
  const int ntiles_b = p.tiles_self + nref * p.tiles_ref;
  const int tile_begin = (int)(((long)ntiles_b * piece) / npiece);
  const int tile_end = (int)(((long)ntiles_b * (piece + 1)) / npiece);
  const int NTILES = tile_end - tile_begin;

  // ---- Q fragments of both row blocks -----------------------------------------------------------
  const int qrowA = qb * QB + wid * 64 + lq, qrowB = qrowA + 32;
  v8 qA[4], qB[4];
  {
    const int ra = qrowA < p.Lq ? qrowA : p.Lq - 1, rb = qrowB < p.Lq ? qrowB : p.Lq - 1;
    const T* base = (const T*)p.q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh + hi * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qA[ks] = *(const v8*)(base + (int64_t)ra * p.q_sl + ks * 16);
      qB[ks] = *(const v8*)(base + (int64_t)rb * p.q_sl + ks * 16);
    }
  }

  int kread[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kread[ks] = lq * 128 + (((2 * ks + hi) ^ ((lq >> 1) & 7)) << 4);
  int vread[2];
  {
    const int m = lane & 15, g = (lane >> 4) & 1;
    const int sw = (m >> 3) & 1;
#pragma unroll
    for (int db = 0; db < 2; ++db)
      vread[db] = (4 * hi + (m >> 2)) * 128 + ((db ^ sw) << 6) + 32 * g + 8 * (m & 3);
  }

  // ---- DMA stream (lane-linear LDS image, swizzle on the source slot) ------------------------------
  const int pslot = tid & 7;
  int srow[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) srow[c] = (tid >> 3) + c * (NT / 8);
  const int nseg = p.include_self + nref;
  i32x4 krw = {0, 0, 0, 0}, vrw = {0, 0, 0, 0};
  int kstep = 0, vstep = 0, sntile = 0, seg = 0, t0 = 0;
  unsigned kvo[CH], vvo[CH];
  auto seg_setup = [&](int s) {
    const KArgs c = cold();
    const T* sk;
    const T* sv;
    int ksl_b, vsl_b, slen;
    if (c->include_self && s == 0) {
      sk = (const T*)c->k_self + (int64_t)b * c->ks_sb + (int64_t)h * c->ks_sh;
      sv = (const T*)c->v_self + (int64_t)b * c->vs_sb + (int64_t)h * c->vs_sh;
      ksl_b = (int)c->ks_sl * 2; vsl_b = (int)c->vs_sl * 2; slen = c->Ls; sntile = c->tiles_self;
    } else {
      const int n = s - c->include_self;
      sk = ir_ref_entry((const T*)c->k_ref + (int64_t)b * c->kr_sb + (int64_t)n * c->kr_sn, c->ref_tables) + (int64_t)h * c->kr_sh;
      sv = ir_ref_entry((const T*)c->v_ref + (int64_t)b * c->vr_sb + (int64_t)n * c->vr_sn, c->ref_tables) + (int64_t)h * c->vr_sh;
      ksl_b = (int)c->kr_sl * 2; vsl_b = (int)c->vr_sl * 2; slen = c->Lr; sntile = c->tiles_ref;
    }
    krw = make_rsrc_words(sk, (unsigned)((slen - 1) * ksl_b + 128));
    vrw = make_rsrc_words(sv, (unsigned)((slen - 1) * vsl_b + 128));
    kstep = KVB * ksl_b;
    vstep = KVB * vsl_b;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      kvo[c] = (unsigned)(srow[c] * ksl_b + ((pslot ^ ((srow[c] >> 1) & 7)) * 16));
      vvo[c] = (unsigned)(srow[c] * vsl_b + ((pslot ^ (((srow[c] >> 1) & 1) << 2)) * 16));
    }
  };
  auto issue_pair = [&](int slot2) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      buffer_load_lds16_async(krw, smem + K_OFF + slot2 * TILE_BYTES + (c * NW + wid) * 1024, kvo[c]);
      buffer_load_lds16_async(vrw, smem + V_OFF + slot2 * TILE_BYTES + (c * NW + wid) * 1024, vvo[c]);
      kvo[c] += kstep;
      vvo[c] += vstep;
    }
    if (++t0 == sntile) {
      t0 = 0;
      if (++seg < nseg) seg_setup(seg);
    }
  };

  // ---- state ------------------------------------------------------------------------------------
  RowBlock A, Bk;
#pragma unroll
  for (int r = 0; r < 16; ++r) { A.o0[r] = 0.f; A.o1[r] = 0.f; Bk.o0[r] = 0.f; Bk.o1[r] = 0.f; }
  A.la = A.lb = Bk.la = Bk.lb = f32x2{0.f, 0.f};
  A.m_run = Bk.m_run = QS ? 0.f : -INFINITY;
  A.l_done = Bk.l_done = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) { A.nm[r] = 0.f; Bk.nm[r] = 0.f; }
  const float c2 = QS ? 1.0f : p.scale_log2;
  const float lazy_thr = 6.0f / c2;

  int seg_b = 0, t0_b = tile_begin;
  if (!(p.include_self && tile_begin < p.tiles_self)) {
    const int r = tile_begin - p.tiles_self;
    seg_b = p.include_self + r / p.tiles_ref;
    t0_b = r - (r / p.tiles_ref) * p.tiles_ref;
  }
  int ct0 = t0_b, cseg = seg_b;
  const bool first_is_self = (p.include_self && seg_b == 0);
  int c_ntile = first_is_self ? p.tiles_self : p.tiles_ref;
  int c_len = first_is_self ? p.Ls : p.Lr;

  // softmax step of one row block on (s0, s1) -> pk, in two parts: the row max of the tile (masking ragged keys
  // first), then rescale check, exponentials, row sums and the 16-bit probabilities
  auto row_max = [&](f32x16& s0, f32x16& s1, int valid) -> float {
    if (valid < KVB) {
      // the compares must stay behind the branch (speculated above it they cost 30 instructions on every tile): the
      // bound goes through a volatile statement, which is not speculated
      int vb = valid;
      asm volatile("" : "+s"(vb));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (key >= vb) s0[r] = -INFINITY;
        if (key + 32 >= vb) s1[r] = -INFINITY;
      }
    }
    float mxa = max3(s0[0], s0[1], s0[2]);
    float mxb = max3(s1[0], s1[1], s1[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) {
      mxa = max3(mxa, s0[r], s0[r + 1]);
      mxb = max3(mxb, s1[r], s1[r + 1]);
    }
    float mx = max3(mxa, mxb, max3(s0[15], s1[15], s1[15]));
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
    return max3(__uint_as_float(sw[0]), __uint_as_float(sw[1]), mx);
  };
  auto softmax_rest = [&](RowBlock& R, f32x16& s0, f32x16& s1, v8 (&pk)[2][2], float mx, bool force) {
    if (QS) {
      // scores are exponents relative to the reference (it came in through the C operand): mx is the growth
      if (force || __any(mx > lazy_thr)) {
        const float d = force ? mx : max3(mx, 0.f, 0.f);
        const float alpha = force ? 1.f : fast_exp2(-d);   // first tile: nothing accumulated yet, and 2^-d may be inf
#pragma unroll
        for (int r = 0; r < 16; ++r) { R.o0[r] *= alpha; R.o1[r] *= alpha; s0[r] -= d; s1[r] -= d; }
        R.la *= alpha;
        R.lb *= alpha;
        if (FOLD) R.l_done *= alpha;
        R.m_run += d;
#pragma unroll
        for (int r = 0; r < 16; ++r) R.nm[r] = -R.m_run;
      }
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        f32x2 t0v = {fast_exp2(s0[r]), fast_exp2(s0[r + 1])};
        f32x2 t1v = {fast_exp2(s1[r]), fast_exp2(s1[r + 1])};
        R.la += t0v;
        R.lb += t1v;
        s0[r] = t0v[0]; s0[r + 1] = t0v[1];
        s1[r] = t1v[0]; s1[r + 1] = t1v[1];
      }
    } else {
    if (__any(mx > R.m_run + lazy_thr)) {  // lazy max: keep the reference while P stays <= 2^6
      const float m_new = max3(R.m_run, mx, mx);
      const float alpha = fast_exp2((R.m_run - m_new) * c2);
#pragma unroll
      for (int r = 0; r < 16; ++r) { R.o0[r] *= alpha; R.o1[r] *= alpha; }
      R.la *= alpha;
      R.lb *= alpha;
      if (FOLD) R.l_done *= alpha;
      R.m_run = m_new;
    }
    const float mc = R.m_run * c2;
    const f32x2 cc = {c2, c2};
    const f32x2 nm = {-mc, -mc};
    {
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      f32x2 t0v = {s0[r], s0[r + 1]};
      f32x2 t1v = {s1[r], s1[r + 1]};
      t0v = __builtin_elementwise_fma(t0v, cc, nm);
      t1v = __builtin_elementwise_fma(t1v, cc, nm);
      t0v[0] = fast_exp2(t0v[0]); t0v[1] = fast_exp2(t0v[1]);
      t1v[0] = fast_exp2(t1v[0]); t1v[1] = fast_exp2(t1v[1]);
      R.la += t0v;
      R.lb += t1v;
      s0[r] = t0v[0]; s0[r + 1] = t0v[1];
      s1[r] = t1v[0]; s1[r + 1] = t1v[1];
    }
    }
    }
    pk[0][0] = __builtin_convertvector(__builtin_shufflevector(s0, s0, 0, 1, 2, 3, 4, 5, 6, 7), v8);
    pk[0][1] = __builtin_convertvector(__builtin_shufflevector(s0, s0, 8, 9, 10, 11, 12, 13, 14, 15), v8);
    pk[1][0] = __builtin_convertvector(__builtin_shufflevector(s1, s1, 0, 1, 2, 3, 4, 5, 6, 7), v8);
    pk[1][1] = __builtin_convertvector(__builtin_shufflevector(s1, s1, 8, 9, 10, 11, 12, 13, 14, 15), v8);
  };

  auto softmax = [&](RowBlock& R, f32x16& s0, f32x16& s1, v8 (&pk)[2][2], int valid, bool force = false) {
    const float mx = row_max(s0, s1, valid);
    softmax_rest(R, s0, s1, pk, mx, force);
  };

  // ABI v9 (seg_mass): the cumulative log-sum-exp through segment s of the rows this lane pair owns (log2 units; a number the
  // running reference cancels out of) goes to seg_cum - or, for a K/V-range piece, to its slot of ws_cum.  Segment boundaries
  // only: nothing here is on the per-tile path.
  auto cum_store = [&](int rowoff, int s, float v2) {
    const KArgs c = cold();
    if (hi != 0) return;
    if (npiece > 1) {
      const int64_t prow = ((int64_t)((xcd * (c->sk_ix - c->sk_full) + (item_local - c->sk_full)) * npiece + piece)) * QB + wid * 64 + rowoff + lq;
      c->ws_cum[prow * c->nseg_out + s] = v2;
    } else if (qrowA + rowoff < c->Lq) {
      c->seg_cum[(((int64_t)b * c->H + h) * c->Lq + qrowA + rowoff) * c->nseg_out + s] = v2 * 0.69314718f;
    }
  };
  auto ref_log2 = [&](const RowBlock& R) { return QS ? R.m_run : R.m_run * c2; };
  auto row_sum_now = [&](const RowBlock& R) {
    const float ls = (R.la[0] + R.la[1]) + (R.lb[0] + R.lb[1]);
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ls), __float_as_uint(ls), false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  };
  auto cum_boundary = [&](int sc) {   // without the fold the row sums run over all segments: they ARE the cumulative sums
    const float la_ = row_sum_now(A), lb_ = row_sum_now(Bk);
    cum_store(0, sc, ref_log2(A) + __log2f(la_));
    cum_store(32, sc, ref_log2(Bk) + __log2f(lb_));
  };
  // FOLD: close segment `sc`; `has_next`: another (reference) segment follows in this piece
  auto seg_row_sum = [&](RowBlock& R) {
    float ls = (R.la[0] + R.la[1]) + (R.lb[0] + R.lb[1]);
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ls), __float_as_uint(ls), false, false);
    ls = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    R.l_done += ls;
    R.la = f32x2{0.f, 0.f};
    R.lb = f32x2{0.f, 0.f};
    return ls;
  };
  auto fold_boundary = [&](int sc, bool has_next) {
    const float lsA = seg_row_sum(A), lsB = seg_row_sum(Bk);
    const KArgs c = cold();
    if (MASS) {
      cum_store(0, sc, ref_log2(A) + __log2f(A.l_done));
      cum_store(32, sc, ref_log2(Bk) + __log2f(Bk.l_done));
    }
    const bool cur_ref = !(c->include_self && sc == 0);
    const int64_t ao_c = ((int64_t)(b * c->N + (cur_ref ? sc - c->include_self : 0)) * c->H + h) * 64 + 4 * hi;
    const int64_t ao_n = ((int64_t)(b * c->N + (has_next ? sc + 1 - c->include_self : 0)) * c->H + h) * 64 + 4 * hi;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      f32x4 ac0 = {1.f, 1.f, 1.f, 1.f}, ac1 = ac0, an0 = ac0, an1 = ac0, bc0 = {0.f, 0.f, 0.f, 0.f}, bc1 = bc0;
      if (cur_ref) {
        ac0 = *(const f32x4*)(c->aa + ao_c + 8 * g4); ac1 = *(const f32x4*)(c->aa + ao_c + 32 + 8 * g4);
        bc0 = *(const f32x4*)(c->ab + ao_c + 8 * g4); bc1 = *(const f32x4*)(c->ab + ao_c + 32 + 8 * g4);
      }
      if (has_next) {
        an0 = *(const f32x4*)(c->aa + ao_n + 8 * g4); an1 = *(const f32x4*)(c->aa + ao_n + 32 + 8 * g4);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 4 * g4 + i;
        const float i0 = 1.0f / an0[i], i1 = 1.0f / an1[i];
        const float sa0 = ac0[i] * i0, sb0 = bc0[i] * i0, sa1 = ac1[i] * i1, sb1 = bc1[i] * i1;
        A.o0[r] = __builtin_fmaf(A.o0[r], sa0, lsA * sb0);
        Bk.o0[r] = __builtin_fmaf(Bk.o0[r], sa0, lsB * sb0);
        A.o1[r] = __builtin_fmaf(A.o1[r], sa1, lsA * sb1);
        Bk.o1[r] = __builtin_fmaf(Bk.o1[r], sa1, lsB * sb1);
      }
    }
  };

  // ---- prologue ---------------------------------------------------------------------------------
  seg = seg_b;
  t0 = t0_b;
  seg_setup(seg);
#pragma unroll
  for (int c = 0; c < CH; ++c) { kvo[c] += (unsigned)(t0 * kstep); vvo[c] += (unsigned)(t0 * vstep); }
  issue_pair(0);
  if ((RING == 3 || (ABL & W64_ABL_NODMA)) && NTILES > 1) issue_pair(1);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) asm volatile("" ::"v"(qA[ks]), "v"(qB[ks]));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (QLDS) {
    unsigned char* ql = smem + Q_OFF + wid * 8192 + lane * 16;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      *(IR_LDS v8*)(IR_LDS unsigned char*)(ql + ks * 1024) = qA[ks];
      *(IR_LDS v8*)(IR_LDS unsigned char*)(ql + (4 + ks) * 1024) = qB[ks];
    }
  }
  __syncthreads();

  // S^T = K Q^T of one tile for both row blocks: every K fragment is fetched once, used twice
  auto qk_tile = [&](const unsigned char* Kb, f32x16& sa0, f32x16& sa1, f32x16& sb0, f32x16& sb1) {
    if (!QS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { sa0[r] = 0.f; sa1[r] = 0.f; sb0[r] = 0.f; sb1[r] = 0.f; }
    }
    if (QLDS) {   // Q fragments from the wave's LDS copy, one step ahead like the K fragments
      const unsigned char* ql = smem + Q_OFF + wid * 8192 + lane * 16;
      v8 kc0 = *(const IR_LDS v8*)(IR_LDS unsigned char*)(Kb + kread[0]);
      v8 kc1 = *(const IR_LDS v8*)(IR_LDS unsigned char*)(Kb + 32 * 128 + kread[0]);
      v8 qa = *(const IR_LDS v8*)(IR_LDS unsigned char*)(ql);
      v8 qb = *(const IR_LDS v8*)(IR_LDS unsigned char*)(ql + 4 * 1024);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        v8 kn0 = kc0, kn1 = kc1, qan = qa, qbn = qb;
        if (ks < 3) {
          kn0 = *(const IR_LDS v8*)(IR_LDS unsigned char*)(Kb + kread[ks + 1]);
          kn1 = *(const IR_LDS v8*)(IR_LDS unsigned char*)(Kb + 32 * 128 + kread[ks + 1]);
          if (!(ABL & W64_ABL_QREUSE)) {
            qan = *(const IR_LDS v8*)(IR_LDS unsigned char*)(ql + (ks + 1) * 1024);
            qbn = *(const IR_LDS v8*)(IR_LDS unsigned char*)(ql + (4 + ks + 1) * 1024);
          }
        }
        if (QLDS) __builtin_amdgcn_sched_barrier(0);
        if (QS && ks == 0) {
          // minus the running reference rides in on the C operand.  Spelled in asm: through the builtin hipcc takes
          // the tied (dst = C) form for three of the four and first copies the 16-register block into the
          // destination - 48 moves per tile where 64 multiply-adds were saved.  Three MFMAs separate each of these
          // from the first MFMA that accumulates onto its result (the sched_barriers keep that order).
          if (std::is_same<T, __bf16>::value) {
            asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(sa0) : "v"(kc0), "v"(qa), "v"(A.nm));
            asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(sa1) : "v"(kc1), "v"(qa), "v"(A.nm));
            asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(sb0) : "v"(kc0), "v"(qb), "v"(Bk.nm));
            asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(sb1) : "v"(kc1), "v"(qb), "v"(Bk.nm));
          } else {
            asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %3" : "=&v"(sa0) : "v"(kc0), "v"(qa), "v"(A.nm));
            asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %3" : "=&v"(sa1) : "v"(kc1), "v"(qa), "v"(A.nm));
            asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %3" : "=&v"(sb0) : "v"(kc0), "v"(qb), "v"(Bk.nm));
            asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %3" : "=&v"(sb1) : "v"(kc1), "v"(qb), "v"(Bk.nm));
          }
        } else {
          sa0 = Tr::mfma(kc0, qa, sa0);
          sa1 = Tr::mfma(kc1, qa, sa1);
          sb0 = Tr::mfma(kc0, qb, sb0);
          sb1 = Tr::mfma(kc1, qb, sb1);
        }
        if (QLDS) __builtin_amdgcn_sched_barrier(0);
        kc0 = kn0; kc1 = kn1; qa = qan; qb = qbn;
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const v8 k0 = *(const IR_LDS v8*)(IR_LDS unsigned char*)(Kb + kread[ks]);
        const v8 k1 = *(const IR_LDS v8*)(IR_LDS unsigned char*)(Kb + 32 * 128 + kread[ks]);
        sa0 = Tr::mfma(k0, qA[ks], sa0);
        sa1 = Tr::mfma(k1, qA[ks], sa1);
        sb0 = Tr::mfma(k0, qB[ks], sb0);
        sb1 = Tr::mfma(k1, qB[ks], sb1);
      }
    }
    asm volatile("s_nop 7\n\ts_nop 4" : "+v"(sa0), "+v"(sa1), "+v"(sb0), "+v"(sb1));  // MFMA -> asm v_max3 pad
  };
  // O^T += V^T P^T of one tile for both row blocks: every V^T fragment is fetched once, used twice
  auto pv_tile = [&](const unsigned char* Vb, v8 (&pkA)[2][2], v8 (&pkB)[2][2]) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int off = (32 * kb + 16 * ks) * 128;
        const v8 v0 = join_tr<v8>(lds_read_tr16(Vb + vread[0] + off), lds_read_tr16(Vb + vread[0] + off + 8 * 128));
        const v8 v1 = join_tr<v8>(lds_read_tr16(Vb + vread[1] + off), lds_read_tr16(Vb + vread[1] + off + 8 * 128));
        A.o0 = Tr::mfma(v0, pkA[kb][ks], A.o0);
        A.o1 = Tr::mfma(v1, pkA[kb][ks], A.o1);
        Bk.o0 = Tr::mfma(v0, pkB[kb][ks], Bk.o0);
        Bk.o1 = Tr::mfma(v1, pkB[kb][ks], Bk.o1);
      }
    }
  };

  {
  int cur = 0;
  for (int t = 0; t < NTILES; ++t) {
    // pair t+RING-1 goes into the slot that was last read in step t-1
    if (!(ABL & W64_ABL_NODMA) && t + RING - 1 < NTILES) issue_pair(RING == 3 ? (cur >= 1 ? cur - 1 : 2) : (cur ^ 1));

    const unsigned char* Kb = smem + K_OFF + cur * TILE_BYTES;
    f32x16 sa0, sa1, sb0, sb1;
    qk_tile(Kb, sa0, sa1, sb0, sb1);

    const int valid = c_len - ct0 * KVB;
    v8 pkA[2][2], pkB[2][2];
    if (QS) {
      // Reference checked AFTER the exponentials: the scores are exponents relative to the running reference
      // already, so P = exp2(S) needs no row max; what has to be caught is a tile that outgrows the reference, and the
      // tile's own row sums (needed anyway) show that: each of a lane's four 8-element partial sums per row block is
      // compared with 2^11, so no probability above 2^11 gets through (one above 2^8 only beside smaller ones) - harmless
      // in the 16-bit operands (bf16 range; fp16 max 65504) and the fp32 accumulators; looser than the 2^6 of the lazy
      // row-max rule of the other kernels, tests/test_gpu_round2.py "mid_jump" pins it - and inf/NaN if one overflowed.  Then (rare; always on the
      // first tile, whose reference is still 0) the scores are formed again - the K tile is still in LDS - and the
      // exact path runs: row max, reference moved, accumulators and sums rescaled.  Saves the 38 v_max3 of every tile.
      auto mask = [&](f32x16& s0, f32x16& s1) {
        int vb = valid;
        asm volatile("" : "+s"(vb));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (key >= vb) s0[r] = -INFINITY;
          if (key + 32 >= vb) s1[r] = -INFINITY;
        }
      };
      auto pack = [&](f32x16& s0, f32x16& s1, v8 (&pk)[2][2]) {
        if (ABL & W64_ABL_NOPACK) {   // the raw bits of four fp32 registers stand for the eight 16-bit probabilities: no instruction
          pk[0][0] = __builtin_bit_cast(v8, __builtin_shufflevector(s0, s0, 0, 1, 2, 3));
          pk[0][1] = __builtin_bit_cast(v8, __builtin_shufflevector(s0, s0, 8, 9, 10, 11));
          pk[1][0] = __builtin_bit_cast(v8, __builtin_shufflevector(s1, s1, 0, 1, 2, 3));
          pk[1][1] = __builtin_bit_cast(v8, __builtin_shufflevector(s1, s1, 8, 9, 10, 11));
          return;
        }
        pk[0][0] = __builtin_convertvector(__builtin_shufflevector(s0, s0, 0, 1, 2, 3, 4, 5, 6, 7), v8);
        pk[0][1] = __builtin_convertvector(__builtin_shufflevector(s0, s0, 8, 9, 10, 11, 12, 13, 14, 15), v8);
        pk[1][0] = __builtin_convertvector(__builtin_shufflevector(s1, s1, 0, 1, 2, 3, 4, 5, 6, 7), v8);
        pk[1][1] = __builtin_convertvector(__builtin_shufflevector(s1, s1, 8, 9, 10, 11, 12, 13, 14, 15), v8);
      };
      // exponentials in place, the 16-bit probabilities, and four partial sums of the TILE's row sum
      auto exp_sum = [&](f32x16& s0, f32x16& s1, float (&ts)[4], v8 (&pk)[2][2]) {
        if (ABL & (W64_ABL_NOEXP | W64_ABL_NOSUM)) {   // ablations: the same walk with the exponentials and / or the sums left out
          ts[0] = ts[1] = ts[2] = ts[3] = 1.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (!(ABL & W64_ABL_NOEXP)) { s0[r] = fast_exp2(s0[r]); s1[r] = fast_exp2(s1[r]); }
            if (!(ABL & W64_ABL_NOSUM)) { ts[r & 1] += s0[r]; ts[2 + (r & 1)] += s1[r]; }
          }
          pack(s0, s1, pk);
          return;
        }
        s0[0] = fast_exp2(s0[0]); s0[1] = fast_exp2(s0[1]); s1[0] = fast_exp2(s1[0]); s1[1] = fast_exp2(s1[1]);
        ts[0] = s0[0]; ts[1] = s0[1]; ts[2] = s1[0]; ts[3] = s1[1];
#pragma unroll
        for (int r = 2; r < 16; r += 2) {
          s0[r] = fast_exp2(s0[r]); s0[r + 1] = fast_exp2(s0[r + 1]);
          s1[r] = fast_exp2(s1[r]); s1[r + 1] = fast_exp2(s1[r + 1]);
          ts[0] += s0[r]; ts[1] += s0[r + 1]; ts[2] += s1[r]; ts[3] += s1[r + 1];
        }
        pack(s0, s1, pk);
      };
      auto redo = [&](RowBlock& R, f32x16& s0, f32x16& s1, float (&ts)[4], v8 (&pk)[2][2]) {
        const float mx = row_max(s0, s1, KVB);   // (masked above)
        const float d = (t == 0) ? mx : max3(mx, 0.f, 0.f);
        const float alpha = (t == 0) ? 1.f : fast_exp2(-d);   // first tile: nothing accumulated yet, and 2^-d may be inf
#pragma unroll
        for (int r = 0; r < 16; ++r) { R.o0[r] *= alpha; R.o1[r] *= alpha; s0[r] -= d; s1[r] -= d; }
        R.la *= alpha;
        R.lb *= alpha;
        if (FOLD) R.l_done *= alpha;
        R.m_run += d;
#pragma unroll
        for (int r = 0; r < 16; ++r) R.nm[r] = -R.m_run;
        exp_sum(s0, s1, ts, pk);
      };
      if (valid < KVB) { mask(sa0, sa1); mask(sb0, sb1); }
      float tsA[4], tsB[4];
      exp_sum(sa0, sa1, tsA, pkA);
      exp_sum(sb0, sb1, tsB, pkB);
      const float big = max3(max3(tsA[0], tsA[1], tsA[2]), max3(tsB[0], tsB[1], tsB[2]), max3(tsA[3], tsB[3], tsB[3]));
      if (t == 0 || (!(ABL & (W64_ABL_NOEXP | W64_ABL_NOSUM)) && __any(!(big <= 2048.f)))) {
        qk_tile(Kb, sa0, sa1, sb0, sb1);
        if (valid < KVB) { mask(sa0, sa1); mask(sb0, sb1); }
        redo(A, sa0, sa1, tsA, pkA);
        redo(Bk, sb0, sb1, tsB, pkB);
      }
      A.la[0] += tsA[0]; A.la[1] += tsA[1]; A.lb[0] += tsA[2]; A.lb[1] += tsA[3];
      Bk.la[0] += tsB[0]; Bk.la[1] += tsB[1]; Bk.lb[0] += tsB[2]; Bk.lb[1] += tsB[3];
    } else
    {
    softmax(A, sa0, sa1, pkA, valid, QS && t == 0);
    softmax(Bk, sb0, sb1, pkB, valid, QS && t == 0);
    }

    pv_tile(smem + V_OFF + cur * TILE_BYTES, pkA, pkB);
    if (++ct0 == c_ntile) {
      if (FOLD) fold_boundary(cseg, t + 1 < NTILES);
      else if (MASS) cum_boundary(cseg);
      const KArgs c = cold();
      ct0 = 0; ++cseg; c_ntile = c->tiles_ref; c_len = c->Lr;
    }

    // pair t+1 has landed; with RING = 3 the 2*CH transfers of pair t+2, issued in this step, stay in flight
    // (vector memory operations retire in issue order and nothing else was issued after them)
    if (RING == 3 && t + 2 < NTILES) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * CH) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!(ABL & W64_ABL_NOBAR)) __syncthreads();
    cur = (RING == 3) ? (cur == 2 ? 0 : cur + 1) : (cur ^ 1);
  }
  }

  // ---- epilogue (per row block) ---------------------------------------------------------------------
  if (FOLD && ct0 != 0) fold_boundary(cseg, false);  // a piece that stops inside a segment closes what it has (an empty piece: zeros)
  constexpr bool want_cum = MASS;
  if (!FOLD && want_cum && ct0 != 0) cum_boundary(cseg);
  const int s_next = cseg + (ct0 != 0 ? 1 : 0);       // first segment whose cumulative value this piece has not stored yet
  if (want_cum && npiece > 1)
    for (int s = 0; s < seg_b; ++s) { cum_store(0, s, -INFINITY); cum_store(32, s, -INFINITY); }   // segments before this piece's range
  float lpreA = -1.f, lpreB = -1.f, pzA = 0.f, pzB = 0.f;   // zero suffix: row sum before it (final frame), weight of one zero segment
  // Zero-filled references in closed form (ABI v8): the nzero * Lr keys of the suffix all score exactly 0.  With the running
  // reference m (exponent domain) a zero score weighs 2^(-m): the reference first moves up to 0 if it was below (exact max,
  // once per launch), then the row sum takes nzero * Lr * 2^(-m) and - with the AdaIN fold - the output takes that weight
  // times the sum of the suffix's shifts b (a * 0 + b per key; the accumulators are the true total here: the last boundary
  // closed the ratio frame with a_next = 1).  Without the fold the value rows are 0 and only the row sum moves.
  if (nref < p.N && piece == npiece - 1) {
    const KArgs c = cold();
    const float nz = (float)(c->N - nref), lr = (float)c->Lr;
    auto zero_suffix = [&](RowBlock& R, float& l_pre) -> float {   // returns the weight of ONE zero segment (Lr keys)
      if (!QS && R.m_run == -INFINITY) R.m_run = 0.f;          // no tile walked at all: the reference starts at the zero score
      const float e = QS ? -R.m_run : -R.m_run * c2;           // exponent of a zero score relative to the reference
      const float up = max3(e, 0.f, 0.f);
      const float alpha = fast_exp2(-up);
#pragma unroll
      for (int r = 0; r < 16; ++r) { R.o0[r] *= alpha; R.o1[r] *= alpha; }
      R.la *= alpha;
      R.lb *= alpha;
      if (FOLD) R.l_done *= alpha;
      R.m_run += QS ? up : up / c2;
      const float pz = fast_exp2(e - up) * lr;
      if (FOLD) l_pre = R.l_done;
      else if (want_cum) l_pre = row_sum_now(R);
      if (FOLD) R.l_done += pz * nz;
      else if (hi == 0) R.la[0] += pz * nz;                    // the two lanes of a row add their partial sums in finish()
      return pz;
    };
    pzA = zero_suffix(A, lpreA);
    pzB = zero_suffix(Bk, lpreB);
    if (FOLD) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 bs0 = {0.f, 0.f, 0.f, 0.f}, bs1 = bs0;
        for (int n = nref; n < c->N; ++n) {
          const int64_t ao = ((int64_t)(b * c->N + n) * c->H + h) * 64 + 4 * hi;
          bs0 += *(const f32x4*)(c->ab + ao + 8 * g4);
          bs1 += *(const f32x4*)(c->ab + ao + 32 + 8 * g4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * g4 + i;
          A.o0[r] = __builtin_fmaf(pzA, bs0[i], A.o0[r]);
          Bk.o0[r] = __builtin_fmaf(pzB, bs0[i], Bk.o0[r]);
          A.o1[r] = __builtin_fmaf(pzA, bs1[i], A.o1[r]);
          Bk.o1[r] = __builtin_fmaf(pzB, bs1[i], Bk.o1[r]);
        }
      }
    }
  }
  auto finish = [&](RowBlock& R, int qrow, int rowoff, float l_pre, float pz) {
    float l_fin;
    if (FOLD) {
      l_fin = R.l_done;
    } else {
      float ls = (R.la[0] + R.la[1]) + (R.lb[0] + R.lb[1]);
      const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ls), __float_as_uint(ls), false, false);
      l_fin = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
    }
    if (want_cum) {
      // segments after the end of this piece's range: the piece's total - and, on the piece that owns the zero-filled suffix,
      // the row sum before the suffix plus j zero segments
      const KArgs c = cold();
      const float lp = l_pre < 0.f ? l_fin : l_pre, mref = ref_log2(R);
      const int sz = c->include_self + nref;
      for (int s = s_next; s < c->nseg_out; ++s) {
        const int j = s - sz + 1;
        cum_store(rowoff, s, mref + __log2f(lp + pz * (float)(j > 0 ? j : 0)));
      }
    }
    const float m_raw = QS ? R.m_run / p.scale_log2 : R.m_run;   // the combine kernel and the LSE work in raw-score units
    if (npiece > 1) {
      const int64_t prow = ((int64_t)((xcd * (p.sk_ix - p.sk_full) + (item_local - p.sk_full)) * npiece + piece)) * QB + wid * 64 + rowoff + lq;
      float* wo = p.ws_o + prow * 64;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 x0, x1;
#pragma unroll
        for (int i = 0; i < 4; ++i) { x0[i] = R.o0[4 * g4 + i]; x1[i] = R.o1[4 * g4 + i]; }
        *(f32x4*)(wo + 8 * g4 + 4 * hi) = x0;
        *(f32x4*)(wo + 32 + 8 * g4 + 4 * hi) = x1;
      }
      if (hi == 0) {
        // an EMPTY piece that does not own the zero-filled suffix stays out of the merge's maximum (QS starts its reference at 0)
        const bool empty_piece = NTILES == 0 && !(nref < p.N && piece == npiece - 1);
        p.ws_ml[prow * 2] = empty_piece ? -INFINITY : m_raw;
        p.ws_ml[prow * 2 + 1] = l_fin;
      }
      return;
    }
    const float inv = 1.0f / l_fin;
    if (qrow < p.Lq) {
      const int64_t ooff = (int64_t)b * p.o_sb + (int64_t)qrow * p.o_sl + (int64_t)h * p.o_sh;
      T* op = (T*)p.out + ooff;
      float* of = (float*)p.out + ooff;   // IR_FLAG_OUT_F32: the result before the 16-bit rounding (strides in fp32 elements)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 x0, x1;
#pragma unroll
        for (int i = 0; i < 4; ++i) { x0[i] = R.o0[4 * g4 + i] * inv; x1[i] = R.o1[4 * g4 + i] * inv; }
        if (p.out_f32) {
          *(f32x4*)(of + 8 * g4 + 4 * hi) = x0;
          *(f32x4*)(of + 32 + 8 * g4 + 4 * hi) = x1;
        } else {
          *(v4*)(op + 8 * g4 + 4 * hi) = __builtin_convertvector(x0, v4);
          *(v4*)(op + 32 + 8 * g4 + 4 * hi) = __builtin_convertvector(x1, v4);
        }
      }
      if (p.lse != nullptr && hi == 0)
        p.lse[((int64_t)b * p.H + h) * p.Lq + qrow] = m_raw * p.scale + __logf(l_fin);
    }
  };
  finish(A, qrowA, 0, lpreA, pzA);
  finish(Bk, qrowB, 32, lpreB, pzB);
}

template <typename T, bool FOLD, int NW = 4, bool QS = false, int ABL = 0, bool MASS = false>
hipError_t launch(const AttnKParams& p0, hipStream_t s) {
  if (!MASS && p0.seg_cum != nullptr) return hipErrorInvalidValue;   // seg_mass: the 8-wave forms carry the MASS instantiation
  constexpr int QB = NW * 64;
  // resident workgroups per CU: 8 waves (two per SIMD at ~256 registers), and the QS form's LDS (K/V ring + NW x 8 KiB of Q)
  constexpr int lds_wg = QS ? (2 * W64_RING * TILE_BYTES + NW * 8192) : (2 * W64_RING * TILE_BYTES);
  constexpr int by_lds = (160 * 1024) / lds_wg, by_waves = 8 / NW;
  const IrAttnPlan pl = ir_attn_plan(ir_attn_plan_in(p0, QB, 32 * (by_lds < by_waves ? by_lds : by_waves)));
  AttnKParams p = p0;
  ir_attn_plan_apply(pl, p);
  size_t dyn_lds = 0;
  if (QS) {
    dyn_lds = (size_t)2 * W64_RING * TILE_BYTES + (size_t)NW * 8192;   // K/V ring + the waves' Q fragments
    static IrOncePerDevice once;   // per instantiation (ir_common.h)
    const hipError_t ea = ir_opt_in_dynamic_lds(once, (const void*)shared_attn_fwd_w64_kernel<T, FOLD, NW, QS, ABL, MASS>, dyn_lds);
    if (ea != hipSuccess) return ea;
  }
  hipLaunchKernelGGL((shared_attn_fwd_w64_kernel<T, FOLD, NW, QS, ABL, MASS>), dim3(pl.grid), dim3(NW * 64), dyn_lds, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || pl.k <= 1) return e;
  return ir_launch_shared_attn_combine(p, std::is_same<T, __bf16>::value ? 1 : 0, QB, pl.rem, s);
}

}  // namespace

template <bool QS, bool MASS>
static hipError_t launch_x8(const AttnKParams& p, int dtype, hipStream_t s) {
  if (p.aa != nullptr) return dtype == 1 ? launch<__bf16, true, 8, QS, 0, MASS>(p, s) : launch<_Float16, true, 8, QS, 0, MASS>(p, s);
  return dtype == 1 ? launch<__bf16, false, 8, QS, 0, MASS>(p, s) : launch<_Float16, false, 8, QS, 0, MASS>(p, s);
}

hipError_t ir_launch_shared_attn_fwd_w64x8(const AttnKParams& p, int dtype, hipStream_t s) {  // 8-wave (512-row) workgroups
  const bool mass = p.seg_cum != nullptr;
  if (p.q_prescaled)   // IR_FLAG_Q_PRESCALED: the QS instantiation
    return mass ? launch_x8<true, true>(p, dtype, s) : launch_x8<true, false>(p, dtype, s);
  return mass ? launch_x8<false, true>(p, dtype, s) : launch_x8<false, false>(p, dtype, s);
}

hipError_t ir_launch_shared_attn_fwd_w64(const AttnKParams& p, int dtype, hipStream_t s) {
  // (round 4: the QS form in 4-wave and in 2-wave workgroups was built and measured for the short query axes - VERDICT r3
  //  item 4 - and loses to the 32-row kernel there, profiles/r4_layer_classes_cfg2.txt; not kept)
  if (p.aa != nullptr) return dtype == 1 ? launch<__bf16, true>(p, s) : launch<_Float16, true>(p, s);
  return dtype == 1 ? launch<__bf16, false>(p, s) : launch<_Float16, false>(p, s);
}

#ifdef IR_ABLATIONS
// energy / timing ablations of the QS form (bf16 / fp16, 8 waves, with or without the fold): tuning values 20 + index
template <typename T, int ABL>
static hipError_t launch_abl(const AttnKParams& p, hipStream_t s) {
  return p.aa != nullptr ? launch<T, true, 8, true, ABL>(p, s) : launch<T, false, 8, true, ABL>(p, s);
}
// ladder (each row ADDS one class to the row before): 63 matrix skeleton | 55 + exponentials | 39 + row sums | 7 + conversions |
// 3 + Q re-reads | (0 = the product kernel: + DMA + barrier); leave-one-out from the product kernel: 8 exponentials, 16 row sums,
// 32 conversions, 4 Q re-reads (3 = DMA + barrier is the ladder's last row)
static const int kW64AblMasks[] = {63, 55, 39, 7, 3, 8, 16, 32, 4};
int ir_w64_abl_count(void) { return (int)(sizeof(kW64AblMasks) / sizeof(kW64AblMasks[0])); }
int ir_w64_abl_mask(int index) { return index >= 0 && index < ir_w64_abl_count() ? kW64AblMasks[index] : -1; }
template <typename T>
static hipError_t launch_abl_t(const AttnKParams& p, int index, hipStream_t s) {
  switch (index) {
    case 0: return launch_abl<T, 63>(p, s);
    case 1: return launch_abl<T, 55>(p, s);
    case 2: return launch_abl<T, 39>(p, s);
    case 3: return launch_abl<T, 7>(p, s);
    case 4: return launch_abl<T, 3>(p, s);
    case 5: return launch_abl<T, 8>(p, s);
    case 6: return launch_abl<T, 16>(p, s);
    case 7: return launch_abl<T, 32>(p, s);
    case 8: return launch_abl<T, 4>(p, s);
    default: return hipErrorInvalidValue;
  }
}
hipError_t ir_launch_shared_attn_fwd_w64_abl(const AttnKParams& p, int dtype, int index, hipStream_t s) {
  if (!p.q_prescaled) return hipErrorInvalidValue;
  return dtype == 1 ? launch_abl_t<__bf16>(p, index, s) : launch_abl_t<_Float16>(p, index, s);
}
#endif
