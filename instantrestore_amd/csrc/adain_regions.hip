// adain_regions.hip - per-REGION AdaIN: token statistics per label in one pass, and an apply whose affine is chosen per token (gfx950).
//
// Token t of matrix (b, m) carries an int32 label.  ir_token_stats_labelled gives, for every region r < R, the mean and the unbiased
// deviation over the tokens with label == r: what ir_token_stats_weighted gives with the fp32 weights (label == r), for all r,
// while x is read ONCE (R weighted calls read it R times).  ir_adain_apply_labelled is ir_adain_apply with the affine slot picked
// by the token's label (slot R for a token of no region).
//
// Statistics: the work split of token_stats_weighted_partial_kernel - ROWS-token chunks, 32 row slots x 8 sixteen-byte column
// slots, 8 rows per thread, all loads issued first.  The regions the chunk carries are then walked AROUND the rows held in
// registers, RG to a round (one merging wave each): the region index is uniform over the workgroup, so no register is indexed
// dynamically.  Per region the thread forms the weighted kernel's shifted sums under `row < end && label == r`; with w == 1 its
// fma(w, d, s1), fma(w * d, d, s2) and cnt += w are s1 + d, fma(d, d, s2) and cnt + 1 bit for bit, and "the first counted token is
// the shift" is the same rule.  The 32 row slots are merged with the same chan_merge in the same order, then the chunks in
// ascending order: the outputs are the bytes of the weighted pass.
// A region that no token of the chunk carries is skipped: its partial is the (n, mean, M2) = (0, 0, 0) the sums would give, and
// chan_merge ignores a partial of n == 0 - so only n is stored for it.  W2 (the sum of squared weights) is W for 0/1 weights and
// is not carried: W - W2 / W is W - 1 exactly.
// A token whose label lies outside [0, R) matches no r: its bytes never enter an operation (NaN / Inf there are inert).
// The order of evaluation is a function of `len` and R alone.  No atomics, one writer per output.
#include "ir_common.h"
#include "ir_kernels.h"
#include "ir_adain_math.h"

namespace {

constexpr int ROWS = IR_ADAIN_ROWS;       // token rows per workgroup
constexpr int AT = 256;                   // threads: 32 row slots x 8 sixteen-byte column slots
constexpr int WS = IR_ADAIN_W_STRIDE;     // floats per (matrix, region, head, chunk) partial: mean[64] | M2[64] | n, pad

// Regions merged at a time, one wave of the workgroup each (<= AT / 64).  Measured at cfg 2's classes (profiles/adain_regions_ab.txt):
// one region a round leaves three waves idle through the 32 dependent chan_merge steps of every region; four a round need 68 KiB
// of LDS, two workgroups a CU, and the reference passes (the bulk of the bytes) lose more on the loads than they win on the
// merges; two a round keep four workgroups a CU (35 KiB each, the limit the registers set anyway).
constexpr int RG = 2;

// grid: (nchunk, H, B*M); one workgroup reduces ROWS tokens of one head of one matrix, for every region.
template <typename T>
__global__ void __launch_bounds__(AT) token_stats_regions_partial_kernel(const TokenStatsRKParams p) {
  using v8 = typename ElemTraits<T>::v8;
  __shared__ float red[RG][32][8][17];  // [region of the round][row slot][col slot][n, mean[8], m2[8]]
  __shared__ unsigned seen[AT / 64];

  const int mat = blockIdx.z;
  const int h = blockIdx.y;
  const int chunk = blockIdx.x;
  const int b = mat / p.M;
  const int m = mat - b * p.M;
  const T* base = (const T*)p.x + (int64_t)b * p.x_sb + (int64_t)m * p.x_sn + (int64_t)h * p.x_sh;
  const int32_t* lrow = p.labels + (int64_t)b * p.lb_sb + (int64_t)m * p.lb_sn;
  const int r_begin = chunk * ROWS;
  const int r_end = (r_begin + ROWS < p.len) ? r_begin + ROWS : p.len;

  const int tid = threadIdx.x;
  const int slot = tid & 7;
  const int rs = tid >> 3;
  const int wave = tid >> 6;

  constexpr int PER = ROWS / 32;
  v8 xs[PER];
  int lab[PER];
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int r = r_begin + rs + it * 32;
    // rows at or behind r_end re-read the last row of the chunk and are selected away below: every address stays inside the
    // `len` rows of x and the `len` ints of the label row (chunk < nchunk = ceil(len / ROWS): r_begin < len, r_end >= 1)
    const int rc = r < r_end ? r : r_end - 1;
    xs[it] = *(const v8*)(base + (int64_t)rc * p.x_sl + slot * 8);
    lab[it] = lrow[rc];
  }
  // which regions this wave / this workgroup holds at all (labels < 32: one bit each); -1 marks a row that does not count
  unsigned mine = 0u;
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const bool counts = (r_begin + rs + it * 32 < r_end) && (unsigned)lab[it] < (unsigned)p.R;
    lab[it] = counts ? lab[it] : -1;
    mine |= counts ? (1u << (lab[it] & 31)) : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mine |= (unsigned)__shfl_xor((int)mine, o, 64);
  mine = (unsigned)__builtin_amdgcn_readfirstlane((int)mine);      // the same in every lane after the butterfly
  if ((tid & 63) == 0) seen[wave] = mine;
  __syncthreads();
  const unsigned any = (unsigned)__builtin_amdgcn_readfirstlane((int)(seen[0] | seen[1] | seen[2] | seen[3]));

  float* ws0 = p.ws + ((((int64_t)mat * p.R) * p.H + h) * p.nchunk + chunk) * WS;    // region r: + r * rstride
  const int64_t rstride = (int64_t)p.H * p.nchunk * WS;
  // a region no token of the chunk carries: n == 0 alone (chan_merge ignores the partial)
  if (tid < p.R && ((any >> tid) & 1u) == 0u) ws0[tid * rstride + 128] = 0.f;

  // the regions the chunk does carry, RG at a time: every thread forms the round's sums, then wave j merges region j of the round
  // (the 32 dependent chan_merge steps of a region are the long pole of this kernel: RG of them run side by side)
  for (unsigned todo = any; todo != 0u;) {      // uniform over the workgroup: no barrier is skipped by a part of it
    int rr[RG];
#pragma unroll
    for (int j = 0; j < RG; ++j) {
      rr[j] = todo != 0u ? __builtin_ctz(todo) : -1;
      todo &= todo - 1u;
    }
#pragma unroll
    for (int j = 0; j < RG; ++j) {
      const int r = rr[j];
      if (r < 0) continue;
      // shifted single-pass sums: K = first value this thread counts (kills cancellation)
      float cnt = 0.f, K[8], s1[8], s2[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { K[i] = 0.f; s1[i] = 0.f; s2[i] = 0.f; }
      if ((mine >> r) & 1u) {          // uniform over the wave
#pragma unroll
        for (int it = 0; it < PER; ++it) {
          if (lab[it] == r) {
            const f32x8 f = __builtin_convertvector(xs[it], f32x8);
            if (cnt == 0.f) {
#pragma unroll
              for (int i = 0; i < 8; ++i) K[i] = f[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const float d = f[i] - K[i];
              s1[i] += d;
              s2[i] = __builtin_fmaf(d, d, s2[i]);
            }
            cnt += 1.f;
          }
        }
      }
      float* o = &red[j][rs][slot][0];
      o[0] = cnt;
      const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        o[1 + i] = K[i] + s1[i] * inv;
        o[9 + i] = s2[i] - s1[i] * s1[i] * inv;
      }
    }
    __syncthreads();
    int r_me = -1;
#pragma unroll
    for (int j = 0; j < RG; ++j) r_me = wave == j ? rr[j] : r_me;
    if (r_me >= 0) {  // one thread per channel merges the 32 row-slot partials of this wave's region
      const int lane = tid & 63, cs = lane >> 3, ci = lane & 7;
      float n = 0.f, mean = 0.f, m2 = 0.f;
      for (int k = 0; k < 32; ++k) {
        const float* o = &red[wave < RG ? wave : 0][k][cs][0];
        chan_merge(n, mean, m2, o[0], o[1 + ci], o[9 + ci]);
      }
      float* wsp = ws0 + r_me * rstride;
      wsp[lane] = mean;
      wsp[64 + lane] = m2;
      if (lane == 0) wsp[128] = n;   // the same for every channel: the labels do not depend on it
    }
    __syncthreads();                // red is written again in the next round
  }
}

// grid: (B*M*R*H); 64 threads = channels.  Merges the chunk partials in ascending order, emits mean / std (and the count once per
// (matrix, region)): token_stats_weighted_finalize_kernel with W2 == W.
__global__ void __launch_bounds__(64) token_stats_regions_finalize_kernel(const TokenStatsRKParams p) {
  const int d = threadIdx.x;
  int idx = blockIdx.x;
  const int h = idx % p.H; idx /= p.H;
  const int r = idx % p.R;
  const int mat = idx / p.R;
  const int b = mat / p.M, m = mat - b * p.M;
  const int nch = (p.len + ROWS - 1) / ROWS;
  const float* w = p.ws + ((((int64_t)mat * p.R + r) * p.H + h) * p.nchunk) * WS;
  float W = 0.f, mean = 0.f, m2 = 0.f;
  // eight chunks' partials in flight at once, then merged in ascending order.  A chunk without the region stored n == 0 alone:
  // its mean / M2 words are whatever the workspace held, loaded and never used (chan_merge returns on n == 0)
  constexpr int G = 8;
  for (int c0 = 0; c0 < nch; c0 += G) {
    float cn[G], cm[G], cq[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int c = c0 + i < nch ? c0 + i : nch - 1;
      cn[i] = w[c * WS + 128]; cm[i] = w[c * WS + d]; cq[i] = w[c * WS + 64 + d];
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      if (c0 + i < nch) chan_merge(W, mean, m2, cn[i], cm[i], cq[i]);
    }
  }
  // W == 0: an empty region - (0, 0).  W == 1: one token - its value, deviation 0.  W - W2 / W of the weighted pass is W - 1 here.
  const float den = W > 0.f ? W - 1.f : 0.f;
  const int64_t om = ((int64_t)b * p.R + r) * p.M + m;                 // region-major: (B, R, M[, H, 64])
  const int64_t o = (om * p.H + h) * 64 + d;
  p.mean[o] = mean;
  p.std[o] = (den > 0.f && m2 > 0.f) ? sqrtf(m2 / den) : 0.f;
  if (p.count != nullptr && h == 0 && d == 0) p.count[om] = W;
}

// y = fma(x, a[slot of the token], b[slot of the token]) over (B, N, L, H, 64).  A work item is one token and a group of up to four
// heads: its 8 threads (the sixteen-byte column slots) read the token's label once and hold the group's four 16-byte pieces in flight;
// grid-stride over the B*N*L*ceil(H / 4) items.  (A first version walked ALL heads of a token in one item: B*N*L / 32 workgroups
// are one per CU at the 256-token class, and the pass sat 1.8 ... 4.6 us behind ir_adain_apply, whose grid is per head row.)
template <typename T>
__global__ void __launch_bounds__(256) adain_apply_regions_kernel(const AdainApplyRKParams p) {
  using v8 = typename ElemTraits<T>::v8;
  const int slot = threadIdx.x & 7;
  const int hg = (p.H + 3) >> 2;
  const int64_t items = (int64_t)p.B * p.N * p.L * hg;
  for (int64_t item = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3); item < items; item += (int64_t)gridDim.x * 32) {
    int64_t t = item;
    const int h0 = (int)(t % hg) * 4; t /= hg;
    const int l = (int)(t % p.L); t /= p.L;
    const int n = (int)(t % p.N);
    const int b = (int)(t / p.N);
    const int lab = p.labels[(int64_t)b * p.lb_sb + (int64_t)n * p.lb_sn + l];
    const int s = (unsigned)lab < (unsigned)p.R ? lab : p.R;
    const T* x = (const T*)p.x + (int64_t)b * p.x_sb + (int64_t)n * p.x_sn + (int64_t)l * p.x_sl + slot * 8;
    T* y = (T*)p.y + (int64_t)b * p.y_sb + (int64_t)n * p.y_sn + (int64_t)l * p.y_sl + slot * 8;
    const int64_t ao = ((((int64_t)b * p.N + n) * (p.R + 1) + s) * p.H) * 64 + slot * 8;
    v8 xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int h = h0 + j < p.H ? h0 + j : p.H - 1;
      xs[j] = *(const v8*)(x + (int64_t)h * p.x_sh);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (h0 + j < p.H) {
        const int h = h0 + j;
        const float* a = p.a + ao + (int64_t)h * 64;
        const float* bb = p.b + ao + (int64_t)h * 64;
        f32x8 f = __builtin_convertvector(xs[j], f32x8);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = __builtin_fmaf(f[i], a[i], bb[i]);
        *(v8*)(y + (int64_t)h * p.y_sh) = __builtin_convertvector(f, v8);
      }
    }
  }
}

}  // namespace

hipError_t ir_launch_token_stats_regions(const TokenStatsRKParams& p, int dtype, hipStream_t s) {
  const dim3 grid(p.nchunk, p.H, p.B * p.M);
  if (dtype == 1) hipLaunchKernelGGL((token_stats_regions_partial_kernel<__bf16>), grid, dim3(AT), 0, s, p);
  else hipLaunchKernelGGL((token_stats_regions_partial_kernel<_Float16>), grid, dim3(AT), 0, s, p);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(token_stats_regions_finalize_kernel, dim3((unsigned)((int64_t)p.B * p.M * p.R * p.H)), dim3(64), 0, s, p);
  return hipGetLastError();
}

hipError_t ir_launch_adain_apply_regions(const AdainApplyRKParams& p, int dtype, hipStream_t s) {
  const int64_t items = (int64_t)p.B * p.N * p.L * ((p.H + 3) / 4);
  int64_t blocks = (items + 31) / 32;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  if (dtype == 1) hipLaunchKernelGGL((adain_apply_regions_kernel<__bf16>), dim3((unsigned)blocks), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((adain_apply_regions_kernel<_Float16>), dim3((unsigned)blocks), dim3(256), 0, s, p);
  return hipGetLastError();
}
