// adain_weighted.hip - token statistics over WEIGHTED or COUNTED tokens, and the AdaIN affine from finished statistics (gfx950).
//
// The statistics of adain.hip reduce a whole token axis with weight 1.  Here token t of matrix (b, m) carries
//     w_t = (t < c[b, m]) ? w[b, m, t] : 0
// and the outputs are the weighted mean and the unbiased deviation under reliability weights:
//     W = sum w_t,  W2 = sum w_t^2,  mean = sum w_t x_t / W,  M2 = sum w_t (x_t - mean)^2,  std = sqrt(M2 / (W - W2 / W)).
// For 0/1 weights W - W2 / W = count - 1: the statistics of the kept tokens alone.
//
// Same work split as adain_partial_kernel: ROWS-token chunks, 32 row slots x 8 sixteen-byte column slots, the shifted
// single-pass sums per thread, Chan's merge over the 32 row slots and then over the chunks in ascending order.  With w == 1
// fma(w, d, s1) == s1 + d and fma(w * d, d, s2) == fma(d, d, s2), every W is an exact integer and W - W2 / W == len - 1: the
// bytes of ir_token_stats.  The order of evaluation is a function of `len` alone (the counts and weights only select).
// A token with w_t == 0 is SELECTED away (its bytes never enter an operation), so NaN / Inf there and behind a count are inert.
#include "ir_common.h"
#include "ir_kernels.h"
#include "ir_adain_math.h"

namespace {

constexpr int ROWS = IR_ADAIN_ROWS;       // token rows per workgroup
constexpr int AT = 256;                   // threads: 32 row slots x 8 sixteen-byte column slots
constexpr int WS = IR_ADAIN_W_STRIDE;     // floats per (matrix, head, chunk) partial: mean[64] | M2[64] | W, W2, pad

__device__ __forceinline__ int effective_len(const TokenStatsWKParams& p, int b, int m) {
  if (p.lens == nullptr) return p.len;
  const int c = p.lens[(int64_t)b * p.ln_sb + m];
  return c < 0 ? 0 : (c > p.len ? p.len : c);
}

// grid: (nchunk, H, B*M); one workgroup reduces ROWS tokens of one head of one matrix.
template <typename T>
__global__ void __launch_bounds__(AT) token_stats_weighted_partial_kernel(const TokenStatsWKParams p) {
  using v8 = typename ElemTraits<T>::v8;
  __shared__ float red[32][8][18];  // [row slot][col slot][W, mean[8], m2[8], W2]

  const int mat = blockIdx.z;
  const int h = blockIdx.y;
  const int chunk = blockIdx.x;
  const int b = mat / p.M;
  const int m = mat - b * p.M;
  const T* base = (const T*)p.x + (int64_t)b * p.x_sb + (int64_t)m * p.x_sn + (int64_t)h * p.x_sh;
  const float* wrow = p.weights != nullptr ? p.weights + (int64_t)b * p.w_sb + (int64_t)m * p.w_sn : nullptr;
  const int len = effective_len(p, b, m);
  const int r_begin = chunk * ROWS;
  const int r_end = (r_begin + ROWS < len) ? r_begin + ROWS : len;   // <= r_begin: nothing of this chunk counts
  float* wsp = p.ws + (((int64_t)mat * p.H + h) * p.nchunk + chunk) * WS;

  const int tid = threadIdx.x;
  const int slot = tid & 7;
  const int rs = tid >> 3;

  // shifted single-pass sums: K = first value this thread counts (kills cancellation)
  float cnt = 0.f, cnt2 = 0.f, K[8], s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { K[i] = 0.f; s1[i] = 0.f; s2[i] = 0.f; }
  constexpr int PER = ROWS / 32;
  v8 xs[PER];
  float wt[PER];
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int r = r_begin + rs + it * 32;
    // rows at or behind r_end re-read the last counted row (row 0 of an empty matrix: len >= 1 rows and floats exist) and are
    // selected away below: every address stays inside the `len` rows of x and the `len` floats of the weights row
    const int rc = r < r_end ? r : (r_end - 1 > 0 ? r_end - 1 : 0);
    xs[it] = *(const v8*)(base + (int64_t)rc * p.x_sl + slot * 8);
    wt[it] = wrow != nullptr ? wrow[rc] : 1.f;
  }
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int r = r_begin + rs + it * 32;
    const float w = wt[it];
    if (r < r_end && w > 0.f) {
      const f32x8 f = __builtin_convertvector(xs[it], f32x8);
      if (cnt == 0.f) {
#pragma unroll
        for (int i = 0; i < 8; ++i) K[i] = f[i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = f[i] - K[i];
        s1[i] = __builtin_fmaf(w, d, s1[i]);
        s2[i] = __builtin_fmaf(w * d, d, s2[i]);
      }
      cnt += w;
      cnt2 = __builtin_fmaf(w, w, cnt2);
    }
  }
  {
    float* o = &red[rs][slot][0];
    o[0] = cnt;
    o[17] = cnt2;
    const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o[1 + i] = K[i] + s1[i] * inv;
      o[9 + i] = s2[i] - s1[i] * s1[i] * inv;
    }
  }
  __syncthreads();
  if (tid < 64) {  // one thread per channel merges the 32 row-slot partials
    const int cs = tid >> 3, ci = tid & 7;
    float n = 0.f, n2 = 0.f, mean = 0.f, m2 = 0.f;
    for (int k = 0; k < 32; ++k) {
      const float* o = &red[k][cs][0];
      chan_merge(n, mean, m2, o[0], o[1 + ci], o[9 + ci]);
      n2 += o[17];
    }
    wsp[tid] = mean;
    wsp[64 + tid] = m2;
    if (tid == 0) { wsp[128] = n; wsp[129] = n2; }   // the same for every channel: the weights do not depend on it
  }
}

// grid: (B*M*H); 64 threads = channels.  Merges the chunk partials in ascending order, emits mean / std (and W once per matrix).
__global__ void __launch_bounds__(64) token_stats_weighted_finalize_kernel(const TokenStatsWKParams p) {
  const int d = threadIdx.x;
  const int h = blockIdx.x % p.H;
  const int mat = blockIdx.x / p.H;
  const int nch = (p.len + ROWS - 1) / ROWS;
  const float* w = p.ws + (((int64_t)mat * p.H + h) * p.nchunk) * WS;
  float W = 0.f, W2 = 0.f, mean = 0.f, m2 = 0.f;
  // eight chunks' partials in flight at once, then merged in ascending order: chan_merge branches on the chunk's W, which is
  // loaded here (token_stats_finalize_kernel computes it from len), and a merge per load would wait a memory latency per chunk
  constexpr int G = 8;
  for (int c0 = 0; c0 < nch; c0 += G) {
    float cn[G], cm[G], cq[G], c2[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int c = c0 + i < nch ? c0 + i : nch - 1;
      cn[i] = w[c * WS + 128]; cm[i] = w[c * WS + d]; cq[i] = w[c * WS + 64 + d]; c2[i] = w[c * WS + 129];
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      if (c0 + i < nch) {
        chan_merge(W, mean, m2, cn[i], cm[i], cq[i]);
        W2 += c2[i];
      }
    }
  }
  // W == 0: no token counts - (0, 0), the statistics of a zero-filled reference (chan_merge never ran: mean is still 0).
  // W - W2 / W <= 0: one effective token - its value, deviation 0.  With unit weights W2 / W == 1 exactly and the divisor is
  // (float)(len - 1), the one of token_stats_finalize_kernel.
  const float den = W > 0.f ? W - W2 / W : 0.f;
  const int64_t o = ((int64_t)mat * p.H + h) * 64 + d;
  p.mean[o] = mean;
  p.std[o] = (den > 0.f && m2 > 0.f) ? sqrtf(m2 / den) : 0.f;
  if (p.wsum != nullptr && h == 0 && d == 0) p.wsum[mat] = W;
}

// a = adain_scale(style_std + eps, content_std + eps, content_std == 0), b = style_mean - content_mean * a: the expression of
// adain_finalize_cached_kernel on finished statistics.  One thread per (b, n, h, channel).
__global__ void __launch_bounds__(256) adain_affine_from_stats_kernel(const float* __restrict__ smean, const float* __restrict__ sstd,
                                                                      const float* __restrict__ cmean, const float* __restrict__ cstd,
                                                                      float eps, float* __restrict__ a_out, float* __restrict__ b_out,
                                                                      int N, int H, int64_t total) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;   // ((b * N + n) * H + h) * 64 + d
  if (o >= total) return;
  const int64_t hd = o % ((int64_t)H * 64);
  const int64_t b = o / ((int64_t)H * 64) / N;
  const int64_t so = b * H * 64 + hd;                          // (b * H + h) * 64 + d
  const float sd_v = sstd[so] + eps;
  const float sd_x = cstd[o] + eps;
  const float a = adain_scale(sd_v, sd_x, cstd[o] == 0.f);
  a_out[o] = a;
  b_out[o] = smean[so] - cmean[o] * a;
}

}  // namespace

hipError_t ir_launch_token_stats_weighted(const TokenStatsWKParams& p, int dtype, hipStream_t s) {
  const dim3 grid(p.nchunk, p.H, p.B * p.M);
  if (dtype == 1) hipLaunchKernelGGL((token_stats_weighted_partial_kernel<__bf16>), grid, dim3(AT), 0, s, p);
  else hipLaunchKernelGGL((token_stats_weighted_partial_kernel<_Float16>), grid, dim3(AT), 0, s, p);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(token_stats_weighted_finalize_kernel, dim3(p.B * p.M * p.H), dim3(64), 0, s, p);
  return hipGetLastError();
}

hipError_t ir_launch_adain_affine_from_stats(const float* smean, const float* sstd, const float* cmean, const float* cstd, float eps,
                                             float* a, float* b, int B, int N, int H, hipStream_t s) {
  const int64_t total = (int64_t)B * N * H * 64;
  hipLaunchKernelGGL(adain_affine_from_stats_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, smean, sstd, cmean, cstd, eps,
                     a, b, N, H, total);
  return hipGetLastError();
}
