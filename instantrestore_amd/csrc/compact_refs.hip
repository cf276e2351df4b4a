// compact_refs.hip - stable stream compaction of reference K/V token rows (gfx950).
//
// ir_compact_ref_tokens: for every (batch entry b, reference n) the rows t of K and V with keep[b, n, t] != 0 move, in their order,
// to rows 0 .. c-1 of the output segment, and ref_lens[b, n] = c.  Rows behind the count are not written.  What the counted
// attention call (ir_shared_attn_ragged_args.ref_lens) then walks is c keys instead of len_ref keys under a mask.
//
// One launch, no host sync, no atomics, deterministic: workgroup (b * N + n, y) scans the mask bytes of its reference in chunks of
// 256 tokens (wave ballots + a 4-entry LDS exchange), keeps the chunk's kept source rows as a list in LDS, and copies the 16-byte
// pieces of the head rows it owns (heads h = y, y + gridDim.y, ...: every workgroup of a reference repeats the cheap scan instead
// of waiting for another one's result).  Workgroup y == 0 stores the count.
#include "ir_kernels.h"

namespace {

constexpr int kChunk = 256;   // tokens per scan step = threads per workgroup

__global__ void __launch_bounds__(kChunk) compact_refs_kernel(const CompactRefsKParams p) {
  __shared__ int wave_cnt[kChunk / 64];
  __shared__ int src_row[kChunk];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int bn = blockIdx.x;
  const int b = bn / p.N, n = bn - b * p.N;
  const uint8_t* keep = p.keep + (int64_t)bn * p.L;
  const char* ki = (const char*)p.k_in + ((int64_t)b * p.ki_sb + (int64_t)n * p.ki_sn) * 2;
  const char* vi = (const char*)p.v_in + ((int64_t)b * p.vi_sb + (int64_t)n * p.vi_sn) * 2;
  char* ko = (char*)p.k_out + ((int64_t)b * p.ko_sb + (int64_t)n * p.ko_sn) * 2;
  char* vo = (char*)p.v_out + ((int64_t)b * p.vo_sb + (int64_t)n * p.vo_sn) * 2;
  const int nh = (p.H - (int)blockIdx.y + (int)gridDim.y - 1) / (int)gridDim.y;   // heads of this workgroup
  int done = 0;                                                                   // kept rows before this chunk
  for (int t0 = 0; t0 < p.L; t0 += kChunk) {
    const int t = t0 + tid;
    const bool k = t < p.L && keep[t] != 0;
    const unsigned long long bal = __ballot(k);
    if (lane == 0) wave_cnt[wid] = __popcll(bal);
    __syncthreads();
    int before = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < kChunk / 64; ++w) {
      const int c = wave_cnt[w];
      if (w < wid) before += c;
      total += c;
    }
    if (k) src_row[before] = t;
    __syncthreads();
    // 16-byte pieces of this chunk's kept rows: (row r, head j of this workgroup, slot) - eight consecutive threads copy one head row
    const int pieces = total * nh * 8;
    for (int i = tid; i < pieces; i += kChunk) {
      const int slot = i & 7, rj = i >> 3;
      const int r = rj / nh, h = (int)blockIdx.y + (rj - r * nh) * (int)gridDim.y;
      const int64_t s = src_row[r], d = done + r;
      const uint4 kx = *(const uint4*)(ki + (s * p.ki_sl + (int64_t)h * p.ki_sh) * 2 + slot * 16);
      const uint4 vx = *(const uint4*)(vi + (s * p.vi_sl + (int64_t)h * p.vi_sh) * 2 + slot * 16);
      *(uint4*)(ko + (d * p.ko_sl + (int64_t)h * p.ko_sh) * 2 + slot * 16) = kx;
      *(uint4*)(vo + (d * p.vo_sl + (int64_t)h * p.vo_sh) * 2 + slot * 16) = vx;
    }
    done += total;
    __syncthreads();   // src_row and wave_cnt are rewritten by the next chunk
  }
  if (blockIdx.y == 0 && tid == 0) p.ref_lens[(int64_t)b * p.rl_sb + n] = done;
}

}  // namespace

hipError_t ir_launch_compact_refs(const CompactRefsKParams& p, hipStream_t s) {
  const int gy = p.H < 8 ? p.H : 8;
  hipLaunchKernelGGL(compact_refs_kernel, dim3((unsigned)(p.B * p.N), (unsigned)gy), dim3(kChunk), 0, s, p);
  return hipGetLastError();
}
