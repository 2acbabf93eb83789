// zh_analyze.hip — the data analysis of LibZPAQ.compressBlock's levels 5..9 on the GPU (LibZPAQ.cs:242-255): the histogram
// of repetition gaps.  With pt[256] and r[4096] all zero,
//
//     for i in 0..n-1:  k = i - pt[p[i]];  if 0 < k < 4096: ++r[k];  pt[p[i]] = i
//
// The walk depends on itself only through pt, and a gap is counted only below 4096.  A walk that starts at w0 = s - 4096 with
// a zero table and counts nothing before s has, from s on, the same pt wherever the true previous occurrence lies less than
// 4096 back; where it lies further back (or does not exist) the table says "at w0 or never", a gap of 4096 or more, which
// the reference does not count either.  For s <= 4096 the walk starts at position 0 with the reference's own zero table and
// reproduces its first-occurrence rule (a value first seen at i < 4096 counts as gap i).  So a block is cut into slices of
// ZH_GAP_SLICE bytes that need nothing from each other.
//
//   zh_gap_hist   one lane per slice, 64 slices per workgroup (one wave).  A lane keeps its pt as 256 16-bit positions
//                 relative to w0 (the walk is at most ZH_GAP_SLICE + 4096 < 65536 bytes long) in LDS at pt[value * 64 +
//                 lane]: the bank is (value & 1) * 32 + lane / 2, so a step of the wave meets two-way conflicts at most.
//                 Gaps are added to the workgroup's 4096 32-bit counters with LDS atomics, except gap 1, which a run of one
//                 value would pile onto a single address: it is counted in a register.  At the end the non-zero counters
//                 go to the block's 4096 counters in global memory with vector atomics.
//
// Every store is a plain C++ store or an atomicAdd on LDS or global memory; every counter is 32 bits wide (a block holds
// fewer than 2^31 bytes).
#include <hip/hip_runtime.h>

#include "zh_analyze.h"

__global__ __launch_bounds__(64) void zh_gap_hist(ZhGapLaunch L) {
  __shared__ uint16_t pt[256 * 64];
  __shared__ uint32_t h[ZH_GAP_NR];
  const uint32_t lane = threadIdx.x;
  const uint64_t off = L.in_off[blockIdx.y] - L.base;
  const uint32_t n = (uint32_t)(L.in_off[blockIdx.y + 1] - L.in_off[blockIdx.y]);
  const uint64_t first = (uint64_t)blockIdx.x * 64 * ZH_GAP_SLICE;   // first byte of this workgroup's 64 slices
  if (first >= n) return;                                            // the grid is sized for the longest block
  for (uint32_t k = lane; k < 256 * 64 / 2; k += 64) ((uint32_t *)pt)[k] = 0;
  for (uint32_t k = lane; k < ZH_GAP_NR; k += 64) h[k] = 0;
  __syncthreads();

  const uint64_t s64 = first + (uint64_t)lane * ZH_GAP_SLICE;
  if (s64 < n) {
    const uint32_t s = (uint32_t)s64;
    const ZhGapSlice c = zh_gap_slice(n, s);
    const uint32_t len = c.e - c.w0, from = s - c.w0;                // the walk; its first counted position
    // 16 bytes per load, aligned on the address itself (the input may be the caller's memory, of any alignment); the bytes
    // in front of w0 and behind e are skipped, and no group without a byte of the walk is loaded (zh_analyze.h)
    const ZhGapFirst f = zh_gap_first_load((uint64_t)(uintptr_t)(L.in + off), c.w0);
    int64_t r0 = f.r0;                                               // walk position of the first byte of the load
    const uint4 *src = (const uint4 *)(uintptr_t)f.addr;
    uint16_t *mine = pt + lane;
    uint32_t ones = 0;
    uint4 next = *src;
    while (r0 < (int64_t)len) {
      const uint4 cur = next;
      if (zh_gap_load_next(r0, len)) next = *++src;
      const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const uint32_t r = (uint32_t)(r0 + t);                       // negative in front of w0: wraps far above len
        if (r < len) {
          const uint32_t v = (w[t >> 2] >> (8 * (t & 3))) & 255u;
          const uint32_t k = r - mine[v * 64];
          mine[v * 64] = (uint16_t)r;
          if (r >= from) {
            if (k == 1) ++ones;
            else if (k > 0 && k < ZH_GAP_NR) atomicAdd(&h[k], 1u);
          }
        }
      }
      r0 += 16;
    }
    if (ones) atomicAdd(&h[1], ones);
  }
  __syncthreads();
  uint32_t *out = L.hist + (uint64_t)blockIdx.y * ZH_GAP_NR;
  for (uint32_t k = lane; k < ZH_GAP_NR; k += 64)
    if (h[k]) atomicAdd(&out[k], h[k]);
}

extern "C" hipError_t zh_launch_gap_hist(const ZhGapLaunch *L, uint32_t n_blocks, uint64_t max_n, hipStream_t stream) {
  const uint64_t groups = (max_n + 64ull * ZH_GAP_SLICE - 1) / (64ull * ZH_GAP_SLICE);
  if (!n_blocks || !groups) return hipSuccess;
  hipLaunchKernelGGL(zh_gap_hist, dim3((uint32_t)groups, n_blocks), dim3(64), 0, stream, *L);
  return hipGetLastError();
}
