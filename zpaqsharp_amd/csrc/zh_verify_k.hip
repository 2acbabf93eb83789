// zh_verify_k.hip — the result side of the verify pass (zh_verify.h): where what the post-processor wrote first differs from
// the plaintext.  A workgroup takes a block at a time from a device-scope queue and walks both byte ranges where they lie,
// 4 KiB a round: every lane loads one aligned 16-byte group of each (the host places the post-processor's output on the
// plaintext's alignment, so the groups pair up), masks the bytes outside the ranges and reports its first differing byte;
// the round's minimum ends the walk.  An aligned load touches only groups that hold a byte of its range (zh_frame.hip's
// rule).  Two ranges on different alignments, which the library itself never makes, are compared a byte per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zh_verify.h"

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// the first byte position p in [0, n) of group g (its byte 0 is position 16 g - ph) at which x is not zero, relative to the
// round (16 per lane); kNone when there is none
__device__ __forceinline__ uint32_t first_set(const uint4 x, uint64_t g, uint32_t ph, uint64_t n, uint32_t slot) {
  if (!(x.x | x.y | x.z | x.w)) return kNone;
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
  for (uint32_t k = 0; k < 16; ++k) {
    if (!((w[k >> 2] >> (8 * (k & 3))) & 255u)) continue;
    const uint64_t at = 16 * g + k;                      // position + ph
    if (at >= ph && at - ph < n) return 16 * slot + k;
  }
  return kNone;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void zh_verify_compare(const uint8_t *A, const uint8_t *B, const ZhVerifyCmp *blocks, uint32_t n_blocks,
                                                                    uint32_t *queue, uint64_t *first_diff) {
  __shared__ uint32_t s_bi, s_min;
  const uint32_t t = threadIdx.x;
  for (;;) {
    __syncthreads();
    if (t == 0) { s_bi = atomicAdd(queue, 1u); s_min = kNone; }
    __syncthreads();
    const uint32_t bi = s_bi;
    if (bi >= n_blocks) break;                          // every wave reaches this exit
    const ZhVerifyCmp c = blocks[bi];
    const uint8_t *pa = A + c.a_off, *pb = B + c.b_off;
    const uint64_t n = c.a_len < c.b_len ? c.a_len : c.b_len;
    uint64_t diff = c.a_len != c.b_len ? n : ~0ull;      // one is a prefix of the other: the shorter length
    if ((((uintptr_t)pa ^ (uintptr_t)pb) & 15) == 0) {
      const uint32_t ph = (uint32_t)((uintptr_t)pa & 15);
      const uint4 *qa = reinterpret_cast<const uint4 *>(pa - ph), *qb = reinterpret_cast<const uint4 *>(pb - ph);
      const uint64_t ng = n ? (ph + n + 15) >> 4 : 0;
      for (uint64_t base = 0; base < ng; base += kThreads) {
        const uint64_t g = base + t;
        uint32_t loc = kNone;
        if (g < ng) {
          const uint4 a = qa[g], b = qb[g];
          loc = first_set(make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w), g, ph, n, t);
        }
        if (loc != kNone) atomicMin(&s_min, loc);
        __syncthreads();
        const uint32_t m = s_min;
        __syncthreads();                                 // (before a lane of the next round writes it)
        if (m != kNone) { diff = 16 * base + m - ph; break; }
      }
    } else {
      for (uint64_t base = 0; base < n; base += kThreads) {
        const uint64_t i = base + t;
        if (i < n && pa[i] != pb[i]) atomicMin(&s_min, t);
        __syncthreads();
        const uint32_t m = s_min;
        __syncthreads();
        if (m != kNone) { diff = base + m; break; }
      }
    }
    if (t == 0) first_diff[bi] = diff;
  }
}

extern "C" hipError_t zh_launch_verify_compare(const uint8_t *A, const uint8_t *B, const ZhVerifyCmp *blocks, uint32_t n_blocks, uint32_t *queue,
                                               uint64_t *first_diff, hipStream_t stream) {
  if (n_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(zh_verify_compare, dim3(n_blocks < 1024u ? n_blocks : 1024u), dim3(kThreads), 0, stream, A, B, blocks, n_blocks, queue, first_diff);
  return hipGetLastError();
}
