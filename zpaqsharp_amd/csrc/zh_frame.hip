// zh_frame.hip — the packing kernel of the device forms of the compressing entry points: a byte-granular gather of a
// batch's heads, bodies and tails into one contiguous stream (zh_frame.h's table).  Workgroup (x, y) takes every
// gridDim.x-th 64 KiB piece of entry y's body; x == 0 also writes head and tail.  The store layout's chunk is such a
// piece behind its 4-byte big-endian length (zh_frame_table.cpp's write_store_body), so every chunk is copied on its own
// alignment.
//
// Sources are 256-byte aligned slots, destinations are not: a head has any length.  copy_bytes therefore aligns on the
// destination: up to 15 bytes one per lane, then one 16-byte store per lane, each put together from the two aligned 16-byte
// loads that hold its bytes, shifted by the source's misalignment (constant for a copy, so the shift is uniform and picked
// outside the loop), then up to 15 bytes one per lane.  An aligned load touches only 16-byte groups that hold a byte of
// the source.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zh_frame.h"

namespace {

constexpr uint32_t kThreads = 256;

__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t r8) { return (uint32_t)(((uint64_t)hi << 32 | lo) >> r8); }

// bytes [4 Q + r, 4 Q + r + 16) of a || b (little-endian dwords); r8 = 8 r
template <int Q>
__device__ __forceinline__ uint4 splice(const uint4 a, const uint4 b, uint32_t r8) {
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return make_uint4(funnel(w[Q + 1], w[Q], r8), funnel(w[Q + 2], w[Q + 1], r8), funnel(w[Q + 3], w[Q + 2], r8),
                    funnel(w[Q + 4], w[Q + 3], r8));
}

// (Every lane loads s[i] and s[i + 1], so each aligned group is asked for by two neighbouring lanes; the second request
// hits the cache.  A lane shuffle of the neighbour's load would halve the requests if this kernel ever became the limit.)
template <int Q>
__device__ __forceinline__ void copy_shifted(uint4 *d, const uint4 *s, uint64_t nv, uint32_t r8) {
  for (uint64_t i = threadIdx.x; i < nv; i += kThreads) d[i] = splice<Q>(s[i], s[i + 1], r8);
}

// dst[0, n) = src[0, n) by the whole workgroup; any alignment of either
__device__ void copy_bytes(uint8_t *dst, const uint8_t *src, uint64_t n) {
  const uint32_t t = threadIdx.x;
  const uint64_t pro = min((uint64_t)((16 - ((uintptr_t)dst & 15)) & 15), n);
  if (t < pro) dst[t] = src[t];
  const uint64_t nv = (n - pro) >> 4, done = pro + (nv << 4);
  if (nv) {
    uint4 *d = reinterpret_cast<uint4 *>(dst + pro);
    const uint32_t sh = (uint32_t)((uintptr_t)(src + pro) & 15), r8 = (sh & 3) * 8;
    const uint4 *s = reinterpret_cast<const uint4 *>(src + pro - sh);
    if (sh == 0)
      for (uint64_t i = t; i < nv; i += kThreads) d[i] = s[i];
    else
      switch (sh >> 2) {
        case 0: copy_shifted<0>(d, s, nv, r8); break;
        case 1: copy_shifted<1>(d, s, nv, r8); break;
        case 2: copy_shifted<2>(d, s, nv, r8); break;
        default: copy_shifted<3>(d, s, nv, r8); break;
      }
  }
  if (t < n - done) dst[done + t] = src[done + t];
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void zh_frame_pack(const ZhFrameLaunch L, uint32_t first) {
  const ZhFrameEntry e = L.table[first + blockIdx.y];
  uint8_t *dst = L.out + e.dst_off;
  const uint8_t *body = L.src[e.src] + e.src_off;
  const uint64_t ns = e.store ? L.sel_len : 0, decoded = ns + e.body_len;
  const uint64_t pieces = (decoded + ZH_FRAME_PIECE - 1) / ZH_FRAME_PIECE;
  if (blockIdx.x == 0) {
    copy_bytes(dst, L.blob + e.head_off, e.head_len);
    copy_bytes(dst + e.head_len + decoded + (e.store ? 4 * pieces : 0), L.blob + e.tail_off, e.tail_len);
  }
  dst += e.head_len;
  for (uint64_t p = blockIdx.x; p < pieces; p += gridDim.x) {
    const uint64_t c = p * ZH_FRAME_PIECE, end = min(c + ZH_FRAME_PIECE, decoded);
    if (!e.store) {
      copy_bytes(dst + c, body + c, end - c);
      continue;
    }
    uint8_t *w = dst + c + 4 * p;
    const uint32_t cl = (uint32_t)(end - c);
    if (threadIdx.x < 4) w[threadIdx.x] = (uint8_t)(cl >> (24 - 8 * threadIdx.x));
    w += 4;
    if (c < ns) copy_bytes(w, L.blob + L.sel_off + c, min(ns, end) - c);
    const uint64_t q = max(c, ns);
    if (q < end) copy_bytes(w + (q - c), body + (q - ns), end - q);
  }
}

extern "C" hipError_t zh_launch_frame_pack(const ZhFrameLaunch *L, hipStream_t stream, uint32_t *launches) {
  const uint32_t gx = L->pieces < 1 ? 1 : L->pieces > 64 ? 64 : L->pieces;
  for (uint32_t first = 0; first < L->n; first += 32768) {
    const uint32_t ny = L->n - first < 32768 ? L->n - first : 32768;
    hipLaunchKernelGGL(zh_frame_pack, dim3(gx, ny), dim3(kThreads), 0, stream, *L, first);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++*launches;
  }
  return hipSuccess;
}
