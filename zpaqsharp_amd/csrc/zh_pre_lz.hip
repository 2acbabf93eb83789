// zh_pre_lz.hip — the pre-processors of LibZPAQ.compressBlock on the GPU (LibZPAQ.cs:296-311): forward E8E9
// (LibZPAQ.cs:372-384) and LZBuffer's levels 1 and 2 (LZBuffer.cs:96-115, write_literal :387-418, write_match :422-485)
// with the parse of tools/methods._matches (zh_pre.h).  Four kernels, in launch order:
//
//   zh_pre_e8e9      one wave per block walks 1 KiB chunks from the top; candidates (E8 / E9 in the ORIGINAL byte) are
//                    found with a ballot and applied highest first in an LDS ring that holds the chunk and the one above
//   zh_pre_lz_prev   one wave per block enters positions in order, 256 per step: a k-byte hash picks a bucket, equal
//                    buckets inside the step are found with ballots over the bucket bits, and the last position of each
//                    bucket swaps itself into the block's table; chain[p] = the previous position of p's bucket
//   zh_pre_lz_verify one thread per position follows chain[] to the nearest position whose k bytes are equal (so
//                    prev[] is exact whatever the hash does) and measures up to ZH_PRE_EXT more matching bytes
//   zh_pre_lz_parse  one wave per block walks the greedy parse, 64 prev[] entries per ballot, extends the rare long
//                    matches 64 bytes per step, and writes the codes as it goes through LzCodes (zh_pre_lzcodes.h:
//                    literal runs 64 bytes per store)
//
// Every store is a plain C++ store to global memory or LDS; out_cap bounds every write to ::out.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "zh_pre.h"
#include "zh_pre_lzcodes.h"

namespace {

__device__ __forceinline__ const uint8_t *src_of(const ZhPreLaunch &L, const ZhPreBlock &B) {
  return (L.doe8 ? L.e8 : L.in) + B.in_off;
}

__device__ __forceinline__ uint32_t bucket_of(const uint8_t *p, uint32_t k, uint32_t bits) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (uint32_t t = 0; t < k; ++t) h = (h ^ p[t]) * 0x100000001B3ull;
  h ^= h >> 31;
  h *= 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  return (uint32_t)(h >> (64 - bits));
}

}  // namespace

// ---- forward E8E9 -----------------------------------------------------------------------------------------------------
// The reference walks i = n-5 .. 0 and, where buf[i] & 254 == 0xE8 and buf[i+4] is 00 or FF, adds i to the 24-bit operand
// buf[i+1..i+3].  A rewrite at i touches bytes above i only, so whether i is a candidate depends on its original byte;
// only buf[i+4] may have changed when i is reached (by candidates at i+1 .. i+3), and the bytes i+1 .. i+4 lie in the
// chunk or the one above it, both in the ring.  A chunk is written when the chunk below it is done.
__global__ __launch_bounds__(64) void zh_pre_e8e9(ZhPreLaunch L) {
  const ZhPreBlock B = L.blocks[blockIdx.x];
  const uint8_t *src = L.in + B.in_off;
  uint8_t *dst = L.level ? L.e8 + B.in_off : L.out + B.out_off;
  const int64_t n = (int64_t)B.n;
  const uint64_t cap = L.level ? B.n : B.out_cap;
  const int lane = threadIdx.x;
  __shared__ uint8_t ring[2048];                  // position p lives at ring[p & 2047]
  if (n == 0) return;
  const int64_t nch = (n + 1023) / 1024;
  for (int64_t c = nch - 1; c >= 0; --c) {
    const int64_t base = c * 1024;
    uint32_t mask = 0;
    for (int t = 0; t < 16; ++t) {
      const int64_t p = base + lane * 16 + t;
      const uint8_t v = p < n ? src[p] : 0;
      ring[p & 2047] = v;
      if (p + 4 < n && (v & 254) == 0xE8) mask |= 1u << t;
    }
    __syncthreads();
    for (;;) {
      const uint64_t bal = __ballot(mask != 0);
      if (!bal) break;
      const int hl = 63 - __clzll((long long)bal);
      const uint32_t ml = __shfl(mask, hl);
      const int hb = 31 - __clz((int)ml);
      if (lane == hl) mask &= ~(1u << hb);
      const int64_t i = base + hl * 16 + hb;
      const uint32_t b4 = ring[(i + 4) & 2047];
      if (((b4 + 1) & 254) == 0) {
        const uint32_t a = (ring[(i + 1) & 2047] | (uint32_t)ring[(i + 2) & 2047] << 8 | (uint32_t)ring[(i + 3) & 2047] << 16) + (uint32_t)i;
        __syncthreads();
        if (lane == 0) {
          ring[(i + 1) & 2047] = (uint8_t)a;
          ring[(i + 2) & 2047] = (uint8_t)(a >> 8);
          ring[(i + 3) & 2047] = (uint8_t)(a >> 16);
        }
      }
      __syncthreads();
    }
    if (c + 1 < nch)                              // the chunk above is final now
      for (int t = 0; t < 16; ++t) {
        const int64_t p = base + 1024 + lane * 16 + t;
        if (p < n && (uint64_t)p < cap) dst[p] = ring[p & 2047];
      }
    __syncthreads();
  }
  for (int t = 0; t < 16; ++t) {
    const int64_t p = lane * 16 + t;
    if (p < n && (uint64_t)p < cap) dst[p] = ring[p & 2047];
  }
  if (!L.level && lane == 0) L.out_len[blockIdx.x] = B.n;
}

// ---- bucket chains --------------------------------------------------------------------------------------------------
// Step s enters positions 256s .. 256s+255 as four rows of 64 lanes.  eq[r][q] is the set of lanes of row q whose bucket
// equals this lane's bucket in row r (one ballot per bucket bit and row).  A position's chain entry is the latest earlier
// position of its bucket in the step, or, for the first of its bucket, what the table held; the last of each bucket
// swaps itself into the table and passes the old value to the first.  The swaps of one step go to distinct entries and
// return before the next step issues its own, so the table sees the positions in order.
__global__ __launch_bounds__(64) void zh_pre_lz_prev(ZhPreLaunch L) {
  const ZhPreBlock B = L.blocks[blockIdx.x];
  const uint8_t *d = src_of(L, B);
  const int64_t n = (int64_t)B.n, k = L.k;
  if (n < k) return;
  const int64_t last = n - k;                     // positions 0 .. last are entered
  int32_t *tab = L.table + B.tab_off;
  int32_t *chain = L.chain + B.scr_off;
  const int lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1, above = ~below & ~(1ull << lane);
  for (int64_t base = 0; base <= last; base += 256) {
    uint32_t bk[4];
    bool act[4];
    uint64_t actm[4];
    for (int r = 0; r < 4; ++r) {
      const int64_t p = base + 64 * r + lane;
      act[r] = p <= last;
      bk[r] = act[r] ? bucket_of(d + p, (uint32_t)k, B.tab_bits) : 0;
      actm[r] = __ballot(act[r]);
    }
    uint64_t eq[4][4];
    for (int r = 0; r < 4; ++r)
      for (int q = 0; q < 4; ++q) eq[r][q] = actm[q];
    for (int q = 0; q < 4; ++q)
      for (uint32_t b = 0; b < B.tab_bits; ++b) {
        const uint64_t bal = __ballot((bk[q] >> b) & 1);
        for (int r = 0; r < 4; ++r) eq[r][q] &= ((bk[r] >> b) & 1) ? bal : ~bal;
      }
    int32_t pred[4], old[4];
    int src_row[4], src_lane[4];
    for (int r = 0; r < 4; ++r) {
      pred[r] = -1;
      if (eq[r][r] & below) pred[r] = (int32_t)(base + 64 * r + 63 - __clzll((long long)(eq[r][r] & below)));
      else
        for (int q = r - 1; q >= 0; --q)
          if (eq[r][q]) { pred[r] = (int32_t)(base + 64 * q + 63 - __clzll((long long)eq[r][q])); break; }
      // the last of this bucket in the step: the highest lane of the highest row that has one (this lane if none above)
      src_row[r] = r;
      src_lane[r] = 63 - __clzll((long long)((eq[r][r] & above) | (1ull << lane)));
      for (int q = 3; q > r; --q)
        if (eq[r][q]) { src_row[r] = q; src_lane[r] = 63 - __clzll((long long)eq[r][q]); break; }
      const bool is_last = act[r] && src_row[r] == r && src_lane[r] == lane;
      old[r] = is_last ? atomicExch(tab + bk[r], (int32_t)(base + 64 * r + lane)) : -1;
    }
    for (int r = 0; r < 4; ++r) {
      int32_t from_tab = -1;
      for (int q = 0; q < 4; ++q) {
        const int32_t v = __shfl(old[q], src_lane[r]);
        if (q == src_row[r]) from_tab = v;
      }
      if (act[r]) chain[base + 64 * r + lane] = pred[r] >= 0 ? pred[r] : from_tab;
    }
  }
}

// ---- exact predecessors ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zh_pre_lz_verify(ZhPreLaunch L) {
  const ZhPreBlock B = L.blocks[blockIdx.y];
  const uint8_t *d = src_of(L, B);
  const int64_t n = (int64_t)B.n, k = L.k;
  const int32_t *chain = L.chain + B.scr_off;
  uint32_t *prev = L.prev + B.scr_off;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t res = 0;
    if (i + k <= n) {
      int64_t j = chain[i];
      while (j >= 0 && i - j <= (int64_t)L.max_off) {
        int64_t t = 0;
        while (t < k && d[j + t] == d[i + t]) ++t;
        if (t == k) break;
        j = chain[j];
      }
      if (j >= 0 && i - j <= (int64_t)L.max_off) {
        const int64_t lim = max(k, min((int64_t)L.max_match, n - i));
        const int64_t stop = min(lim, k + (int64_t)ZH_PRE_EXT);
        int64_t t = k;
        while (t < stop && d[j + t] == d[i + t]) ++t;
        res = (uint32_t)(i - j) << 8 | (uint32_t)(t - k);
      }
    }
    prev[i] = res;
  }
}

// ---- the greedy walk and the codes -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void zh_pre_lz_parse(ZhPreLaunch L) {
  const ZhPreBlock B = L.blocks[blockIdx.x];
  const uint8_t *d = src_of(L, B);
  const int64_t n = (int64_t)B.n, k = L.k;
  const uint32_t *prev = L.prev + B.scr_off;
  const int lane = threadIdx.x;
  LzCodes w(L.out + B.out_off, B.out_cap, L.level, (int)L.m, (int)L.rb);

  int64_t cur = 0, lit0 = 0, wbase = -64;
  uint32_t wv = 0;
  const int64_t last = n - k;                     // the last position a match can start at
  while (cur <= last) {
    if (cur >= wbase + 64) {
      wbase = cur;
      wv = wbase + lane <= last ? prev[wbase + lane] : 0;
    }
    const uint64_t cand = __ballot(wv != 0) & (~0ull << (cur - wbase));
    if (!cand) {
      cur = wbase + 64;
      continue;
    }
    const int t = __ffsll((unsigned long long)cand) - 1;
    const int64_t i = wbase + t;
    const uint32_t v = __shfl(wv, t);
    const int64_t dist = v >> 8;
    int64_t len = k + (v & 255);
    const int64_t lim = max(k, min((int64_t)L.max_match, n - i));
    if ((v & 255) == ZH_PRE_EXT && len < lim)
      for (;;) {                                  // a long match: 64 bytes per step
        const int64_t q = len + lane;
        const bool same = q < lim && d[i - dist + q] == d[i + q];
        const uint64_t diff = __ballot(!same);
        if (diff) {
          len += __ffsll((unsigned long long)diff) - 1;
          break;
        }
        len += 64;
      }
    w.literals(d, lit0, i);
    w.match((uint64_t)len, (uint64_t)dist);
    cur = lit0 = i + len;
  }
  w.literals(d, lit0, n);
  const uint64_t pos = w.finish();
  if (lane == 0) L.out_len[blockIdx.x] = pos;
}

// the coded sequence's post-processor header in front of each block's pre-processed bytes (Compressor.postProcess)
__global__ __launch_bounds__(64) void zh_pre_prefix(ZhPreLaunch L, const uint8_t *prefix, uint32_t np) {
  const ZhPreBlock B = L.blocks[blockIdx.x];
  for (uint32_t t = threadIdx.x; t < np; t += blockDim.x) L.out[B.out_off - np + t] = prefix[t];
}

// Each launcher adds the kernels it launched to *launches.
extern "C" hipError_t zh_launch_pre_prefix(const ZhPreLaunch *L, const uint8_t *prefix, uint32_t np, hipStream_t stream, uint32_t *launches) {
  if (!L->n_blocks || !np) return hipSuccess;
  hipLaunchKernelGGL(zh_pre_prefix, dim3(L->n_blocks), dim3(64), 0, stream, *L, prefix, np);
  ++*launches;
  return hipGetLastError();
}

extern "C" hipError_t zh_launch_pre_e8e9(const ZhPreLaunch *L, hipStream_t stream, uint32_t *launches) {
  if (!L->n_blocks) return hipSuccess;
  hipLaunchKernelGGL(zh_pre_e8e9, dim3(L->n_blocks), dim3(64), 0, stream, *L);
  ++*launches;
  return hipGetLastError();
}

extern "C" hipError_t zh_launch_pre_lz(const ZhPreLaunch *L, uint64_t max_n, hipStream_t stream, uint32_t *launches) {
  if (!L->n_blocks) return hipSuccess;
  hipLaunchKernelGGL(zh_pre_lz_prev, dim3(L->n_blocks), dim3(64), 0, stream, *L);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint64_t gx = std::min<uint64_t>(std::max<uint64_t>(1, (max_n + 2047) / 2048), 4096);
  hipLaunchKernelGGL(zh_pre_lz_verify, dim3((uint32_t)gx, L->n_blocks), dim3(256), 0, stream, *L);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(zh_pre_lz_parse, dim3(L->n_blocks), dim3(64), 0, stream, *L);
  *launches += 3;
  return hipGetLastError();
}
