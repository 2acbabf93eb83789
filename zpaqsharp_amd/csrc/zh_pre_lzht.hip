// zh_pre_lzht.hip — LZBuffer's hash-table match search on the GPU (LZBuffer.cs:285-327, :349-368): what the reference does
// for a level 1 / 2 method with args[5] - args[0] < 21, byte for byte (tools/methods.lz77_ht is the port), with
// minMatch2 = args[3] = 0 and lookahead = args[6] = 0.  Refused by the host (ZPAQHIP_E_ARG): args[3] != 0, args[6] != 0,
// level 1 with args[2] < 4, level 2 with args[2] < 2, args[2] > 255, args[0] > 11, args[4] > args[5] or above
// ZH_LZHT_MAX_BUCKET_BITS, args[5] > 30 and blocks over 2^24 bytes.
//
// The reference stores every position j the walk passes with j + minMatchBoth < n in ht[h1 ^ ih(j)] and searches
// ht[h1 ^ 0 .. bucket] at i.  h1 before the step at j is a function of in[max(j, minMatch) .. j + minMatch - 1] alone (a
// term is multiplied by 5 * 2^shift1 per later step and shift1 * minMatch >= args[5]), frozen from n - minMatchBoth on;
// the walk passes every position; so ht[s] at time i is the largest stored j < i whose slot is s, whatever was parsed.
// The table is never built.  All blocks of a launch share the slot space of zh_pre_bwt.hip:
//
//   zh_lzht_keys    one thread per position: key = its slot h1 ^ ih (1 << args[5] where it is not stored), val = position.
//                   zh_pre_bwt.hip's stable radix passes (zh_launch_pre_sort) then order the pairs by (slot, position);
//                   a block's positions are consecutive, so within a slot the blocks follow each other
//   zh_lzht_search  one lane per position i: for k = 0 .. bucket the predecessor of (h1 ^ k, i) in that order, by a binary
//                   search of at most 32 steps whatever the data, is ht[h1 ^ k] if it lies in i's block; then the
//                   reference's filters and score.  A lane compares at most ZH_LZHT_CMP = 256 bytes: every earlier best
//                   has blen < 128 (or the loop had ended), so scores at most 8 * 127 - 12, a candidate reaching 256
//                   scores at least 8 * 256 - 24 - 13: it wins and ends the loop under either lit, and its exact length
//                   only decides how far the walk advances, so it is stored as "to be extended" (bit 48).  The lane
//                   decides for lit > 0, and again for lit == 0 only where a candidate scored 1 or 2 before the
//                   2 * (lit > 0) term, which is the same for every candidate and so can only flip a comparison with 0
//   zh_lzht_walk    one wave per block: zh_lz_walk of zh_pre_lzwalk.h, which extends a flagged match 64 bytes per step
//
// Every store is a plain C++ store to global memory; out_cap bounds every write to ::out.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "zh_pre.h"
#include "zh_pre_lzwalk.h"

namespace {

// h1 before the step at position e <= max(0, n - minMatchBoth) (LZBuffer.cs:364): the last min(e, minMatch) steps
__device__ __forceinline__ uint32_t h1_at(const ZhLzhtLaunch &L, const uint8_t *d, uint32_t e) {
  const uint32_t mm = L.min_match;
  uint32_t h = 0;
  for (uint32_t t = e > mm ? e - mm : 0; t < e; ++t) h = ((h * 5) << L.shift1) + (d[t + mm] + 1u) * 123456791u;
  return h & ((1u << L.ht_bits) - 1);
}

// ht[slot] when position x (a slot number of the launch, in the block that starts at s) is searched: the largest stored
// position below x with that slot, or ~0u
__device__ __forceinline__ uint32_t stored(const ZhLzhtLaunch &L, uint32_t slot, uint32_t x, uint32_t s) {
  uint32_t lo = 0, hi = L.n;                      // the first pair that is not below (slot, x)
  while (lo < hi) {
    const uint32_t mid = (uint32_t)(((uint64_t)lo + hi) >> 1);
    const uint32_t k = L.key[mid];
    if (k < slot || (k == slot && L.val[mid] < x)) lo = mid + 1;
    else hi = mid;
  }
  if (!lo || L.key[lo - 1] != slot) return ~0u;
  const uint32_t v = L.val[lo - 1];
  return v >= s ? v : ~0u;
}

// LZBuffer.cs:313-326 and the accept rule :332-346 at position i of a block of n bytes whose first slot is s.
// Returns the decision; *dep is set when a candidate scored 1 or 2 before the literal term.
__device__ uint64_t decide(const ZhLzhtLaunch &L, const uint8_t *d, uint32_t s, uint32_t n, uint32_t i, uint32_t h1, bool lit, bool *dep) {
  const uint32_t mask = (1u << L.checkbits) - 1;
  uint32_t blen = L.min_match - 1, bp = 0;
  int bscore = 0;
  bool ext = false;
  for (uint32_t k = 0; k <= L.bucket; ++k) {
    if (i + 3 < n) {
      const uint32_t v = stored(L, h1 ^ k, s + i, s);
      const uint32_t p = v - s;
      // position 0 with in[3] & mask == 0 is stored as the word 0, an empty slot to the reference
      if (v != ~0u && (p || (d[3] & mask)) && (d[p + 3] & mask) == (d[i + 3] & mask) && i + blen <= n && d[p + blen - 1] == d[i + blen - 1]) {
        const uint32_t lim = min(n - i, ZH_LZHT_CMP);
        uint32_t l = 0;
        while (l < lim && d[p + l] == d[i + l]) ++l;
        const int s0 = (int)l * 8 - lg(i - p) - 11;
        if (s0 == 1 || s0 == 2) *dep = true;
        const int score = s0 - 2 * lit;
        if (score > bscore) { blen = l; bp = p; bscore = score; ext = l == ZH_LZHT_CMP; }
      }
    }
    if (blen >= 128) break;
  }
  const uint32_t off = i - bp;
  if (off > 0 && bscore > 0 && blen >= L.min_match + (L.level == 2 ? (off >= (1u << 16)) + (off >= (1u << 24)) : 0))
    return (uint64_t)off | (uint64_t)blen << 24 | (uint64_t)ext << 48;
  return 0;
}

}  // namespace

// ---- the slot of every position -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zh_lzht_keys(ZhLzhtLaunch L, uint32_t *key, uint32_t *val) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= L.n) return;
  const uint32_t b = block_of(L.starts, L.n_blocks, (uint32_t)x), s = L.starts[b], n = L.starts[b + 1] - s, j = (uint32_t)x - s;
  uint32_t k = 1u << L.ht_bits;                   // not stored (LZBuffer.cs:353)
  if ((uint64_t)j + L.min_match + 4 < n) k = h1_at(L, L.src + L.blocks[b].in_off, j) ^ (((j * 1234547u) >> 19) & L.bucket);
  key[x] = k;
  val[x] = (uint32_t)x;
}

// ---- the decisions -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zh_lzht_search(ZhLzhtLaunch L) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= L.n) return;
  uint64_t v0 = 0, v1 = 0;
  if (L.search) {
    const uint32_t b = block_of(L.starts, L.n_blocks, (uint32_t)x), s = L.starts[b], n = L.starts[b + 1] - s, i = (uint32_t)x - s;
    const uint8_t *d = L.src + L.blocks[b].in_off;
    const uint32_t both = L.min_match + 4, frozen = n > both ? n - both : 0;
    const uint32_t h1 = h1_at(L, d, min(i, frozen));
    bool dep = false;
    v1 = decide(L, d, s, n, i, h1, true, &dep);
    v0 = dep ? decide(L, d, s, n, i, h1, false, &dep) : v1;
  }
  L.dec[1][x] = v1;
  L.dec[0][x] = v0;
}

// ---- the walk and the codes --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void zh_lzht_walk(ZhLzhtLaunch L) {
  const ZhPreBlock B = L.blocks[blockIdx.x];
  const uint64_t pos = zh_lz_walk(L.src + B.in_off, (int64_t)B.n, L.dec[0] + L.starts[blockIdx.x], L.dec[1] + L.starts[blockIdx.x],
                                  L.out + B.out_off, B.out_cap, L.level, (int)L.min_match, (int)L.rb);
  if (threadIdx.x == 0) L.out_len[blockIdx.x] = pos;
}

// The codes of L_->n_blocks blocks.  W holds the sort's buffers for the same slot space and words[q] its pair q as one array
// of 64-bit words (zh_pre.cpp's SortArena): the pairs are written to W->key[0] / val[0] and sorted; the pair of arrays the
// sort ends in becomes ::key / ::val, the other one ::dec[1].  The caller sets everything else.  *launches grows by the
// kernels launched.
extern "C" hipError_t zh_launch_pre_lzht(const ZhLzhtLaunch *L_, const ZhBwtLaunch *W, uint64_t *const words[2], hipStream_t stream,
                                         uint32_t *launches) {
  ZhLzhtLaunch L = *L_;
  if (!L.n_blocks) return hipSuccess;
  hipError_t e;
  if (L.n) {
    const dim3 grid((uint32_t)(((uint64_t)L.n + 255) / 256));
    uint32_t c = 0;
    if (L.search) {
      hipLaunchKernelGGL(zh_lzht_keys, grid, dim3(256), 0, stream, L, W->key[0], W->val[0]);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if (launches) ++*launches;
      if ((e = zh_launch_pre_sort(W, stream, launches, &c, L.ht_bits + 1)) != hipSuccess) return e;
    }
    L.key = W->key[c];
    L.val = W->val[c];
    L.dec[1] = words[c ^ 1];
    hipLaunchKernelGGL(zh_lzht_search, grid, dim3(256), 0, stream, L);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (launches) ++*launches;
  }
  hipLaunchKernelGGL(zh_lzht_walk, dim3(L.n_blocks), dim3(64), 0, stream, L);
  if (launches) ++*launches;
  return hipGetLastError();
}
