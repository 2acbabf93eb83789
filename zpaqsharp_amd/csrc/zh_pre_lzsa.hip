// zh_pre_lzsa.hip — LZBuffer's suffix-array match search on the GPU (LZBuffer.cs:246-283, :329-383): what the reference does
// for a level 1 / 2 method with args[5] - args[0] >= 21, byte for byte (tools/methods.lz77_sa is the literal port).  The
// suffix array and its inverse come from zh_pre_bwt.hip's sort (zh_launch_pre_sufsort): all blocks of a launch share one
// slot space, sa[] and rank[] hold slot numbers.  Three kernels, in launch order:
//
//   zh_lzsa_lcp     lcp[j] = min(common prefix of the suffixes in slots j - 1 and j, maxMatch).  One wave owns 1024
//                   consecutive POSITIONS and takes them in order: the prefix a position shares with its predecessor in
//                   suffix order is at least the previous position's less one, so the wave compares 64 bytes per step from
//                   there and the compares of a chunk add up to its size plus one start of at most maxMatch bytes —
//                   whatever the data (one byte value, period 2) looks like
//   zh_lzsa_search  one lane per position i: the reference's loop over look-ahead h, direction and up to `bucket` neighbours
//                   of h + i in suffix order.  The match with the k-th neighbour is the minimum of the lcp[] entries on the
//                   way (neighbours that are skipped count too), so every length is exact and costs one load.  A decision
//                   depends on the walk only through lit == 0, in the -4 term of a candidate with look-ahead and leading
//                   literals: the lane decides for lit > 0, and again for lit == 0 only where such a candidate was scored
//   zh_lzsa_walk    one wave per block follows the decisions from 0 to n: a position reached with lit == 0 reads its own
//                   decision, runs of literals are skipped 64 decisions per ballot up to the next match or the flush at
//                   maxLiteral, and the codes are written as zh_pre_lz_parse writes them (level 1 bits, level 2 bytes):
//                   zh_lz_walk of zh_pre_lzwalk.h, which zh_pre_lzht.hip shares
//
// Every store is a plain C++ store to global memory; out_cap bounds every write to ::out.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "zh_pre.h"
#include "zh_pre_lzwalk.h"

namespace {

constexpr uint32_t kLcpChunk = 1024;      // positions per wave of zh_lzsa_lcp

// LZBuffer.cs:249-283 and the accept rule :332-346 at position i of a block of n bytes whose first slot is s.
// Returns the decision; *dep is set when a candidate with look-ahead and leading literals was scored.
__device__ uint64_t decide(const ZhLzsaLaunch &L, const uint8_t *d, uint32_t s, uint32_t n, uint32_t i, bool lit0, bool *dep) {
  const int min_match = (int)L.min_match;
  int blen = min_match - 1, blit = 0, bscore = 0;
  uint32_t bp = 0;
  for (uint32_t h = 0; h <= L.lookahead; ++h) {
    // the reference's inverse array holds the window of i alone (:256-264): look-ahead past it, or past the block, is dropped
    if (i + h >= n || ((i + h) >> L.win_bits) != (i >> L.win_bits)) break;
    const uint32_t q = L.rank[s + i + h] - s;
    for (int dir = 0; dir < 2; ++dir) {
      uint32_t m = ZH_LZSA_MAX_MATCH;             // the prefix h + i shares with the k-th neighbour
      for (uint32_t k = 1; k <= L.bucket; ++k) {
        uint32_t slot;
        if (dir == 0) {
          if (k > q) break;                       // q + j * k < n fails for every further k
          slot = q - k;
          m = min(m, L.lcp[s + slot + 1]);
        } else {
          if (q + k >= n) break;
          slot = q + k;
          m = min(m, L.lcp[s + slot]);
        }
        const uint32_t pp = L.sa[s + slot] - s;
        if (pp < h || pp - h >= i) continue;      // not earlier than i: skipped, not a stop
        const uint32_t p = pp - h;
        const int l = (int)min(h + m, ZH_LZSA_MAX_MATCH);
        int l1 = (int)h;
        while (l1 > 0 && d[p + l1 - 1] == d[i + l1 - 1]) --l1;
        int score = (l - l1) * 8 - lg(i - p) - 4 * (lit0 && l1 > 0) - 11;
        if (l1 > 0) *dep = true;
        for (uint32_t a = 0; a < h; ++a) score = score * 5 / 8;
        if (score > bscore) { blen = l; bp = p; blit = l1; bscore = score; }
        if (l < blen || l < min_match || l > 255) break;
      }
    }
    if (bscore <= 0 || blen < min_match) break;
  }
  const uint32_t off = i - bp;
  if (off > 0 && bscore > 0 && blen - blit >= min_match + (L.level == 2 ? (off >= (1u << 16)) + (off >= (1u << 24)) : 0))
    return (uint64_t)off | (uint64_t)blen << 24 | (uint64_t)blit << 40;
  return 0;
}

}  // namespace

// ---- common prefixes of neighbours in suffix order ----------------------------------------------------------------------
__global__ __launch_bounds__(64) void zh_lzsa_lcp(ZhLzsaLaunch L) {
  const uint32_t lane = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x * kLcpChunk;
  if (base >= L.n) return;
  const uint32_t end = (uint32_t)min<uint64_t>(base + kLcpChunk, L.n);
  uint32_t b = block_of(L.starts, L.n_blocks, (uint32_t)base), s = L.starts[b], e = L.starts[b + 1];
  const uint8_t *d = L.src + L.blocks[b].in_off - s;          // d[x] = the byte of slot-numbered position x
  uint32_t carry = 0;
  for (uint32_t g = (uint32_t)base; g < end; g += 64) {
    const uint32_t pos = g + lane;
    const uint32_t my_slot = pos < end ? L.rank[pos] : 0u;
    const uint32_t my_prev = pos < end && my_slot > 0 ? L.sa[my_slot - 1] : 0u;
    const uint32_t cnt = min(64u, end - g);
    for (uint32_t t = 0; t < cnt; ++t) {
      const uint32_t x = g + t;
      while (x >= e) {                            // the next block (empty blocks own no slot)
        ++b;
        s = e;
        e = L.starts[b + 1];
        d = L.src + L.blocks[b].in_off - s;
        carry = 0;
      }
      const uint32_t slot = __shfl(my_slot, t), pv = __shfl(my_prev, t);
      uint32_t l = 0;
      if (slot > s) {                             // the predecessor in suffix order is a suffix of the same block
        l = carry ? carry - 1 : 0;
        const uint32_t maxl = min(ZH_LZSA_MAX_MATCH, e - max(x, pv));
        for (;;) {
          const uint32_t q = l + lane;
          const bool same = q < maxl && d[x + q] == d[pv + q];
          const uint64_t diff = __ballot(!same);
          if (diff) {
            l += __ffsll((unsigned long long)diff) - 1;
            break;
          }
          l += 64;
        }
      }
      carry = l;
      if (lane == 0) L.lcp[slot] = l;
    }
  }
}

// ---- the decisions -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zh_lzsa_search(ZhLzsaLaunch L) {
  const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= L.n) return;
  const uint32_t b = block_of(L.starts, L.n_blocks, (uint32_t)x), s = L.starts[b], n = L.starts[b + 1] - s;
  const uint8_t *d = L.src + L.blocks[b].in_off;
  bool dep = false;
  const uint64_t v1 = decide(L, d, s, n, (uint32_t)x - s, false, &dep);
  L.dec[1][x] = v1;
  L.dec[0][x] = dep ? decide(L, d, s, n, (uint32_t)x - s, true, &dep) : v1;
}

// ---- the walk and the codes --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void zh_lzsa_walk(ZhLzsaLaunch L) {
  const ZhPreBlock B = L.blocks[blockIdx.x];
  const uint64_t pos = zh_lz_walk(L.src + B.in_off, (int64_t)B.n, L.dec[0] + L.starts[blockIdx.x], L.dec[1] + L.starts[blockIdx.x],
                                  L.out + B.out_off, B.out_cap, L.level, (int)L.min_match, (int)L.rb);
  if (threadIdx.x == 0) L.out_len[blockIdx.x] = pos;
}

// The codes of L->n_blocks blocks whose suffixes are sorted.  *launches grows by the kernels launched.
extern "C" hipError_t zh_launch_pre_lzsa(const ZhLzsaLaunch *L, hipStream_t stream, uint32_t *launches) {
  if (!L->n_blocks) return hipSuccess;
  hipError_t e;
  if (L->n) {
    hipLaunchKernelGGL(zh_lzsa_lcp, dim3((L->n + kLcpChunk - 1) / kLcpChunk), dim3(64), 0, stream, *L);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(zh_lzsa_search, dim3((uint32_t)(((uint64_t)L->n + 255) / 256)), dim3(256), 0, stream, *L);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (launches) *launches += 2;
  }
  hipLaunchKernelGGL(zh_lzsa_walk, dim3(L->n_blocks), dim3(64), 0, stream, *L);
  if (launches) ++*launches;
  return hipGetLastError();
}
