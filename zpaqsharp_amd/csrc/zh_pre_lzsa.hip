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
//                   maxLiteral, and the codes are written as zh_pre_lz_parse writes them (level 1 bits, level 2 bytes)
//
// Every store is a plain C++ store to global memory; out_cap bounds every write to ::out.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "zh_pre.h"

namespace {

constexpr uint32_t kLcpChunk = 1024;      // positions per wave of zh_lzsa_lcp

__device__ __forceinline__ uint32_t block_of(const ZhLzsaLaunch &L, uint32_t slot) {   // the block that owns a slot
  uint32_t lo = 0, hi = L.n_blocks - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (L.starts[mid] <= slot) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int lg(uint64_t x) { return x ? 64 - __clzll((long long)x) : 0; }   // LZBuffer.cs:116-126

// the bit writer of LZBuffer level 1 (LSB first, LZBuffer.cs:50-63); every lane holds the same state, lane 0 stores
struct Bits {
  uint8_t *out;
  uint64_t cap, pos;
  uint64_t acc;
  int n;
  __device__ void put(uint64_t x, int k) {
    if (k == 0) return;
    x &= (1ull << k) - 1;
    acc |= x << n;
    n += k;
    while (n > 7) {
      if (threadIdx.x == 0 && pos < cap) out[pos] = (uint8_t)acc;
      ++pos;
      acc >>= 8;
      n -= 8;
    }
  }
};

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
  uint32_t b = block_of(L, (uint32_t)base), s = L.starts[b], e = L.starts[b + 1];
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
  const uint32_t b = block_of(L, (uint32_t)x), s = L.starts[b], n = L.starts[b + 1] - s;
  const uint8_t *d = L.src + L.blocks[b].in_off;
  bool dep = false;
  const uint64_t v1 = decide(L, d, s, n, (uint32_t)x - s, false, &dep);
  L.dec[1][x] = v1;
  L.dec[0][x] = dep ? decide(L, d, s, n, (uint32_t)x - s, true, &dep) : v1;
}

// ---- the walk and the codes --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void zh_lzsa_walk(ZhLzsaLaunch L) {
  const ZhPreBlock B = L.blocks[blockIdx.x];
  const uint8_t *d = L.src + B.in_off;
  const int64_t n = (int64_t)B.n;
  const uint64_t *dec0 = L.dec[0] + L.starts[blockIdx.x], *dec1 = L.dec[1] + L.starts[blockIdx.x];
  uint8_t *out = L.out + B.out_off;
  const uint64_t cap = B.out_cap;
  const int lane = threadIdx.x;
  const int m = (int)L.min_match, rb = (int)L.rb;
  Bits w{out, cap, 0, 0, 0};                      // level 1 writer; level 2 uses w.pos only

  auto literals = [&](int64_t a, int64_t b) {     // write_literal (LZBuffer.cs:387-419) of d[a .. b)
    if (b <= a) return;
    if (L.level == 1) {
      const uint64_t lit = (uint64_t)(b - a);
      int ll = lg(lit);
      w.put(0, 2);
      --ll;
      while (ll > 0) {
        --ll;
        w.put(1, 1);
        w.put((lit >> ll) & 1, 1);
      }
      w.put(0, 1);
      for (int64_t q = a; q < b; q += 64) {       // whole bytes at a bit offset of w.n
        const int cnt = (int)min((int64_t)64, b - q);
        const uint32_t v = lane < cnt ? d[q + lane] : 0;
        const uint32_t lo = __shfl(v, lane > 0 ? lane - 1 : 0);
        const uint32_t byte = ((v << w.n) | (lane == 0 ? (uint32_t)w.acc : lo >> (8 - w.n))) & 255;
        if (lane < cnt && w.pos + lane < cap) out[w.pos + lane] = (uint8_t)byte;
        w.acc = __shfl(v, cnt - 1) >> (8 - w.n);
        w.pos += cnt;
      }
    } else {
      for (int64_t q = a; q < b; q += 64) {       // 64-byte chunks, each after its length - 1
        const int cnt = (int)min((int64_t)64, b - q);
        if (lane == 0 && w.pos < cap) out[w.pos] = (uint8_t)(cnt - 1);
        if (lane < cnt && w.pos + 1 + lane < cap) out[w.pos + 1 + lane] = d[q + lane];
        w.pos += cnt + 1;
      }
    }
  };
  auto match = [&](uint64_t ln, uint64_t off) {   // write_match (LZBuffer.cs:422-485); offsets stay below 2^24
    if (L.level == 1) {
      int ll = lg(ln) - 1;
      off += (1ull << rb) - 1;
      const int lo = lg(off) - 1 - rb;
      w.put((uint64_t)(lo + 8) >> 3, 2);
      w.put((uint64_t)lo & 7, 3);
      while (ll > 2) {
        --ll;
        w.put(1, 1);
        w.put((ln >> ll) & 1, 1);
      }
      w.put(0, 1);
      w.put(ln & 3, 2);
      w.put(off, rb);
      w.put(off >> rb, lo);
    } else {
      --off;
      while (ln > 0) {
        const uint64_t len1 = ln > (uint64_t)(2 * m + 63) ? (uint64_t)(m + 63) : ln > (uint64_t)(m + 63) ? ln - m : ln;
        uint8_t c[4];
        int nc;
        if (off < (1u << 16)) {
          c[0] = (uint8_t)(64 + len1 - m); c[1] = (uint8_t)(off >> 8); c[2] = (uint8_t)off; nc = 3;
        } else {
          c[0] = (uint8_t)(128 + len1 - m); c[1] = (uint8_t)(off >> 16); c[2] = (uint8_t)(off >> 8); c[3] = (uint8_t)off; nc = 4;
        }
        if (lane == 0)
          for (int t = 0; t < nc; ++t)
            if (w.pos + t < cap) out[w.pos + t] = c[t];
        w.pos += nc;
        ln -= len1;
      }
    }
  };

  int64_t i = 0, lit = 0, wbase = -64;
  uint32_t wlo = 0, whi = 0;                      // this lane's entry of the window of lit > 0 decisions
  while (i < n) {
    uint64_t v;
    if (lit == 0) v = dec0[i];
    else {
      if (i < wbase || i >= wbase + 64) {
        wbase = i;
        const uint64_t e = wbase + lane < n ? dec1[wbase + lane] : 0;
        wlo = (uint32_t)e;
        whi = (uint32_t)(e >> 32);
      }
      const uint64_t cand = __ballot((wlo & 0xFFFFFFu) != 0) & (~0ull << (i - wbase));
      const int t = cand ? __ffsll((unsigned long long)cand) - 1 : 64;
      const int64_t stop = min(wbase + t, n);     // the next match, or the end of the window or of the block
      const int64_t room = (int64_t)ZH_LZSA_MAX_LITERAL - lit;
      if (stop - i >= room) {                     // the literal run is flushed first (LZBuffer.cs:370-373)
        i += room;
        literals(i - ZH_LZSA_MAX_LITERAL, i);
        lit = 0;
        continue;
      }
      lit += stop - i;
      i = stop;
      if (!cand) continue;
      v = (uint64_t)__shfl(wlo, t) | (uint64_t)__shfl(whi, t) << 32;
    }
    const int64_t off = (int64_t)(v & 0xFFFFFFu), blen = (int64_t)(v >> 24 & 0xFFFFu), blit = (int64_t)(v >> 40 & 0xFFu);
    if (off) {
      lit += blit;
      literals(i + blit - lit, i + blit);
      lit = 0;
      match((uint64_t)(blen - blit), (uint64_t)off);
      i += blen;
    } else {
      ++lit;
      ++i;
    }
  }
  literals(n - lit, n);
  if (L.level == 1 && w.n > 0) {                  // flush
    if (lane == 0 && w.pos < cap) out[w.pos] = (uint8_t)w.acc;
    ++w.pos;
  }
  if (lane == 0) L.out_len[blockIdx.x] = w.pos;
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
