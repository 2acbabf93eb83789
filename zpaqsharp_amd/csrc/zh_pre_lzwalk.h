// zh_pre_lzwalk.h — the walk over the decisions of a match search and LZBuffer's code writers (LZBuffer.cs:329-383,
// :387-485), shared by zh_pre_lzsa.hip and zh_pre_lzht.hip.  One wave per block; every lane holds the same state, the
// stores are plain C++ stores bounded by `cap`.
#pragma once
#include <hip/hip_runtime.h>

#include "zh_pre.h"

namespace {

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

// Follows the decisions of a block of n bytes at d from 0 to n: dec0[i] is the decision of position i when it is reached
// with lit == 0, dec1[i] with lit > 0 (ZhLzsaLaunch's words; bit 48: the match goes on past blen, which the walk then
// finds out).  A position reached with lit == 0 reads its own decision, runs of literals are skipped 64 decisions per
// ballot up to the next match or the flush at maxLiteral, and the codes are written as zh_pre_lz_parse writes them
// (level 1 bits, level 2 bytes; m = args[2], rb as in ZhPreLaunch).  Returns the bytes written, counted past cap.
__device__ inline uint64_t zh_lz_walk(const uint8_t *d, int64_t n, const uint64_t *dec0, const uint64_t *dec1, uint8_t *out, uint64_t cap,
                                      uint32_t level, int m, int rb) {
  const int lane = threadIdx.x;
  Bits w{out, cap, 0, 0, 0};                      // level 1 writer; level 2 uses w.pos only

  auto literals = [&](int64_t a, int64_t b) {     // write_literal (LZBuffer.cs:387-419) of d[a .. b)
    if (b <= a) return;
    if (level == 1) {
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
    if (level == 1) {
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
    const int64_t off = (int64_t)(v & 0xFFFFFFu), blit = (int64_t)(v >> 40 & 0xFFu);
    int64_t blen = (int64_t)(v >> 24 & 0xFFFFu);
    if (off) {
      if (v >> 48 & 1) {                          // the search stopped comparing at blen: the match goes on, 64 bytes per step
        const int64_t lim = min(n - i, (int64_t)ZH_LZSA_MAX_MATCH);
        while (blen < lim) {
          const int64_t q = blen + lane;
          const bool same = q < lim && d[i - off + q] == d[i + q];
          const uint64_t diff = __ballot(!same);
          if (diff) {
            blen += __ffsll((unsigned long long)diff) - 1;
            break;
          }
          blen += 64;
        }
      }
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
  if (level == 1 && w.n > 0) {                  // flush
    if (lane == 0 && w.pos < cap) out[w.pos] = (uint8_t)w.acc;
    ++w.pos;
  }
  return w.pos;
}

}  // namespace
