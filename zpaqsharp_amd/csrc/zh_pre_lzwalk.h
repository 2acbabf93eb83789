// zh_pre_lzwalk.h — the walk over the decisions of a match search (LZBuffer.cs:329-383), shared by zh_pre_lzsa.hip and
// zh_pre_lzht.hip; the codes go through LzCodes (zh_pre_lzcodes.h).  One wave per block; every lane holds the same state.
#pragma once
#include <hip/hip_runtime.h>

#include "zh_pre.h"
#include "zh_pre_lzcodes.h"

namespace {

// Follows the decisions of a block of n bytes at d from 0 to n: dec0[i] is the decision of position i when it is reached
// with lit == 0, dec1[i] with lit > 0 (ZhLzsaLaunch's words; bit 48: the match goes on past blen, which the walk then
// finds out).  A position reached with lit == 0 reads its own decision, runs of literals are skipped 64 decisions per
// ballot up to the next match or the flush at maxLiteral (level, m and rb as LzCodes takes them).  Returns the bytes
// written, counted past cap.
__device__ inline uint64_t zh_lz_walk(const uint8_t *d, int64_t n, const uint64_t *dec0, const uint64_t *dec1, uint8_t *out, uint64_t cap,
                                      uint32_t level, int m, int rb) {
  const int lane = threadIdx.x;
  LzCodes w(out, cap, level, m, rb);

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
        w.literals(d, i - ZH_LZSA_MAX_LITERAL, i);
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
      w.literals(d, i + blit - lit, i + blit);
      lit = 0;
      w.match((uint64_t)(blen - blit), (uint64_t)off);
      i += blen;
    } else {
      ++lit;
      ++i;
    }
  }
  w.literals(d, n - lit, n);
  return w.finish();
}

}  // namespace
