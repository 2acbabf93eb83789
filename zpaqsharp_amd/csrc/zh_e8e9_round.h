// zh_e8e9_round.h — a round of zh_e8e9_wave.h's schedule in and out of its slot buffers, for a caller whose bytes lie in a
// flat buffer that begins anywhere (zh_nibble.hip: M, or the Writer's region after the inverse BWT; zh_store.hip: M).  Plain integer code
// like the schedule itself: the caller says how a dword of the flat buffer is read and written, the slot buffers are
// addressed in dwords (kZhE8wSlot and kZhE8wSlice are multiples of 4, and so is every round's base).
// The kernels' driver (zh_e8e9_pass.h) and the tests' harness (tests/e8w_harness.py) both load and store their rounds with it.
#pragma once
#include <stdint.h>

#include "zh_e8e9_wave.h"

static_assert(kZhE8wSlot % 4u == 0u && kZhE8wSlice % 4u == 0u && kZhE8wRound % 256u == 0u, "dword slots, 64 lanes x 4 bytes per step");

// bytes of the round that begins at `base` of a segment of d bytes
ZH_E8W_FN uint32_t zh_e8w_round_len(uint32_t base, uint32_t d) { return d - base < kZhE8wRound ? d - base : kZhE8wRound; }

// Lane `lane`'s share of loading the round at `base`: the original bytes base .. base + nr + 4 of the segment, zeros from d
// on, into the slot layout — each dword into its slice's slot, and the first dword of a slice into the look-ahead of the
// slice before as well.  rd(p, k): bytes p .. p + k - 1 of the flat buffer (1 <= k <= 4, p + k <= d) as a little-endian dword.
template <class RD, class PW>
ZH_E8W_FN void zh_e8w_load(RD rd, PW in_w, uint32_t base, uint32_t d, uint32_t lane) {
  const uint32_t nr = zh_e8w_round_len(base, d);
  for (uint32_t q = 4u * lane; q < nr + 4u; q += 256u) {
    const uint32_t p = base + q;
    const uint32_t v = p < d ? rd(p, d - p < 4u ? d - p : 4u) : 0u;
    const uint32_t l = q / kZhE8wSlice, i = q % kZhE8wSlice;
    if (l < kZhE8wLanes) in_w[(l * kZhE8wSlot + i) / 4u] = v;
    if (i == 0u && l > 0u) in_w[((l - 1u) * kZhE8wSlot + kZhE8wSlice) / 4u] = v;
  }
}

// Lane `lane`'s share of storing the settled round at `base`: its final bytes back to the flat buffer.  wr(p, k, v): bytes
// p .. p + k - 1 (1 <= k <= 4, p + k <= d) from the little-endian dword v.
template <class WR, class PW>
ZH_E8W_FN void zh_e8w_store(WR wr, PW out_w, uint32_t base, uint32_t d, uint32_t lane) {
  const uint32_t nr = zh_e8w_round_len(base, d);
  for (uint32_t q = 4u * lane; q < nr; q += 256u) {
    const uint32_t p = base + q;
    wr(p, d - p < 4u ? d - p : 4u, out_w[((q / kZhE8wSlice) * kZhE8wSlot + q % kZhE8wSlice) / 4u]);
  }
}

// The machine's registers as the end-of-segment loop of the lzpre program with E8E9 leaves them (LibZPAQ.cs:601:
// `b=0 c=0 d=0 a=0 r=a 1 r=a 2`; F is the loop's last comparison, `a==d`, which held)
ZH_E8W_FN void zh_e8w_regs_after(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, uint32_t &f, uint32_t &r1, uint32_t &r2) {
  a = 0; b = 0; c = 0; d = 0; f = 1; r1 = 0; r2 = 0;
}
