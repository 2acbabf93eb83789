// zh_e8e9_wave.h — the inverse E8E9 pass at the end of a segment of the reference's LZ77 post-processors with E8E9 (lazy2:
// LibZPAQ.cs:441-462, lzpre: :581-601) as a schedule that a wave executes.  Plain integer code over two byte buffers that
// the caller owns: the kernels' one driver (zh_e8e9_pass.h) runs it with both in LDS, the tests' one harness
// (tests/e8w_harness.py) compiles it for the host and plays the 64 lanes one after the other against the oracle's run of the
// program.  What a lane does in steps 1 to 3 below is here (zh_e8w_first, zh_e8w_retake); a caller's own is the exchange
// between the lanes.
//
// The program, with d = the bytes the segment wrote into M (d <= |M|: no index wraps):
//   for b = 0 .. d-1:
//     if b + 4 < d and (M[b] & 254) == 232 and ((M[b+4] + 1) & 254) == 0:
//       a = M[b+1] | M[b+2] << 8 | M[b+3] << 16;  a -= b;  M[b+1] = a;  M[b+2] = a >> 8;  M[b+3] = a >> 16
//     out(M[b])
// A trigger at b writes b+1 .. b+3 only.  So when b is visited M[b+3] and M[b+4] still hold what the LZ77 codes wrote (the
// ORIGINAL bytes), M[b], M[b+1], M[b+2] may have been rewritten by the triggers at b-3 .. b-1, and nothing after b is visited
// changes M[b]: the byte written out at b is the final M[b].  All that one position hands to the next is the STATE
//   st(b) = M[b] | M[b+1] << 8 | M[b+2] << 16      as the positions before b left them;
// a position takes st(b) and the original bytes at b+3 and b+4 and gives the final M[b] and st(b+1) (zh_e8w_step).  A trigger
// can write an E8 that makes the next position trigger, so no look at the original bytes tells where the state is clean:
// a run of 00 or FF makes every position a candidate.
//
// THE SCHEDULE.  A round is kZhE8wLanes slices of kZhE8wSlice positions, one slice per lane.  The caller puts the round's
// original bytes into `in` and gets the final bytes in `out`, both in the slot layout below (a slice and the four bytes after
// it side by side, so that a lane looks ahead without leaving its slot; the slots' stride keeps the lanes on different LDS
// banks).  Every lane keeps the incoming state its slice was last walked from and the outgoing state that walk gave:
//   1. every lane walks its slice from the CLEAN state (the original bytes at its first three positions), lane 0 from the
//      state the round before handed over (clean in the first round);
//   2. every lane takes the outgoing state of the lane before it as its new incoming state;
//   3. if no lane's incoming state has changed the round is settled: `out` is final, lane 63's outgoing state is the next
//      round's.  Otherwise the lanes whose state changed walk again (zh_e8w_walk with the old state) and the wave goes to 2.
// EXACT: in a settled round every slice was walked from the outgoing state of the slice before it and lane 0's from the true
// state, so by induction over the lanes every walk is the program's.  TERMINATES: lane 0 never changes; after the k-th time
// through 2 the lanes 0 .. k have their true incoming state for good, so 3 is passed 64 times at most, whatever the data.
// A walk from a changed state runs the old and the new state side by side and stops where they meet: from there on the
// positions see what they saw before, so what `out` holds and the outgoing state stand (the old walk's outputs are, by the
// same induction, those of a full walk from the old state).  On executables a changed state meets the old one a few
// positions in; a chain in which every trigger writes the next E8 is walked to its end, one slice per pass.
#pragma once
#include <stdint.h>

#ifndef ZH_E8W_FN
#define ZH_E8W_FN __device__ __forceinline__
#endif

constexpr uint32_t kZhE8wLanes = 64u;                                 // slices of a round
constexpr uint32_t kZhE8wSlice = 64u;                                 // positions of a slice
constexpr uint32_t kZhE8wRound = kZhE8wLanes * kZhE8wSlice;           // positions of a round
constexpr uint32_t kZhE8wSlot = kZhE8wSlice + 4u;                     // bytes of a slice's slot: the slice and its look-ahead
constexpr uint32_t kZhE8wBuf = kZhE8wLanes * kZhE8wSlot;              // bytes of `in` and of `out`
constexpr uint32_t kZhE8wNone = 0xFFFFFFFFu;                          // "no walk before this one" (a state has 24 bits)

// where position r of a round (r < kZhE8wRound) lies in `in` / `out`
ZH_E8W_FN uint32_t zh_e8w_slot(uint32_t r) { return (r / kZhE8wSlice) * kZhE8wSlot + (r % kZhE8wSlice); }

// positions lane `lane` has in the round that begins at `base` of a segment of d bytes
ZH_E8W_FN uint32_t zh_e8w_count(uint32_t base, uint32_t lane, uint32_t d) {
  const uint32_t p0 = base + lane * kZhE8wSlice;
  return p0 >= d ? 0u : (d - p0 < kZhE8wSlice ? d - p0 : kZhE8wSlice);
}

// one position p of a segment of d bytes: st = st(p), o3 / o4 = the original bytes at p + 3 / p + 4.  Returns the final M[p]
// in the low byte and st(p + 1) above it
ZH_E8W_FN uint32_t zh_e8w_step(uint32_t st, uint32_t o3, uint32_t o4, uint32_t p, uint32_t d) {
  uint32_t w = st | o3 << 24;
  if (p + 4u < d && (w & 254u) == 232u && ((o4 + 1u) & 254u) == 0u) w = (w & 255u) | (((w >> 8) - p) << 8);
  return w;
}

// the state nothing has touched: the original bytes at the slot's first three positions
template <class P> ZH_E8W_FN uint32_t zh_e8w_clean(P in) { return (uint32_t)in[0] | (uint32_t)in[1] << 8 | (uint32_t)in[2] << 16; }

// Walk the n positions p0 .. of a slot (in[i] = the original byte at p0 + i for i < n + 4, zeros from d on) from the incoming
// state `st`.  `old`: the incoming state of the walk whose results out[] holds, kZhE8wNone for the first.  Returns the
// outgoing state st(p0 + n), or kZhE8wNone when the walk met the old one before the slot's end (out[] and the outgoing state
// of the old walk stand from there on).  *steps counts the positions walked.
template <class PI, class PO>
ZH_E8W_FN uint32_t zh_e8w_walk(PI in, PO out, uint32_t p0, uint32_t n, uint32_t d, uint32_t st, uint32_t old, uint32_t *steps) {
  uint32_t o3 = n ? (uint32_t)in[3] : 0u;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t o4 = (uint32_t)in[i + 4u];
    const uint32_t w = zh_e8w_step(st, o3, o4, p0 + i, d);
    out[i] = (uint8_t)w;
    st = w >> 8;
    ++*steps;
    if (old != kZhE8wNone) {
      old = zh_e8w_step(old, o3, o4, p0 + i, d) >> 8;
      if (old == st && i + 1u < n) return kZhE8wNone;
    }
    o3 = o4;
  }
  return st;
}

// What a lane keeps through a round: the incoming state its slice was last walked from and the outgoing state it has now
struct ZhE8wLane { uint32_t ist, ost; };

// Step 1 for lane `lane` of the round at `base` (`in` / `out`: the slot buffers): the walk from the clean state, lane 0's
// from `carry`, the outgoing state of lane 63 in the round before (kZhE8wNone in the first round)
template <class PI, class PO>
ZH_E8W_FN void zh_e8w_first(ZhE8wLane &s, PI in, PO out, uint32_t base, uint32_t lane, uint32_t d, uint32_t carry, uint32_t *steps) {
  in += lane * kZhE8wSlot;
  s.ist = lane == 0u && carry != kZhE8wNone ? carry : zh_e8w_clean(in);
  s.ost = zh_e8w_walk(in, out + lane * kZhE8wSlot, base + lane * kZhE8wSlice, zh_e8w_count(base, lane, d), d, s.ist, kZhE8wNone, steps);
}

// Steps 2 and 3 for lane `lane`: `nin` is the outgoing state the lane before it had when this time through step 2 began
// (lane 0 has no lane before it: whatever it is given, its incoming state stands).  Returns whether the incoming state
// changed, and has walked the slice again if so; the round is settled when no lane's did.
template <class PI, class PO>
ZH_E8W_FN bool zh_e8w_retake(ZhE8wLane &s, PI in, PO out, uint32_t base, uint32_t lane, uint32_t d, uint32_t nin, uint32_t *steps) {
  if (lane == 0u || nin == s.ist) return false;
  const uint32_t o = zh_e8w_walk(in + lane * kZhE8wSlot, out + lane * kZhE8wSlot, base + lane * kZhE8wSlice, zh_e8w_count(base, lane, d), d, nin, s.ist, steps);
  if (o != kZhE8wNone) s.ost = o;                         // (the walk met the old one: its outgoing state stands)
  s.ist = nin;
  return true;
}
