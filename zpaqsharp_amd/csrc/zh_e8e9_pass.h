// zh_e8e9_pass.h — the one driver of zh_e8e9_wave.h's schedule on a wave: the end-of-segment E8E9 loop over the d bytes of
// a flat buffer, round by round.  A round is loaded into the slot buffers (zh_e8e9_round.h), walked by every lane
// (zh_e8w_first), settled — outgoing states pass up one lane and the lanes whose incoming state changed walk again
// (zh_e8w_retake) until a ballot is empty — and its final bytes are stored back to the flat buffer and, below `room`, to
// `outp`, a byte per lane (it begins anywhere).  Lane 63's outgoing state is carried to the next round.
// The callers (zh_store.hip e8_pass, zh_nibble.hip nb_e8_pass) are noinline wrappers: they own the two slot buffers
// (kZhE8wBuf bytes each in LDS, at the 4-aligned byte offsets in0 and out0), say how the flat buffer is read and written
// (rd, wr: zh_e8e9_round.h) and whether it is written at all (to_dst), and do what their kernel needs before and after.
// All 64 lanes of the wave call it with the same arguments but `lane`; it waits on no other wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zh_e8e9_round.h"

template <class RD, class WR>
__device__ __forceinline__ void zh_e8w_pass(RD rd, WR wr, bool to_dst, uint32_t in0, uint32_t out0, uint8_t *outp, uint64_t room, uint32_t d, uint32_t lane) {
  static_assert(kZhE8wLanes == 64u && kZhE8wBuf % 4u == 0u, "a lane per slice, dword slots");
  typedef __attribute__((address_space(3))) uint8_t *u8_p;
  typedef __attribute__((address_space(3))) uint32_t *u32_p;
  uint32_t carry = kZhE8wNone;
  for (uint32_t base = 0; base < d; base += kZhE8wRound) {
    zh_e8w_load(rd, (u32_p)in0, base, d, lane);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    ZhE8wLane s;
    uint32_t steps = 0;
    zh_e8w_first(s, (u8_p)in0, (u8_p)out0, base, lane, d, carry, &steps);
    // (the ballot is empty after 64 walks at most, whatever the data: zh_e8e9_wave.h.  The bound is a safety net on a shared
    // machine, not an exit the loop can take; tests/e8w_harness.py fails where it would be reached)
    for (uint32_t pass = 0; pass <= kZhE8wLanes; ++pass) {
      const uint32_t prev = (uint32_t)__shfl_up((int)s.ost, 1);
      if (__ballot(zh_e8w_retake(s, (u8_p)in0, (u8_p)out0, base, lane, d, prev, &steps)) == 0ull) break;
    }
    carry = (uint32_t)__builtin_amdgcn_readlane((int)s.ost, 63);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (to_dst) zh_e8w_store(wr, (u32_p)out0, base, d, lane);
    const uint32_t nr = zh_e8w_round_len(base, d);
    for (uint32_t j = lane; j < nr; j += 64u) {
      const uint32_t p = base + j;
      if ((uint64_t)p < room) outp[p] = *(u8_p)(out0 + zh_e8w_slot(j));
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  __builtin_amdgcn_s_waitcnt(0);                          // the flat buffer is complete (L2) before anything reads it again
}
