// zh_analyze.h — shared by the host side of zpaqhip_gap_hist_blocks (zh_pre.cpp) and its kernel (zh_analyze.hip); the load
// rule below is plain arithmetic, so a host program can play it too (tests/native/gap_walk_main.cpp).
#pragma once
#include <stdint.h>

#define ZH_GAP_NR 4096u            // gaps below this are counted (LibZPAQ.cs:243); also the warm-up of a slice
#define ZH_GAP_SLICE 12288u        // bytes one lane counts; with the warm-up its walk stays below 2^16 positions

#ifdef __HIPCC__
#define ZH_GAP_HD __host__ __device__
#else
#define ZH_GAP_HD
#endif

struct ZhGapLaunch {
  const uint8_t *in;         // the plaintext: the call's aligned copy of a batch, or the caller's device memory as it is
  const uint64_t *in_off;    // n_blocks + 1 offsets; block b's bytes start at in + in_off[b] - base
  uint64_t base;
  uint32_t *hist;            // n_blocks x ZH_GAP_NR counters, zero before the launch
};

// The slice that starts at byte s of a block of n bytes (s < n): it counts positions [s, e) and walks [w0, e), the
// warm-up of at most ZH_GAP_NR bytes included.
struct ZhGapSlice { uint32_t w0, e; };
ZH_GAP_HD inline ZhGapSlice zh_gap_slice(uint32_t n, uint32_t s) {
  ZhGapSlice c;
  c.e = n - s < ZH_GAP_SLICE ? n : s + ZH_GAP_SLICE;
  c.w0 = s >= ZH_GAP_NR ? s - ZH_GAP_NR : 0;
  return c;
}

// The load rule of a walk [w0, e) of the block whose first byte has the absolute address `block`: 16 bytes per load, each
// aligned on the address itself, and only groups that hold at least one byte of the walk.  The first load is the group at
// `addr`, whose first byte has walk position r0 (-15..0, relative to w0); with the first byte of a loaded group at walk
// position r, the group behind it is loaded iff zh_gap_load_next(r, e - w0), which is how the one-ahead load stops at the
// last such group.
struct ZhGapFirst { uint64_t addr; int32_t r0; };
ZH_GAP_HD inline ZhGapFirst zh_gap_first_load(uint64_t block, uint32_t w0) {
  const uint64_t p = block + w0;
  ZhGapFirst f;
  f.addr = p & ~15ull;
  f.r0 = -(int32_t)(p & 15);
  return f;
}
ZH_GAP_HD inline bool zh_gap_load_next(int64_t r, uint32_t len) { return r + 16 < (int64_t)len; }
