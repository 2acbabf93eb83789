// zh_pre.h — structures shared by the host side of the method path (zh_pre.cpp) and the pre-processing kernels
// (zh_pre_lz.hip): LibZPAQ.compressBlock's E8E9 and LZBuffer levels 1 / 2 (LibZPAQ.cs:296-311, LZBuffer.cs:96-115).
//
// The parse is the one tools/methods._matches writes: every position p <= n - k is a dictionary entry, prev[i] is the
// largest j < i whose k bytes equal those at i, position i starts a match iff prev[i] exists within max_off, the match is
// as long as it can be (up to max_match and the end of the block) and the walk is greedy.
#pragma once
#include <stdint.h>

#define ZH_PRE_EXT 32u             // zh_pre_lz_prev stores min(LCP - k, ZH_PRE_EXT); the walk extends a match that reaches it

struct ZhPreBlock {
  uint64_t in_off;       // plaintext in ZhPreLaunch::in; its E8E9 copy (levels 1 / 2) at the same offset in ::e8
  uint64_t n;            // plaintext bytes
  uint64_t out_off;      // pre-processed bytes in ::out
  uint64_t out_cap;      // their bound (zh::pre_bound); the kernels count past it but never write past it
  uint64_t scr_off;      // first element of this block in ::chain / ::prev
  uint64_t tab_off;      // first element of this block's hash table in ::table
  uint32_t tab_bits;     // the table has 1 << tab_bits entries
  uint32_t pad;
};

struct ZhPreLaunch {
  const uint8_t *in;
  uint8_t *e8;           // E8E9 output when the level is 1 or 2 (the parse reads it); level 0 writes E8E9 to ::out
  uint8_t *out;
  const ZhPreBlock *blocks;
  uint64_t *out_len;     // per block: pre-processed bytes (counted past out_cap)
  int32_t *table;        // per block: last position entered per bucket, -1 = none (the host clears it)
  int32_t *chain;        // per position: the previous position of the same bucket, or -1
  uint32_t *prev;        // per position: distance to prev[i] << 8 | min(LCP - k, ZH_PRE_EXT), or 0 (no match starts here)
  uint32_t n_blocks;
  uint32_t level;        // 0, 1 or 2 (args[1] & 3)
  uint32_t doe8;         // 4 <= args[1] <= 7
  uint32_t k;            // key length: max(4, args[2]) for level 1, max(args[2], 3) for level 2
  uint32_t m;            // level 2: args[2]
  uint32_t rb;           // level 1: args[0] - 4 when args[0] > 4, else 0
  uint32_t max_match;    // 2^16 (level 1), m + 63 + 256 (level 2)
  uint32_t max_off;      // 2^23 - 1 (level 1), 2^24 - 1 (level 2)
};
