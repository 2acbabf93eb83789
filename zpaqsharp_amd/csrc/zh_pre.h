// zh_pre.h — structures shared by the host side of the method path (zh_pre.cpp) and the pre-processing kernels
// (zh_pre_lz.hip, zh_pre_bwt.hip, zh_pre_lzsa.hip, zh_pre_lzht.hip): LibZPAQ.compressBlock's E8E9 and LZBuffer levels
// 1 / 2 / 3 (LibZPAQ.cs:296-311, LZBuffer.cs:96-115, :205-240).  ZhPreLaunch serves E8E9, the prefix and the greedy
// parse; the routes that sort (BWT, suffix-array and hash-table search) share ZhSlotSpace and its block_of, and their
// arrays are laid out by zh_pre.cpp's SortArena.
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
  uint64_t scr_off;      // first element of this block in ::chain / ::prev; in a ZhSlotSpace: its first slot
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
  uint32_t level;        // args[1] & 3; 3 (BWT): zh_pre_e8e9 writes ::e8 as for 1 / 2, the rest is ZhBwtLaunch's
  uint32_t doe8;         // 4 <= args[1] <= 7
  uint32_t k;            // key length: max(4, args[2]) for level 1, max(args[2], 3) for level 2
  uint32_t m;            // level 2: args[2]
  uint32_t rb;           // level 1: args[0] - 4 when args[0] > 4, else 0
  uint32_t max_match;    // 2^16 (level 1), m + 63 + 256 (level 2)
  uint32_t max_off;      // 2^23 - 1 (level 1), 2^24 - 1 (level 2)
};

// The slot space of one launch of the sort (zh_pre_bwt.hip) and of the routes built on it: the blocks of the launch share
// n = the sum of their sizes <= 2^31 - 1 slots, block b owns the slots starts[b] .. starts[b + 1] - 1.
struct ZhSlotSpace {
  const uint8_t *src;        // block b's bytes at src + blocks[b].in_off (the E8E9 copy when the method asks for it)
  uint8_t *out;              // block b's pre-processed bytes at out + blocks[b].out_off
  const ZhPreBlock *blocks;
  uint64_t *out_len;         // per block (counted past out_cap)
  const uint32_t *starts;    // n_blocks + 1: starts[b] = blocks[b].scr_off, starts[n_blocks] = n
  uint32_t n_blocks, n;
};

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t block_of(const uint32_t *starts, uint32_t n_blocks, uint32_t slot) {   // the block that owns a slot
  uint32_t lo = 0, hi = n_blocks - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (starts[mid] <= slot) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
#endif

// Level 3 (zh_pre_bwt.hip): block b's n + 5 bytes go to ::out.  The arrays are laid out by zh_pre.cpp's SortArena.
struct ZhBwtLaunch : ZhSlotSpace {
  uint32_t *key[2];          // n each: the radix sort's keys, ping and pong
  uint32_t *val[2];          // n each: positions; after a sort, the suffix array
  uint32_t *rank;            // n: first slot of the group of a position
  uint32_t *counts;          // 256 * ceil(n / 4096): digit counts per tile
  uint32_t *sums;            // 2 * ceil(max(n, 256 * tiles) / 4096) + 2: partial results of a scan
  uint32_t *multi;           // positions in groups of two or more after a round
  uint32_t max_n;            // the longest block
  uint32_t pad;
};

// LZBuffer's suffix-array search for levels 1 / 2 (zh_pre_lzsa.hip, LZBuffer.cs:246-283): the slot space, suffix array and
// ranks of a finished ZhBwtLaunch, searched for all blocks of the launch at once.
#define ZH_LZSA_MAX_MATCH 49152u   // maxMatch = BUFSIZE * 3 (LZBuffer.cs:45, :172)
#define ZH_LZSA_MAX_LITERAL 4096u  // maxLiteral = BUFSIZE / 4 (LZBuffer.cs:174)

// a decision: offset (24 bits, 0 = a literal) | blen << 24 (16 bits) | blit << 40 (8 bits) | 1 << 48 where the compare
// stopped at blen and the walk extends the match (zh_pre_lzht.hip only)
struct ZhLzsaLaunch : ZhSlotSpace {
  const uint32_t *sa;        // n: the position (as a slot number) of the suffix in each slot
  const uint32_t *rank;      // n: the slot of each position
  uint32_t *lcp;             // n: min(common prefix of the suffixes in slots j - 1 and j, ZH_LZSA_MAX_MATCH); 0 at a block's first slot
  uint64_t *dec[2];          // n each: the decision of a position visited with lit == 0 ([0]) or lit > 0 ([1])
  uint32_t level;            // 1 or 2
  uint32_t min_match;        // args[2]
  uint32_t bucket;           // 2^args[4] - 1 neighbours per side
  uint32_t lookahead;        // args[6], at most 255
  uint32_t win_bits;         // 17 + args[0]: the window of the reference's inverse array
  uint32_t rb;               // level 1: args[0] - 4 when args[0] > 4, else 0
};

// LZBuffer's hash-table search for levels 1 / 2 (zh_pre_lzht.hip, LZBuffer.cs:285-327, :349-368) with minMatch2 = lookahead
// = 0.  The table is never built: the positions of a launch are sorted by the slot they are stored in, and ht[s] when i
// is searched is the predecessor of (s, i) in that order.
#define ZH_LZHT_CMP 256u           // bytes a lane of zh_lzht_search compares at most; a match that reaches it is extended by the walk
#define ZH_LZHT_MAX_BUCKET_BITS 6  // args[4] at most on this route

struct ZhLzhtLaunch : ZhSlotSpace {
  const uint32_t *key;       // n: the slots of the stored positions in ascending order, then `absent` for the others
  const uint32_t *val;       // n: the position (as a slot number of the launch) of each key; ascending among equal keys
  uint64_t *dec[2];          // n each: the decision of a position visited with lit == 0 ([0]) or lit > 0 ([1]); key, val and
                             // dec[1] are set by zh_launch_pre_lzht
  uint32_t level;            // 1 or 2
  uint32_t min_match;        // args[2]
  uint32_t bucket;           // 2^args[4] - 1: slots h1 ^ 0 .. h1 ^ bucket are searched
  uint32_t ht_bits;          // args[5]: a slot has this many bits; the key of a position that is not stored is 1 << ht_bits
  uint32_t checkbits;        // 12 - args[0]
  uint32_t shift1;           // (args[5] - 1) / args[2] + 1
  uint32_t search;           // 0: level 2 with args[2] > 64, all literals (LZBuffer.cs:288)
  uint32_t rb;               // level 1: args[0] - 4 when args[0] > 4, else 0
};

// zh_pre_bwt.hip's stable radix sort of the pairs (key[*c], val[*c]) of a launch by the low `bits` bits of the key; the
// result is in key[*c] / val[*c] again (rank, multi and out are not touched).  *launches grows by the kernels launched.
extern "C" hipError_t zh_launch_pre_sort(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *c, uint32_t bits);
