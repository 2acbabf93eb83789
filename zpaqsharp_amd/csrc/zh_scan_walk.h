// zh_scan_walk.h — the framing scan of a device-resident stream (zpaqhip_scan_device), as plain integer code shared by
// device and host.  No HIP in here: zh_scan.hip runs it on the GPU over the two lists its streaming pass makes,
// tests/native/scan_walk_main.cpp runs it on the host over lists from a ten-line loop, against zh_framing.cpp's scan_stream.
//
// scan_stream is byte-serial, but only two of its loops are long, and both are searches that are independent per position:
//   findBlock        a rolling hash with multipliers 12 / 20 / 28 / 44.  All are multiples of 4, so after 16 bytes the start
//                    value has left the 32-bit hash: away from a restart, "tag found behind position q" is a pure function of
//                    in[q-16, q).  The TAG HITS are every q in [16, n] whose window has the four target values.
//   Decoder.skip     a modelled segment ends with the first run of at least four zero bytes behind its first non-zero byte,
//                    and takes the whole run.  The ZERO RUNS are every maximal run of at least four zero bytes, (start, end),
//                    a run that reaches n with end = n.
// Everything else touches a few dozen bytes per segment: zh_scan_parse_block is scan_blocks' body for the block whose tag
// ends at q, restated over the bytes and the run list; it runs once per tag hit, all hits in parallel.  zh_scan_chain then
// picks the blocks: from e = 0, the next block is the first position at which findBlock RESTARTED AT e matches.  For
// q - e >= 16 that is the first tag hit; for q - e < 16 the hash still carries the start constants (a bare "zPQ" matches
// three bytes behind a restart, and a full tag whose window straddles e does not match at all), so those at most 15
// positions are tested with the restarted hash and such a block is parsed on the spot.  Hits below the previous block's end
// (a tag in a name, a comment, stored payload or coded data) are passed over.  The chain stops at the first block whose
// parse failed; that block's status is the scan's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zpaqhip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZH_HD __host__ __device__ inline
#else
#define ZH_HD inline
#endif

#define ZH_SCAN_PIECE 4096u               // bytes of the stream per wave of zh_scan.hip's streaming pass (64 lanes x 16 bytes x 4)

// the two lists, sorted by position; run k is [run_start[k], run_end[k])
struct ZhScanLists {
  const uint64_t *tag;
  const uint64_t *run_start, *run_end;
  uint64_t n_tag, n_run;
};

enum {                                    // ZhScanRec::msg
  ZH_SCAN_MSG_NONE = 0, ZH_SCAN_MSG_LEVEL, ZH_SCAN_MSG_TYPE, ZH_SCAN_MSG_EOF, ZH_SCAN_MSG_COMP_TYPE, ZH_SCAN_MSG_COMP_OVER,
  ZH_SCAN_MSG_COMP_END, ZH_SCAN_MSG_HCOMP, ZH_SCAN_MSG_HCOMP_END, ZH_SCAN_MSG_LEVEL1, ZH_SCAN_MSG_SEGMENT,
  ZH_SCAN_MSG_FRAMING_EOF, ZH_SCAN_MSG_RESERVED, ZH_SCAN_MSG_SKIPPED, ZH_SCAN_MSG_SEGEND, ZH_SCAN_N_MSG
};

inline const char *zh_scan_message(uint32_t id) {  // the wording of zh_framing.cpp
  static const char *const kMsg[ZH_SCAN_N_MSG] = {
      "", "unsupported ZPAQ level", "unsupported ZPAQL type", "unexpected end of file", "Invalid component type",
      "COMP overflows header", "missing COMP END", "missing HCOMP", "missing HCOMP END",
      "ZPAQ level 1 requires at least 1 component", "missing segment or end of block", "unexpected EOF",
      "missing reserved byte", "skipped to EOF", "missing end of segment marker"};
  return id < ZH_SCAN_N_MSG ? kMsg[id] : "";
}

// The block whose tag ends at q, as parsed on its own: first_seg is not known yet (0), `seg` counts within the block.
struct ZhScanRec {
  zpaqhip_block b;
  int32_t status;                         // zpaqhip_status
  int32_t seg;                            // segment of the block the status belongs to, or -1
  uint32_t msg;                           // ZH_SCAN_MSG_*
  uint32_t hit_eof;                       // the parse ran into the end of the buffer
};

// What zh_scan_chain found: the counts of the good prefix, and the first damaged block's error (indices of the stream)
struct ZhScanResult {
  uint64_t n_blocks, n_segs;
  int32_t status, err_block, err_seg;
  uint32_t msg, hit_eof;
  uint32_t reserved;
};

struct ZhScanCur {
  const uint8_t *p;
  uint64_t n, pos;
  uint32_t eof_hit;
};
ZH_HD int zh_scan_get(ZhScanCur &c) {
  if (c.pos < c.n) return c.p[c.pos++];
  c.eof_hit = 1;
  return -1;
}

ZH_HD int zh_scan_comp_size(int type) {   // Component.cs:27-43: {0, 2, 3, 2, 3, 4, 6, 6, 3, 5}
  return type >= 0 && type < 10 ? (int)((0x5366432320ull >> (4 * type)) & 15u) : 0;
}

// findBlock's hash (Decompresser.cs:34-45)
struct ZhScanHash { uint32_t h1, h2, h3, h4; };
ZH_HD ZhScanHash zh_scan_hash_start() { return ZhScanHash{0x3D49B113u, 0x29EB7F93u, 0x2614BE13u, 0x3828EB13u}; }
ZH_HD void zh_scan_hash_add(ZhScanHash &h, uint32_t ch) {
  h.h1 = h.h1 * 12 + ch; h.h2 = h.h2 * 20 + ch; h.h3 = h.h3 * 28 + ch; h.h4 = h.h4 * 44 + ch;
}
ZH_HD bool zh_scan_hash_hit(const ZhScanHash &h) {
  return h.h1 == 0xB16B88F1u && h.h2 == 0xFF5376F1u && h.h3 == 0x72AC5BF1u && h.h4 == 0x2F909AF1u;
}
// the tag-hit test of one position: the hashes of in[q-16, q), 16 <= q <= n, from any start value
ZH_HD bool zh_scan_tag_at(const uint8_t *in, uint64_t q) {
  ZhScanHash h{0, 0, 0, 0};
  for (uint64_t i = q - 16; i < q; ++i) zh_scan_hash_add(h, in[i]);
  return zh_scan_hash_hit(h);
}

// ZPAQL.memory(), ZPAQL.cs:58-81 (zh_framing.cpp's model_memory)
ZH_HD double zh_scan_pow2(int x) { double r = 1; for (; x > 0; --x) r += r; return r; }
ZH_HD double zh_scan_model_memory(const uint8_t *hd, uint64_t hsize) {
  double mem = zh_scan_pow2(hd[2] + 2) + zh_scan_pow2(hd[3]) + zh_scan_pow2(hd[4] + 2) + zh_scan_pow2(hd[5]) + (double)(hsize + 300);
  uint64_t cp = 7;
  for (int i = 0; i < hd[6]; ++i) {
    const double size = zh_scan_pow2(hd[cp + 1]);
    switch (hd[cp]) {
      case 2: mem += 4 * size; break;                            // CM
      case 3: mem += 64 * size + 1024; break;                    // ICM
      case 4: mem += 4 * size + zh_scan_pow2(hd[cp + 2]); break; // MATCH
      case 6: mem += 2 * size; break;                            // MIX2
      case 7: mem += 4 * size * hd[cp + 3]; break;               // MIX
      case 8: mem += 64 * size + 2048; break;                    // ISSE
      case 9: mem += 128 * size; break;                          // SSE
    }
    cp += (uint64_t)zh_scan_comp_size(hd[cp]);
  }
  return mem;
}

// The structural checks of ZPAQL.read (zh_framing.cpp's check_header): the header length (hsize + 2), or a negative status
// with *msg.
ZH_HD long zh_scan_check_header(ZhScanCur &c, uint32_t *msg) {
  const uint64_t start = c.pos;
  const int lo = zh_scan_get(c), hi = zh_scan_get(c);
  if (lo < 0 || hi < 0) { *msg = ZH_SCAN_MSG_EOF; return ZPAQHIP_E_EOF; }
  const uint64_t hsize = (uint64_t)lo + 256 * (uint64_t)hi;
  uint64_t cend = 2;
  int n = 0;
  for (int i = 0; i < 5; ++i) {
    const int v = zh_scan_get(c);
    if (v < 0) { *msg = ZH_SCAN_MSG_EOF; return ZPAQHIP_E_EOF; }
    n = v; ++cend;
  }
  for (int i = 0; i < n; ++i) {
    const int type = zh_scan_get(c);
    if (type < 0) { *msg = ZH_SCAN_MSG_EOF; return ZPAQHIP_E_EOF; }
    ++cend;
    const int size = zh_scan_comp_size(type);
    if (size < 1) { *msg = ZH_SCAN_MSG_COMP_TYPE; return ZPAQHIP_E_HEADER; }
    if (cend + (uint64_t)size > hsize) { *msg = ZH_SCAN_MSG_COMP_OVER; return ZPAQHIP_E_HEADER; }
    for (int j = 1; j < size; ++j) {
      if (zh_scan_get(c) < 0) { *msg = ZH_SCAN_MSG_EOF; return ZPAQHIP_E_EOF; }
      ++cend;
    }
  }
  int e = zh_scan_get(c);
  if (e < 0) { *msg = ZH_SCAN_MSG_EOF; return ZPAQHIP_E_EOF; }
  ++cend;
  if (e != 0) { *msg = ZH_SCAN_MSG_COMP_END; return ZPAQHIP_E_HEADER; }
  if (cend + 128 > hsize + 129) { *msg = ZH_SCAN_MSG_HCOMP; return ZPAQHIP_E_HEADER; }
  const uint64_t hlen = hsize + 129 - (cend + 128);     // HCOMP bytes before the END byte: only their presence matters
  if (c.n - c.pos < hlen) { c.pos = c.n; c.eof_hit = 1; *msg = ZH_SCAN_MSG_EOF; return ZPAQHIP_E_EOF; }
  c.pos += hlen;
  e = zh_scan_get(c);
  if (e < 0) { *msg = ZH_SCAN_MSG_EOF; return ZPAQHIP_E_EOF; }
  if (e != 0) { *msg = ZH_SCAN_MSG_HCOMP_END; return ZPAQHIP_E_HEADER; }
  return (long)(c.pos - start);
}

ZH_HD uint64_t zh_scan_parse_size(const uint8_t *p, uint64_t n) {
  if (n == 0 || p[0] < '0' || p[0] > '9') return UINT64_MAX;
  uint64_t v = 0;
  for (uint64_t i = 0; i < n && p[i] >= '0' && p[i] <= '9'; ++i) {
    if (v > (UINT64_MAX - 9) / 10) return UINT64_MAX;
    v = v * 10 + (uint64_t)(p[i] - '0');
  }
  return v;
}

// the first listed run that starts at or behind `from`: its index, or n_run
ZH_HD uint64_t zh_scan_first_run_from(const ZhScanLists &L, uint64_t from) {
  uint64_t lo = 0, hi = L.n_run;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (L.run_start[mid] < from) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Decoder.skip's modelled branch (Decoder.cs:73-81) from c.pos = data_off: leaves c.pos behind the coded data and returns the
// byte that follows it (the cursor past that byte), or -1 at the end of the buffer.
ZH_HD int zh_scan_skip_modelled(ZhScanCur &c, const ZhScanLists &L) {
  // leading zeros: a listed run that holds data_off is jumped through; fewer than four are read
  if (c.pos < c.n && c.p[c.pos] == 0) {
    const uint64_t k = zh_scan_first_run_from(L, c.pos + 1);    // the run before it is the last that starts at or before pos
    if (k > 0 && L.run_end[k - 1] > c.pos) c.pos = L.run_end[k - 1];
  }
  int v;
  do v = zh_scan_get(c); while (v == 0);
  if (v < 0) return -1;                                         // nothing but zeros up to the end
  // c.pos - 1 holds the first non-zero byte: the data ends with the first listed run behind it, whole
  const uint64_t k = zh_scan_first_run_from(L, c.pos);
  if (k == L.n_run) { c.pos = c.n; c.eof_hit = 1; return -1; }
  c.pos = L.run_end[k];
  return zh_scan_get(c);
}

// scan_blocks' body for the block whose tag ends at q (the level byte is in[q]).  With `segs` the block's segment records
// are written to segs[0 .. min(n_seg, seg_cap)), their owner being `block`.
ZH_HD void zh_scan_parse_block(const uint8_t *in, uint64_t n, const ZhScanLists &L, uint64_t q, ZhScanRec &r,
                               zpaqhip_segment *segs, uint64_t seg_cap, uint32_t block) {
  ZhScanCur c{in, n, q, 0};
  zpaqhip_block b{};
  r.status = ZPAQHIP_OK; r.seg = -1; r.msg = ZH_SCAN_MSG_NONE;
#define ZH_SCAN_FAIL(code, s, m) do { r.status = (code); r.seg = (s); r.msg = (m); r.hit_eof = c.eof_hit; r.b = b; return; } while (0)
  b.tag_off = q >= 16 ? q - 16 : 0;
  const int level = zh_scan_get(c);
  if (level != 1 && level != 2) ZH_SCAN_FAIL(ZPAQHIP_E_LEVEL, -1, ZH_SCAN_MSG_LEVEL);
  if (zh_scan_get(c) != 1) ZH_SCAN_FAIL(ZPAQHIP_E_LEVEL, -1, ZH_SCAN_MSG_TYPE);
  b.level = (uint8_t)level;
  b.hdr_off = c.pos;
  uint32_t msg = 0;
  const long hl = zh_scan_check_header(c, &msg);
  if (hl < 0) ZH_SCAN_FAIL((int)hl, -1, msg);
  b.hdr_len = (uint32_t)hl;
  const uint8_t *hd = in + b.hdr_off;
  b.hh = hd[2]; b.hm = hd[3]; b.ph = hd[4]; b.pm = hd[5]; b.n_comp = hd[6];
  if (level == 1 && b.n_comp == 0) ZH_SCAN_FAIL(ZPAQHIP_E_LEVEL, -1, ZH_SCAN_MSG_LEVEL1);
  b.model_mem = zh_scan_model_memory(hd, (uint64_t)hl - 2);
  b.usize_hint = 0;
  uint32_t ns = 0;
  for (;;) {
    const int t = zh_scan_get(c);                               // findFilename, Decompresser.cs:67-93
    if (t == 255) break;
    if (t != 1) ZH_SCAN_FAIL(ZPAQHIP_E_SEGMENT, (int)ns, ZH_SCAN_MSG_SEGMENT);
    zpaqhip_segment s{};
    s.block = block;
    s.name_off = c.pos;
    for (;;) {
      const int v = zh_scan_get(c);
      if (v == -1) ZH_SCAN_FAIL(ZPAQHIP_E_FRAMING_EOF, (int)ns, ZH_SCAN_MSG_FRAMING_EOF);
      if (v == 0) break;
    }
    s.name_len = (uint32_t)(c.pos - 1 - s.name_off);
    s.comment_off = c.pos;                                      // readComment, Decompresser.cs:96-108
    for (;;) {
      const int v = zh_scan_get(c);
      if (v == -1) ZH_SCAN_FAIL(ZPAQHIP_E_FRAMING_EOF, (int)ns, ZH_SCAN_MSG_FRAMING_EOF);
      if (v == 0) break;
    }
    s.comment_len = (uint32_t)(c.pos - 1 - s.comment_off);
    if (zh_scan_get(c) != 0) ZH_SCAN_FAIL(ZPAQHIP_E_RESERVED, (int)ns, ZH_SCAN_MSG_RESERVED);
    s.usize_hint = zh_scan_parse_size(in + s.comment_off, s.comment_len);
    s.data_off = c.pos;
    int nx;                                                     // byte after the coded data
    if (b.n_comp) {
      nx = zh_scan_skip_modelled(c, L);
    } else {
      // unmodelled store path (Decoder.cs:84-96): [len32 big-endian, bytes]*, len 0 ends
      uint32_t curr = 0;
      int v = 0;
      for (int i = 0; i < 4 && (v = zh_scan_get(c)) >= 0; ++i) curr = curr << 8 | (uint32_t)v;
      while (curr > 0 && v >= 0) {
        if (c.n - c.pos < curr) { c.eof_hit = 1; ZH_SCAN_FAIL(ZPAQHIP_E_EOF, (int)ns, ZH_SCAN_MSG_SKIPPED); }
        c.pos += curr;
        curr = 0;
        for (int i = 0; i < 4 && (v = zh_scan_get(c)) >= 0; ++i) curr = curr << 8 | (uint32_t)v;
      }
      nx = v >= 0 ? zh_scan_get(c) : -1;
    }
    s.data_len = (nx >= 0 ? c.pos - 1 : c.pos) - s.data_off;
    if (nx == 254) s.flags = 0;                                 // readSegmentEnd, Decompresser.cs:177-193
    else if (nx == 253) {
      s.flags = 1;
      for (int i = 0; i < 20; ++i) s.sha1[i] = (uint8_t)zh_scan_get(c);   // the reference stores get() even at EOF
    } else ZH_SCAN_FAIL(ZPAQHIP_E_SEGEND, (int)ns, ZH_SCAN_MSG_SEGEND);
    if (b.usize_hint != UINT64_MAX) {
      if (s.usize_hint == UINT64_MAX) b.usize_hint = UINT64_MAX;
      else b.usize_hint += s.usize_hint;
    }
    if (segs && ns < seg_cap) segs[ns] = s;
    ++ns;
  }
#undef ZH_SCAN_FAIL
  b.n_seg = ns;
  b.end_off = c.pos;
  r.b = b;
  r.hit_eof = c.eof_hit;
}

// The chain over the per-hit records recs[0 .. L.n_tag).  The first block_cap chosen blocks are written to `blocks` with
// their first_seg; R counts all of them.
ZH_HD void zh_scan_chain(const uint8_t *in, uint64_t n, const ZhScanLists &L, const ZhScanRec *recs, zpaqhip_block *blocks,
                         uint64_t block_cap, ZhScanResult &R) {
  R = ZhScanResult{};
  R.err_block = R.err_seg = -1;
  uint64_t e = 0, ti = 0;
  for (;;) {
    // findBlock restarted at e: the at most 15 positions at which the hash still carries the start constants
    ZhScanHash h = zh_scan_hash_start();
    const uint64_t last = n - e < 15 ? n : e + 15;
    uint64_t q = e;
    bool near = false;
    while (q < last) {
      zh_scan_hash_add(h, in[q++]);
      if (zh_scan_hash_hit(h)) { near = true; break; }
    }
    ZhScanRec own;
    const ZhScanRec *r = &own;
    if (near) zh_scan_parse_block(in, n, L, q, own, nullptr, 0, 0);
    else {
      while (ti < L.n_tag && L.tag[ti] < e + 16) ++ti;          // inside the previous block, or a window that straddles e
      if (ti == L.n_tag) return;
      r = &recs[ti];
    }
    if (r->status) {
      R.status = r->status; R.msg = r->msg; R.hit_eof = r->hit_eof;
      R.err_block = (int32_t)R.n_blocks;
      R.err_seg = r->seg < 0 ? -1 : (int32_t)(R.n_segs + (uint64_t)r->seg);
      return;
    }
    if (R.n_blocks < block_cap) {
      zpaqhip_block b = r->b;
      b.first_seg = (uint32_t)R.n_segs;
      blocks[R.n_blocks] = b;
    }
    ++R.n_blocks;
    R.n_segs += r->b.n_seg;
    e = r->b.end_off;
  }
}

// The segment records of chosen block `bi` at their final indices in segs[0 .. seg_cap): the block parsed once more, writing.
ZH_HD void zh_scan_fill_segments(const uint8_t *in, uint64_t n, const ZhScanLists &L, const zpaqhip_block &b, uint32_t bi,
                                 zpaqhip_segment *segs, uint64_t seg_cap) {
  if (b.first_seg >= seg_cap) return;
  ZhScanRec r;
  zh_scan_parse_block(in, n, L, b.hdr_off - 2, r, segs + b.first_seg, seg_cap - b.first_seg, bi);
}
