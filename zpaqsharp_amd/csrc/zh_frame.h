// zh_frame.h — block framing: the bytes around a block's coded data (BlockFrame), the store layout, and the frame table
// of a batch, which says where every block's head, body and tail go in the stream.  The host forms of the compressing entry
// points copy by it on the host; the device forms upload it and zh_frame.hip packs the stream on the GPU.  Nothing here
// needs HIP: zh_frame_table.cpp builds alone (the programs under tests/native link it under the sanitizers).
#pragma once
#include <stdint.h>

// One block of the stream, for zh_frame.hip: head || body || tail at out + dst_off.  head and tail lie in the batch's blob;
// the body is body_len bytes at src_off of the buffer `src` selects, written as they are or, with `store`, behind the
// selector in the store layout (write_store_body).
struct ZhFrameEntry {
  uint64_t dst_off;
  uint64_t src_off, body_len;
  uint64_t head_off, tail_off;
  uint32_t head_len, tail_len;
  uint32_t src;                           // ZH_FRAME_SRC_*
  uint32_t store;
};

enum {
  ZH_FRAME_SRC_FIRST = 0,                 // the slots of the batch's first encoder run
  ZH_FRAME_SRC_REDO = 1,                  // the worst-case slots of the overflow retry
  ZH_FRAME_SRC_PRE = 2,                   // the batch's coded sequences (store layout: the pre-processed bytes)
  ZH_FRAME_SRC_INPUT = 3,                 // the caller's device input (staging)
  ZH_FRAME_N_SRC = 4
};

struct ZhFrameLaunch {
  const ZhFrameEntry *table;
  const uint8_t *blob;
  const uint8_t *src[ZH_FRAME_N_SRC];
  uint8_t *out;
  uint64_t sel_off, sel_len;              // store layout: the selector prefix in the blob
  uint32_t n;                             // entries
  uint32_t pieces;                        // 64 KiB pieces of the longest body: sizes the grid
};

#define ZH_FRAME_PIECE 65536u             // body bytes per workgroup step; the store layout's chunk

#include <string>
#include <vector>

namespace zh {

// What the coded sequence starts with (Compressor.postProcess, Compressor.cs:156-190): 0, or 1, len lo, len hi, pcomp
std::vector<uint8_t> selector_prefix(const uint8_t *pcomp, size_t pcomp_len);

// The bytes around one block's coded data (LibZPAQ.cs:296-323; BlockWriter::write_block): tag, block and segment header
// with the size comment in `head`, end of segment (with the SHA-1 when `digest` gives its five words) and of block in `tail`.
struct BlockFrame {
  std::string head, tail;
  // One segment of a block (Compressor.startSegment .. endSegment, repeated for a block that holds several): tag and block
  // header go in front of the `first` segment's head only, the end of block behind the `last` one's tail only.
  BlockFrame(bool tag, uint8_t level, const uint8_t *hdr, size_t hdr_len, const char *filename, uint64_t plain_len,
             const uint32_t *digest, bool first, bool last);
};
// Encoder.compress without a model (Encoder.cs:39-73): the decoded stream, `sel` then `pre`, in chunks of at most 65 536
// bytes behind their 4-byte big-endian lengths.
uint64_t store_body_len(uint64_t decoded);
void write_store_body(uint8_t *w, const std::vector<uint8_t> &sel, const uint8_t *pre, uint64_t pre_len);

// One block of a batch as the framing sees it: its segments' coded bytes lie back to back at src_off of the buffer `src`
// selects.  Segment s has the bytes [seg[s - 1].end, seg[s].end) of them (from 0 for the first): `end` is the encoder's count
// right behind the segment's end-of-segment bit (ZhEncLaunch::seg_end), or, for the one segment of a block that no encoder
// cut, the length of the whole (store layout: of the pre-processed bytes).
struct TableSeg {
  const char *filename;                   // NULL = empty
  uint64_t plain_len;                     // the size comment
  const uint32_t *digest;                 // five words, or NULL = no SHA-1
  uint64_t end;
};
struct TableBlock {
  uint32_t src;
  uint64_t src_off;
  std::vector<TableSeg> seg;              // at least one
};

struct FrameTable {
  std::vector<ZhFrameEntry> entry;        // the segments of the blocks that fit under out_cap, in stream order
  std::vector<size_t> item;               // entry[e] frames a segment of item[e] of the batch
  std::vector<uint8_t> blob;              // the selector (store layout), then head and tail of every entry
  uint64_t sel_len = 0;
  uint32_t pieces = 1;                    // 64 KiB pieces of the longest sel_len + body_len
};

// The frame table of a batch whose first block starts at stream offset `pos`: an entry per segment, head || body || tail,
// the first segment's head behind the tag and the block header (with `level`), the last one's tail in front of the end of
// block (BlockFrame writes them all).  block_pos[j] (optional) is where block j starts; a block's entries are in the table
// when the WHOLE block fits under out_cap, else none of them is.  `sel` non-NULL selects the store layout, which is one
// segment per block: a block of several is refused (kFrameRefused comes back, T is empty).  Returns the stream offset
// behind the batch.
constexpr uint64_t kFrameRefused = ~0ull;
uint64_t build_frame_table(bool tag, uint8_t level, const uint8_t *hdr, size_t hdr_len, const std::vector<TableBlock> &items,
                           const std::vector<uint8_t> *sel, uint64_t pos, uint64_t out_cap, FrameTable &T, uint64_t *block_pos);

// The gather table of a mixed call (zpaqhip_compress_mixed_blocks_device): item i is block i of the call, framed already,
// `len` bytes at `src_off` of the call's scratch stream, where the blocks lie group by group.  The stream has them in input
// order from offset 0: block_pos[i] (optional) is the running sum, and every block that fits in whole under out_cap gets a
// body-only entry (no head, no tail, src = ZH_FRAME_SRC_FIRST, as they are).  build_frame_table's rule, settled: the
// offsets only grow, so a block behind one that did not fit starts past out_cap and does not fit either, not even an
// empty one; the entries are a prefix of the blocks, item[e] == e.  Returns the bytes the whole stream needs.
struct GatherItem { uint64_t src_off, len; };
uint64_t build_gather_table(const std::vector<GatherItem> &items, uint64_t out_cap, FrameTable &T, uint64_t *block_pos);

}  // namespace zh
