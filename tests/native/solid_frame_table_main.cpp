// A stand-alone check of zh_frame.h's frame table (zh_frame_table.cpp's build_frame_table) on blocks of several segments,
// whose coded bytes lie back to back in one slot, cut at the ends the encoders record.  The table is played
// the way the host copy and zh_frame.hip play it (head || body || tail of every entry at its dst_off) into a buffer of
// sentinels, against a stream assembled byte by byte from the format alone.  tests/test_solid_frame.py builds it with
// -fsanitize=address,undefined and runs it; it prints one line per check and exits non-zero at the first that fails.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zh_frame.h"

using namespace zh;

static int n_checks = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    ++n_checks;                                                        \
    if (!(c)) {                                                        \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);            \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

static const uint8_t kHdr[] = {7, 0, 1, 2, 3, 4, 9, 0, 0};           // any bytes: the frame copies them
static const uint8_t kSentinel = 0xA5;

struct Seg { std::string name; bool named; uint64_t plain, coded; };
struct Block { std::vector<Seg> seg; };

struct Batch {
  std::vector<Block> blocks;
  std::vector<uint8_t> slots;                       // every block's slot, 256-byte aligned, filled with a pattern
  std::vector<uint64_t> slot_off;
  std::vector<std::vector<uint32_t>> digest;        // five words per segment
  std::vector<TableBlock> items;
};

static Batch make_batch(const std::vector<Block> &blocks, bool sha) {
  Batch B;
  B.blocks = blocks;
  uint32_t salt = 1;
  for (const Block &b : blocks) {
    uint64_t total = 0;
    for (const Seg &s : b.seg) total += s.coded;
    B.slot_off.push_back(B.slots.size());
    const size_t at = B.slots.size();
    B.slots.resize(at + (total + 255) / 256 * 256 + 256);
    for (size_t i = at; i < B.slots.size(); ++i) B.slots[i] = (uint8_t)((i * 131 + salt * 17) ^ (i >> 8));
    ++salt;
  }
  for (const Block &b : blocks) {
    B.digest.emplace_back();
    for (size_t s = 0; s < b.seg.size(); ++s)
      for (uint32_t w = 0; w < 5; ++w) B.digest.back().push_back(0x01020304u * (w + 1) + (uint32_t)s * 0x10001u + salt++);
  }
  for (size_t j = 0; j < blocks.size(); ++j) {
    TableBlock it;
    it.src = ZH_FRAME_SRC_FIRST;
    it.src_off = B.slot_off[j];
    uint64_t end = 0;
    for (size_t s = 0; s < blocks[j].seg.size(); ++s) {
      const Seg &sg = blocks[j].seg[s];
      end += sg.coded;
      it.seg.push_back({sg.named ? sg.name.c_str() : nullptr, sg.plain, sha ? &B.digest[j][5 * s] : nullptr, end});
    }
    B.items.push_back(it);
  }
  for (size_t j = 0; j < blocks.size(); ++j)          // (the names' storage moved with the copy of `blocks`: point at B's own)
    for (size_t s = 0; s < blocks[j].seg.size(); ++s)
      if (B.blocks[j].seg[s].named) B.items[j].seg[s].filename = B.blocks[j].seg[s].name.c_str();
  return B;
}

// the stream of one block, byte by byte, from the format: tag, block header, segments, end of block
static std::vector<uint8_t> assemble(const Batch &B, size_t j, bool tag, bool sha) {
  static const uint8_t kTag[13] = {0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3};
  std::vector<uint8_t> w;
  if (tag) w.insert(w.end(), kTag, kTag + 13);
  for (char c : {'z', 'P', 'Q'}) w.push_back((uint8_t)c);
  w.push_back(1);
  w.push_back(1);
  w.insert(w.end(), kHdr, kHdr + sizeof kHdr);
  uint64_t from = 0;
  for (size_t s = 0; s < B.blocks[j].seg.size(); ++s) {
    const Seg &sg = B.blocks[j].seg[s];
    w.push_back(1);
    if (sg.named) for (char c : sg.name) w.push_back((uint8_t)c);
    w.push_back(0);
    char num[32];
    snprintf(num, sizeof num, "%llu", (unsigned long long)sg.plain);
    for (const char *p = num; *p; ++p) w.push_back((uint8_t)*p);
    w.push_back(0);
    w.push_back(0);
    for (uint64_t i = 0; i < sg.coded; ++i) w.push_back(B.slots[B.slot_off[j] + from + i]);
    from += sg.coded;
    for (int i = 0; i < 4; ++i) w.push_back(0);
    if (sha) {
      w.push_back(253);
      for (uint32_t k = 0; k < 5; ++k)
        for (int sh = 24; sh >= 0; sh -= 8) w.push_back((uint8_t)(B.digest[j][5 * s + k] >> sh));
    } else w.push_back(254);
  }
  w.push_back(255);
  return w;
}

// what the host copy and the packing kernel do with a table
static void play(const FrameTable &T, const Batch &B, std::vector<uint8_t> &out) {
  for (const ZhFrameEntry &e : T.entry) {
    CHECK(e.store == 0 && e.src == ZH_FRAME_SRC_FIRST);
    CHECK(e.head_off + e.head_len <= T.blob.size() && e.tail_off + e.tail_len <= T.blob.size());
    CHECK(e.src_off + e.body_len <= B.slots.size());
    CHECK(e.dst_off + e.head_len + e.body_len + e.tail_len <= out.size());
    uint8_t *w = out.data() + e.dst_off;
    for (uint64_t i = 0; i < e.head_len + e.body_len + e.tail_len; ++i) CHECK(w[i] == kSentinel);   // no byte is written twice
    if (e.head_len) memcpy(w, T.blob.data() + e.head_off, e.head_len);
    if (e.body_len) memcpy(w + e.head_len, B.slots.data() + e.src_off, e.body_len);
    if (e.tail_len) memcpy(w + e.head_len + e.body_len, T.blob.data() + e.tail_off, e.tail_len);
  }
}

// the whole batch at every interesting capacity: block_pos, the return value, which blocks are in, and the bytes
static void run(const char *what, const std::vector<Block> &blocks, bool sha, bool tag, uint64_t pos0, uint32_t want_pieces = 0) {
  const Batch B = make_batch(blocks, sha);
  std::vector<std::vector<uint8_t>> want;
  std::vector<uint64_t> pos(blocks.size() + 1, pos0);
  for (size_t j = 0; j < blocks.size(); ++j) {
    want.push_back(assemble(B, j, tag, sha));
    pos[j + 1] = pos[j] + want[j].size();
  }
  std::vector<uint64_t> caps = {~0ull, pos.back(), pos.back() - 1, pos0, 0};
  for (size_t j = 0; j < blocks.size(); ++j) {
    caps.push_back(pos[j]);                            // between two blocks
    caps.push_back(pos[j] + 1);                        // inside one: in its head,
    caps.push_back(pos[j] + want[j].size() / 2);       // in its middle
    caps.push_back(pos[j + 1] - 1);                    // and one byte short of its end
  }
  for (uint64_t cap : caps) {
    FrameTable T;
    std::vector<uint64_t> bp(blocks.size(), 77);
    CHECK(build_frame_table(tag, 1, kHdr, sizeof kHdr, B.items, nullptr, pos0, cap, T, bp.data()) == pos.back());
    CHECK(T.entry.size() == T.item.size() && T.sel_len == 0);
    const uint64_t size = cap == ~0ull ? pos.back() : cap;
    std::vector<uint8_t> out(size + 64, kSentinel);    // (+ 64: what lies behind out_cap must stay as it is)
    for (const ZhFrameEntry &e : T.entry) CHECK(e.dst_off + e.head_len + e.body_len + e.tail_len <= size);
    play(T, B, out);
    std::vector<size_t> n_entries(blocks.size(), 0);
    for (size_t e = 0; e < T.entry.size(); ++e) {
      CHECK(T.item[e] < blocks.size() && (e == 0 || T.item[e] >= T.item[e - 1]));
      ++n_entries[T.item[e]];
    }
    uint32_t pieces = 1;
    for (size_t j = 0; j < blocks.size(); ++j) {
      CHECK(bp[j] == pos[j]);
      const bool fits = pos[j + 1] <= size;            // whole blocks only; offsets only grow, so the blocks that fit are a prefix
      CHECK(n_entries[j] == (fits ? blocks[j].seg.size() : 0));
      for (uint64_t i = pos[j]; i < pos[j + 1] && i < out.size(); ++i) CHECK(out[i] == (fits ? want[j][i - pos[j]] : kSentinel));
      if (fits)
        for (const Seg &s : blocks[j].seg) pieces = std::max<uint32_t>(pieces, (uint32_t)((s.coded + ZH_FRAME_PIECE - 1) / ZH_FRAME_PIECE));
    }
    for (uint64_t i = 0; i < pos0 && i < out.size(); ++i) CHECK(out[i] == kSentinel);
    for (uint64_t i = pos.back(); i < out.size(); ++i) CHECK(out[i] == kSentinel);
    CHECK(T.pieces == pieces);
    if (want_pieces && cap == ~0ull) CHECK(T.pieces == want_pieces);
  }
  // without block_pos
  FrameTable T;
  CHECK(build_frame_table(tag, 1, kHdr, sizeof kHdr, B.items, nullptr, pos0, ~0ull, T, nullptr) == pos.back());
  printf("ok %s\n", what);
}

static Seg seg(const char *name, uint64_t plain, uint64_t coded) { return {name ? name : "", name != nullptr, plain, coded}; }

int main() {
  // one segment: the same bytes, and the single entry of a block framed by hand
  {
    const std::vector<Block> one = {{{seg("file", 1234, 777)}}};
    run("one_segment", one, true, true, 0);
    const Batch B = make_batch(one, true);
    FrameTable S;
    build_frame_table(true, 1, kHdr, sizeof kHdr, B.items, nullptr, 5, ~0ull, S, nullptr);
    const BlockFrame f(true, 1, kHdr, sizeof kHdr, "file", 1234, &B.digest[0][0], true, true);
    ZhFrameEntry want;
    memset(&want, 0, sizeof want);
    want.dst_off = 5;
    want.src = ZH_FRAME_SRC_FIRST;
    want.src_off = B.slot_off[0];
    want.body_len = 777;
    want.head_off = 0;
    want.head_len = (uint32_t)f.head.size();
    want.tail_off = f.head.size();
    want.tail_len = (uint32_t)f.tail.size();
    const std::string blob = f.head + f.tail;
    CHECK(S.entry.size() == 1 && S.item.size() == 1 && S.item[0] == 0 && S.pieces == 1 && S.sel_len == 0);
    CHECK(S.blob == std::vector<uint8_t>(blob.begin(), blob.end()));
    CHECK(memcmp(&S.entry[0], &want, sizeof(ZhFrameEntry)) == 0);
    puts("ok one_segment_is_the_block_form");
  }
  run("empty_first_segment", {{{seg("", 0, 1), seg("b", 500, 300)}}}, true, true, 0);
  run("empty_last_segment", {{{seg("a", 500, 300), seg("b", 0, 1)}}}, true, true, 3);
  run("empty_bodies", {{{seg("a", 0, 0), seg("b", 0, 0), seg("c", 9, 5)}}, {{seg("d", 0, 0)}}}, true, false, 0);   // (an encoder never
                                                       // ends a segment on the byte it began at; the table does not care)
  {
    std::vector<Block> many(1);
    std::vector<std::string> names;
    for (int s = 0; s < 120; ++s) names.push_back("dir/file" + std::to_string(s));
    for (int s = 0; s < 120; ++s) many[0].seg.push_back(seg(names[s].c_str(), (uint64_t)(s * 21) % 2501, (uint64_t)(s * 37) % 1400));
    run("120_segments", many, true, true, 0);
  }
  {
    const std::string long_name(300, 'n');
    run("filenames_0_and_300", {{{seg(nullptr, 5, 9), seg("", 6, 10), seg(long_name.c_str(), 7, 11)}}}, true, true, 0);
  }
  run("no_sha1", {{{seg("a", 100, 64), seg("b", 200, 65)}}, {{seg("c", 300, 255), seg("d", 1, 256), seg("e", 2, 257)}}}, false, true, 0);
  run("no_tag_later_batch", {{{seg("a", 100, 64)}}, {{seg("c", 300, 255), seg("d", 1, 1)}}, {{seg("e", 2, 3)}}}, true, false, 100000);
  run("pieces", {{{seg("a", 1, 10), seg("b", 200000, 70000), seg("c", 3, 4)}}}, true, true, 0, 2);
  // a block of three segments whose first two would fit under out_cap but whose third does not: none of its entries is in
  // the table, the block behind it is out as well, and block_pos and the end are the unbounded ones
  {
    const std::vector<Block> blocks = {{{seg("a", 10, 20)}}, {{seg("b", 100, 64), seg("c", 200, 65), seg("d", 300, 66)}}, {{seg("e", 1, 2)}}};
    const Batch B = make_batch(blocks, true);
    FrameTable full, T;
    std::vector<uint64_t> pos(3), bp(3, 77);
    const uint64_t end = build_frame_table(true, 1, kHdr, sizeof kHdr, B.items, nullptr, 9, ~0ull, full, pos.data());
    CHECK(full.entry.size() == 5 && full.item[1] == 1 && full.item[3] == 1);
    const ZhFrameEntry &third = full.entry[3];
    for (uint64_t cap : {third.dst_off, third.dst_off + third.head_len + third.body_len, pos[2] - 1}) {
      CHECK(full.entry[2].dst_off + full.entry[2].head_len + full.entry[2].body_len + full.entry[2].tail_len <= cap);   // two fit
      CHECK(build_frame_table(true, 1, kHdr, sizeof kHdr, B.items, nullptr, 9, cap, T, bp.data()) == end && bp == pos);
      CHECK(T.entry.size() == 1 && T.item.size() == 1 && T.item[0] == 0);
      CHECK(memcmp(&T.entry[0], &full.entry[0], sizeof(ZhFrameEntry)) == 0);
      CHECK(T.blob.size() == T.entry[0].tail_off + T.entry[0].tail_len);      // and nothing of the block stays in the blob
    }
    CHECK(build_frame_table(true, 1, kHdr, sizeof kHdr, B.items, nullptr, 9, pos[2], T, bp.data()) == end && T.entry.size() == 4);
    puts("ok third_segment_does_not_fit");
  }
  printf("ok %d checks\n", n_checks);
  return 0;
}
