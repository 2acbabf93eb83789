// A stand-alone check of zh_frame.h's host side (zh_frame_table.cpp): BlockFrame's bytes, the store layout and the frame
// table of hand-made batches.  tests/test_compress_device.py builds it with -fsanitize=address,undefined and runs it; it
// prints one line per check and exits non-zero at the first that fails.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static const uint8_t kHdr[] = {5, 0, 1, 2, 3, 4, 0};                 // any bytes: the frame copies them
static const char *kNames[] = {nullptr, "a", "bc", "def", "ghij"};

// a batch of one-segment blocks, and the frame BlockFrame gives each on its own
struct Items {
  std::vector<TableBlock> blocks;
  std::vector<BlockFrame> f;
  std::vector<std::vector<uint32_t>> digest;
};
static Items make_items(const std::vector<uint64_t> &body, bool sha, bool tag, uint32_t src) {
  Items it;
  it.digest.resize(body.size());
  uint64_t off = 0;
  for (size_t j = 0; j < body.size(); ++j) {
    it.digest[j] = {0x01020304u + (uint32_t)j, 0x05060708u, 0x090a0b0cu, 0x0d0e0f10u, 0x11121314u};
    const uint32_t *digest = sha ? it.digest[j].data() : nullptr;
    it.blocks.push_back({src, off, {{kNames[j % 5], 1000 * j + 7, digest, body[j]}}});
    it.f.push_back(BlockFrame(tag, 1, kHdr, sizeof kHdr, kNames[j % 5], 1000 * j + 7, digest, true, true));
    off += (body[j] + 255) / 256 * 256;
  }
  return it;
}

static uint64_t build(const Items &it, bool tag, const std::vector<uint8_t> *sel, uint64_t pos, uint64_t cap, FrameTable &T,
                      uint64_t *block_pos) {
  return build_frame_table(tag, 1, kHdr, sizeof kHdr, it.blocks, sel, pos, cap, T, block_pos);
}

static std::string blob_at(const FrameTable &T, uint64_t off, uint32_t len) {
  CHECK(off + len <= T.blob.size());
  return std::string((const char *)T.blob.data() + off, len);
}

// every entry of T against the items it frames: place, source, and head and tail equal to BlockFrame's
static void check_entries(const Items &items, const FrameTable &T, const std::vector<uint64_t> &pos, bool store) {
  CHECK(T.entry.size() == T.item.size());
  for (size_t e = 0; e < T.entry.size(); ++e) {
    const ZhFrameEntry &x = T.entry[e];
    const TableBlock &it = items.blocks[T.item[e]];
    CHECK(e == 0 || T.item[e] > T.item[e - 1]);
    CHECK(x.dst_off == pos[T.item[e]]);
    CHECK(x.src == it.src && x.src_off == it.src_off && x.body_len == it.seg[0].end && x.store == (store ? 1u : 0u));
    CHECK(blob_at(T, x.head_off, x.head_len) == items.f[T.item[e]].head);
    CHECK(blob_at(T, x.tail_off, x.tail_len) == items.f[T.item[e]].tail);
  }
}

static void test_block_frame() {
  const uint32_t digest[5] = {0x00010203u, 0x04050607u, 0x08090a0bu, 0x0c0d0e0fu, 0x10111213u};
  const BlockFrame f(true, 2, kHdr, sizeof kHdr, "name", 1234, digest, true, true);
  const uint8_t tag[13] = {0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3};
  std::string want((const char *)tag, 13);
  want += std::string("zPQ\x02\x01", 5) + std::string((const char *)kHdr, sizeof kHdr) + std::string("\x01name\0" "1234\0\0", 12);
  CHECK(f.head == want);
  std::string tail(4, '\0');
  tail.push_back((char)253);
  for (int i = 0; i < 20; ++i) tail.push_back((char)i);
  tail.push_back((char)255);
  CHECK(f.tail == tail);
  const BlockFrame g(false, 1, kHdr, sizeof kHdr, nullptr, 0, nullptr, true, true);
  CHECK(g.head == std::string("zPQ\x01\x01", 5) + std::string((const char *)kHdr, sizeof kHdr) + std::string("\x01\0" "0\0\0", 5));
  CHECK(g.tail == std::string("\0\0\0\0\xfe\xff", 6));
  puts("ok block_frame");
}

static void test_running_sum() {
  const std::vector<uint64_t> body = {0, 1, 15, 16, 17, 4096, 70000, 3};
  for (int sha = 0; sha < 2; ++sha)
    for (int tag = 0; tag < 2; ++tag)
      for (uint64_t pos0 : {0ull, 12345ull}) {
        const auto items = make_items(body, sha, tag, ZH_FRAME_SRC_FIRST);
        FrameTable T;
        std::vector<uint64_t> pos(items.blocks.size());
        const uint64_t end = build(items, tag, nullptr, pos0, ~0ull, T, pos.data());
        uint64_t run = pos0;
        for (size_t j = 0; j < items.blocks.size(); ++j) {
          CHECK(pos[j] == run);
          run += items.f[j].head.size() + body[j] + items.f[j].tail.size();
        }
        CHECK(end == run);
        CHECK(T.entry.size() == items.blocks.size() && T.sel_len == 0);
        CHECK(T.pieces == 2);               // 70 000 bytes: two 64 KiB pieces
        check_entries(items, T, pos, false);
      }
  puts("ok running_sum");
}

static void test_output_full() {
  const std::vector<uint64_t> body = {100, 200, 5000, 1, 0, 2};
  const auto items = make_items(body, true, true, ZH_FRAME_SRC_REDO);
  FrameTable full;
  std::vector<uint64_t> pos(items.blocks.size());
  const uint64_t end = build(items, true, nullptr, 0, ~0ull, full, pos.data());
  // a capacity that ends inside block k, just before its end, and exactly at it.  The stream offsets only grow, so a block
  // behind one that did not fit starts past the capacity and cannot fit either: the table holds blocks 0 .. k - 1 (or k).
  const size_t n = items.blocks.size();
  for (size_t k = 0; k < n; ++k)
    for (uint64_t cap : {pos[k], pos[k] + 1, (k + 1 < n ? pos[k + 1] : end) - 1, k + 1 < n ? pos[k + 1] : end}) {
      FrameTable T;
      std::vector<uint64_t> p(n);
      CHECK(build(items, true, nullptr, 0, cap, T, p.data()) == end);
      CHECK(p == pos);
      size_t fit = 0;
      while (fit < n && (fit + 1 < n ? pos[fit + 1] : end) <= cap) ++fit;
      CHECK(T.entry.size() == fit);
      for (size_t e = 0; e < T.entry.size(); ++e) {
        CHECK(T.item[e] == e);
        const ZhFrameEntry &x = T.entry[e];
        CHECK(x.dst_off + x.head_len + x.body_len + x.tail_len <= cap);
      }
      check_entries(items, T, pos, false);
    }
  // a later batch of a call that is already past the capacity holds nothing
  FrameTable T;
  CHECK(build(items, true, nullptr, 1000, 999, T, nullptr) == 1000 + end && T.entry.empty());
  // ... and with room for its first two blocks only, those two
  CHECK(build(items, true, nullptr, 1000, 1000 + pos[2], T, nullptr) == 1000 + end && T.entry.size() == 2);
  CHECK(T.entry[1].dst_off == 1000 + pos[1]);
  puts("ok output_full");
}

static void test_store_layout() {
  std::vector<uint8_t> pcomp(300);
  for (size_t i = 0; i < pcomp.size(); ++i) pcomp[i] = (uint8_t)(i * 7 + 1);
  for (const auto &sel : {selector_prefix(nullptr, 0), selector_prefix(pcomp.data(), pcomp.size())}) {
    CHECK(sel.size() == (sel[0] ? 3 + pcomp.size() : 1));
    const uint64_t ns = sel.size(), chunk = ZH_FRAME_PIECE;
    const std::vector<uint64_t> lens = {0, 1, chunk - ns - 1, chunk - ns, chunk - ns + 1, 2 * chunk - ns + 5};
    const auto items = make_items(lens, true, true, ZH_FRAME_SRC_PRE);
    FrameTable T;
    std::vector<uint64_t> pos(items.blocks.size());
    const uint64_t end = build(items, true, &sel, 0, ~0ull, T, pos.data());
    CHECK(T.sel_len == ns && std::vector<uint8_t>(T.blob.begin(), T.blob.begin() + ns) == sel);
    CHECK(T.pieces == 3);
    uint64_t run = 0;
    for (size_t j = 0; j < items.blocks.size(); ++j) {
      CHECK(pos[j] == run);
      const uint64_t dec = ns + lens[j];
      CHECK(store_body_len(dec) == dec + 4 * ((dec + chunk - 1) / chunk));
      run += items.f[j].head.size() + store_body_len(dec) + items.f[j].tail.size();
      // the layout itself: every chunk behind its big-endian length, the selector first
      std::vector<uint8_t> pre(lens[j]), got(store_body_len(dec)), flat;
      for (size_t i = 0; i < pre.size(); ++i) pre[i] = (uint8_t)(i * 13 + j);
      write_store_body(got.data(), sel, pre.data(), pre.size());
      const uint8_t *r = got.data();
      while (r < got.data() + got.size()) {
        const uint64_t cl = (uint64_t)r[0] << 24 | r[1] << 16 | r[2] << 8 | r[3];
        CHECK(cl >= 1 && cl <= chunk && r + 4 + cl <= got.data() + got.size());
        CHECK(cl == chunk || r + 4 + cl == got.data() + got.size());
        flat.insert(flat.end(), r + 4, r + 4 + cl);
        r += 4 + cl;
      }
      CHECK(flat.size() == dec && std::equal(sel.begin(), sel.end(), flat.begin()) &&
            std::equal(pre.begin(), pre.end(), flat.begin() + ns));
    }
    CHECK(end == run);
    check_entries(items, T, pos, true);
  }
  puts("ok store_layout");
}

// the rules that the store layout and the one-segment form once had a builder of their own for
static void test_store_rules() {
  std::vector<uint8_t> pcomp(40, 9);
  const auto sel = selector_prefix(pcomp.data(), pcomp.size());
  const uint64_t ns = sel.size();
  // a block that does not fit, then a shorter one: block_pos and the end are the unbounded ones.  The shorter one is judged by
  // the same rule as any block, pos + need <= out_cap; it starts behind the block that did not fit, so past out_cap, and is
  // left out too (the stream offsets only grow: test_output_full's prefix rule holds in the store layout as well)
  {
    const auto items = make_items({10, 5000, 3}, true, true, ZH_FRAME_SRC_PRE);
    FrameTable full, T;
    std::vector<uint64_t> pos(3), p(3);
    const uint64_t end = build(items, true, &sel, 0, ~0ull, full, pos.data());
    CHECK(full.entry.size() == 3);
    const uint64_t short_need = end - pos[2];
    for (uint64_t cap : {pos[1] + short_need, pos[2] - 1}) {      // room for the short block where the long one starts, but not for the long one
      CHECK(build(items, true, &sel, 0, cap, T, p.data()) == end && p == pos);
      CHECK(T.entry.size() == 1 && T.item[0] == 0);
      check_entries(items, T, pos, true);
    }
    CHECK(build(items, true, &sel, 0, end, T, p.data()) == end && T.entry.size() == 3);
  }
  // the store layout is one segment per block: a block of two is refused, wherever it stands, and nothing is in the table
  {
    auto items = make_items({10, 20}, true, true, ZH_FRAME_SRC_PRE);
    items.blocks[1].seg.push_back({"x", 1, nullptr, 25});
    FrameTable T;
    std::vector<uint64_t> p(2, 77);
    CHECK(build(items, true, &sel, 0, ~0ull, T, p.data()) == kFrameRefused);
    CHECK(T.entry.empty() && T.blob.empty() && p[0] == 77 && p[1] == 77);
    CHECK(build(items, true, nullptr, 0, ~0ull, T, p.data()) != kFrameRefused && T.entry.size() == 3);   // (without sel it is a solid block)
  }
  // T.pieces counts 64 KiB pieces of sel_len + body_len: a body that fills the piece exactly, one byte more, and none
  for (const std::vector<uint8_t> *s : {(const std::vector<uint8_t> *)&sel, (const std::vector<uint8_t> *)nullptr}) {
    const uint64_t sl = s ? ns : 0;
    const uint64_t lens[3] = {ZH_FRAME_PIECE - sl, ZH_FRAME_PIECE - sl + 1, 0};
    const uint32_t want[3] = {1, 2, 1};
    for (int k = 0; k < 3; ++k) {
      const auto items = make_items({lens[k]}, false, false, s ? ZH_FRAME_SRC_PRE : ZH_FRAME_SRC_FIRST);
      FrameTable T;
      build(items, false, s, 0, ~0ull, T, nullptr);
      CHECK(T.entry.size() == 1 && T.entry[0].body_len == lens[k] && T.sel_len == sl);
      CHECK(T.pieces == want[k]);
    }
  }
  puts("ok store_rules");
}

int main() {
  test_block_frame();
  test_running_sum();
  test_output_full();
  test_store_layout();
  test_store_rules();
  printf("ok %d checks\n", n_checks);
  return 0;
}
