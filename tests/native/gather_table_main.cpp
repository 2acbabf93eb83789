// A stand-alone check of build_gather_table (zh_frame_table.cpp): the table that puts the blocks of a mixed call, which lie
// group by group in the call's scratch stream, into the output in input order.  tests/test_compress_mixed.py builds it with
// -fsanitize=address,undefined and runs it; it prints one line per check and exits non-zero at the first that fails.
#include <stdio.h>
#include <stdlib.h>

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

// three groups interleaved as A B A C B A; the scratch holds group A's blocks, then B's, then C's
static const int kGroup[6] = {0, 1, 0, 2, 1, 0};

struct Layout {
  std::vector<GatherItem> items;
  uint64_t g0[3], g1[3];                  // each group's part of the scratch
  uint64_t total = 0;
};

static Layout lay_out(const std::vector<uint64_t> &len) {
  Layout Y;
  Y.items.resize(len.size());
  uint64_t at = 0;
  for (int g = 0; g < 3; ++g) {
    Y.g0[g] = at;
    for (size_t i = 0; i < len.size(); ++i)
      if (kGroup[i] == g) {
        Y.items[i] = {at, len[i]};
        at += len[i];
      }
    Y.g1[g] = at;
  }
  Y.total = at;
  return Y;
}

static void check_order(const std::vector<uint64_t> &len) {
  const Layout Y = lay_out(len);
  FrameTable T;
  std::vector<uint64_t> pos(len.size());
  CHECK(build_gather_table(Y.items, ~0ull, T, pos.data()) == Y.total);
  CHECK(T.entry.size() == len.size() && T.blob.empty() && T.sel_len == 0);
  uint64_t run = 0, longest = 0;
  for (size_t i = 0; i < len.size(); ++i) {
    const ZhFrameEntry &e = T.entry[i];
    CHECK(T.item[i] == i && pos[i] == run && e.dst_off == run);          // the prefix sum in input order
    CHECK(e.body_len == len[i] && e.head_len == 0 && e.tail_len == 0 && e.store == 0 && e.src == ZH_FRAME_SRC_FIRST);
    CHECK(e.src_off >= Y.g0[kGroup[i]] && e.src_off + e.body_len <= Y.g1[kGroup[i]]);   // inside its group's part
    run += len[i];
    longest = len[i] > longest ? len[i] : longest;
  }
  CHECK(T.pieces == (longest + ZH_FRAME_PIECE - 1) / ZH_FRAME_PIECE || (longest == 0 && T.pieces == 1));
  // the sources do not overlap: sorted by place they tile the scratch
  std::vector<uint8_t> seen(Y.total, 0);
  for (const ZhFrameEntry &e : T.entry)
    for (uint64_t k = 0; k < e.body_len; ++k) CHECK(!seen[e.src_off + k]++);
}

static void check_caps(const std::vector<uint64_t> &len, uint64_t step) {
  const Layout Y = lay_out(len);
  std::vector<uint64_t> want(len.size() + 1, 0);
  for (size_t i = 0; i < len.size(); ++i) want[i + 1] = want[i] + len[i];
  for (uint64_t cap = 0; cap <= Y.total + 1; cap += step) {
    FrameTable T;
    std::vector<uint64_t> pos(len.size());
    CHECK(build_gather_table(Y.items, cap, T, pos.data()) == Y.total);    // the need, whatever fits
    size_t e = 0;
    for (size_t i = 0; i < len.size(); ++i) {
      CHECK(pos[i] == want[i]);
      const bool fits = want[i + 1] <= cap;                               // in whole
      const bool has = e < T.entry.size() && T.item[e] == i;
      CHECK(fits == has);
      if (has) {
        CHECK(T.entry[e].dst_off == want[i] && T.entry[e].dst_off + T.entry[e].body_len <= cap);
        CHECK(T.entry[e].src_off == Y.items[i].src_off && T.entry[e].body_len == len[i]);
        ++e;
      }
    }
    CHECK(e == T.entry.size());
  }
}

int main() {
  const std::vector<uint64_t> len = {0, 1, 15, 16, 17, 65537};
  check_order(len);
  check_order({65537, 17, 16, 15, 1, 0});
  check_order({0, 0, 0, 0, 0, 0});
  puts("ok order");
  check_caps(len, 1);                                                     // every out_cap from 0 to total + 1
  check_caps({65537, 17, 0, 15, 1, 0}, 1);
  puts("ok output_full");
  FrameTable T;
  CHECK(build_gather_table({}, 10, T, nullptr) == 0 && T.entry.empty());
  puts("ok empty");
  printf("ok %d checks\n", n_checks);
  return 0;
}
