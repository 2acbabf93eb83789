// A stand-alone check of the load rule of zh_gap_hist (zh_analyze.h): the kernel's load sequence, its one-ahead load
// included, is played on the host against a buffer that holds exactly the aligned 16-byte groups the rule permits (those
// with at least one byte of the walk), for every residue of the block's address and walks of every length at which the
// sequence can go wrong.  tests/test_compress_mixed.py builds it with -fsanitize=address,undefined and runs it: a load
// outside the buffer is a heap overflow there, and is checked here as well.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zh_analyze.h"

static int n_checks = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    ++n_checks;                                                        \
    if (!(c)) {                                                        \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);            \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

// the reference's loop (LibZPAQ.cs:242-255)
static std::vector<uint32_t> plain_hist(const std::vector<uint8_t> &p) {
  std::vector<uint32_t> r(ZH_GAP_NR, 0);
  uint32_t pt[256] = {0};
  for (uint32_t i = 0; i < p.size(); ++i) {
    const uint32_t k = i - pt[p[i]];
    if (k > 0 && k < ZH_GAP_NR) ++r[k];
    pt[p[i]] = i;
  }
  return r;
}

// One lane of zh_gap_hist on the slice that starts at byte s of the block `p`, whose first byte has the address `block`:
// the same statements in the same order, with a load taken from `mem`, which stands for the addresses [mem_addr, mem_addr +
// mem.size()).  Returns the longest walk it played.
static uint32_t play_slice(const std::vector<uint8_t> &p, uint64_t block, uint32_t s, std::vector<uint32_t> &h) {
  const uint32_t n = (uint32_t)p.size();
  const ZhGapSlice c = zh_gap_slice(n, s);
  const uint32_t len = c.e - c.w0, from = s - c.w0;
  CHECK(c.w0 <= s && s < c.e && c.e <= n && len <= ZH_GAP_SLICE + ZH_GAP_NR);
  // exactly the permitted groups: from the one with byte w0 to the one with byte e - 1
  const uint64_t lo = (block + c.w0) & ~15ull, hi = ((block + c.e - 1) & ~15ull) + 16;
  std::vector<uint8_t> mem(hi - lo, 0xEE);
  for (uint64_t a = lo; a < hi; ++a)
    if (a >= block && a < block + n) mem[a - lo] = p[a - block];      // (bytes of the block outside the walk are mapped too)
  size_t loads = 0;
  auto load = [&](uint64_t addr, uint8_t out[16]) {
    CHECK(addr % 16 == 0 && addr >= lo && addr + 16 <= hi);
    memcpy(out, mem.data() + (addr - lo), 16);
    ++loads;
  };

  const ZhGapFirst f = zh_gap_first_load(block, c.w0);
  CHECK(f.addr == lo && f.r0 <= 0 && f.r0 > -16 && f.addr - f.r0 == block + c.w0);
  int64_t r0 = f.r0;
  uint64_t src = f.addr;
  std::vector<uint16_t> pt(256, 0);
  uint8_t next[16], cur[16];
  load(src, next);
  while (r0 < (int64_t)len) {
    memcpy(cur, next, 16);
    if (zh_gap_load_next(r0, len)) load(src += 16, next);
    for (int t = 0; t < 16; ++t) {
      const uint32_t r = (uint32_t)(r0 + t);
      if (r < len) {
        const uint32_t v = cur[t];
        CHECK(v == p[c.w0 + r]);                                       // the bytes walked are the block's
        const uint32_t k = r - pt[v];
        pt[v] = (uint16_t)r;
        if (r >= from && k > 0 && k < ZH_GAP_NR) ++h[k];
      }
    }
    r0 += 16;
  }
  CHECK(loads == (hi - lo) / 16);                                      // every permitted group once, none twice
  return len;
}

int main() {
  const uint32_t S = ZH_GAP_SLICE;
  // blocks of one slice walk their own length; the second slice of 2 S bytes walks S + 4096, the third of 2 S + 1 walks 4097
  const uint32_t sizes[] = {1, 15, 16, 17, 4095, 4096, 4097, S - 1, S, S + 1, 2 * S, 2 * S + 1};
  bool seen_len[11] = {false};
  const uint32_t want_len[11] = {1, 15, 16, 17, 4095, 4096, 4097, S - 1, S, S + 4096, S + 4096};
  uint32_t seed = 12345;
  for (uint32_t n : sizes) {
    std::vector<uint8_t> p(n);
    for (uint32_t i = 0; i < n; ++i) {      // a period of 7, one of 300 and noise over a small alphabet, in turns of 1000 bytes
      seed = seed * 1664525u + 1013904223u;
      const uint32_t turn = (i / 1000) % 3;
      p[i] = turn == 0 ? (uint8_t)(i % 7) : turn == 1 ? (uint8_t)(i % 300) : (uint8_t)(seed >> 28);
    }
    const std::vector<uint32_t> want = plain_hist(p);
    for (uint64_t residue = 0; residue < 16; ++residue) {
      const uint64_t block = 0x7f1200004000ull + residue;
      std::vector<uint32_t> h(ZH_GAP_NR, 0);
      for (uint32_t s = 0; s < n; s += S) {
        const uint32_t len = play_slice(p, block, s, h);
        for (int q = 0; q < 11; ++q) seen_len[q] |= len == want_len[q];
      }
      CHECK(h == want);
    }
  }
  for (int q = 0; q < 11; ++q) CHECK(seen_len[q]);
  puts("ok load_rule");
  printf("ok %d checks\n", n_checks);
  return 0;
}
