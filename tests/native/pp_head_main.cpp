// A stand-alone drive of zh_core.h's pp_head_step (PostProcessor.write, states 0 and 2-4).  tests/test_pp_head.py builds it
// with -fsanitize=address,undefined, runs it and compares every line with its own restatement of PostProcessor.cs:37-79.
// One line per step: "<scenario> <c> -> <state> <hsize> <return> <stores>", where stores counts the program bytes the
// step handed to the caller's store (the program buffer here is exactly as long as the announced length: a byte too many
// is the sanitizer's to report).
#include <stdio.h>
#include <stdint.h>

#include <vector>

#include "zh_core.h"

using namespace zhcore;

static std::vector<uint8_t> buf;
static unsigned n_stores;

static int step(const char *what, PpHead &pp, int c) {
  n_stores = 0;
  const int rc = pp_head_step(pp, c, [&](uint32_t i, uint8_t v) { buf.at(i) = v; ++n_stores; });
  printf("%s %d -> %d %d %d %u\n", what, c, pp.state, pp.hsize, rc, n_stores);
  return rc;
}

// a whole header that announces `len` program bytes: selector, length, the bytes; then the buffer must hold them
static void load(const char *what, int len) {
  PpHead pp{0, 0, 0};
  step(what, pp, 1);
  step(what, pp, len & 255);
  step(what, pp, len >> 8);
  buf.assign((size_t)len, 0);
  for (int i = 0; i < len; ++i) step(what, pp, (i * 7 + 3) & 255);
  int bad = 0;
  for (int i = 0; i < len; ++i) bad += buf[(size_t)i] != (uint8_t)((i * 7 + 3) & 255);
  printf("%s stored %d wrong %d len %u\n", what, len, bad, pp.len);
}

int main() {
  buf.assign(4, 0);
  for (int c = 0; c < 256; ++c) { PpHead pp{0, 0, 0}; step("first", pp, c); }                    // selector: PASS, PROG, unknown
  for (int c = 0; c < 256; ++c) { PpHead pp{2, 0, 0}; step("low", pp, c); }                      // PCOMP length, low byte
  for (int lo = 0; lo < 256; lo += 255)                                                          // ... high byte, after low 0 and 255
    for (int c = 0; c < 256; ++c) { PpHead pp{3, lo, 0}; step(lo ? "high255" : "high0", pp, c); }
  {                                                                                              // end of segment in every state
    PpHead p0{0, 0, 0}, p2{2, 0, 0}, p3{3, 7, 0}, p4{4, 3, 1};
    step("eos0", p0, -1); step("eos2", p2, -1); step("eos3", p3, -1); step("eos4", p4, -1);
  }
  load("len1", 1);
  load("len65535", 65535);
  {                                                                                              // hsize 0: "Empty PCOMP"
    PpHead pp{0, 0, 0};
    step("len0", pp, 1); step("len0", pp, 0); step("len0", pp, 0);
  }
  return 0;
}
