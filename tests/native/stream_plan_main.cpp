// A stand-alone drive of zh_stream_plan.h: the rules of the whole-stream pipeline and of zpaqhip_decompress_multi without a
// GPU.  tests/test_stream_plan.py builds it with -fsanitize=address,undefined next to zh_framing.cpp (scan_stream,
// build_model), writes the cases to a file, runs it and compares what it prints with expectations of its own.  Where the
// driver in zh_api.cpp enqueues a copy from a device buffer, this program does a memcpy from a heap buffer of exactly the
// planned size into a heap buffer of exactly the caller's capacity, so a copy that leaves either is an ASan report.
//
// A case in the file (blank-separated tokens; U64 "-" = UINT64_MAX, an absent size hint):
//   limit BATCH_BLOCKS DEC_WAVES
//   slots NAME BUDGET N  (HINT CODED)...
//   batches NAME PATH BATCH_BLOCKS DEC_WAVES READ            READ = 0: memory source, else a callback that gives READ bytes
//   second NAME N  (CAP NSEG (STATUS OUT_LEN)...)...
//   deliver NAME FORM CAP UPTO PARTIAL TOTAL0 BLK0 N  (REAL SLOT FIX PLACE PLACE_CAP)...     FORM = mem | writer | placed
//   queue NAME N_DEV ALL_CM1 N  COST...
//   places NAME OUT_CAP DAMAGED N  (HINT REAL)...            DAMAGED = -1: none
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "zh_stream_plan.h"

using namespace zh;

static std::istream *g_in;

static uint64_t u64() {
  std::string w;
  if (!(*g_in >> w)) { fprintf(stderr, "case file ends early\n"); exit(2); }
  return w == "-" ? UINT64_MAX : std::stoull(w);
}
static long i64() {
  std::string w;
  if (!(*g_in >> w)) { fprintf(stderr, "case file ends early\n"); exit(2); }
  return std::stol(w);
}
static std::string word() {
  std::string w;
  if (!(*g_in >> w)) { fprintf(stderr, "case file ends early\n"); exit(2); }
  return w;
}

static void list(const char *what, const std::vector<uint64_t> &v) {
  printf("%s=", what);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
  printf("\n");
}
static void hex(const char *what, const uint8_t *p, size_t n) {
  printf("%s=", what);
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
  printf("\n");
}

// byte i of the plaintext of block g (global index)
static uint8_t plain(size_t g, size_t i) { return (uint8_t)(g * 53 + i * 7 + 1); }

// A decoded batch of blocks blk0.. with plaintext sizes real[], as the driver holds it after settle_batch: block b in its
// staging slot of slot[b] bytes, or (fix[b]) in the second-pass buffer with its exact size.  The two buffers have exactly
// the planned sizes; bytes of no block are 0xEE.
struct FakeBatch {
  Batch bt;
  std::vector<uint8_t> staging, fixbuf;
  FakeBatch(size_t blk0, const std::vector<uint64_t> &real, const std::vector<uint64_t> &slot, const std::vector<int> &fix) {
    const size_t n = real.size();
    bt.blk0 = blk0;
    bt.so.blocks.resize(n);
    bt.real = real; bt.cap = slot; bt.off.assign(n, 0);
    uint64_t pos = 0, pos2 = 0;
    for (size_t b = 0; b < n; ++b) {
      if (fix[b]) { bt.off[b] = pos2 | kInFix; bt.cap[b] = real[b]; pos2 += real[b]; }
      else bt.off[b] = pos;
      pos += slot[b];
    }
    staging.assign((size_t)pos, 0xEE); fixbuf.assign((size_t)pos2, 0xEE);
    for (size_t b = 0; b < n; ++b) {
      uint8_t *p = fix[b] ? fixbuf.data() + (bt.off[b] & ~kInFix) : staging.data() + bt.off[b];
      for (size_t i = 0; i < real[b]; ++i) p[i] = plain(blk0 + b, i);
    }
  }
  const uint8_t *src(const Copy &c) const { return (c.fix ? fixbuf.data() : staging.data()) + c.src_off; }
};

static void print_copies(const Delivery &d) {
  for (const Copy &c : d.copies)
    printf("copy fix=%d src=%llu n=%llu dst=%llu spill=%ld\n", (int)c.fix, (unsigned long long)c.src_off, (unsigned long long)c.n,
           (unsigned long long)c.dst, c.spill);
  printf("total=%llu\n", (unsigned long long)d.total);
}

// The copies of a placed delivery done on the host, as drain_batch enqueues them
static void run_placed(const FakeBatch &fb, const Delivery &d, Sinkk &sink) {
  for (const Copy &c : d.copies) {
    uint8_t *dst = sink.mem + c.dst;
    if (c.spill >= 0) {
      std::vector<uint8_t> &sp = (*sink.spill)[(size_t)c.spill];
      sp.resize((size_t)c.n);
      dst = sp.data();
    }
    memcpy(dst, fb.src(c), (size_t)c.n);
  }
  sink.total = d.total;
}

static void do_limit() {
  const size_t bb = (size_t)u64(), dw = (size_t)u64();
  const ScanLimit lim = batch_limit(bb, dw);
  printf("limit %zu %zu min_blocks=%zu min_blocks_other=%zu min_bytes=%zu max_blocks=%zu\n", bb, dw, lim.min_blocks, lim.min_blocks_other,
         lim.min_bytes, lim.max_blocks);
}

static void do_slots() {
  const std::string name = word();
  const uint64_t budget = u64();
  const size_t n = (size_t)u64();
  std::vector<zpaqhip_block> blocks(n);
  std::vector<zpaqhip_segment> segs(n);
  for (size_t b = 0; b < n; ++b) {
    memset(&blocks[b], 0, sizeof blocks[b]); memset(&segs[b], 0, sizeof segs[b]);
    blocks[b].usize_hint = u64();
    blocks[b].first_seg = (uint32_t)b; blocks[b].n_seg = 1;
    segs[b].data_len = u64();
  }
  std::vector<uint64_t> cap, off;
  const uint64_t total = plan_slots(blocks, segs, budget, cap, off);
  printf("slots %s total=%llu\n", name.c_str(), (unsigned long long)total);
  list("cap", cap);
  list("off", off);
}

struct FileReader { std::vector<uint8_t> data; size_t pos = 0, step = 0; };
static int read_some(void *user, uint8_t *buf, int n) {
  FileReader &f = *(FileReader *)user;
  const size_t k = std::min<size_t>({(size_t)n, f.step, f.data.size() - f.pos});
  memcpy(buf, f.data.data() + f.pos, k);
  f.pos += k;
  return (int)k;
}

static void do_batches() {
  const std::string name = word(), path = word();
  const size_t bb = (size_t)u64(), dw = (size_t)u64();
  FileReader f;
  f.step = (size_t)u64();
  std::ifstream file(path, std::ios::binary);
  if (!file) { fprintf(stderr, "%s: cannot open %s\n", name.c_str(), path.c_str()); exit(2); }
  f.data.assign(std::istreambuf_iterator<char>(file), std::istreambuf_iterator<char>());
  Source src;
  if (f.step) { src.rd = read_some; src.user = &f; }
  else { src.mem = f.data.empty() ? (const uint8_t *)"" : f.data.data(); src.mem_len = f.data.size(); }
  printf("batches %s\n", name.c_str());
  size_t blk0 = 0, seg0 = 0;
  for (;;) {                                            // as the pipeline asks: until a batch is empty or the last
    Batch bt;
    zpaqhip_err err{};
    const int rc = next_batch(src, bt, blk0, seg0, bb, dw, &err);
    if (rc) { printf("error %d\n", rc); return; }
    printf("batch blk0=%zu seg0=%zu stream_off=%llu len=%zu last=%d rc_after=%d err_block=%d err_seg=%d blocks=%zu segs=%zu\n", bt.blk0, bt.seg0,
           (unsigned long long)bt.stream_off, bt.len, (int)bt.last, bt.rc_after, bt.rc_after ? bt.err_after.block : -1,
           bt.rc_after ? bt.err_after.segment : -1, bt.so.blocks.size(), bt.so.segs.size());
    for (const zpaqhip_block &B : bt.so.blocks) {
      printf("block tag=%llu hdr=%llu+%u end=%llu segs=%u+%u comps=%u hint=%llu sum=%u\n", (unsigned long long)B.tag_off,
             (unsigned long long)B.hdr_off, B.hdr_len, (unsigned long long)B.end_off, B.first_seg, B.n_seg, (unsigned)B.n_comp,
             (unsigned long long)B.usize_hint, (unsigned)std::accumulate(bt.h + B.tag_off, bt.h + B.end_off, 0u) & 0xffffu);
    }
    for (const zpaqhip_segment &S : bt.so.segs)
      printf("seg block=%u data=%llu+%llu\n", S.block, (unsigned long long)S.data_off, (unsigned long long)S.data_len);
    if (bt.so.blocks.empty() || bt.last) break;
    blk0 += bt.so.blocks.size(); seg0 += bt.so.segs.size();
  }
}

static void do_second() {
  const std::string name = word();
  const size_t n = (size_t)u64();
  Batch bt;
  bt.blk0 = 10; bt.seg0 = 20;
  bt.so.blocks.resize(n);
  bt.cap.assign(n, 0); bt.off.assign(n, 0); bt.real.assign(n, 0);
  uint64_t pos = 0;
  for (size_t b = 0; b < n; ++b) {
    zpaqhip_block &B = bt.so.blocks[b];
    memset(&B, 0, sizeof B);
    bt.cap[b] = u64(); bt.off[b] = pos;
    B.first_seg = (uint32_t)bt.res.size(); B.n_seg = (uint32_t)u64();
    uint64_t at = pos;
    for (uint32_t i = 0; i < B.n_seg; ++i) {
      zpaqhip_seg_result r{};
      r.status = (int32_t)i64(); r.out_len = u64(); r.out_off = at;
      at += r.out_len;
      bt.res.push_back(r);
      zpaqhip_segment s;
      memset(&s, 0, sizeof s);
      s.block = (uint32_t)b;
      bt.so.segs.push_back(s);
    }
    pos += bt.cap[b];
  }
  const SecondPass sp = plan_second_pass(bt);
  printf("second %s bytes=%llu\n", name.c_str(), (unsigned long long)sp.bytes);
  list("real", bt.real);
  list("redo", std::vector<uint64_t>(sp.redo.begin(), sp.redo.end()));
  list("off2", sp.off2);
  list("cap2", sp.cap2);
  const FirstBad f = first_failure(bt);
  printf("first found=%d ok_blocks=%zu partial=%llu rc=%d code=%d block=%d seg=%d\n", (int)f.found, f.ok_blocks, (unsigned long long)f.partial, f.rc,
         f.err.code, f.found ? f.err.block : -1, f.found ? f.err.segment : -1);
  SegSink ss;
  append_segment_records(bt, 1000, ss);
  std::vector<uint64_t> offs, blks;
  for (size_t s = 0; s < ss.res.size(); ++s) { offs.push_back(ss.res[s].out_off); blks.push_back(ss.segs[s].block); }
  list("rec_off", offs);
  list("rec_block", blks);
}

static void do_deliver() {
  const std::string name = word(), form = word();
  const size_t cap = (size_t)u64(), upto = (size_t)u64();
  const uint64_t partial = u64(), total0 = u64();
  const size_t blk0 = (size_t)u64(), n = (size_t)u64();
  std::vector<uint64_t> real(n), slot(n), place(blk0 + n, 0), place_cap(blk0 + n, 0), sizes(blk0 + n, 0);
  std::vector<int> fix(n);
  for (size_t b = 0; b < n; ++b) { real[b] = u64(); slot[b] = u64(); fix[b] = (int)u64(); place[blk0 + b] = u64(); place_cap[blk0 + b] = u64(); }
  const FakeBatch fb(blk0, real, slot, fix);
  std::unique_ptr<uint8_t[]> mem(new uint8_t[cap]);     // exactly the caller's capacity
  memset(mem.get(), 0xEE, cap);
  std::vector<std::vector<uint8_t>> spill(blk0 + n);
  Sinkk sink;
  sink.total = total0;
  printf("deliver %s\n", name.c_str());
  if (form == "writer") {
    sink.wr = [](void *, const uint8_t *, int) { return 0; };
    const Delivery d = plan_delivery(fb.bt, upto, partial, sink);
    print_copies(d);
    std::vector<uint8_t> got;
    for (const Copy &c : d.copies) {
      if (c.dst != total0 + got.size() || c.spill >= 0) { printf("writer copy out of order\n"); exit(1); }
      got.insert(got.end(), fb.src(c), fb.src(c) + c.n);
    }
    hex("out", got.data(), got.size());
    return;
  }
  sink.mem = mem.get(); sink.cap = cap;
  if (form == "placed") { sink.place = place.data(); sink.place_cap = place_cap.data(); sink.sizes = &sizes; sink.spill = &spill; }
  const Delivery d = plan_delivery(fb.bt, upto, partial, sink);
  print_copies(d);
  run_placed(fb, d, sink);
  hex("out", mem.get(), cap);
  if (form == "placed") {
    list("sizes", sizes);
    for (size_t g = 0; g < spill.size(); ++g)
      if (!spill[g].empty()) { printf("spill %zu ", g); hex("bytes", spill[g].data(), spill[g].size()); }
  }
}

static void do_queue() {
  const std::string name = word();
  const size_t n_dev = (size_t)u64();
  const bool all_cm1 = u64() != 0;
  const size_t nb = (size_t)u64();
  std::vector<uint64_t> cost(nb);
  for (uint64_t &c : cost) c = u64();
  const size_t chunk = default_chunk_blocks(nb, n_dev, all_cm1), K = (nb + chunk - 1) / chunk;
  printf("queue %s chunk=%zu K=%zu\n", name.c_str(), chunk, K);
  const std::vector<size_t> order = queue_order(cost);
  std::vector<size_t> ids;
  for (size_t k = 0; k < K; ++k) {
    const bool run = queue_chunk(order, k, K, ids);
    printf("chunk run=%d ", (int)run);
    list("ids", std::vector<uint64_t>(ids.begin(), ids.end()));
  }
}

static void do_places() {
  const std::string name = word();
  const size_t out_cap = (size_t)u64();
  const long damaged = i64();
  const size_t nb = (size_t)u64();
  std::vector<zpaqhip_block> blocks(nb);
  std::vector<uint64_t> want(nb);
  for (size_t b = 0; b < nb; ++b) { memset(&blocks[b], 0, sizeof blocks[b]); blocks[b].usize_hint = u64(); want[b] = u64(); }
  std::vector<uint64_t> slot_off, slot_cap, real(nb, 0);
  place_slots(blocks, out_cap, slot_off, slot_cap);
  printf("places %s\n", name.c_str());
  list("slot_off", slot_off);
  list("slot_cap", slot_cap);
  std::unique_ptr<uint8_t[]> out(new uint8_t[out_cap]);
  memset(out.get(), 0xEE, out_cap);
  std::vector<std::vector<uint8_t>> spill(nb);
  // every block but the damaged one delivered as a chunk of its own, the way a device thread's pipeline does it
  for (size_t b = 0; b < nb; ++b) {
    if ((long)b == damaged) continue;
    const FakeBatch fb(b, {want[b]}, {want[b]}, {0});
    Sinkk sink;
    sink.mem = out.get(); sink.cap = out_cap; sink.place = slot_off.data(); sink.place_cap = slot_cap.data(); sink.sizes = &real; sink.spill = &spill;
    run_placed(fb, plan_delivery(fb.bt, 1, 0, sink), sink);
  }
  const std::vector<uint8_t> before(out.get(), out.get() + out_cap);
  const size_t limit = damaged < 0 ? nb : (size_t)damaged;
  size_t out_len = 0;
  const int rc = settle_places(out.get(), out_cap, limit, slot_off, slot_cap, real, spill, &out_len);
  printf("rc=%d out_len=%zu moved=%d\n", rc, out_len, (int)(memcmp(before.data(), out.get(), out_cap) != 0));
  hex("out", out.get(), std::min(out_len, out_cap));
}

int main(int argc, char **argv) {
  std::ifstream file;
  if (argc > 1) file.open(argv[1]);
  g_in = argc > 1 ? (std::istream *)&file : &std::cin;
  std::string w;
  while (*g_in >> w) {
    if (w == "limit") do_limit();
    else if (w == "slots") do_slots();
    else if (w == "batches") do_batches();
    else if (w == "second") do_second();
    else if (w == "deliver") do_deliver();
    else if (w == "queue") do_queue();
    else if (w == "places") do_places();
    else { fprintf(stderr, "case file: unknown case '%s'\n", w.c_str()); return 2; }
  }
  return 0;
}
