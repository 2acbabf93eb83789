// A stand-alone drive of zh_stream_plan.h: the rules of the whole-stream pipeline, of zpaqhip_decompress_multi and of
// zpaqhip_decompress_device without a GPU.  tests/test_stream_plan.py builds it with -fsanitize=address,undefined next to zh_framing.cpp (scan_stream,
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
//   device NAME OUT_CAP BUDGET NO_STAGING DAMAGED DAMAGED_AT SHA_BAD N  (HINT REAL NSEG)...
//       the whole sequence of zpaqhip_decompress_device.  NO_STAGING = 1: the staging buffer cannot be reserved; DAMAGED: a
//       segment (stream index, -1: none) that fails from its block's DAMAGED_AT-th decode on; SHA_BAD: a segment whose
//       checksum differs
//   modelcut NAME PATH
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

// ---- zpaqhip_decompress_device, played with heap buffers in place of device buffers
struct Heap {                             // exactly n bytes: an access outside them is an ASan report
  std::unique_ptr<uint8_t[]> p;
  size_t n = 0;
  void reserve(size_t bytes) { p.reset(new uint8_t[bytes]); n = bytes; memset(p.get(), 0xEE, bytes); }
};

// What decode_launch + decode_finish leave of blocks `ids` decoded to base + off[i] with room cap[i], as the kernels' segment
// epilogue reports it (seg_done / seg_skipped, zh_dev.h) and decode_finish copies it: a segment's out_off = the block's
// offset + the bytes of the block before it, its out_len what it produced, both counted past the room; bytes are written
// only inside the room; status ZPAQHIP_E_OUTPUT_FULL when the block's bytes up to and with the segment exceed the room,
// which does not stop the block; any other error does, and the segments behind it are ZH_E_SKIPPED with out_len 0.
// (decode_finish's ZH_E_STOPPED and in_used rules do not come up: every segment here ends where its coded data ends.)
struct FakeDecoder {
  long damaged, damaged_at;
  std::vector<uint64_t> seg_len;          // plaintext of every segment
  std::vector<int> decodes;               // per block
  void run(DevPlan &pl, const DevDecode &d, Heap &base) {
    for (size_t j = 0; j < d.ids.size(); ++j) {
      const size_t b = d.ids[j];
      const zpaqhip_block &B = pl.blocks[b];
      ++decodes[b];
      uint64_t produced = 0;
      bool failed = false;
      for (uint32_t i = 0; i < B.n_seg; ++i) {
        const size_t s = B.first_seg + i;
        zpaqhip_seg_result &r = pl.res[s];
        r = zpaqhip_seg_result{};
        r.out_off = d.off[j] + produced;
        if (failed) { r.status = ZH_E_SKIPPED; continue; }
        const bool bad = (long)s == damaged && decodes[b] >= damaged_at;
        const uint64_t n = bad ? seg_len[s] / 2 : seg_len[s];
        for (uint64_t q = produced; q < produced + n && q < d.cap[j]; ++q) {
          if (d.off[j] + q >= base.n) { printf("decoder writes outside its buffer\n"); exit(1); }
          base.p[d.off[j] + q] = plain(b, (size_t)q);
        }
        produced += n;
        r.out_len = n;
        r.status = bad ? ZPAQHIP_E_CORRUPT : produced > d.cap[j] ? ZPAQHIP_E_OUTPUT_FULL : ZPAQHIP_OK;
        failed = bad;
      }
    }
    note_decoded(pl, d.ids);
  }
};

static void run_entries(const std::vector<ZhFrameEntry> &tab, Heap &dst, const Heap &d_out, const Heap &staging, const Heap &fix) {
  for (const ZhFrameEntry &e : tab) {
    const Heap &src = e.src == ZH_FRAME_SRC_INPUT ? d_out : e.src == ZH_FRAME_SRC_FIRST ? staging : fix;
    memcpy(dst.p.get() + e.dst_off, src.p.get() + e.src_off, (size_t)e.body_len);
  }
}

static void do_device() {
  const std::string name = word();
  const uint64_t out_cap = u64(), budget = u64();
  const bool no_staging = u64() != 0;
  const long damaged = i64(), damaged_at = i64(), sha_bad = i64();
  const size_t nb = (size_t)u64();
  DevPlan p;
  p.blocks.resize(nb);
  std::vector<uint64_t> seg_len;
  for (size_t b = 0; b < nb; ++b) {
    zpaqhip_block &B = p.blocks[b];
    memset(&B, 0, sizeof B);
    B.usize_hint = u64();
    const uint64_t real = u64();
    B.first_seg = (uint32_t)seg_len.size(); B.n_seg = (uint32_t)u64();
    for (uint32_t i = 0; i < B.n_seg; ++i) {
      zpaqhip_segment g;
      memset(&g, 0, sizeof g);
      g.block = (uint32_t)b; g.flags = 1; g.data_len = 40;
      p.segs.push_back(g);
      seg_len.push_back(i + 1 < B.n_seg ? real / B.n_seg : real - real / B.n_seg * (B.n_seg - 1));
    }
  }
  p.cut(nb);
  FakeDecoder dec{damaged, damaged_at, seg_len, std::vector<int>(nb, 0)};
  Heap d_out, staging, fix;
  d_out.reserve((size_t)out_cap);
  staging.reserve(0); fix.reserve(0);

  // ---- the driver's sequence (zpaqhip_decompress_device, zh_api.cpp)
  dec.run(p, plan_direct(p, out_cap), d_out);
  if (p.bad.limit > p.k) {
    const std::vector<zpaqhip_block> rest(p.blocks.begin() + (ptrdiff_t)p.k, p.blocks.end());
    std::vector<uint64_t> cap, off;
    uint64_t bytes = plan_slots(rest, p.segs, budget, cap, off);
    if (no_staging) { count_only_slots(cap, off); bytes = 0; }
    staging.reserve((size_t)bytes);
    dec.run(p, plan_staged(p, cap, off), staging);
  }
  const size_t k = p.k;
  const DevSecond second = plan_device_second(p);
  fix.reserve((size_t)second.fix_bytes);
  run_entries(second.move, fix, d_out, staging, fix);
  dec.run(p, second.redo, fix);
  const Heap *base[3] = {&d_out, &staging, &fix};
  for (DevWhere w : {DevWhere::kOut, DevWhere::kStaging, DevWhere::kFix}) {
    const Sha1Table t = device_sha1_table(p, w);
    for (size_t j = 0; j < t.which.size(); ++j) {         // the digest kernel reads these bytes: they are the segment's
      const size_t s = t.which[j], b = p.segs[s].block;
      uint64_t before = 0;
      for (size_t s2 = p.blocks[b].first_seg; s2 < s; ++s2) before += seg_len[s2];
      for (uint64_t q = 0; q < t.pairs[2 * j + 1]; ++q)
        if (base[(int)w]->p[t.pairs[2 * j] + q] != plain(b, (size_t)(before + q))) { printf("checksum table: segment %zu is not at its offset\n", s); exit(1); }
      if (t.pairs[2 * j + 1] != seg_len[s]) { printf("checksum table: segment %zu has the wrong length\n", s); exit(1); }
      if ((long)s == sha_bad) p.res[s].status = ZPAQHIP_E_SHA1;
    }
  }
  lowest_failed_block(p.blocks, p.res, p.bad);
  const DevGather g = plan_gather(p, out_cap);
  run_entries(g.entries, d_out, d_out, staging, fix);
  const size_t n_res = device_result_count(p);
  std::vector<zpaqhip_seg_result> results(p.segs.size());
  for (zpaqhip_seg_result &r : results) r.status = 12345;  // (not written)
  device_results(p, g, results.data());
  const int rc = p.bad.rc ? p.bad.rc : g.out_len() > out_cap ? ZPAQHIP_E_OUTPUT_FULL : ZPAQHIP_OK;

  printf("device %s rc=%d block=%d seg=%d out_len=%llu n_res=%zu k=%zu staging=%zu fix=%llu moves=%zu\n", name.c_str(), rc,
         p.bad.rc ? p.bad.err.block : -1, p.bad.rc ? p.bad.err.segment : -1, (unsigned long long)g.out_len(), n_res, k, staging.n,
         (unsigned long long)second.fix_bytes, second.move.size());
  list("decodes", std::vector<uint64_t>(dec.decodes.begin(), dec.decodes.end()));
  std::vector<uint64_t> off, len;
  for (size_t s = 0; s < n_res; ++s) { off.push_back(results[s].out_off); len.push_back(results[s].out_len); }
  printf("res_status=");
  for (size_t s = 0; s < n_res; ++s) printf("%s%d", s ? "," : "", results[s].status);
  printf("\n");
  list("res_off", off);
  list("res_len", len);
  for (size_t s = n_res; s < results.size(); ++s)
    if (results[s].status != 12345) { printf("a record behind n_res was written\n"); exit(1); }
  hex("out", d_out.p.get(), (size_t)out_cap);
}

// The model cut through an accessor that hands out a copy of one header at a time (the device form's), against the batch's
static void do_modelcut() {
  const std::string name = word(), path = word();
  std::ifstream file(path, std::ios::binary);
  if (!file) { fprintf(stderr, "%s: cannot open %s\n", name.c_str(), path.c_str()); exit(2); }
  const std::vector<uint8_t> data((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
  Source src;
  src.mem = data.data(); src.mem_len = data.size();
  Batch bt;
  zpaqhip_err err{};
  if (next_batch(src, bt, 0, 0, 0, 0, &err)) { printf("error\n"); return; }
  ScanOut so;
  zpaqhip_err e2{};
  (void)scan_stream(data.data(), data.size(), so, &e2, batch_limit(0, 0));
  ModelCut cut;
  std::unique_ptr<uint8_t[]> hdr;
  size_t fetched = 0;
  const int rc = first_bad_model(so.blocks, [&](size_t b, const uint8_t *&h) {
    hdr.reset(new uint8_t[so.blocks[b].hdr_len]);
    memcpy(hdr.get(), data.data() + so.blocks[b].hdr_off, so.blocks[b].hdr_len);
    h = hdr.get();
    ++fetched;
    return ZPAQHIP_OK;
  }, cut);
  printf("modelcut %s\n", name.c_str());
  printf("batch nb=%zu rc=%d block=%d seg=%d msg=%s\n", bt.so.blocks.size(), bt.rc_after, bt.err_after.block, bt.err_after.segment, bt.err_after.msg);
  printf("accessor nb=%zu rc=%d block=%d seg=%d msg=%s call=%d fetched=%zu\n", cut.nb, cut.rc, cut.err.block, cut.err.segment, cut.err.msg, rc, fetched);
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
    else if (w == "device") do_device();
    else if (w == "modelcut") do_modelcut();
    else { fprintf(stderr, "case file: unknown case '%s'\n", w.c_str()); return 2; }
  }
  return 0;
}
