// zh_stream_plan.h — the rules of the whole-stream forms: how a stream is cut into batches, where a batch's blocks are staged,
// which blocks are decoded a second time, what is delivered where, and how zpaqhip_decompress_multi queues, places and
// settles its blocks; and the rules of zpaqhip_decompress_device, the form whose stream and output both lie in device
// memory: what is decoded straight to its place, what is staged, moved, decoded again and gathered.  Host C++ only (no
// HIP): zh_api.cpp's drivers enqueue what these functions decide, tests/native/stream_plan_main.cpp runs them without a
// GPU.  Every rule here reads untrusted input (a comment's text as a size, a truncated stream, a caller's out_cap) and
// decides where bytes are written.
#pragma once
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "zh_frame.h"
#include "zh_host.h"

namespace zh {

// A size hint is untrusted text (a comment that merely starts with digits, or a hostile archive): it only sizes or places a
// block when it is plausible.  The staging plan adds "within the budget", the multi-device placing "within out_cap".
inline bool plausible_hint(uint64_t h) { return h != UINT64_MAX && h <= (1ull << 40); }

inline bool data_error(int rc) {          // per-segment outcomes, as opposed to failures of the call itself
  return rc < 0 && rc != ZPAQHIP_E_HIP && rc != ZPAQHIP_E_ARG && rc != ZPAQHIP_E_DEVICE_MEM && rc != ZPAQHIP_E_NO_DEVICE &&
         rc != ZPAQHIP_E_HEADER && rc != ZPAQHIP_E_COMPONENT && rc != ZPAQHIP_E_HM_TOO_BIG && rc != ZPAQHIP_E_CALLBACK;
}

// ---- batches
constexpr size_t kBatchMinBlocks = 512, kBatchMinBlocksOther = 256, kBatchMinBytes = 32u << 20, kBatchMaxBlocks = 4096;   // 512: single-CM blocks run two per CU (zh_decode_cm_x2); every other kernel holds 256 blocks per launch, and a second batch overlaps its copies with this one's kernels
constexpr size_t kReadChunk = 4u << 20, kPinChunk = 32u << 20;

inline ScanLimit batch_limit(size_t batch_blocks, size_t dec_waves) {
  ScanLimit lim;
  lim.min_blocks = kBatchMinBlocks; lim.min_blocks_other = kBatchMinBlocksOther; lim.min_bytes = kBatchMinBytes; lim.max_blocks = kBatchMaxBlocks;
  // opts.dec_waves >= 2: a batch of 256 blocks would leave zh_chain's second to fourth wave of a compute unit without a block
  if (dec_waves > 1) lim.min_blocks_other = kBatchMinBlocksOther * dec_waves;
  if (batch_blocks) { lim.min_blocks = lim.max_blocks = batch_blocks; lim.min_blocks_other = 0; lim.min_bytes = 0; }   // zpaqhip_opts.batch_blocks
  return lim;
}

struct Source {
  const uint8_t *mem = nullptr;           // memory form
  size_t mem_len = 0, mem_pos = 0;
  zpaqhip_read_fn rd = nullptr;           // callback form (Reader.read, Reader.cs:14-25)
  void *user = nullptr;
  std::vector<uint8_t> buf;               // bytes read and not yet handed to a batch
  bool eof = false;
  uint64_t consumed = 0;                  // stream offset of the next unconsumed byte
};

constexpr uint64_t kInFix = 1ull << 63;   // Batch::off: the block lives in the second-pass buffer (offset | top bit)

struct Batch {
  std::vector<uint8_t> own;               // callback form: the batch's bytes (moved out of Source::buf)
  const uint8_t *h = nullptr;             // host bytes [0, len): whole blocks; tables in `so` are relative to h
  size_t len = 0;
  uint64_t stream_off = 0;
  ScanOut so;
  size_t blk0 = 0, seg0 = 0;              // global index of the first block / segment
  std::vector<uint64_t> off, cap, real;   // staging offset / capacity / plaintext length per block
  std::vector<zpaqhip_seg_result> res;    // per segment; out_off relative to the staging buffer
  int slot = 0;
  int rc_after = 0;                       // framing error that follows the last block of this batch ...
  zpaqhip_err err_after{};                // ... reported once everything before it has been delivered
  bool last = false;
};

// A header the framing scan accepts can still be refused when the model is built (component limits, table sizes:
// Predictor.cs:94-167).  The reference raises that at the block's Predictor.init, after everything before the block has
// been written; so the stream is cut in front of the first such block and the error is reported behind the cut.
// `header(b, p)` points p at block b's header bytes (valid until its next call) or returns the error of the call.
struct ModelCut {
  size_t nb = 0;                          // the blocks in front of the cut
  int rc = ZPAQHIP_OK;                    // what build_model says of block nb, with its message; OK: no cut
  zpaqhip_err err{};
};
template <class Header>
inline int first_bad_model(const std::vector<zpaqhip_block> &blocks, Header header, ModelCut &cut) {
  std::map<std::string, int> seen;
  for (cut.nb = 0; cut.nb < blocks.size(); ++cut.nb) {
    const uint32_t len = blocks[cut.nb].hdr_len;
    const uint8_t *h = nullptr;
    if (int rc = header(cut.nb, h)) return rc;
    const std::string key((const char *)h, len);
    const auto it = seen.find(key);
    if (it != seen.end() && !it->second) continue;
    ZhModel m;
    std::vector<uint8_t> code;
    zpaqhip_err e2{};
    cut.rc = seen[key] = build_model(h, len, m, code, &e2);             // (a bad header seen before: again, for the message)
    if (!cut.rc) continue;
    e2.block = (int32_t)cut.nb; e2.segment = -1;
    cut.err = e2;
    break;
  }
  return ZPAQHIP_OK;
}
inline void cut_at_bad_model(Batch &bt) {
  ModelCut cut;
  (void)first_bad_model(bt.so.blocks, [&](size_t b, const uint8_t *&p) { p = bt.h + bt.so.blocks[b].hdr_off; return ZPAQHIP_OK; }, cut);
  if (!cut.rc) return;
  const size_t b = cut.nb;
  bt.rc_after = cut.rc; bt.err_after = cut.err; bt.last = true;
  bt.so.blocks.resize(b);
  bt.so.segs.resize(b ? bt.so.blocks.back().first_seg + bt.so.blocks.back().n_seg : 0);
  bt.so.stopped = false;
  bt.len = b ? (size_t)bt.so.blocks.back().end_off : 0;
}

// Next batch of whole blocks, or batch.so.blocks.empty() at the end of the stream.  Returns a call-level error only.
inline int next_batch(Source &src, Batch &bt, size_t blk0, size_t seg0, size_t batch_blocks, size_t dec_waves, zpaqhip_err *err) {
  const ScanLimit lim = batch_limit(batch_blocks, dec_waves);
  bt = Batch();
  bt.blk0 = blk0; bt.seg0 = seg0;
  zpaqhip_err e2{};
  if (src.mem || !src.rd) {
    const uint8_t *w = src.mem + src.mem_pos;
    const size_t wl = src.mem_len - src.mem_pos;
    int rc = scan_stream(w, wl, bt.so, &e2, lim);
    bt.h = w; bt.stream_off = src.mem_pos;
    bt.len = bt.so.blocks.empty() ? 0 : (size_t)bt.so.blocks.back().end_off;
    if (rc) { bt.rc_after = rc; bt.err_after = e2; bt.last = true; src.mem_pos = src.mem_len; }
    else if (bt.so.stopped) src.mem_pos += bt.so.resume_off;
    else { bt.last = true; src.mem_pos = src.mem_len; }
    cut_at_bad_model(bt);
    if (bt.last) src.mem_pos = src.mem_len;
    return ZPAQHIP_OK;
  }
  for (;;) {                                            // Reader form: read until a batch is complete or the input ends
    int rc = scan_stream(src.buf.data(), src.buf.size(), bt.so, &e2, lim);
    const bool complete = bt.so.stopped || src.eof;
    if (rc && !(bt.so.hit_eof && !src.eof)) {           // damage that more input cannot repair
      bt.rc_after = rc; bt.err_after = e2; bt.last = true;
    } else if (!complete) {
      const size_t old = src.buf.size();
      src.buf.resize(old + kReadChunk);
      int n = src.rd(src.user, src.buf.data() + old, (int)kReadChunk);
      if (n < 0) { set_err(err, ZPAQHIP_E_CALLBACK, -1, -1); return ZPAQHIP_E_CALLBACK; }
      src.buf.resize(old + (size_t)n);
      if (n == 0) src.eof = true;
      continue;
    } else if (rc) {                                    // input ended inside a block
      bt.rc_after = rc; bt.err_after = e2; bt.last = true;
    }
    if (!bt.so.stopped) bt.last = true;
    bt.len = bt.so.blocks.empty() ? 0 : (size_t)bt.so.blocks.back().end_off;
    bt.stream_off = src.consumed;
    // hand the batch its bytes; keep the unconsumed tail for the next one
    const size_t keep_from = bt.last ? src.buf.size() : bt.so.resume_off;
    bt.own.assign(src.buf.begin(), src.buf.begin() + (ptrdiff_t)bt.len);
    src.buf.erase(src.buf.begin(), src.buf.begin() + (ptrdiff_t)keep_from);
    src.consumed += keep_from;
    bt.h = bt.own.data();
    cut_at_bad_model(bt);
    return ZPAQHIP_OK;
  }
}

inline void rebase_err(zpaqhip_err *err, const Batch &bt) {
  if (!err) return;
  if (err->block >= 0) err->block += (int)bt.blk0;
  if (err->segment >= 0) err->segment += (int)bt.seg0;
}

// ---- staging slots of a batch: the size hint of a block when it is plausible and within `budget`, else a provisional slot
// (a block that overflows it gets an exact second pass); when the sum exceeds the budget, the largest slots become
// count-only (0) until it fits.  Fills cap[] and off[]; returns the bytes of the staging buffer.
inline uint64_t provisional_slot(uint64_t coded) {
  return std::min<uint64_t>(std::max<uint64_t>(16 * coded, 64u << 10), 256ull << 20);
}
inline uint64_t plan_slots(const std::vector<zpaqhip_block> &blocks, const std::vector<zpaqhip_segment> &segs, uint64_t budget,
                           std::vector<uint64_t> &cap, std::vector<uint64_t> &off) {
  const size_t nb = blocks.size();
  cap.assign(nb, 0); off.assign(nb, 0);
  uint64_t sum = 0;
  for (size_t b = 0; b < nb; ++b) {
    const zpaqhip_block &B = blocks[b];
    uint64_t coded = 0;
    for (uint32_t i = 0; i < B.n_seg; ++i) coded += segs[B.first_seg + i].data_len;
    cap[b] = plausible_hint(B.usize_hint) && B.usize_hint <= budget ? B.usize_hint : provisional_slot(coded);
    sum += cap[b];
  }
  if (sum > budget) {                                   // does not fit: count-only for the largest slots until it does
    std::vector<size_t> order(nb);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b2) { return cap[a] > cap[b2]; });
    for (size_t k = 0; k < nb && sum > budget; ++k) { sum -= cap[order[k]]; cap[order[k]] = 0; }
  }
  uint64_t pos = 0;
  for (size_t b = 0; b < nb; ++b) { off[b] = pos; pos += cap[b]; }
  return pos;
}
// ... and when not even that can be reserved: every slot count-only, an exact second pass for every block
inline void count_only_slots(std::vector<uint64_t> &cap, std::vector<uint64_t> &off) {
  std::fill(cap.begin(), cap.end(), 0ull);
  std::fill(off.begin(), off.end(), 0ull);
}

// ---- second pass: plaintext sizes of a decoded batch (bt.real), and the blocks that did not fit their staging slot with
// their exact layout in a buffer of their own
struct SecondPass {
  std::vector<uint32_t> redo;
  std::vector<uint64_t> off2, cap2;
  uint64_t bytes = 0;
};
inline SecondPass plan_second_pass(Batch &bt) {
  SecondPass sp;
  for (size_t b = 0; b < bt.so.blocks.size(); ++b) {
    const zpaqhip_block &B = bt.so.blocks[b];
    uint64_t real = 0;
    bool full = false;
    for (uint32_t i = 0; i < B.n_seg; ++i) {
      real += bt.res[B.first_seg + i].out_len;
      full |= bt.res[B.first_seg + i].status == ZPAQHIP_E_OUTPUT_FULL;
    }
    bt.real[b] = real;
    if (full || real > bt.cap[b]) sp.redo.push_back((uint32_t)b);
  }
  for (uint32_t b : sp.redo) { sp.off2.push_back(sp.bytes); sp.cap2.push_back(bt.real[b]); sp.bytes += bt.real[b]; }
  return sp;
}

// ---- first segment that failed: everything before it is delivered, then the call ends with its error (the reference
// raises on reaching the damaged segment, Decompresser.cs:121-153)
struct FirstBad {
  bool found = false;
  size_t ok_blocks = 0;                   // whole blocks in front of it ...
  uint64_t partial = 0;                   // ... and bytes of its own block
  int rc = ZPAQHIP_OK;
  zpaqhip_err err{};                      // global block and segment
};
inline FirstBad first_failure(const Batch &B) {
  FirstBad f;
  f.ok_blocks = B.so.blocks.size();
  for (size_t b = 0; b < B.so.blocks.size(); ++b) {
    const zpaqhip_block &Bk = B.so.blocks[b];
    uint64_t before = 0;
    for (uint32_t i = 0; i < Bk.n_seg; ++i) {
      const zpaqhip_seg_result &r = B.res[Bk.first_seg + i];
      if (r.status != ZPAQHIP_OK) {
        f.found = true; f.ok_blocks = b; f.partial = before;
        f.rc = r.status == ZH_E_SKIPPED ? ZPAQHIP_E_CORRUPT : r.status;
        set_err(&f.err, f.rc, (int)(B.blk0 + b), (int)(B.seg0 + Bk.first_seg + i));
        return f;
      }
      before += r.out_len;
    }
  }
  return f;
}
// ... and the lowest block below f.limit with a failed segment, for zpaqhip_decompress_device.  Not first_failure: there
// ZPAQHIP_E_OUTPUT_FULL is a failure and the bytes in front of the failed segment are delivered; here a block that was
// clipped is decoded again, and whole blocks only are delivered.  Block and segment are the stream's.
struct FailedBlock {
  size_t limit = 0;                       // nothing from this block on is delivered
  int rc = ZPAQHIP_OK;
  zpaqhip_err err{};
};
inline void lowest_failed_block(const std::vector<zpaqhip_block> &blocks, const std::vector<zpaqhip_seg_result> &res, FailedBlock &f) {
  for (size_t b = 0; b < f.limit; ++b)
    for (uint32_t i = 0; i < blocks[b].n_seg; ++i) {
      const int st = res[blocks[b].first_seg + i].status;
      if (st == ZPAQHIP_OK || st == ZPAQHIP_E_OUTPUT_FULL) continue;
      f.limit = b;
      f.rc = st == ZH_E_SKIPPED ? ZPAQHIP_E_CORRUPT : st;
      set_err(&f.err, f.rc, (int)b, (int)(blocks[b].first_seg + i));
      return;
    }
}

// ---- zpaqhip_decompress_segments: per-segment records in stream order
struct SegSink {
  std::vector<zpaqhip_seg_result> res;
  std::vector<zpaqhip_segment> segs;
};
// The records of a settled batch, rebased: out_off from the staging buffers to the stream (`base`: the stream-order offset
// of the batch's first byte), block numbers to the stream's.
inline void append_segment_records(const Batch &B, uint64_t base, SegSink &out) {
  uint64_t run = 0;
  for (size_t b = 0; b < B.so.blocks.size(); ++b) {
    const zpaqhip_block &Bk = B.so.blocks[b];
    const uint64_t st_off = B.off[b] & ~kInFix;
    for (uint32_t i = 0; i < Bk.n_seg; ++i) {
      zpaqhip_seg_result r = B.res[Bk.first_seg + i];
      r.out_off = base + run + (r.out_off - st_off);
      out.res.push_back(r);
      zpaqhip_segment sg = B.so.segs[Bk.first_seg + i];
      sg.block += (uint32_t)B.blk0;
      out.segs.push_back(sg);
    }
    run += B.real[b];
  }
}

// ---- delivery
struct Sinkk {
  uint8_t *mem = nullptr; size_t cap = 0; // memory form
  zpaqhip_write_fn wr = nullptr;          // callback form (Writer.write, Writer.cs:19-24)
  void *user = nullptr;
  uint64_t total = 0;                     // plaintext bytes so far (counted past `cap` too)
  // multi-device form: block k of this source goes to mem + place[k] (sizes promised by the caller); sizes[k] = what
  // it really produced
  const uint64_t *place = nullptr;
  std::vector<uint64_t> *sizes = nullptr;
  // ... and at most place_cap[k] bytes of it; a block that is larger (a wrong or missing size in its comment) is kept
  // whole in spill[k] and put in place by the caller once every size is known
  const uint64_t *place_cap = nullptr;
  std::vector<std::vector<uint8_t>> *spill = nullptr;
  bool writer() const { return !place && !mem && wr; }
};

// One copy of a delivery: n bytes at src_off of the batch's staging (fix = false) or second-pass buffer, to dst: an offset
// in Sinkk::mem (memory and placed forms), the stream-order position (Writer form), or, with spill >= 0, the start of
// (*Sinkk::spill)[spill], which takes the whole block.
struct Copy {
  bool fix;
  uint64_t src_off, n, dst;
  long spill;
};
struct Delivery {
  std::vector<Copy> copies;
  uint64_t total = 0;                     // Sinkk::total once the copies are done
};

// What delivers the first `upto_blocks` blocks (plus `partial` bytes of the next one) of a decoded batch, in order.
// Memory and Writer forms: one copy per run of blocks that are contiguous in one buffer, clipped at the sink's capacity
// (the Writer form has none).  Placed form: whole blocks only, each at its place, clipped at the capacity; a block larger
// than its slot is spilled and nothing of it is written in place; sizes[] is filled.
inline Delivery plan_delivery(const Batch &bt, size_t upto_blocks, uint64_t partial, const Sinkk &sink) {
  Delivery d;
  d.total = sink.total;
  const size_t nb = bt.so.blocks.size();
  if (sink.place) {
    for (size_t b = 0; b < upto_blocks && b < nb; ++b) {
      const size_t g = bt.blk0 + b;
      const uint64_t n = bt.real[b], at = sink.place[g];
      if (sink.sizes) (*sink.sizes)[g] = n;
      if (sink.place_cap && n > sink.place_cap[g]) {
        if (sink.spill) d.copies.push_back({(bt.off[b] & kInFix) != 0, bt.off[b] & ~kInFix, n, 0, (long)g});
      } else if (n && at < sink.cap)
        d.copies.push_back({(bt.off[b] & kInFix) != 0, bt.off[b] & ~kInFix, std::min<uint64_t>(n, sink.cap - at), at, -1});
      d.total += n;
    }
    return d;
  }
  std::vector<Copy> pieces;                             // whole, dst not set yet
  for (size_t b = 0; b <= upto_blocks && b < nb; ++b) {
    const uint64_t n = b < upto_blocks ? bt.real[b] : std::min<uint64_t>(partial, bt.real[b]);
    if (!n) continue;
    const bool fix = (bt.off[b] & kInFix) != 0;
    const uint64_t src = bt.off[b] & ~kInFix;
    if (!pieces.empty() && pieces.back().fix == fix && pieces.back().src_off + pieces.back().n == src) pieces.back().n += n;
    else pieces.push_back({fix, src, n, 0, -1});
  }
  const uint64_t cap = sink.writer() ? UINT64_MAX : sink.cap;
  for (Copy pc : pieces) {
    const uint64_t n = pc.n;
    if (d.total < cap) { pc.n = std::min<uint64_t>(n, cap - d.total); pc.dst = d.total; d.copies.push_back(pc); }
    d.total += n;
  }
  return d;
}

// ---- zpaqhip_decompress_multi
// Blocks per pull of the queue when the caller does not say: a chunk that fills a GPU (256: one block per CU; 512 where every
// block is a single-CM one: two per CU) — but at least four pulls per device, or the queue has nothing to rebalance with
// (multigpu.default_queue_blocks is the same rule: tests/test_stream_plan.py)
inline size_t default_chunk_blocks(size_t nb, size_t n_dev, bool all_cm1) {
  const size_t full = all_cm1 ? 512 : 256, per4 = (nb + 4 * n_dev - 1) / (4 * n_dev);
  return n_dev <= 1 ? full : std::max<size_t>(1, std::min(full, per4));     // (one taker: nothing to balance)
}

// The queue: the blocks by estimated cost, descending (equal costs in stream order) ...
inline std::vector<size_t> queue_order(const std::vector<uint64_t> &cost) {
  std::vector<size_t> order(cost.size());
  std::iota(order.begin(), order.end(), (size_t)0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cost[a] > cost[b]; });
  return order;
}
// ... dealt into K chunks: chunk k = every K-th block of that order starting at k, in stream order (the pipeline delivers in
// order).  True when the chunk is a run of consecutive blocks (one chunk for the whole archive, typically): it is decoded
// where it lies, a strided one is gathered first.
inline bool queue_chunk(const std::vector<size_t> &order, size_t k, size_t K, std::vector<size_t> &ids) {
  ids.clear();
  for (size_t i = k; i < order.size(); i += K) ids.push_back(order[i]);
  std::sort(ids.begin(), ids.end());
  return ids.back() - ids.front() + 1 == ids.size();
}

// Placing: block b goes to out + (sum of the promised sizes before it), with the size its comment promises when that is
// plausible and ends inside out_cap, else 0 (the block is held back whole).  slot_off has one entry more than blocks.
inline void place_slots(const std::vector<zpaqhip_block> &blocks, uint64_t out_cap, std::vector<uint64_t> &slot_off,
                        std::vector<uint64_t> &slot_cap) {
  const size_t nb = blocks.size();
  slot_off.assign(nb + 1, 0); slot_cap.assign(nb, 0);
  for (size_t b = 0; b < nb; ++b) {
    const uint64_t h = blocks[b].usize_hint;
    slot_cap[b] = plausible_hint(h) && slot_off[b] + h <= out_cap ? h : 0;
    slot_off[b + 1] = slot_off[b] + slot_cap[b];
  }
}

// What a device thread has seen: the failure of a call itself (bad < 0), else the lowest block whose data was bad
struct MultiJob { int rc = 0; zpaqhip_err err{}; long bad = -1; zpaqhip_stats st{}; };

// The outcome of one chunk (blocks `ids`, the pipeline's rc / err / stream_error) noted in its thread's job.  Returns how
// many blocks of the chunk are good; *call_failed: the call itself failed, no thread goes on.
inline size_t note_chunk(MultiJob &J, const std::vector<size_t> &ids, int rc, const zpaqhip_err &e2, bool stream_error, bool *call_failed) {
  *call_failed = false;
  if (!rc) return ids.size();
  const bool at_block = (stream_error || data_error(rc)) && e2.block >= 0 && (size_t)e2.block < ids.size();
  if (!at_block) { if (!J.rc) { J.rc = rc; J.err = e2; J.bad = -1; } *call_failed = true; return 0; }
  const size_t good = (size_t)e2.block;
  const long g = (long)ids[good];
  if (J.bad < 0 || g < J.bad) { J.rc = rc; J.err = e2; J.bad = g; }
  return good;
}

// All threads' outcomes: a failure of the call itself first (rc, err); else the first damaged block of the stream
// (limit < nb, data_rc, data_err), in front of which everything is delivered.
struct MultiOutcome { int rc = 0; zpaqhip_err err{}; size_t limit = 0; int data_rc = 0; zpaqhip_err data_err{}; };
inline MultiOutcome merge_jobs(const std::vector<MultiJob> &jobs, size_t nb) {
  MultiOutcome o;
  o.limit = nb;
  for (const MultiJob &J : jobs)
    if (J.rc && J.bad < 0) { o.rc = J.rc; o.err = J.err; return o; }
  for (const MultiJob &J : jobs)
    if (J.rc && (size_t)J.bad < o.limit) { o.limit = (size_t)J.bad; o.data_rc = J.rc; o.data_err = J.err; o.data_err.block = (int32_t)o.limit; o.data_err.segment = -1; }
  return o;
}

// Puts the blocks whose size was not the promised one in place: blocks [0, limit) lie at out + slot_off[b] (real[b] bytes) or,
// held back, in spill[b]; afterwards they are consecutive from out.  *out_len = their bytes; ZPAQHIP_E_OUTPUT_FULL, and
// nothing moved, when that is more than out_cap.
inline int settle_places(uint8_t *out, size_t out_cap, size_t limit, const std::vector<uint64_t> &slot_off,
                         const std::vector<uint64_t> &slot_cap, const std::vector<uint64_t> &real,
                         const std::vector<std::vector<uint8_t>> &spill, size_t *out_len) {
  std::vector<uint64_t> new_off(limit + 1, 0);
  bool moved = false;
  for (size_t b = 0; b < limit; ++b) { new_off[b + 1] = new_off[b] + real[b]; moved |= real[b] != slot_cap[b]; }
  *out_len = (size_t)new_off[limit];
  if (new_off[limit] > out_cap) return ZPAQHIP_E_OUTPUT_FULL;
  if (!moved) return ZPAQHIP_OK;
  // blocks that lie in their slot (real <= promised) and move up: last first; those that move down: first first;
  // a block kept in a host buffer is written last, when every other block is where it belongs
  for (size_t b = limit; b-- > 0;)
    if (spill[b].empty() && real[b] && new_off[b] > slot_off[b]) memmove(out + new_off[b], out + slot_off[b], (size_t)real[b]);
  for (size_t b = 0; b < limit; ++b)
    if (spill[b].empty() && real[b] && new_off[b] < slot_off[b]) memmove(out + new_off[b], out + slot_off[b], (size_t)real[b]);
  for (size_t b = 0; b < limit; ++b)
    if (!spill[b].empty()) memcpy(out + new_off[b], spill[b].data(), (size_t)real[b]);
  return ZPAQHIP_OK;
}

// ---- zpaqhip_decompress_device: stream and plaintext both in device memory, one batch, no copy to the host.  The
// blocks in front of the first one without a plausible size are decoded straight to d_out, the rest to staging slots; a
// block that outgrew its room is decoded again with its exact size; one gather puts everything in place.
enum class DevWhere : uint8_t { kOut, kStaging, kFix };     // the caller's d_out, the staging buffer, the second-pass buffer
inline uint32_t frame_src(DevWhere w) {                     // ... as zh_frame.hip's entries name them
  return w == DevWhere::kOut ? ZH_FRAME_SRC_INPUT : w == DevWhere::kStaging ? ZH_FRAME_SRC_FIRST : ZH_FRAME_SRC_REDO;
}
// Where a block lies.  (Batch::off | kInFix does not carry this: its one bit tells two buffers apart and here are three, and
// a moved block's segment records keep speaking of the place it was decoded to.)
struct DevBlock {
  DevWhere buf = DevWhere::kOut;
  uint64_t off = 0;                       // of the block in buf
  uint64_t rec_off = 0;                   // the offset its segment records count from: off, or for a moved block its first place
  uint64_t cap = 0, real = 0;             // room it was decoded with / plaintext length
};
struct DevDecode {                        // one decode launch: blocks ids[i] to base + off[i], at most cap[i] bytes
  std::vector<uint32_t> ids;
  std::vector<uint64_t> off, cap;
  void add(size_t b, uint64_t o, uint64_t c) { ids.push_back((uint32_t)b); off.push_back(o); cap.push_back(c); }
};
struct DevPlan {
  std::vector<zpaqhip_block> blocks;      // the stream's tables, cut in front of the first block whose model is refused
  std::vector<zpaqhip_segment> segs;
  std::vector<zpaqhip_seg_result> res;    // per segment, as the last decode of its block left it
  std::vector<DevBlock> at;
  size_t k = 0;                           // blocks [0, k) went straight to d_out
  FailedBlock bad;
  void cut(size_t nb) {
    blocks.resize(nb);
    segs.resize(nb ? blocks[nb - 1].first_seg + blocks[nb - 1].n_seg : 0);
    res.assign(segs.size(), zpaqhip_seg_result{});
    at.assign(nb, DevBlock{});
    bad.limit = nb;
  }
};

// Direct phase: every leading block with a plausible size at the sum of the sizes before it; what lies behind out_cap is
// counted, not written (capacity clipped at out_cap, 0 at or beyond it).
inline DevDecode plan_direct(DevPlan &p, uint64_t out_cap) {
  DevDecode d;
  uint64_t place = 0;
  for (p.k = 0; p.k < p.blocks.size() && plausible_hint(p.blocks[p.k].usize_hint); ++p.k) {
    const uint64_t hint = p.blocks[p.k].usize_hint;
    DevBlock &B = p.at[p.k];
    B.buf = DevWhere::kOut; B.off = B.rec_off = place;
    B.cap = place >= out_cap ? 0 : std::min<uint64_t>(hint, out_cap - place);
    d.add(p.k, place, B.cap);
    place += hint;
  }
  return d;
}
// Staging phase: blocks [k, nb) in the slots plan_slots gave blocks.begin() + k ...
inline DevDecode plan_staged(DevPlan &p, const std::vector<uint64_t> &cap, const std::vector<uint64_t> &off) {
  DevDecode d;
  for (size_t b = p.k; b < p.blocks.size(); ++b) {
    DevBlock &B = p.at[b];
    B.buf = DevWhere::kStaging; B.off = B.rec_off = off[b - p.k]; B.cap = cap[b - p.k];
    d.add(b, B.off, B.cap);
  }
  return d;
}
// After a decode: the plaintext sizes of its blocks (segments count past the capacity), and the lowest failed block
inline void note_decoded(DevPlan &p, const std::vector<uint32_t> &ids) {
  for (uint32_t b : ids) {
    p.at[b].real = 0;
    for (uint32_t i = 0; i < p.blocks[b].n_seg; ++i) p.at[b].real += p.res[p.blocks[b].first_seg + i].out_len;
  }
  lowest_failed_block(p.blocks, p.res, p.bad);
}

// After the first decode.  A size comment that was wrong: the first such block keeps its place when it is shorter,
// every directly placed block behind it is whole but in the wrong place, and is moved out of the way (d_out to the
// second-pass buffer) before anything is gathered.  Every block that outgrew its room is decoded a second time, with its
// exact size, into the same buffer (a block is decoded twice at most).
struct DevSecond {
  DevDecode redo;
  std::vector<ZhFrameEntry> move;
  uint64_t fix_bytes = 0;                 // of the second-pass buffer
};
inline DevSecond plan_device_second(DevPlan &p) {
  DevSecond s;
  size_t wrong = p.k;
  for (size_t b = 0; b < p.k && b < p.bad.limit; ++b)
    if (p.at[b].real != p.blocks[b].usize_hint) { wrong = b; break; }
  for (size_t b = 0; b < p.bad.limit; ++b) {
    DevBlock &B = p.at[b];
    if (B.real > B.cap) {
      s.redo.add(b, s.fix_bytes, B.real);
      B.off = B.rec_off = s.fix_bytes; B.cap = B.real;
    } else if (b < p.k && b > wrong) {
      ZhFrameEntry e{};
      e.dst_off = s.fix_bytes; e.src_off = B.off; e.body_len = B.real; e.src = frame_src(DevWhere::kOut);
      if (B.real) s.move.push_back(e);
      B.off = s.fix_bytes;
    } else continue;
    B.buf = DevWhere::kFix;
    s.fix_bytes += B.real;
  }
  return s;
}

// Checksums: the (offset, length) pairs of buffer w's segments that store a SHA-1 and decoded without an error
struct Sha1Table {
  std::vector<uint64_t> pairs;
  std::vector<uint32_t> which;            // pair j is segment which[j]
  void add(const zpaqhip_segment &g, const zpaqhip_seg_result &r, size_t s, uint64_t off) {
    if (!(g.flags & 1) || r.status != ZPAQHIP_OK) return;
    pairs.push_back(off); pairs.push_back(r.out_len); which.push_back((uint32_t)s);
  }
};
inline Sha1Table device_sha1_table(const DevPlan &p, DevWhere w) {
  Sha1Table t;
  for (size_t b = 0; b < p.bad.limit; ++b) {
    if (p.at[b].buf != w) continue;
    for (uint32_t i = 0; i < p.blocks[b].n_seg; ++i) {
      const size_t s = p.blocks[b].first_seg + i;
      t.add(p.segs[s], p.res[s], s, p.at[b].off + (p.res[s].out_off - p.at[b].rec_off));
    }
  }
  return t;
}

// Gather: blocks [0, limit) consecutive from d_out; every one that does not lie there already copied in, clipped at out_cap
struct DevGather {
  std::vector<uint64_t> dst;              // final offset of block b; dst[limit] = out_len
  std::vector<ZhFrameEntry> entries;
  uint64_t out_len() const { return dst.back(); }
};
inline DevGather plan_gather(const DevPlan &p, uint64_t out_cap) {
  DevGather g;
  g.dst.assign(p.bad.limit + 1, 0);
  for (size_t b = 0; b < p.bad.limit; ++b) {
    const DevBlock &B = p.at[b];
    g.dst[b + 1] = g.dst[b] + B.real;
    if (B.buf == DevWhere::kOut || !B.real || g.dst[b] >= out_cap) continue;
    ZhFrameEntry e{};
    e.dst_off = g.dst[b]; e.src_off = B.off; e.body_len = std::min<uint64_t>(B.real, out_cap - g.dst[b]); e.src = frame_src(B.buf);
    g.entries.push_back(e);
  }
  return g;
}

// Result records: those of the delivered blocks with out_off in stream order, and the failed block's as they are
inline size_t device_result_count(const DevPlan &p) {
  const size_t l = p.bad.limit;
  return l < p.blocks.size() ? p.blocks[l].first_seg + p.blocks[l].n_seg : p.segs.size();
}
inline void device_results(const DevPlan &p, const DevGather &g, zpaqhip_seg_result *results) {
  for (size_t b = 0; b < p.blocks.size() && b <= p.bad.limit; ++b)
    for (uint32_t i = 0; i < p.blocks[b].n_seg; ++i) {
      const size_t s = p.blocks[b].first_seg + i;
      results[s] = p.res[s];
      if (b < p.bad.limit) results[s].out_off = g.dst[b] + (p.res[s].out_off - p.at[b].rec_off);
    }
}

// ---- statistics: what the sums of the pipeline, the second pass and the multi-device threads have in common
inline void add_kernel_stats(zpaqhip_stats &acc, const zpaqhip_stats &s) {   // a launch's kernel work
  acc.kernel_ms += s.kernel_ms; acc.launches += s.launches; acc.e8_wave_segs += s.e8_wave_segs;
}
inline void add_block_stats(zpaqhip_stats &acc, const zpaqhip_stats &s) {    // ... and what it decoded, once per block
  acc.blocks += s.blocks; acc.in_bytes += s.in_bytes; acc.model_bytes += s.model_bytes;
  acc.concurrent = std::max(acc.concurrent, s.concurrent); acc.kernel_kind = std::max(acc.kernel_kind, s.kernel_kind);
}

}  // namespace zh
