// zh_compress.h — the host side of the compress path, shared by zpaqhip_compress_blocks (zh_compress.cpp) and the method
// entry points (zh_pre.cpp): call-scoped device resources, the device-memory budget (zh_api.cpp's too), the batch rule,
// block framing, the SHA-1 step, the call epilogue, the device pre-processing stage and the batch loop itself.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zh_ctx_view.h"
#include "zh_frame.h"

namespace zh {

struct DevMem {                           // device buffer owned by one call
  void *p = nullptr;
  ~DevMem() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) {
    if (p) { (void)hipFree(p); p = nullptr; }
    return hipMalloc(&p, std::max<size_t>(n, 256));
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

struct Event {                            // one event owned by one call
  hipEvent_t e = nullptr;
  ~Event() { if (e) (void)hipEventDestroy(e); }
};

inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// Device bytes a call may plan with: what is free (plus `reusable`, the caller's own cached bytes) less 1 GiB of headroom,
// or half of it when little is free, divided among the contexts that share the device.
hipError_t device_budget(uint32_t mem_share, uint64_t reusable, uint64_t *budget);

// opts as the call uses them (struct_size-aware copy); NULL means SHA-1 and tag (flags = 3)
zpaqhip_compress_opts resolve_compress_opts(const zpaqhip_compress_opts *opts);

// End of the batch that starts at block b0: opts.batch_blocks blocks when set, else blocks while their cost fits half the
// budget (at least one block, at most 4096).
template <class Cost>
size_t batch_end(size_t b0, size_t n_blocks, uint64_t batch_blocks, uint64_t budget, Cost cost_of) {
  if (batch_blocks) return std::min<size_t>(n_blocks, b0 + batch_blocks);
  size_t b1 = b0 + 1;
  uint64_t cost = cost_of(b0);
  while (b1 < n_blocks && b1 - b0 < 4096 && cost + cost_of(b1) <= budget / 2) cost += cost_of(b1++);
  return b1;
}

// SHA-1 (zh_sha1_dev.hip) of the segments d_base + seg[2k] of seg[2k + 1] bytes: five words per segment in `digest`.
int sha1_segments(const CtxView &v, const uint8_t *d_base, const std::vector<uint64_t> &seg, std::vector<uint32_t> &digest,
                  zpaqhip_err *err);

// The end of every call: off[n_blocks], zpaqhip_last_stats and *out_len from the bytes needed; ZPAQHIP_E_OUTPUT_FULL when
// they exceed out_cap.
int finish_call(const CtxView &v, zpaqhip_stats st, uint64_t pos, size_t n_blocks, uint64_t *off, size_t out_cap, size_t *out_len,
                zpaqhip_err *err);

// How a method's blocks are pre-processed (zh_pre.cpp): what args[1] and the caller's opt-ins select
enum class Route : uint32_t {
  Copy,                                   // level 0: the plaintext is the coded data
  E8E9,                                   // level 0 with E8E9: the transform is the coded data
  Greedy,                                 // levels 1 / 2, the parse of tools/methods._matches (zh_pre_lz.hip)
  Bwt,                                    // level 3 (zh_pre_bwt.hip)
  Sa,                                     // levels 1 / 2, the reference's suffix-array search (tools/methods.lz77_sa, zh_pre_lzsa.hip)
  Ht,                                     // levels 1 / 2, the reference's hash-table search (tools/methods.lz77_ht, zh_pre_lzht.hip)
};

// the method's numbers (tools/methods.preprocess / lz77_level1 / lz77_level2)
struct Method {
  Route route = Route::Copy;
  uint32_t level = 0;                     // args[1] & 3: the format of the codes
  uint32_t doe8 = 0;                      // 4 <= args[1] <= 7; from Greedy on the route reads the E8E9 copy of a block
  uint32_t k = 0, m = 0, rb = 0, max_match = 0, max_off = 0;        // k, max_match, max_off: Greedy only
  uint64_t max_block = ~0ull;             // levels 1 / 2: 2^(args[0] + 20), the PCOMP's M; level 3: 4096 less (LibZPAQ.cs:289)
  uint32_t bucket = 0, lookahead = 0, win_bits = 0;                 // Sa (bucket: Ht too)
  uint32_t ht_bits = 0, checkbits = 0, shift1 = 0, search = 0;      // Ht
  bool slots() const { return route == Route::Bwt || route == Route::Sa || route == Route::Ht; }   // routes in the sort's slot space
  bool e8_copy() const { return doe8 && route != Route::E8E9; }
};

struct PreBatch {                         // what DevPre::run leaves of a batch [b0, b1)
  std::vector<uint64_t> len;              // pre-processed bytes of block b0 + j
  const uint8_t *plain = nullptr;         // device copy of in[in_off[b0], in_off[b1]), valid until the next run
  float ms = 0;                           // device time of the pre-processing
};

// Device pre-processing of a batch of blocks (zh_pre.cpp), in place of the host copy of their coded bytes.
class DevPre {
 public:
  // `in_dev`: `in` is device memory; run then copies the batch device to device (the kernels read past a block's end in
  // aligned groups, so they always work on the stage's own aligned copy)
  // `src_off` (with in_dev): block i's bytes are at in + src_off[i] instead of in + in_off[i], which then only gives the
  // lengths: the blocks of one group of a mixed call, which lie anywhere in the caller's memory
  DevPre(const Method &M, const uint8_t *in, const uint64_t *in_off, bool in_dev = false, const uint64_t *src_off = nullptr)
      : M_(M), in_(in), in_off_(in_off), in_dev_(in_dev), src_off_(src_off) {}
  uint64_t n_of(size_t i) const { return in_off_[i + 1] - in_off_[i]; }
  uint64_t bound(size_t i) const;         // pre-processed bytes of block i at most
  uint64_t scratch(size_t i) const;       // device bytes the stage needs for block i
  // Write the coded sequence of block b0 + j (prefix, then its pre-processed bytes) at d_out + off[j], for j < b1 - b0.
  int run(const CtxView &v, size_t b0, size_t b1, uint8_t *d_out, const std::vector<uint64_t> &off,
          const std::vector<uint8_t> &prefix, PreBatch &r, zpaqhip_err *err);
  uint32_t launches = 0;

 private:
  Method M_;
  const uint8_t *in_;
  const uint64_t *in_off_;
  bool in_dev_;
  const uint64_t *src_off_;
  DevMem plain_, e8_, len_, desc_, pref_;
  DevMem tab_, chain_, prev_;             // Greedy: ZhPreLaunch's table, chain and prev
  DevMem starts_, arena_;                 // slot routes: the slot starts of every launch; zh_pre.cpp's SortArena
};

// A stream in device memory that a call owns and several compress_impl runs append to (the scratch of a mixed call): it
// grows to what the runs turn out to need, keeping what it holds.
struct DevSink {
  DevMem mem;
  uint64_t cap = 0, used = 0;
  uint8_t *base() const { return mem.as<uint8_t>(); }
  // room for `need` bytes, keeping [0, keep): when it grows, to at least twice the old capacity
  hipError_t reserve(uint64_t need, uint64_t keep, hipStream_t stream);
};
// With `sink`, `out` and `out_cap` are not used: the stream is appended to the sink at sink->used (block_off counts from
// there) and nothing is ever too small.
struct DeviceEnds { hipStream_t stream = nullptr; DevSink *sink = nullptr; };
// The solid form (zpaqhip_compress_solid_blocks): block i holds the segments [seg_first[i], seg_first[i + 1]), whose coded
// bytes, described bytes and names the per-segment `in_off`, `orig_off` (NULL without `orig`) and the call's `filenames`
// give; the call's own in_off / orig_off are then the blocks' view of them (in_off[seg_first[i]]).  Without `pre` and
// without a sink only.
struct SolidSegs { const uint64_t *seg_first, *in_off, *orig_off; };

// The batch loop and its arguments.  Without `pre`, block i's coded bytes are in[in_off[i], in_off[i+1]) and `orig`, when
// given, is what the size comment and SHA-1 describe.  With `pre` (the method path) `in` is the plaintext and `orig` NULL; a
// header with n = 0 then gets the store layout instead of an encoder.  `dev`, when given, is the device form: `in`, `orig`
// and `out` are then device pointers on the context's device, `pre` was made with in_dev, and the work runs on dev->stream
// when that is set.  Without `solid` every block is one segment.
struct CompressCall {
  zpaqhip_ctx *ctx = nullptr;
  const uint8_t *hdr = nullptr; size_t hdr_len = 0;
  const uint8_t *pcomp = nullptr; size_t pcomp_len = 0;
  const uint8_t *in = nullptr; const uint64_t *in_off = nullptr; size_t n_blocks = 0;
  const uint8_t *orig = nullptr; const uint64_t *orig_off = nullptr;
  const char *const *filenames = nullptr;
  uint8_t *out = nullptr; size_t out_cap = 0; size_t *out_len = nullptr; uint64_t *block_off = nullptr;
  const zpaqhip_compress_opts *opts = nullptr;
  DevPre *pre = nullptr;
  zpaqhip_err *err = nullptr;
  const DeviceEnds *dev = nullptr;
  const SolidSegs *solid = nullptr;
};
int compress_impl(const CompressCall &a);

}  // namespace zh
