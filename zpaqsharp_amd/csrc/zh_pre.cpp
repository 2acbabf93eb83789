// zh_pre.cpp — LibZPAQ.compressBlock for a method (LibZPAQ.cs:296-323): the pre-processing of a method's blocks on the GPU,
// by one of the routes of zh_compress.h's Route.  parse_method turns args and the caller's opt-ins into a Method (the route
// and its numbers); DevPre is the stage: compress_impl (zh_compress.cpp) runs it in place of its host copy and then codes
// the bytes where the kernels left them (n >= 1 headers) or stores them (n = 0 headers); zpaqhip_preprocess_blocks,
// zpaqhip_bwt_blocks, zpaqhip_lzsa_blocks and zpaqhip_lzht_blocks return them as they are.  DevPre::run is a sequence:
// describe the batch, upload, prefix / E8E9, the route's launches, read the lengths back.  The device arrays of the sort
// that the Bwt, Sa and Ht routes share are laid out by SortArena below, and nowhere else.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "zh_analyze.h"
#include "zh_compress.h"
#include "zh_ctx_view.h"
#include "zh_pre.h"

// every launcher adds the kernels it launched to *launches
extern "C" hipError_t zh_launch_pre_prefix(const ZhPreLaunch *L, const uint8_t *prefix, uint32_t np, hipStream_t stream, uint32_t *launches);
extern "C" hipError_t zh_launch_pre_e8e9(const ZhPreLaunch *L, hipStream_t stream, uint32_t *launches);
extern "C" hipError_t zh_launch_pre_lz(const ZhPreLaunch *L, uint64_t max_n, hipStream_t stream, uint32_t *launches);
extern "C" hipError_t zh_launch_pre_bwt(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *rounds);
extern "C" hipError_t zh_launch_pre_sufsort(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *c);
extern "C" hipError_t zh_launch_pre_lzsa(const ZhLzsaLaunch *L, hipStream_t stream, uint32_t *launches);
extern "C" hipError_t zh_launch_pre_lzht(const ZhLzhtLaunch *L, const ZhBwtLaunch *W, uint64_t *const words[2], hipStream_t stream,
                                         uint32_t *launches);
extern "C" hipError_t zh_launch_gap_hist(const ZhGapLaunch *L, uint32_t n_blocks, uint64_t max_n, hipStream_t stream);

using namespace zh;

namespace {

constexpr uint32_t kFlagBwt = 4;          // zpaqhip_compress_opts.flags: accept level 3
constexpr uint32_t kFlagSa = 8;           // ... the reference's suffix-array search where the method selects it
constexpr uint32_t kFlagHt = 16;          // ... the reference's hash-table search where the method selects it

int refuse(zpaqhip_err *err, const char *why = nullptr) {
  set_err(err, ZPAQHIP_E_ARG, -1, -1, why);
  return ZPAQHIP_E_ARG;
}

// ---- the method: its route, the route's rules, its numbers ------------------------------------------------------------
Route route_of(const int32_t *args, uint32_t flags) {
  const uint32_t level = (uint32_t)args[1] & 3;
  if (level == 0) return args[1] >= 4 && args[1] <= 7 ? Route::E8E9 : Route::Copy;
  if (level == 3) return Route::Bwt;
  if (!(flags & (kFlagSa | kFlagHt))) return Route::Greedy;
  if (args[5] - args[0] >= 21) return flags & kFlagSa ? Route::Sa : Route::Greedy;      // LZBuffer.cs:153-158
  return flags & kFlagHt ? Route::Ht : Route::Greedy;
}

int check_bwt(const int32_t *args, uint32_t flags, zpaqhip_err *err) {
  if (!(flags & kFlagBwt)) return refuse(err, "BWT (level 3) pre-processing is not available on the GPU");
  if (args[0] < 0 || args[2] < 0) return refuse(err);
  return ZPAQHIP_OK;
}

int check_greedy(const int32_t *args, uint32_t level, zpaqhip_err *err) {
  if (level == 2 && (args[2] < 1 || args[2] > 64)) return refuse(err, "level 2 needs a minimum match length of 1 to 64 (args[2])");
  if (args[0] < 0 || args[2] < 0) return refuse(err);
  return ZPAQHIP_OK;
}

int check_sa(const int32_t *args, uint32_t level, zpaqhip_err *err) {             // LZBuffer.cs:205
  if (const int rc = check_greedy(args, level, err)) return rc;                  // the rules of the greedy route hold here too
  if (level == 1 && args[2] < 4)                                                 // LZBuffer.cs:198-199
    return refuse(err, "level 1 needs a minimum match length of 4 or more (args[2])");
  if (args[3] < 0 || args[4] < 0 || args[4] > 30 || args[6] < 0 || args[6] > 255 || args[2] > 255)
    return refuse(err, "the suffix-array search takes args[2] and args[6] up to 255 and args[4] up to 30");
  return ZPAQHIP_OK;
}

int check_ht(const int32_t *args, uint32_t level, zpaqhip_err *err) {
  if (args[0] < 0 || args[0] > 11) return refuse(err, "the hash-table search takes args[0] up to 11");
  if (args[3] != 0 || args[6] != 0)
    return refuse(err, "the hash-table search takes neither a second hash order (args[3]) nor look-ahead (args[6])");
  if (args[2] < (level == 1 ? 4 : 2) || args[2] > 255)                           // LZBuffer.cs:198-199, :317
    return refuse(err, "the hash-table search needs a minimum match length (args[2]) of 4 (level 1) or 2 (level 2) to 255");
  if (args[5] < 0 || args[5] > 30 || args[4] < 0 || args[4] > args[5] || args[4] > (int32_t)ZH_LZHT_MAX_BUCKET_BITS)
    return refuse(err, "the hash-table search takes args[5] up to 30 and args[4] up to args[5] and 6");
  return ZPAQHIP_OK;
}

void fill_numbers(const int32_t *args, Method &M) {
  if (M.level == 1) {
    M.k = (uint32_t)std::max(4, args[2]);
    M.rb = args[0] > 4 ? (uint32_t)(args[0] - 4) : 0;
    M.max_match = 1u << 16;
    M.max_off = (1u << 23) - 1;
  } else if (M.level == 2) {
    M.m = (uint32_t)args[2];
    M.k = std::max<uint32_t>(M.m, 3);
    M.max_match = M.m + 63 + 256;
    M.max_off = (1u << 24) - 1;
  }
  if (M.level) M.max_block = std::min<uint64_t>((1ull << std::min(args[0] + 20, 62)) - (M.level == 3 ? 4096 : 0), (1ull << 31) - 1);
  if (M.route != Route::Sa && M.route != Route::Ht) return;
  M.m = (uint32_t)args[2];
  M.bucket = (1u << args[4]) - 1;
  M.max_block = std::min<uint64_t>(M.max_block, 1ull << 24);                    // offsets of 2^24 and more are not written
  if (M.route == Route::Sa) {
    M.lookahead = (uint32_t)args[6];
    M.win_bits = (uint32_t)std::min(17 + args[0], 31);
  } else {
    M.ht_bits = (uint32_t)args[5];
    M.checkbits = (uint32_t)(12 - args[0]);
    M.shift1 = (uint32_t)((args[5] - 1) / args[2] + 1);                         // C division: args[5] = 0 gives 1
    M.search = M.level == 1 || args[2] <= 64;                                   // LZBuffer.cs:288
  }
}

int parse_method(const int32_t *args, uint32_t flags, Method &M, zpaqhip_err *err) {
  if (!args) return refuse(err);
  M.level = (uint32_t)args[1] & 3;
  M.doe8 = args[1] >= 4 && args[1] <= 7;
  M.route = route_of(args, flags);
  int rc = ZPAQHIP_OK;
  switch (M.route) {
    case Route::Copy: case Route::E8E9: break;
    case Route::Greedy: rc = check_greedy(args, M.level, err); break;
    case Route::Bwt: rc = check_bwt(args, flags, err); break;
    case Route::Sa: rc = check_sa(args, M.level, err); break;
    case Route::Ht: rc = check_ht(args, M.level, err); break;
  }
  if (!rc) fill_numbers(args, M);
  return rc;
}

// pre-processed bytes at most: a literal run of L costs 8L + 2 lg(L) + 1 <= 11L bits and a match of l >= 4 at most 8l bits
// (level 1); a literal costs at most 2 bytes and a match piece at most 4 bytes for 3 or more bytes (level 2).  The
// hash-table search accepts a match of l bytes at offset o only with 8 l > lg(o) + 11: at level 2 that is
// l >= 2, 3 bytes for 2, and a piece of a split match has args[2] >= 2 bytes for at most 4
uint64_t pre_bound(const Method &M, uint64_t n) {
  if (M.level == 1) return (11 * n + 7) / 8 + 16;
  if (M.level == 2) return 2 * n + 64;
  if (M.level == 3) return n + 5;         // LZBuffer.cs:233-239
  return n;
}

uint32_t tab_bits(uint64_t n) {           // Greedy: at least two table entries per position
  uint32_t b = 10;
  while (b < 30 && (1ull << b) < 2 * n) ++b;
  return b;
}

// ---- the sort's arena ---------------------------------------------------------------------------------------------------
// The device arrays of zh_pre_bwt.hip's sort over a slot space of n slots, in one allocation, in this order:
//   key[0], val[0], key[1], val[1]   4n bytes each: the pairs of the radix sort, ping and pong
//   dec                              8n bytes, Sa and Ht only: the decisions of positions reached with lit == 0
//   rank                             4n bytes
//   counts                           1024 bytes per radix tile of 4096 pairs: the digit counts
//   sums                             4 bytes per partial result of a scan
//   multi                            4 bytes
// Every offset is a multiple of 4, and those of the pairs and of dec multiples of 8.
struct SortArena {
  uint64_t n, tiles, nsums;
  bool has_dec;
  uint8_t *base = nullptr;                // set once the arena is allocated
  SortArena(uint64_t n, bool has_dec)
      : n(n), tiles((n + 4095) / 4096), nsums(2 * ((std::max<uint64_t>(n, 256 * tiles) + 4095) / 4096) + 2), has_dec(has_dec) {}
  uint64_t pair_at(uint32_t q) const { return 8 * n * q; }
  uint64_t dec_at() const { return 16 * n; }
  uint64_t rank_at() const { return dec_at() + (has_dec ? 8 * n : 0); }
  uint64_t counts_at() const { return rank_at() + 4 * n; }
  uint64_t sums_at() const { return counts_at() + 1024 * tiles; }
  uint64_t multi_at() const { return sums_at() + 4 * nsums; }
  uint64_t bytes() const { return multi_at() + 4; }
  // what DevPre::scratch plans with: DevMem hands out at least 256 bytes per buffer, and the estimate has always carried 4 more
  uint64_t budget() const { return bytes() + 5 * 256 + 4; }
  template <class T> T *at(uint64_t off) const { return reinterpret_cast<T *>(base + off); }
  uint64_t *dec() const { return at<uint64_t>(dec_at()); }
  // key[q] and val[q] are adjacent, so a pair the sort is done with is one array of n 64-bit words: the routes that search
  // a finished sort keep the decisions of positions reached with lit > 0 in the pair the sort did not end in
  uint64_t *pair_words(uint32_t q) const { return at<uint64_t>(pair_at(q)); }
  void fill(ZhBwtLaunch &W) const {
    for (uint32_t q = 0; q < 2; ++q) {
      W.key[q] = at<uint32_t>(pair_at(q));
      W.val[q] = W.key[q] + n;
    }
    W.rank = at<uint32_t>(rank_at());
    W.counts = at<uint32_t>(counts_at());
    W.sums = at<uint32_t>(sums_at());
    W.multi = at<uint32_t>(multi_at());
  }
};

// ---- the launches of a batch in the slot space --------------------------------------------------------------------------
constexpr uint64_t kMaxSlots = (1ull << 31) - 1;

struct LaunchCuts {
  std::vector<size_t> cut;                // first block of each launch, then the number of blocks
  std::vector<uint32_t> starts;           // ZhSlotSpace::starts of launch u at starts[cut[u] + u ..]
  uint64_t max_slots = 0;                 // of the largest launch
};

// Cuts the blocks of a batch into launches of at most kMaxSlots slots and sets every block's scr_off, its first slot
LaunchCuts cut_launches(std::vector<ZhPreBlock> &desc) {
  LaunchCuts C;
  C.cut.push_back(0);
  uint64_t scr = 0;
  for (size_t j = 0; j < desc.size(); ++j) {
    if (scr + desc[j].n > kMaxSlots) {    // the next launch starts here
      C.cut.push_back(j);
      C.max_slots = std::max(C.max_slots, scr);
      scr = 0;
    }
    desc[j].scr_off = scr;
    scr += desc[j].n;
  }
  C.max_slots = std::max(C.max_slots, scr);
  C.cut.push_back(desc.size());
  for (size_t u = 0; u + 1 < C.cut.size(); ++u) {
    for (size_t j = C.cut[u]; j < C.cut[u + 1]; ++j) C.starts.push_back((uint32_t)desc[j].scr_off);
    C.starts.push_back((uint32_t)(desc[C.cut[u + 1] - 1].scr_off + desc[C.cut[u + 1] - 1].n));
  }
  return C;
}

// ---- the routes in the slot space: one launch W each --------------------------------------------------------------------
int run_bwt(const ZhBwtLaunch &W, const CtxView &v, uint32_t &launches, zpaqhip_err *err) {
  uint32_t rounds = 0;                    // the launcher reports its doubling rounds; nothing here uses them
  HIPCHK(zh_launch_pre_bwt(&W, v.stream, &launches, &rounds));
  return ZPAQHIP_OK;
}

int run_sa(const Method &M, const ZhBwtLaunch &W, const SortArena &A, const CtxView &v, uint32_t &launches, zpaqhip_err *err) {
  uint32_t c = 0;
  HIPCHK(zh_launch_pre_sufsort(&W, v.stream, &launches, &c));
  ZhLzsaLaunch S{};
  static_cast<ZhSlotSpace &>(S) = W;
  S.sa = W.val[c];
  S.rank = W.rank;
  S.lcp = W.key[c];                       // the sort is done with its keys and with the other pair of arrays
  S.dec[0] = A.dec();
  S.dec[1] = A.pair_words(c ^ 1);
  S.level = M.level; S.min_match = M.m; S.bucket = M.bucket; S.lookahead = M.lookahead; S.win_bits = M.win_bits; S.rb = M.rb;
  HIPCHK(zh_launch_pre_lzsa(&S, v.stream, &launches));
  return ZPAQHIP_OK;
}

int run_ht(const Method &M, const ZhBwtLaunch &W, const SortArena &A, const CtxView &v, uint32_t &launches, zpaqhip_err *err) {
  ZhLzhtLaunch H{};
  static_cast<ZhSlotSpace &>(H) = W;
  H.dec[0] = A.dec();
  H.level = M.level; H.min_match = M.m; H.bucket = M.bucket; H.ht_bits = M.ht_bits; H.checkbits = M.checkbits;
  H.shift1 = M.shift1; H.search = M.search; H.rb = M.rb;
  uint64_t *const words[2] = {A.pair_words(0), A.pair_words(1)};
  HIPCHK(zh_launch_pre_lzht(&H, &W, words, v.stream, &launches));
  return ZPAQHIP_OK;
}

}  // namespace

uint64_t zh::DevPre::bound(size_t i) const { return pre_bound(M_, n_of(i)); }

uint64_t zh::DevPre::scratch(size_t i) const {
  const uint64_t n = n_of(i), c = n + 64 + (M_.e8_copy() ? n : 0);
  if (M_.slots()) return c + SortArena(n, M_.route != Route::Bwt).budget();
  if (M_.route == Route::Greedy) return c + 8 * n + (4ull << tab_bits(n));
  return c;
}

int zh::DevPre::run(const CtxView &v, size_t b0, size_t b1, uint8_t *d_out, const std::vector<uint64_t> &off,
                    const std::vector<uint8_t> &prefix, PreBatch &r, zpaqhip_err *err) {
  // the batch: its blocks and, in the slot space, the launches they are cut into
  const size_t nb = b1 - b0;
  const uint64_t np = prefix.size(), base = in_off_[b0], plain = in_off_[b1] - base;
  std::vector<ZhPreBlock> desc(nb);
  uint64_t scr = 0, tab = 0, max_n = 0;
  for (size_t j = 0; j < nb; ++j) {
    ZhPreBlock &d = desc[j];
    memset(&d, 0, sizeof d);
    d.in_off = in_off_[b0 + j] - base;
    d.n = n_of(b0 + j);
    d.out_off = off[j] + np;
    d.out_cap = pre_bound(M_, d.n);
    d.scr_off = scr;
    scr += d.n;
    d.tab_bits = tab_bits(d.n);
    d.tab_off = tab;
    tab += 1ull << d.tab_bits;
    max_n = std::max<uint64_t>(max_n, d.n);
  }
  const LaunchCuts C = M_.slots() ? cut_launches(desc) : LaunchCuts();
  SortArena A(C.max_slots, M_.route != Route::Bwt);

  // upload, and every buffer the route needs
  HIPCHK(plain_.alloc(plain));
  HIPCHK(desc_.alloc(nb * sizeof(ZhPreBlock)));
  HIPCHK(len_.alloc(nb * 8));
  if (plain && in_dev_ && src_off_) {     // blocks from anywhere: one copy per run of blocks that lie back to back at the caller's
    for (size_t j = 0, k; j < nb; j = k) {
      for (k = j + 1; k < nb && src_off_[b0 + k] == src_off_[b0 + k - 1] + desc[k - 1].n;) ++k;
      const uint64_t bytes = desc[k - 1].in_off + desc[k - 1].n - desc[j].in_off;
      if (bytes)
        HIPCHK(hipMemcpyAsync(plain_.as<uint8_t>() + desc[j].in_off, in_ + src_off_[b0 + j], bytes, hipMemcpyDeviceToDevice, v.stream));
    }
  } else if (plain && in_dev_) HIPCHK(hipMemcpyAsync(plain_.p, in_ + base, plain, hipMemcpyDeviceToDevice, v.stream));
  else if (plain) HIPCHK(hipMemcpy(plain_.p, in_ + base, plain, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(desc_.p, desc.data(), nb * sizeof(ZhPreBlock), hipMemcpyHostToDevice));
  if (np) {
    HIPCHK(pref_.alloc(np));
    HIPCHK(hipMemcpy(pref_.p, prefix.data(), np, hipMemcpyHostToDevice));
  }
  if (M_.e8_copy()) HIPCHK(e8_.alloc(plain));
  if (M_.slots()) {
    HIPCHK(starts_.alloc(C.starts.size() * 4));
    HIPCHK(hipMemcpy(starts_.p, C.starts.data(), C.starts.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(arena_.alloc(A.bytes()));
    A.base = arena_.as<uint8_t>();
  } else if (M_.route == Route::Greedy) {
    HIPCHK(tab_.alloc(tab * 4));
    HIPCHK(chain_.alloc(scr * 4));
    HIPCHK(prev_.alloc(scr * 4));
  }
  ZhPreLaunch L;
  memset(&L, 0, sizeof L);
  L.in = plain_.as<uint8_t>();
  L.e8 = e8_.as<uint8_t>();
  L.out = d_out;
  L.blocks = desc_.as<ZhPreBlock>();
  L.out_len = len_.as<uint64_t>();
  L.table = tab_.as<int32_t>(); L.chain = chain_.as<int32_t>(); L.prev = prev_.as<uint32_t>();
  L.n_blocks = (uint32_t)nb;
  L.level = M_.level; L.doe8 = M_.doe8; L.k = M_.k; L.m = M_.m; L.rb = M_.rb;
  L.max_match = M_.max_match; L.max_off = M_.max_off;

  // prefix and E8E9, then the route
  HIPCHK(hipMemsetAsync(len_.p, 0, nb * 8, v.stream));
  HIPCHK(hipEventRecord(v.ev0, v.stream));
  HIPCHK(zh_launch_pre_prefix(&L, pref_.as<uint8_t>(), (uint32_t)np, v.stream, &launches));
  if (M_.doe8) HIPCHK(zh_launch_pre_e8e9(&L, v.stream, &launches));
  if (M_.route == Route::Copy) {          // no pre-processing: the plaintext is the coded data
    for (size_t j = 0; j < nb; ++j)
      if (desc[j].n)
        HIPCHK(hipMemcpyAsync(d_out + desc[j].out_off, plain_.as<uint8_t>() + desc[j].in_off, desc[j].n, hipMemcpyDeviceToDevice, v.stream));
  } else if (M_.route == Route::Greedy) {
    HIPCHK(hipMemsetAsync(tab_.p, 0xFF, tab * 4, v.stream));
    HIPCHK(zh_launch_pre_lz(&L, max_n, v.stream, &launches));
  }
  for (size_t u = 0; M_.slots() && u + 1 < C.cut.size(); ++u) {
    const size_t j0 = C.cut[u], j1 = C.cut[u + 1];
    ZhBwtLaunch W{};
    W.src = M_.doe8 ? e8_.as<uint8_t>() : plain_.as<uint8_t>();
    W.out = d_out;
    W.blocks = desc_.as<ZhPreBlock>() + j0;
    W.out_len = len_.as<uint64_t>() + j0;
    W.starts = starts_.as<uint32_t>() + j0 + u;
    W.n_blocks = (uint32_t)(j1 - j0);
    W.n = C.starts[j1 + u];
    for (size_t j = j0; j < j1; ++j) W.max_n = std::max<uint32_t>(W.max_n, (uint32_t)desc[j].n);
    A.fill(W);
    const int rc = M_.route == Route::Bwt ? run_bwt(W, v, launches, err)
                 : M_.route == Route::Sa  ? run_sa(M_, W, A, v, launches, err)
                                          : run_ht(M_, W, A, v, launches, err);
    if (rc) return rc;
  }
  HIPCHK(hipEventRecord(v.ev1, v.stream));
  HIPCHK(hipStreamSynchronize(v.stream));
  HIPCHK(hipEventElapsedTime(&r.ms, v.ev0, v.ev1));

  // the lengths, and their bounds
  r.len.assign(nb, 0);
  if (M_.route != Route::Copy) HIPCHK(hipMemcpy(r.len.data(), len_.p, nb * 8, hipMemcpyDeviceToHost));
  else
    for (size_t j = 0; j < nb; ++j) r.len[j] = desc[j].n;
  for (size_t j = 0; j < nb; ++j)
    if (r.len[j] > desc[j].out_cap) {
      set_err(err, ZPAQHIP_E_HIP, (int)(b0 + j), -1, "pre-processed block exceeds its bound");
      return ZPAQHIP_E_HIP;
    }
  r.plain = plain_.as<uint8_t>();
  return ZPAQHIP_OK;
}

namespace {

// offsets must not decrease (nor advance without data), and no block may be longer than max_block
int check_offsets(const uint8_t *in, const uint64_t *in_off, size_t n_blocks, uint64_t max_block, const char *too_long, zpaqhip_err *err) {
  for (size_t i = 0; i < n_blocks; ++i) {
    if (in_off[i + 1] < in_off[i] || (!in && in_off[i + 1] > in_off[i])) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, "block offsets must not decrease");
      return ZPAQHIP_E_ARG;
    }
    if (in_off[i + 1] - in_off[i] > max_block) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, too_long);
      return ZPAQHIP_E_ARG;
    }
  }
  return ZPAQHIP_OK;
}

int check_blocks(const Method &M, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, zpaqhip_err *err) {
  return check_offsets(in, in_off, n_blocks, M.max_block,
                       M.route == Route::Bwt  ? "block longer than the BWT method allows (2^(args[0] + 20) - 4096, at most 2^31 - 1 bytes)"
                       : M.route == Route::Sa ? "block longer than the suffix-array search takes (2^(args[0] + 20), at most 2^24 bytes)"
                       : M.route == Route::Ht ? "block longer than the hash-table search takes (2^(args[0] + 20), at most 2^24 bytes)"
                                              : "block longer than the post-processor's M (2^(args[0] + 20) bytes)",
                       err);
}

// the pre-processed bytes of a method's blocks, back to back (zpaqhip_preprocess_blocks, zpaqhip_bwt_blocks)
int preprocess_impl(zpaqhip_ctx *ctx, const Method &M, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, uint8_t *out,
                    size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err) {
  int rc = check_blocks(M, in, in_off, n_blocks, err);
  if (rc) return rc;
  CtxView v = ctx_view(ctx);
  HIPCHK(hipSetDevice(v.device));
  DevPre P(M, in, in_off);
  uint64_t budget = 0;
  HIPCHK(device_budget(v.mem_share, 0, &budget));
  zpaqhip_stats st{};
  st.blocks = n_blocks;
  uint64_t pos = 0;
  for (size_t b0 = 0; b0 < n_blocks;) {
    const size_t b1 = batch_end(b0, n_blocks, 0, budget, [&](size_t i) { return P.bound(i) + P.scratch(i); }), nb = b1 - b0;
    std::vector<uint64_t> off(nb);
    uint64_t total = 0;
    for (size_t j = 0; j < nb; ++j) { off[j] = total; total += align_up(P.bound(b0 + j), 16); }
    DevMem d_out;
    HIPCHK(d_out.alloc(total));
    PreBatch r;
    if ((rc = P.run(v, b0, b1, d_out.as<uint8_t>(), off, std::vector<uint8_t>(), r, err))) return rc;
    st.kernel_ms += r.ms;
    st.init_ms += r.ms;
    for (size_t j = 0; j < nb; ++j) {
      if (out_off) out_off[b0 + j] = pos;
      if (pos + r.len[j] <= out_cap && r.len[j]) HIPCHK(hipMemcpy(out + pos, d_out.as<uint8_t>() + off[j], r.len[j], hipMemcpyDeviceToHost));
      pos += r.len[j];
      st.in_bytes += P.n_of(b0 + j);
    }
    b0 = b1;
  }
  st.launches = P.launches;
  return finish_call(v, st, pos, n_blocks, out_off, out_cap, out_len, err);
}

// What the four pre-processing entry points share.  `wrong_route`, when given, refuses a method that does not select `want`.
int preprocess_entry(zpaqhip_ctx *ctx, const int32_t *args, uint32_t flags, Route want, const char *wrong_route, const uint8_t *in,
                     const uint64_t *in_off, size_t n_blocks, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off,
                     zpaqhip_err *err) {
  if (!ctx || !out_len || (!out && out_cap) || (n_blocks && !in_off)) return refuse(err);
  *out_len = 0;
  Method M;
  if (const int rc = parse_method(args, flags, M, err)) return rc;
  if (wrong_route && M.route != want) return refuse(err, wrong_route);
  return preprocess_impl(ctx, M, in, in_off, n_blocks, out, out_cap, out_len, out_off, err);
}

// the repetition-gap histograms of compressBlock's levels 5..9 (LibZPAQ.cs:242-255), zh_analyze.hip
// (`dev`: `in` is device memory, read where it is on dev->stream)
int gap_hist_impl(zpaqhip_ctx *ctx, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, uint32_t *hist, zpaqhip_err *err,
                  const DeviceEnds *dev = nullptr) {
  // 32-bit positions and counters
  if (const int rc = check_offsets(in, in_off, n_blocks, (1ull << 31) - 1, "block longer than 2^31 - 1 bytes", err)) return rc;
  CtxView v = ctx_view(ctx);
  if (dev && dev->stream) v.stream = dev->stream;
  HIPCHK(hipSetDevice(v.device));
  uint64_t budget = 0;
  HIPCHK(device_budget(v.mem_share, 0, &budget));
  zpaqhip_stats st{};
  st.blocks = n_blocks;
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  DevMem d_in, d_off, d_hist;
  for (size_t b0 = 0; b0 < n_blocks;) {
    const size_t b1 = batch_end(b0, n_blocks, 0, budget, [&](size_t i) { return (dev ? 0 : in_off[i + 1] - in_off[i]) + 4 * ZH_GAP_NR + 8; });
    const size_t nb = b1 - b0;
    const uint64_t base = in_off[b0], plain = in_off[b1] - base;
    uint64_t max_n = 0;
    for (size_t i = b0; i < b1; ++i) max_n = std::max(max_n, in_off[i + 1] - in_off[i]);
    if (!dev) HIPCHK(d_in.alloc(plain + 16));       // the kernel loads aligned 16-byte groups: the last may reach past the data
    HIPCHK(d_off.alloc((nb + 1) * 8));
    HIPCHK(d_hist.alloc(nb * 4 * ZH_GAP_NR));
    auto t = clk::now();
    if (plain && !dev) HIPCHK(hipMemcpy(d_in.p, in + base, plain, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_off.p, in_off + b0, (nb + 1) * 8, hipMemcpyHostToDevice));
    if (!dev) st.h2d_ms += ms_since(t);   // (the device form uploads the offsets only)
    ZhGapLaunch L;
    L.in = dev ? in : d_in.as<uint8_t>();
    L.in_off = d_off.as<uint64_t>();
    L.base = dev ? 0 : base;
    L.hist = d_hist.as<uint32_t>();
    HIPCHK(hipMemsetAsync(d_hist.p, 0, nb * 4 * ZH_GAP_NR, v.stream));
    HIPCHK(hipEventRecord(v.ev0, v.stream));
    HIPCHK(zh_launch_gap_hist(&L, (uint32_t)nb, max_n, v.stream));
    HIPCHK(hipEventRecord(v.ev1, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, v.ev0, v.ev1));
    st.kernel_ms += ms;
    st.launches += max_n ? 1 : 0;
    t = clk::now();
    HIPCHK(hipMemcpy(hist + b0 * ZH_GAP_NR, d_hist.p, nb * 4 * ZH_GAP_NR, hipMemcpyDeviceToHost));
    st.d2h_ms += ms_since(t);
    st.in_bytes += plain;
    b0 = b1;
  }
  st.init_ms = st.kernel_ms;
  st.out_bytes = n_blocks * 4ull * ZH_GAP_NR;
  *v.stats = st;
  return ZPAQHIP_OK;
}

}  // namespace

extern "C" int zpaqhip_gap_hist_blocks(zpaqhip_ctx *ctx, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, uint32_t *hist,
                                       zpaqhip_err *err) {
  if (!ctx || (n_blocks && (!in_off || !hist))) return refuse(err);
  return gap_hist_impl(ctx, in, in_off, n_blocks, hist, err);
}

extern "C" int zpaqhip_gap_hist_blocks_device(zpaqhip_ctx *ctx, const void *d_in, const uint64_t *in_off, size_t n_blocks,
                                              uint32_t *hist, void *hip_stream, zpaqhip_err *err) {
  if (!ctx || (n_blocks && (!in_off || !hist))) return refuse(err);
  const DeviceEnds dev{(hipStream_t)hip_stream};
  return gap_hist_impl(ctx, (const uint8_t *)d_in, in_off, n_blocks, hist, err, &dev);
}

extern "C" int zpaqhip_preprocess_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *in, const uint64_t *in_off,
                                         size_t n_blocks, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off,
                                         zpaqhip_err *err) {
  return preprocess_entry(ctx, args, 0, Route::Copy, nullptr, in, in_off, n_blocks, out, out_cap, out_len, out_off, err);
}

extern "C" int zpaqhip_lzsa_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                                   uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err) {
  return preprocess_entry(ctx, args, kFlagSa, Route::Sa, "not a level 1 / 2 method with args[5] - args[0] >= 21", in, in_off, n_blocks,
                          out, out_cap, out_len, out_off, err);
}

extern "C" int zpaqhip_lzht_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                                   uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err) {
  return preprocess_entry(ctx, args, kFlagHt, Route::Ht, "not a level 1 / 2 method with args[5] - args[0] < 21", in, in_off, n_blocks,
                          out, out_cap, out_len, out_off, err);
}

extern "C" int zpaqhip_bwt_blocks(zpaqhip_ctx *ctx, int doe8, const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                                  uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err) {
  // no post-processor here: args[0] = 12 lifts the method's limit to that of the suffix array's 32-bit slots, 2^31 - 1 bytes
  const int32_t args[9] = {12, doe8 ? 7 : 3};
  return preprocess_entry(ctx, args, kFlagBwt, Route::Bwt, nullptr, in, in_off, n_blocks, out, out_cap, out_len, out_off, err);
}

namespace {

int compress_method_impl(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp,
                         size_t pcomp_len, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, const char *const *filenames,
                         uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *block_off, const zpaqhip_compress_opts *opts,
                         zpaqhip_err *err, const DeviceEnds *dev) {
  if (!ctx || !hdr || !out_len || (!out && out_cap) || (n_blocks && !in_off) || (pcomp_len && !pcomp) || pcomp_len > 65535)
    return refuse(err);
  *out_len = 0;
  Method M;
  int rc = parse_method(args, resolve_compress_opts(opts).flags, M, err);
  if (rc) return rc;
  if ((rc = check_blocks(M, in, in_off, n_blocks, err))) return rc;
  DevPre P(M, in, in_off, dev != nullptr);
  CompressCall a;
  a.ctx = ctx; a.hdr = hdr; a.hdr_len = hdr_len; a.pcomp = pcomp; a.pcomp_len = pcomp_len;
  a.in = in; a.in_off = in_off; a.n_blocks = n_blocks; a.filenames = filenames;
  a.out = out; a.out_cap = out_cap; a.out_len = out_len; a.block_off = block_off; a.opts = opts; a.pre = &P; a.err = err; a.dev = dev;
  return compress_impl(a);
}

}  // namespace

extern "C" int zpaqhip_compress_method_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *hdr, size_t hdr_len,
                                              const uint8_t *pcomp, size_t pcomp_len, const uint8_t *in, const uint64_t *in_off,
                                              size_t n_blocks, const char *const *filenames, uint8_t *out, size_t out_cap,
                                              size_t *out_len, uint64_t *block_off, const zpaqhip_compress_opts *opts,
                                              zpaqhip_err *err) {
  return compress_method_impl(ctx, args, hdr, hdr_len, pcomp, pcomp_len, in, in_off, n_blocks, filenames, out, out_cap, out_len,
                              block_off, opts, err, nullptr);
}

extern "C" int zpaqhip_compress_method_blocks_device(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *hdr, size_t hdr_len,
                                                     const uint8_t *pcomp, size_t pcomp_len, const void *d_in, const uint64_t *in_off,
                                                     size_t n_blocks, const char *const *filenames, void *d_out, size_t out_cap,
                                                     size_t *out_len, uint64_t *block_off, const zpaqhip_compress_opts *opts,
                                                     void *hip_stream, zpaqhip_err *err) {
  const DeviceEnds dev{(hipStream_t)hip_stream};
  return compress_method_impl(ctx, args, hdr, hdr_len, pcomp, pcomp_len, (const uint8_t *)d_in, in_off, n_blocks, filenames,
                              (uint8_t *)d_out, out_cap, out_len, block_off, opts, err, &dev);
}

// ---- a method per block ---------------------------------------------------------------------------------------------------
// The blocks of every method that is used run as one group through compress_impl's device form, which appends the group's
// stream to a sink the call owns; one launch of the packing kernel over build_gather_table's entries then puts the blocks
// into d_out in input order.
extern "C" hipError_t zh_launch_frame_pack(const ZhFrameLaunch *L, hipStream_t stream, uint32_t *launches);

namespace {

int refuse_block(zpaqhip_err *err, size_t block, const char *why) {
  set_err(err, ZPAQHIP_E_ARG, (int)block, -1, why);
  return ZPAQHIP_E_ARG;
}

// the gather: uploads the table and packs d_out from the scratch stream; its time and its launches
int gather(const CtxView &v, hipStream_t stream, const FrameTable &T, const uint8_t *scratch, uint8_t *d_out, float *ms,
           uint32_t *launches, zpaqhip_err *err) {
  if (T.entry.empty()) return ZPAQHIP_OK;
  const size_t tb = T.entry.size() * sizeof(ZhFrameEntry);
  DevMem d_tab;
  HIPCHK(d_tab.alloc(tb));
  HIPCHK(hipMemcpy(d_tab.p, T.entry.data(), tb, hipMemcpyHostToDevice));
  ZhFrameLaunch L;
  memset(&L, 0, sizeof L);
  L.table = d_tab.as<ZhFrameEntry>();
  L.blob = d_tab.as<uint8_t>();             // no entry has a head or a tail: nothing of it is read
  L.src[ZH_FRAME_SRC_FIRST] = scratch;
  L.out = d_out;
  L.n = (uint32_t)T.entry.size();
  L.pieces = T.pieces;
  HIPCHK(hipEventRecord(v.ev0, stream));
  HIPCHK(zh_launch_frame_pack(&L, stream, launches));
  HIPCHK(hipEventRecord(v.ev1, stream));
  HIPCHK(hipStreamSynchronize(stream));
  HIPCHK(hipEventElapsedTime(ms, v.ev0, v.ev1));
  return ZPAQHIP_OK;
}

}  // namespace

extern "C" int zpaqhip_compress_mixed_blocks_device(zpaqhip_ctx *ctx, const zpaqhip_method *methods, size_t n_methods,
                                                    const uint32_t *method_of, const void *d_in, const uint64_t *in_off,
                                                    size_t n_blocks, const char *const *filenames, void *d_out, size_t out_cap,
                                                    size_t *out_len, uint64_t *block_off, const zpaqhip_compress_opts *opts,
                                                    void *hip_stream, zpaqhip_err *err) {
  if (!ctx || !out_len || (!d_out && out_cap) || (n_blocks && (!in_off || !method_of)) || (n_methods && !methods)) return refuse(err);
  *out_len = 0;
  if (n_blocks && !n_methods) return refuse(err, "blocks, but no method");
  if (n_blocks > 0x7FFFFFFFull) return refuse(err, "more blocks than a call takes (2^31 - 1)");
  for (size_t g = 0; g < n_methods; ++g)
    if (methods[g].reserved) return refuse(err, "zpaqhip_method.reserved must be 0");

  // every argument check, in block order, before anything touches the device
  const uint32_t flags = resolve_compress_opts(opts).flags;
  std::vector<Method> M(n_methods);
  std::vector<std::vector<size_t>> ids(n_methods);          // the blocks of each method, in input order
  for (size_t i = 0; i < n_blocks; ++i) {
    if (in_off[i + 1] < in_off[i] || (!d_in && in_off[i + 1] > in_off[i])) return refuse_block(err, i, "block offsets must not decrease");
    const size_t g = method_of[i];
    if (g >= n_methods) return refuse_block(err, i, "method_of names no entry of the method list");
    const zpaqhip_method &m = methods[g];
    if (ids[g].empty()) {                                    // the method's first block: the method itself
      int rc = ZPAQHIP_OK;
      if (!m.hdr || (m.pcomp_len && !m.pcomp) || m.pcomp_len > 65535) rc = refuse(err);
      else rc = parse_method(m.args, flags, M[g], err);
      if (rc) {
        if (err) err->block = (int32_t)i;
        return rc;
      }
    }
    if (const int rc = check_blocks(M[g], (const uint8_t *)d_in, in_off + i, 1, err)) {
      if (err) err->block = (int32_t)i;
      return rc;
    }
    ids[g].push_back(i);
  }

  CtxView v = ctx_view(ctx);
  const hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : v.stream;
  DevSink sink;
  std::vector<GatherItem> items(n_blocks);
  zpaqhip_stats st{};
  for (size_t g = 0; g < n_methods; ++g) {
    const size_t ng = ids[g].size();
    if (!ng) continue;
    std::vector<uint64_t> len_off(ng + 1, 0), src_off(ng), at(ng + 1);
    std::vector<const char *> names(ng, nullptr);
    for (size_t j = 0; j < ng; ++j) {
      const size_t i = ids[g][j];
      src_off[j] = in_off[i];
      len_off[j + 1] = len_off[j] + (in_off[i + 1] - in_off[i]);
      if (filenames) names[j] = filenames[i];
    }
    const zpaqhip_method &m = methods[g];
    DevPre P(M[g], (const uint8_t *)d_in, len_off.data(), true, src_off.data());
    const DeviceEnds dev{stream, &sink};
    size_t end = 0;
    CompressCall a;
    a.ctx = ctx; a.hdr = m.hdr; a.hdr_len = m.hdr_len; a.pcomp = m.pcomp; a.pcomp_len = m.pcomp_len;
    a.in = (const uint8_t *)d_in; a.in_off = len_off.data(); a.n_blocks = ng; a.filenames = filenames ? names.data() : nullptr;
    a.out_len = &end; a.block_off = at.data(); a.opts = opts; a.pre = &P; a.err = err; a.dev = &dev;
    const int rc = compress_impl(a);
    if (rc) {
      if (err && err->block >= 0 && (size_t)err->block < ng) err->block = (int32_t)ids[g][err->block];
      return rc;
    }
    for (size_t j = 0; j < ng; ++j) items[ids[g][j]] = {at[j], at[j + 1] - at[j]};
    const zpaqhip_stats &s = *v.stats;
    st.kernel_ms += s.kernel_ms;
    st.init_ms += s.init_ms;
    st.launches += s.launches;
    st.in_bytes += s.in_bytes;
    st.kernel_kind = std::max(st.kernel_kind, s.kernel_kind);
    st.concurrent = std::max(st.concurrent, s.concurrent);
  }

  FrameTable T;
  std::vector<uint64_t> pos(n_blocks + 1);
  const uint64_t need = build_gather_table(items, out_cap, T, pos.data());
  if (block_off) std::copy(pos.begin(), pos.begin() + n_blocks, block_off);
  float ms = 0;
  if (const int rc = gather(v, stream, T, sink.base(), (uint8_t *)d_out, &ms, &st.launches, err)) return rc;
  st.kernel_ms += ms;
  st.blocks = n_blocks;
  st.model_bytes = sink.cap;
  st.e8_wave_segs = (uint32_t)(ms * 1000.0f + 0.5f);
  return finish_call(v, st, need, n_blocks, block_off, out_cap, out_len, err);
}
