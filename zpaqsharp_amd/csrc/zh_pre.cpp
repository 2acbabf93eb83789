// zh_pre.cpp — LibZPAQ.compressBlock for a method (LibZPAQ.cs:296-323): the pre-processing of levels 0, 1 and 2 and, where
// the caller asks for it, 3 (BWT) and the reference's suffix-array and hash-table parses of levels 1 / 2 (zh_pre_lzsa.hip,
// zh_pre_lzht.hip), with or without E8E9, on the GPU (zh_pre_lz.hip, zh_pre_bwt.hip).  DevPre is that stage;
// compress_impl (zh_compress.cpp) runs it in place of its host copy and then codes the bytes where the kernels left them
// (n >= 1 headers) or stores them (n = 0 headers).  zpaqhip_preprocess_blocks / zpaqhip_bwt_blocks return them as they are.
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

extern "C" hipError_t zh_launch_pre_prefix(const ZhPreLaunch *L, const uint8_t *prefix, uint32_t np, hipStream_t stream);
extern "C" hipError_t zh_launch_pre_e8e9(const ZhPreLaunch *L, hipStream_t stream);
extern "C" hipError_t zh_launch_pre_lz(const ZhPreLaunch *L, uint64_t max_n, hipStream_t stream);
extern "C" hipError_t zh_launch_pre_bwt(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *rounds);
extern "C" hipError_t zh_launch_pre_sufsort(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *c);
extern "C" hipError_t zh_launch_pre_lzsa(const ZhLzsaLaunch *L, hipStream_t stream, uint32_t *launches);
extern "C" hipError_t zh_launch_pre_lzht(const ZhLzhtLaunch *L, const ZhBwtLaunch *W, hipStream_t stream, uint32_t *launches);
extern "C" hipError_t zh_launch_gap_hist(const ZhGapLaunch *L, uint32_t n_blocks, uint64_t max_n, hipStream_t stream);

using namespace zh;

namespace {

constexpr uint32_t kFlagBwt = 4;          // zpaqhip_compress_opts.flags: accept level 3
constexpr uint32_t kFlagSa = 8;           // ... the reference's suffix-array search where the method selects it
constexpr uint32_t kFlagHt = 16;          // ... the reference's hash-table search where the method selects it

int parse_method(const int32_t *args, bool bwt, bool sa, bool ht, Method &M, zpaqhip_err *err) {
  if (!args) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  M.level = (uint32_t)args[1] & 3;
  M.doe8 = args[1] >= 4 && args[1] <= 7;
  ht = ht && (M.level == 1 || M.level == 2) && args[5] - args[0] < 21;       // LZBuffer.cs:153-158
  if (ht) {
    const char *why = nullptr;
    if (args[0] < 0 || args[0] > 11) why = "the hash-table search takes args[0] up to 11";
    else if (args[3] != 0 || args[6] != 0) why = "the hash-table search takes neither a second hash order (args[3]) nor look-ahead (args[6])";
    else if (args[2] < (M.level == 1 ? 4 : 2) || args[2] > 255)             // LZBuffer.cs:198-199, :317
      why = "the hash-table search needs a minimum match length (args[2]) of 4 (level 1) or 2 (level 2) to 255";
    else if (args[5] < 0 || args[5] > 30 || args[4] < 0 || args[4] > args[5] || args[4] > (int32_t)ZH_LZHT_MAX_BUCKET_BITS)
      why = "the hash-table search takes args[5] up to 30 and args[4] up to args[5] and 6";
    if (why) { set_err(err, ZPAQHIP_E_ARG, -1, -1, why); return ZPAQHIP_E_ARG; }
  }
  if (M.level == 3 && !bwt) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "BWT (level 3) pre-processing is not available on the GPU");
    return ZPAQHIP_E_ARG;
  }
  if (M.level == 2 && (args[2] < 1 || args[2] > 64) && !ht) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "level 2 needs a minimum match length of 1 to 64 (args[2])");
    return ZPAQHIP_E_ARG;
  }
  if (M.level && (args[0] < 0 || args[2] < 0)) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
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
  if (sa && (M.level == 1 || M.level == 2) && args[5] - args[0] >= 21) {    // LZBuffer.cs:153-158, :205
    if (M.level == 1 && args[2] < 4) {                                        // LZBuffer.cs:198-199
      set_err(err, ZPAQHIP_E_ARG, -1, -1, "level 1 needs a minimum match length of 4 or more (args[2])");
      return ZPAQHIP_E_ARG;
    }
    if (args[3] < 0 || args[4] < 0 || args[4] > 30 || args[6] < 0 || args[6] > 255 || args[2] > 255) {
      set_err(err, ZPAQHIP_E_ARG, -1, -1, "the suffix-array search takes args[2] and args[6] up to 255 and args[4] up to 30");
      return ZPAQHIP_E_ARG;
    }
    M.sa = 1;
    M.m = (uint32_t)args[2];
    M.bucket = (1u << args[4]) - 1;
    M.lookahead = (uint32_t)args[6];
    M.win_bits = (uint32_t)std::min(17 + args[0], 31);
    M.max_block = std::min<uint64_t>(M.max_block, 1ull << 24);                // offsets of 2^24 and more are not written
  }
  if (ht) {
    M.ht = 1;
    M.m = (uint32_t)args[2];
    M.bucket = (1u << args[4]) - 1;
    M.ht_bits = (uint32_t)args[5];
    M.checkbits = (uint32_t)(12 - args[0]);
    M.shift1 = (uint32_t)((args[5] - 1) / args[2] + 1);                       // C division: args[5] = 0 gives 1
    M.search = M.level == 1 || args[2] <= 64;                                 // LZBuffer.cs:288
    M.max_block = std::min<uint64_t>(M.max_block, 1ull << 24);
  }
  return ZPAQHIP_OK;
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

uint32_t tab_bits(uint64_t n) {           // at least two table entries per position
  uint32_t b = 10;
  while (b < 30 && (1ull << b) < 2 * n) ++b;
  return b;
}

// zh_pre_bwt.hip's buffers for n slots: two key and two position arrays and the ranks (20 bytes per slot), the digit
// counts of the radix tiles (1 / 4 byte per slot) and the partial results of the scans
constexpr uint64_t kBwtSlots = (1ull << 31) - 1;
uint64_t bwt_tiles(uint64_t n) { return (n + 4095) / 4096; }
uint64_t bwt_sums(uint64_t n) { return 2 * ((std::max<uint64_t>(n, 256 * bwt_tiles(n)) + 4095) / 4096) + 2; }
uint64_t bwt_bytes(uint64_t n) { return 20 * n + 1024 * bwt_tiles(n) + 4 * bwt_sums(n) + 5 * 256; }

}  // namespace

uint64_t zh::DevPre::bound(size_t i) const { return pre_bound(M_, n_of(i)); }

uint64_t zh::DevPre::scratch(size_t i) const {
  const uint64_t n = n_of(i);
  uint64_t c = n + 64;
  if (M_.level == 3) return c + (M_.doe8 ? n : 0) + bwt_bytes(n) + 8;
  if (M_.sa || M_.ht) return c + (M_.doe8 ? n : 0) + bwt_bytes(n) + 8 * n + 8;         // the sort's arrays and one decision array
  if (M_.level) c += (M_.doe8 ? n : 0) + 8 * n + (4ull << tab_bits(n));
  return c;
}

int zh::DevPre::run(const CtxView &v, size_t b0, size_t b1, uint8_t *d_out, const std::vector<uint64_t> &off,
                    const std::vector<uint8_t> &prefix, PreBatch &r, zpaqhip_err *err) {
  const size_t nb = b1 - b0;
  const uint64_t np = prefix.size(), base = in_off_[b0], plain = in_off_[b1] - base;
  std::vector<ZhPreBlock> desc(nb);
  uint64_t scr = 0, tab = 0, max_n = 0, max_scr = 0;
  const bool slots = M_.level == 3 || M_.sa || M_.ht;      // the sort's slot space (BWT, suffix-array and hash-table search)
  std::vector<size_t> cut(1, 0);        // slots: first block of each launch (at most 2^31 - 1 slots per launch)
  for (size_t j = 0; j < nb; ++j) {
    ZhPreBlock &d = desc[j];
    memset(&d, 0, sizeof d);
    d.in_off = in_off_[b0 + j] - base;
    d.n = n_of(b0 + j);
    d.out_off = off[j] + np;
    d.out_cap = pre_bound(M_, d.n);
    if (slots && scr + d.n > kBwtSlots) {      // the next launch of zh_launch_pre_bwt starts here
      cut.push_back(j);
      max_scr = std::max(max_scr, scr);
      scr = 0;
    }
    d.scr_off = scr;
    scr += d.n;
    d.tab_bits = tab_bits(d.n);
    d.tab_off = tab;
    tab += 1ull << d.tab_bits;
    max_n = std::max<uint64_t>(max_n, d.n);
  }
  HIPCHK(plain_.alloc(plain));
  HIPCHK(desc_.alloc(nb * sizeof(ZhPreBlock)));
  HIPCHK(len_.alloc(nb * 8));
  if (plain) HIPCHK(hipMemcpy(plain_.p, in_ + base, plain, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(desc_.p, desc.data(), nb * sizeof(ZhPreBlock), hipMemcpyHostToDevice));
  ZhPreLaunch L;
  memset(&L, 0, sizeof L);
  L.in = plain_.as<uint8_t>();
  L.out = d_out;
  L.blocks = desc_.as<ZhPreBlock>();
  L.out_len = len_.as<uint64_t>();
  L.n_blocks = (uint32_t)nb;
  L.level = M_.level; L.doe8 = M_.doe8; L.k = M_.k; L.m = M_.m; L.rb = M_.rb;
  L.max_match = M_.max_match; L.max_off = M_.max_off;
  if (np) {
    HIPCHK(pref_.alloc(np));
    HIPCHK(hipMemcpy(pref_.p, prefix.data(), np, hipMemcpyHostToDevice));
  }
  std::vector<uint32_t> starts;
  if (slots) {
    max_scr = std::max(max_scr, scr);
    cut.push_back(nb);
    for (size_t u = 0; u + 1 < cut.size(); ++u) {      // starts of launch u at starts[cut[u] + u ..]
      for (size_t j = cut[u]; j < cut[u + 1]; ++j) starts.push_back((uint32_t)desc[j].scr_off);
      starts.push_back((uint32_t)(desc[cut[u + 1] - 1].scr_off + desc[cut[u + 1] - 1].n));
    }
    HIPCHK(tab_.alloc(starts.size() * 4));
    HIPCHK(hipMemcpy(tab_.p, starts.data(), starts.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(chain_.alloc(16 * max_scr));             // key[2], val[2]
    HIPCHK(prev_.alloc(4 * max_scr + 1024 * bwt_tiles(max_scr) + 4 * bwt_sums(max_scr) + 4));   // rank, counts, sums, multi
    if (M_.sa || M_.ht) HIPCHK(dec_.alloc(8 * max_scr));
    if (M_.doe8) HIPCHK(e8_.alloc(plain));
    L.e8 = e8_.as<uint8_t>();
  } else if (M_.level) {
    HIPCHK(tab_.alloc(tab * 4));
    HIPCHK(chain_.alloc(scr * 4));
    HIPCHK(prev_.alloc(scr * 4));
    if (M_.doe8) HIPCHK(e8_.alloc(plain));
    L.e8 = e8_.as<uint8_t>(); L.table = tab_.as<int32_t>(); L.chain = chain_.as<int32_t>(); L.prev = prev_.as<uint32_t>();
  }
  HIPCHK(hipMemsetAsync(len_.p, 0, nb * 8, v.stream));
  HIPCHK(hipEventRecord(v.ev0, v.stream));
  HIPCHK(zh_launch_pre_prefix(&L, pref_.as<uint8_t>(), (uint32_t)np, v.stream));
  if (M_.doe8) HIPCHK(zh_launch_pre_e8e9(&L, v.stream));
  else if (!M_.level)                   // no pre-processing: the plaintext is the coded data
    for (size_t j = 0; j < nb; ++j)
      if (desc[j].n)
        HIPCHK(hipMemcpyAsync(d_out + desc[j].out_off, plain_.as<uint8_t>() + desc[j].in_off, desc[j].n, hipMemcpyDeviceToDevice, v.stream));
  if (slots) {
    for (size_t u = 0; u + 1 < cut.size(); ++u) {
      ZhBwtLaunch W;
      memset(&W, 0, sizeof W);
      W.src = M_.doe8 ? e8_.as<uint8_t>() : plain_.as<uint8_t>();
      W.out = d_out;
      W.blocks = desc_.as<ZhPreBlock>() + cut[u];
      W.out_len = len_.as<uint64_t>() + cut[u];
      W.starts = tab_.as<uint32_t>() + cut[u] + u;
      W.n_blocks = (uint32_t)(cut[u + 1] - cut[u]);
      W.n = starts[cut[u + 1] + u];
      for (size_t j = cut[u]; j < cut[u + 1]; ++j) W.max_n = std::max<uint32_t>(W.max_n, (uint32_t)desc[j].n);
      for (int q = 0; q < 2; ++q) {
        W.key[q] = chain_.as<uint32_t>() + (2 * q) * max_scr;
        W.val[q] = chain_.as<uint32_t>() + (2 * q + 1) * max_scr;
      }
      W.rank = prev_.as<uint32_t>();
      W.counts = W.rank + max_scr;
      W.sums = W.counts + 256 * bwt_tiles(max_scr);
      W.multi = W.sums + bwt_sums(max_scr);
      uint32_t rounds = 0;                // the launcher reports its doubling rounds; nothing here uses them
      if (M_.ht) {
        ZhLzhtLaunch H;
        memset(&H, 0, sizeof H);
        H.src = W.src; H.out = d_out; H.blocks = W.blocks; H.out_len = W.out_len; H.starts = W.starts;
        H.dec[0] = dec_.as<uint64_t>();
        H.n_blocks = W.n_blocks; H.n = W.n;
        H.level = M_.level; H.min_match = M_.m; H.bucket = M_.bucket; H.ht_bits = M_.ht_bits; H.checkbits = M_.checkbits;
        H.shift1 = M_.shift1; H.search = M_.search; H.rb = M_.rb;
        HIPCHK(zh_launch_pre_lzht(&H, &W, v.stream, &launches));
        continue;
      }
      if (!M_.sa) {
        HIPCHK(zh_launch_pre_bwt(&W, v.stream, &launches, &rounds));
        continue;
      }
      uint32_t c = 0;
      HIPCHK(zh_launch_pre_sufsort(&W, v.stream, &launches, &c));
      ZhLzsaLaunch S;
      memset(&S, 0, sizeof S);
      S.src = W.src; S.out = d_out; S.blocks = W.blocks; S.out_len = W.out_len; S.starts = W.starts;
      S.sa = W.val[c];
      S.rank = W.rank;
      S.lcp = W.key[c];                   // the sort is done with its keys and with the other pair of arrays
      S.dec[0] = dec_.as<uint64_t>();
      S.dec[1] = reinterpret_cast<uint64_t *>(W.key[c ^ 1]);      // key and val of a pair are adjacent: n 64-bit words
      S.n_blocks = W.n_blocks; S.n = W.n;
      S.level = M_.level; S.min_match = M_.m; S.bucket = M_.bucket; S.lookahead = M_.lookahead; S.win_bits = M_.win_bits; S.rb = M_.rb;
      HIPCHK(zh_launch_pre_lzsa(&S, v.stream, &launches));
    }
  } else if (M_.level) {
    HIPCHK(hipMemsetAsync(tab_.p, 0xFF, tab * 4, v.stream));
    HIPCHK(zh_launch_pre_lz(&L, max_n, v.stream));
  }
  HIPCHK(hipEventRecord(v.ev1, v.stream));
  HIPCHK(hipStreamSynchronize(v.stream));
  HIPCHK(hipEventElapsedTime(&r.ms, v.ev0, v.ev1));
  launches += (np ? 1 : 0) + (M_.doe8 ? 1 : 0) + (slots ? 0 : M_.level ? 3 : 0);
  r.len.assign(nb, 0);
  if (M_.level || M_.doe8) HIPCHK(hipMemcpy(r.len.data(), len_.p, nb * 8, hipMemcpyDeviceToHost));
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

int check_blocks(const Method &M, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, zpaqhip_err *err) {
  for (size_t i = 0; i < n_blocks; ++i) {
    if (in_off[i + 1] < in_off[i] || (!in && in_off[i + 1] > in_off[i])) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, "block offsets must not decrease");
      return ZPAQHIP_E_ARG;
    }
    if (in_off[i + 1] - in_off[i] > M.max_block) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1,
              M.level == 3 ? "block longer than the BWT method allows (2^(args[0] + 20) - 4096, at most 2^31 - 1 bytes)"
              : M.sa       ? "block longer than the suffix-array search takes (2^(args[0] + 20), at most 2^24 bytes)"
              : M.ht       ? "block longer than the hash-table search takes (2^(args[0] + 20), at most 2^24 bytes)"
                           : "block longer than the post-processor's M (2^(args[0] + 20) bytes)");
      return ZPAQHIP_E_ARG;
    }
  }
  return ZPAQHIP_OK;
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

// the repetition-gap histograms of compressBlock's levels 5..9 (LibZPAQ.cs:242-255), zh_analyze.hip
int gap_hist_impl(zpaqhip_ctx *ctx, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, uint32_t *hist, zpaqhip_err *err) {
  for (size_t i = 0; i < n_blocks; ++i) {
    if (in_off[i + 1] < in_off[i] || (!in && in_off[i + 1] > in_off[i])) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, "block offsets must not decrease");
      return ZPAQHIP_E_ARG;
    }
    if (in_off[i + 1] - in_off[i] > (1ull << 31) - 1) {      // 32-bit positions and counters
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, "block longer than 2^31 - 1 bytes");
      return ZPAQHIP_E_ARG;
    }
  }
  CtxView v = ctx_view(ctx);
  HIPCHK(hipSetDevice(v.device));
  uint64_t budget = 0;
  HIPCHK(device_budget(v.mem_share, 0, &budget));
  zpaqhip_stats st{};
  st.blocks = n_blocks;
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  DevMem d_in, d_off, d_hist;
  for (size_t b0 = 0; b0 < n_blocks;) {
    const size_t b1 = batch_end(b0, n_blocks, 0, budget, [&](size_t i) { return in_off[i + 1] - in_off[i] + 4 * ZH_GAP_NR + 8; });
    const size_t nb = b1 - b0;
    const uint64_t base = in_off[b0], plain = in_off[b1] - base;
    uint64_t max_n = 0;
    for (size_t i = b0; i < b1; ++i) max_n = std::max(max_n, in_off[i + 1] - in_off[i]);
    HIPCHK(d_in.alloc(plain + 16));       // the kernel loads aligned 16-byte groups: the last may reach past the data
    HIPCHK(d_off.alloc((nb + 1) * 8));
    HIPCHK(d_hist.alloc(nb * 4 * ZH_GAP_NR));
    auto t = clk::now();
    if (plain) HIPCHK(hipMemcpy(d_in.p, in + base, plain, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_off.p, in_off + b0, (nb + 1) * 8, hipMemcpyHostToDevice));
    st.h2d_ms += ms_since(t);
    ZhGapLaunch L;
    L.in = d_in.as<uint8_t>();
    L.in_off = d_off.as<uint64_t>();
    L.base = base;
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
  if (!ctx || (n_blocks && (!in_off || !hist))) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  return gap_hist_impl(ctx, in, in_off, n_blocks, hist, err);
}

extern "C" int zpaqhip_preprocess_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *in, const uint64_t *in_off,
                                         size_t n_blocks, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off,
                                         zpaqhip_err *err) {
  if (!ctx || !out_len || (!out && out_cap) || (n_blocks && !in_off)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *out_len = 0;
  Method M;
  const int rc = parse_method(args, false, false, false, M, err);
  if (rc) return rc;
  return preprocess_impl(ctx, M, in, in_off, n_blocks, out, out_cap, out_len, out_off, err);
}

extern "C" int zpaqhip_lzsa_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                                   uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err) {
  if (!ctx || !out_len || (!out && out_cap) || (n_blocks && !in_off)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *out_len = 0;
  Method M;
  const int rc = parse_method(args, false, true, false, M, err);
  if (rc) return rc;
  if (!M.sa) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "not a level 1 / 2 method with args[5] - args[0] >= 21");
    return ZPAQHIP_E_ARG;
  }
  return preprocess_impl(ctx, M, in, in_off, n_blocks, out, out_cap, out_len, out_off, err);
}

extern "C" int zpaqhip_lzht_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                                   uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err) {
  if (!ctx || !out_len || (!out && out_cap) || (n_blocks && !in_off)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *out_len = 0;
  Method M;
  const int rc = parse_method(args, false, false, true, M, err);
  if (rc) return rc;
  if (!M.ht) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "not a level 1 / 2 method with args[5] - args[0] < 21");
    return ZPAQHIP_E_ARG;
  }
  return preprocess_impl(ctx, M, in, in_off, n_blocks, out, out_cap, out_len, out_off, err);
}

extern "C" int zpaqhip_bwt_blocks(zpaqhip_ctx *ctx, int doe8, const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                                  uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off, zpaqhip_err *err) {
  if (!ctx || !out_len || (!out && out_cap) || (n_blocks && !in_off)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *out_len = 0;
  Method M;
  M.level = 3;
  M.doe8 = doe8 != 0;
  M.max_block = (1ull << 31) - 1;         // no post-processor here: the suffix array's 32-bit slots are the only limit
  return preprocess_impl(ctx, M, in, in_off, n_blocks, out, out_cap, out_len, out_off, err);
}

extern "C" int zpaqhip_compress_method_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *hdr, size_t hdr_len,
                                              const uint8_t *pcomp, size_t pcomp_len, const uint8_t *in, const uint64_t *in_off,
                                              size_t n_blocks, const char *const *filenames, uint8_t *out, size_t out_cap,
                                              size_t *out_len, uint64_t *block_off, const zpaqhip_compress_opts *opts,
                                              zpaqhip_err *err) {
  if (!ctx || !hdr || !out_len || (!out && out_cap) || (n_blocks && !in_off) || (pcomp_len && !pcomp) || pcomp_len > 65535) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *out_len = 0;
  Method M;
  const uint32_t flags = resolve_compress_opts(opts).flags;
  int rc = parse_method(args, (flags & kFlagBwt) != 0, (flags & kFlagSa) != 0, (flags & kFlagHt) != 0, M, err);
  if (rc) return rc;
  if ((rc = check_blocks(M, in, in_off, n_blocks, err))) return rc;
  DevPre P(M, in, in_off);
  return compress_impl(ctx, hdr, hdr_len, pcomp, pcomp_len, in, in_off, n_blocks, nullptr, nullptr, filenames, out, out_cap, out_len,
                       block_off, opts, &P, err);
}
