// zh_pre.cpp — LibZPAQ.compressBlock for a method (LibZPAQ.cs:296-323): the pre-processing of levels 0, 1 and 2 and, where
// the caller asks for it, 3 (BWT), with or without E8E9, on the GPU (zh_pre_lz.hip, zh_pre_bwt.hip), then either the existing encoders (n >= 1 headers, through compress_impl,
// which reads the pre-processed bytes where the kernels left them) or the unmodelled store layout (n = 0 headers,
// Encoder.cs:39-73: the decoded stream in 4-byte big-endian length-prefixed chunks of 65 536 bytes).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zh_compress.h"
#include "zh_ctx_view.h"
#include "zh_pre.h"

extern "C" hipError_t zh_launch_pre_prefix(const ZhPreLaunch *L, const uint8_t *prefix, uint32_t np, hipStream_t stream);
extern "C" hipError_t zh_launch_pre_e8e9(const ZhPreLaunch *L, hipStream_t stream);
extern "C" hipError_t zh_launch_pre_lz(const ZhPreLaunch *L, uint64_t max_n, hipStream_t stream);
extern "C" hipError_t zh_launch_pre_bwt(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *rounds);
extern "C" hipError_t zh_launch_sha1(const uint8_t *data, const uint64_t *seg, uint32_t n_seg, uint32_t *digest, hipStream_t stream);

using namespace zh;

namespace {

#define HIPCHK(expr)                                                          \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                   \
      char m_[112];                                                           \
      snprintf(m_, sizeof m_, "HIP: %s (%s)", hipGetErrorString(e_), #expr);  \
      set_err(err, ZPAQHIP_E_HIP, -1, -1, m_);                                \
      return ZPAQHIP_E_HIP;                                                   \
    }                                                                         \
  } while (0)

struct DevMem {                           // device buffer owned by one call
  void *p = nullptr;
  ~DevMem() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) {
    if (p) { (void)hipFree(p); p = nullptr; }
    return hipMalloc(&p, std::max<size_t>(n, 256));
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

constexpr uint8_t kTag[13] = {0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3};   // Compressor.cs:27-43

uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// the method's numbers (tools/methods.preprocess / lz77_level1 / lz77_level2)
struct Method {
  uint32_t level = 0, doe8 = 0, k = 0, m = 0, rb = 0, max_match = 0, max_off = 0;
  uint64_t max_block = ~0ull;             // levels 1 / 2: 2^(args[0] + 20), the PCOMP's M; level 3: 4096 less (LibZPAQ.cs:289)
};

constexpr uint32_t kFlagBwt = 4;          // zpaqhip_compress_opts.flags: accept level 3

int parse_method(const int32_t *args, bool bwt, Method &M, zpaqhip_err *err) {
  if (!args) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  M.level = (uint32_t)args[1] & 3;
  M.doe8 = args[1] >= 4 && args[1] <= 7;
  if (M.level == 3 && !bwt) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "BWT (level 3) pre-processing is not available on the GPU");
    return ZPAQHIP_E_ARG;
  }
  if (M.level == 2 && (args[2] < 1 || args[2] > 64)) {
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
  return ZPAQHIP_OK;
}

// pre-processed bytes at most: a literal run of L costs 8L + 2 lg(L) + 1 <= 11L bits and a match of l >= 4 at most 8l bits
// (level 1); a literal costs at most 2 bytes and a match piece at most 4 bytes for 3 or more bytes (level 2)
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

class DevPre : public PreStage {
 public:
  DevPre(const Method &M, const uint8_t *in, const uint64_t *in_off) : M_(M), in_(in), in_off_(in_off) {}
  uint64_t n_of(size_t i) const { return in_off_[i + 1] - in_off_[i]; }
  uint64_t bound(size_t i) const override { return pre_bound(M_, n_of(i)); }
  uint64_t scratch(size_t i) const override {
    const uint64_t n = n_of(i);
    uint64_t c = n + 64;
    if (M_.level == 3) return c + (M_.doe8 ? n : 0) + bwt_bytes(n) + 8;
    if (M_.level) c += (M_.doe8 ? n : 0) + 8 * n + (4ull << tab_bits(n));
    return c;
  }
  int run(const CtxView &v, size_t b0, size_t b1, uint8_t *d_out, const std::vector<uint64_t> &off,
          const std::vector<uint8_t> &prefix, std::vector<uint64_t> &len, const uint8_t **sha_base,
          std::vector<uint64_t> &sha_off, float &ms, zpaqhip_err *err) override {
    const size_t nb = b1 - b0;
    const uint64_t np = prefix.size(), base = in_off_[b0], plain = in_off_[b1] - base;
    std::vector<ZhPreBlock> desc(nb);
    uint64_t scr = 0, tab = 0, max_n = 0, max_scr = 0;
    std::vector<size_t> cut(1, 0);        // level 3: first block of each launch (at most 2^31 - 1 slots per launch)
    sha_off.resize(nb);
    for (size_t j = 0; j < nb; ++j) {
      ZhPreBlock &d = desc[j];
      memset(&d, 0, sizeof d);
      d.in_off = in_off_[b0 + j] - base;
      d.n = n_of(b0 + j);
      d.out_off = off[j] + np;
      d.out_cap = pre_bound(M_, d.n);
      if (M_.level == 3 && scr + d.n > kBwtSlots) {      // the next launch of zh_launch_pre_bwt starts here
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
      sha_off[j] = d.in_off;
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
    if (M_.level == 3) {
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
    if (M_.level == 3) {
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
        HIPCHK(zh_launch_pre_bwt(&W, v.stream, &launches, &bwt_rounds));
      }
    } else if (M_.level) {
      HIPCHK(hipMemsetAsync(tab_.p, 0xFF, tab * 4, v.stream));
      HIPCHK(zh_launch_pre_lz(&L, max_n, v.stream));
    }
    HIPCHK(hipEventRecord(v.ev1, v.stream));
    HIPCHK(hipStreamSynchronize(v.stream));
    HIPCHK(hipEventElapsedTime(&ms, v.ev0, v.ev1));
    launches += (np ? 1 : 0) + (M_.doe8 ? 1 : 0) + (M_.level == 3 ? 0 : M_.level ? 3 : 0);
    len.assign(nb, 0);
    if (M_.level || M_.doe8) HIPCHK(hipMemcpy(len.data(), len_.p, nb * 8, hipMemcpyDeviceToHost));
    else
      for (size_t j = 0; j < nb; ++j) len[j] = desc[j].n;
    for (size_t j = 0; j < nb; ++j)
      if (len[j] > desc[j].out_cap) {
        set_err(err, ZPAQHIP_E_HIP, (int)(b0 + j), -1, "pre-processed block exceeds its bound");
        return ZPAQHIP_E_HIP;
      }
    *sha_base = plain_.as<uint8_t>();
    return ZPAQHIP_OK;
  }
  uint32_t launches = 0;
  uint32_t bwt_rounds = 0;                // level 3: doubling rounds after the first sort, over all launches

 private:
  Method M_;
  const uint8_t *in_;
  const uint64_t *in_off_;
  DevMem plain_, e8_, tab_, chain_, prev_, len_, desc_, pref_;
};

uint64_t budget_of(const CtxView &v) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 1ull << 30;
  return (free_b > (2ull << 30) ? free_b - (1ull << 30) : free_b / 2) / std::max(1u, v.mem_share);
}

// batches [b0, b1) of blocks whose bound and scratch fit half the budget (at least one block, at most 4096)
size_t batch_end(const DevPre &P, size_t b0, size_t n_blocks, uint64_t batch_blocks, uint64_t budget) {
  if (batch_blocks) return std::min<size_t>(n_blocks, b0 + batch_blocks);
  size_t b1 = b0 + 1;
  uint64_t cost = P.bound(b0) + P.scratch(b0);
  while (b1 < n_blocks && b1 - b0 < 4096 && cost + P.bound(b1) + P.scratch(b1) <= budget / 2) cost += P.bound(b1) + P.scratch(b1++);
  return b1;
}

int check_blocks(const Method &M, const uint8_t *in, const uint64_t *in_off, size_t n_blocks, zpaqhip_err *err) {
  for (size_t i = 0; i < n_blocks; ++i) {
    if (in_off[i + 1] < in_off[i] || (!in && in_off[i + 1] > in_off[i])) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, "block offsets must not decrease");
      return ZPAQHIP_E_ARG;
    }
    if (in_off[i + 1] - in_off[i] > M.max_block) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1,
              M.level == 3 ? "block longer than the BWT method allows (2^(args[0] + 20) - 4096, at most 2^31 - 1 bytes)"
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
  const uint64_t budget = budget_of(v);
  zpaqhip_stats st{};
  st.blocks = n_blocks;
  uint64_t pos = 0;
  for (size_t b0 = 0; b0 < n_blocks;) {
    const size_t b1 = batch_end(P, b0, n_blocks, 0, budget), nb = b1 - b0;
    std::vector<uint64_t> off(nb), len, sha_off;
    uint64_t total = 0;
    for (size_t j = 0; j < nb; ++j) { off[j] = total; total += align_up(P.bound(b0 + j), 16); }
    DevMem d_out;
    HIPCHK(d_out.alloc(total));
    const uint8_t *sha_base = nullptr;
    float ms = 0;
    if ((rc = P.run(v, b0, b1, d_out.as<uint8_t>(), off, std::vector<uint8_t>(), len, &sha_base, sha_off, ms, err))) return rc;
    st.kernel_ms += ms;
    st.init_ms += ms;
    for (size_t j = 0; j < nb; ++j) {
      if (out_off) out_off[b0 + j] = pos;
      if (pos + len[j] <= out_cap && len[j]) HIPCHK(hipMemcpy(out + pos, d_out.as<uint8_t>() + off[j], len[j], hipMemcpyDeviceToHost));
      pos += len[j];
      st.in_bytes += P.n_of(b0 + j);
    }
    b0 = b1;
  }
  if (out_off) out_off[n_blocks] = pos;
  st.out_bytes = pos;
  st.launches = P.launches;
  *v.stats = st;
  *out_len = pos;
  if (pos > out_cap) {
    set_err(err, ZPAQHIP_E_OUTPUT_FULL, -1, -1);
    return ZPAQHIP_E_OUTPUT_FULL;
  }
  return ZPAQHIP_OK;
}

}  // namespace

extern "C" int zpaqhip_preprocess_blocks(zpaqhip_ctx *ctx, const int32_t *args, const uint8_t *in, const uint64_t *in_off,
                                         size_t n_blocks, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *out_off,
                                         zpaqhip_err *err) {
  if (!ctx || !out_len || (!out && out_cap) || (n_blocks && !in_off)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *out_len = 0;
  Method M;
  const int rc = parse_method(args, false, M, err);
  if (rc) return rc;
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
  zpaqhip_compress_opts o;
  memset(&o, 0, sizeof o);
  if (opts) memcpy(&o, opts, std::min<size_t>(sizeof o, opts->struct_size ? opts->struct_size : sizeof o));
  else o.flags = 3;
  Method M;
  int rc = parse_method(args, (o.flags & kFlagBwt) != 0, M, err);
  if (rc) return rc;
  if ((rc = check_blocks(M, in, in_off, n_blocks, err))) return rc;
  ZhModel model;
  std::vector<uint8_t> code;
  if ((rc = build_model(hdr, hdr_len, model, code, err))) return rc;
  DevPre P(M, in, in_off);
  if (model.n) return compress_impl(ctx, hdr, hdr_len, pcomp, pcomp_len, in, in_off, n_blocks, nullptr, nullptr, filenames, out, out_cap,
                                    out_len, block_off, opts, &P, err);

  // n = 0: the store layout of Encoder.compress with no model; the block is level 2 (Compressor.cs:92-96)
  const bool want_sha = (o.flags & 1) != 0, want_tag = (o.flags & 2) != 0;
  std::vector<uint8_t> sel;                       // the post-processor's header (Compressor.postProcess)
  if (pcomp_len) {
    sel.push_back(1);
    sel.push_back((uint8_t)(pcomp_len & 255));
    sel.push_back((uint8_t)(pcomp_len >> 8));
    sel.insert(sel.end(), pcomp, pcomp + pcomp_len);
  } else sel.push_back(0);
  CtxView v = ctx_view(ctx);
  HIPCHK(hipSetDevice(v.device));
  const uint64_t budget = budget_of(v);
  zpaqhip_stats st{};
  st.blocks = n_blocks;
  uint64_t pos = 0;
  for (size_t b0 = 0; b0 < n_blocks;) {
    const size_t b1 = batch_end(P, b0, n_blocks, o.batch_blocks, budget), nb = b1 - b0;
    std::vector<uint64_t> off(nb), len, sha_off;
    uint64_t total = 0;
    for (size_t j = 0; j < nb; ++j) { off[j] = total; total += align_up(P.bound(b0 + j), 16); }
    DevMem d_out, d_seg, d_dig;
    HIPCHK(d_out.alloc(total));
    const uint8_t *sha_base = nullptr;
    float ms = 0;
    if ((rc = P.run(v, b0, b1, d_out.as<uint8_t>(), off, std::vector<uint8_t>(), len, &sha_base, sha_off, ms, err))) return rc;
    st.kernel_ms += ms;
    st.init_ms += ms;
    std::vector<uint32_t> digest(5 * nb);
    if (want_sha) {                               // SHA-1 of the plaintext (Compressor.endSegment)
      std::vector<uint64_t> seg(2 * nb);
      for (size_t j = 0; j < nb; ++j) { seg[2 * j] = sha_off[j]; seg[2 * j + 1] = P.n_of(b0 + j); }
      HIPCHK(d_seg.alloc(seg.size() * 8));
      HIPCHK(d_dig.alloc(nb * 20));
      HIPCHK(hipMemcpy(d_seg.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice));
      HIPCHK(zh_launch_sha1(sha_base, d_seg.as<uint64_t>(), (uint32_t)nb, d_dig.as<uint32_t>(), v.stream));
      HIPCHK(hipStreamSynchronize(v.stream));
      HIPCHK(hipMemcpy(digest.data(), d_dig.p, nb * 20, hipMemcpyDeviceToHost));
    }
    std::vector<uint8_t> h_out;
    if (pos < out_cap) {
      h_out.resize(total);
      HIPCHK(hipMemcpy(h_out.data(), d_out.p, total, hipMemcpyDeviceToHost));
    }
    for (size_t j = 0; j < nb; ++j) {
      const size_t i = b0 + j;
      std::string head;
      if (want_tag) head.append((const char *)kTag, 13);
      head.append("zPQ\x02\x01", 5);
      head.append((const char *)hdr, hdr_len);
      head.push_back(1);
      if (filenames && filenames[i]) head.append(filenames[i]);
      head.push_back(0);
      head.append(std::to_string(P.n_of(i)));
      head.push_back(0);
      head.push_back(0);
      std::string tail(4, '\0');
      if (want_sha) {
        tail.push_back((char)253);
        for (int w = 0; w < 5; ++w)
          for (int s = 24; s >= 0; s -= 8) tail.push_back((char)(digest[5 * j + w] >> s));
      } else tail.push_back((char)254);
      tail.push_back((char)255);
      const uint64_t dec = sel.size() + len[j], body = dec + 4 * ((dec + 65535) / 65536), need = head.size() + body + tail.size();
      if (block_off) block_off[i] = pos;
      if (pos + need <= out_cap) {
        uint8_t *w = out + pos;
        memcpy(w, head.data(), head.size());
        w += head.size();
        const uint8_t *pre = h_out.data() + off[j];
        for (uint64_t c = 0; c < dec; c += 65536) {     // chunks of the decoded stream: selector [+ PCOMP], then the bytes
          const uint64_t cl = std::min<uint64_t>(65536, dec - c);
          *w++ = (uint8_t)(cl >> 24); *w++ = (uint8_t)(cl >> 16); *w++ = (uint8_t)(cl >> 8); *w++ = (uint8_t)cl;
          for (uint64_t t = c; t < c + cl;) {
            if (t < sel.size()) { const uint64_t e = std::min<uint64_t>(sel.size(), c + cl); memcpy(w, sel.data() + t, e - t); w += e - t; t = e; }
            else { memcpy(w, pre + (t - sel.size()), c + cl - t); w += c + cl - t; t = c + cl; }
          }
        }
        memcpy(w, tail.data(), tail.size());
      }
      pos += need;
      st.in_bytes += P.n_of(i);
    }
    b0 = b1;
  }
  if (block_off) block_off[n_blocks] = pos;
  st.out_bytes = pos;
  st.launches = P.launches;
  st.kernel_kind = 0;
  *v.stats = st;
  *out_len = pos;
  if (pos > out_cap) {
    set_err(err, ZPAQHIP_E_OUTPUT_FULL, -1, -1);
    return ZPAQHIP_E_OUTPUT_FULL;
  }
  return ZPAQHIP_OK;
}
