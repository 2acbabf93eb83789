// zh_compress.h — the batch loop of zpaqhip_compress_blocks (zh_compress.cpp), shared with the method path (zh_pre.cpp),
// which fills the coded sequences on the device instead of copying them from the host.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "zh_ctx_view.h"

namespace zh {

// Device pre-processing of a batch of blocks in place of the host copy of their coded bytes.
class PreStage {
 public:
  virtual ~PreStage() = default;
  virtual uint64_t bound(size_t i) const = 0;        // pre-processed bytes of block i at most
  virtual uint64_t scratch(size_t i) const = 0;      // device bytes the stage needs for block i
  // Write the coded sequence of block b0 + j (prefix[0..np), then its pre-processed bytes) at d_in + off[j], for j < b1 - b0;
  // len[j] = pre-processed bytes.  sha_base + sha_off[j] is the block's plaintext in device memory (valid until the next
  // run).  ms = device time of the pre-processing.
  virtual int run(const CtxView &v, size_t b0, size_t b1, uint8_t *d_in, const std::vector<uint64_t> &off,
                  const std::vector<uint8_t> &prefix, std::vector<uint64_t> &len, const uint8_t **sha_base,
                  std::vector<uint64_t> &sha_off, float &ms, zpaqhip_err *err) = 0;
};

int compress_impl(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                  const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                  const uint8_t *orig, const uint64_t *orig_off, const char *const *filenames,
                  uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                  const zpaqhip_compress_opts *opts, PreStage *pre, zpaqhip_err *err);

}  // namespace zh
