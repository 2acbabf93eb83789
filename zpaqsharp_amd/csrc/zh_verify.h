// zh_verify.h — the verify pass (Compressor.setVerify, Compressor.cs:118-121; endSegmentChecksum, :251-281): the blocks'
// pre-processed bytes run through the block's own post-processor on the device, and what comes out is sized, hashed and
// compared with the plaintext.  Shared by zpaqhip_verify_blocks[_device] (zh_verify.cpp) and the batch loop of the
// compressing entry points (zh_compress.cpp, bit 5 of zpaqhip_compress_opts.flags).
#pragma once
#include <stdint.h>

// One block of zh_verify_compare (zh_verify_k.hip): `a` is what the post-processor wrote, `b` the plaintext
struct ZhVerifyCmp {
  uint64_t a_off, a_len;
  uint64_t b_off, b_len;
};

#include <vector>

#include "zh_compress.h"

namespace zh {

constexpr uint32_t kFlagVerify = 32;      // zpaqhip_compress_opts.flags, bit 5

// What the post-processor reads, block by block, in device memory: the selector (0, or 1, len lo, len hi, PCOMP) and
// behind it the pre-processed bytes, as PostProcessor.write gets them from the decoder.  `d_plain`, when given, is what
// they must turn back into.
struct VerifyIn {
  const uint8_t *d_in = nullptr;
  std::vector<uint64_t> off, len;
  const uint8_t *d_plain = nullptr;
  std::vector<uint64_t> poff, plen;
};

// sel || in[src_off[j], + src_len[j]) for every block j at dst + off[j] (zh_frame.hip), off[j] 16-byte aligned; `dst` is
// allocated here
int verify_stage(const CtxView &v, const std::vector<uint8_t> &sel, const uint8_t *d_src, const std::vector<uint64_t> &src_off,
                 const std::vector<uint64_t> &src_len, DevMem &dst, VerifyIn &in, uint32_t *launches, zpaqhip_err *err);

// The pass over the blocks of `in` with a post-processor of 2^ph words of H and 2^pm bytes of M: one record per block.
// `ms` and `launches` are added to; `out_bytes` gets the bytes post-processed.  Returns ZPAQHIP_OK when it ran, whatever the
// records say.
int verify_pass(const CtxView &v, uint8_t ph, uint8_t pm, const VerifyIn &in, uint64_t mem_budget,
                std::vector<zpaqhip_verify_result> &rec, double *ms, uint32_t *launches, uint64_t *out_bytes, zpaqhip_err *err);

}  // namespace zh
