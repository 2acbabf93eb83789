// zh_compress.cpp — zpaqhip_compress_blocks: Compressor.startBlock / startSegment / postProcess / compress / endSegment /
// endBlock (Compressor.cs:27-299) for a batch of blocks, one segment each (LibZPAQ.cs:296-323 framing), coded on the GPU.
//
// The host validates the header with the decoder's framing code, picks an encoder per block (route_encode), lays the
// coded sequences of a batch out in device memory, launches the encoders, re-encodes a block whose slot was too small on
// the generic encoder with a worst-case slot, and writes tag, block, segment and end framing around each slot's bytes.
// Every coded byte comes out of a HIP kernel (zh_enc_cm.hip, zh_enc_generic.hip); there is no CPU encoder here.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zh_compress.h"
#include "zh_ctx_view.h"
#include "zh_enc.h"

extern "C" hipError_t zh_launch_enc_generic(const ZhEncLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_enc_cm_model(const ZhEncLaunch *L, uint32_t n_blocks, hipStream_t stream);
extern "C" hipError_t zh_launch_enc_cm_code(const ZhEncLaunch *L, uint32_t n_blocks, hipStream_t stream);
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

struct Event {                            // one event owned by one call
  hipEvent_t e = nullptr;
  ~Event() { if (e) (void)hipEventDestroy(e); }
};

// ---- which kernel encodes a block (the encode-side twin of zh_api.cpp's route_block): the window-parallel CM encoder for
// ZH_FAM_CM1 models with opts.kernel 0, the generic encoder for everything else (and for a block too long for zh_enc_cm's
// 28-bit positions)
enum class EncKernel { Generic, Cm };
EncKernel route_encode(const ZhModel &m, const zpaqhip_compress_opts &o, uint64_t coded) {
  if ((m.kind & 255u) == ZH_FAM_CM1 && o.kernel == 0 && coded < ZH_ENC_CM_MAX_N) return EncKernel::Cm;
  return EncKernel::Generic;
}

constexpr uint8_t kTag[13] = {0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3};   // Compressor.cs:27-43

uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
uint64_t auto_slot(uint64_t coded) { return coded + coded / 8 + 4096; }
uint64_t worst_slot(uint64_t coded) { return 16 * coded + 4096; }    // 2 bytes per coded bit, plus the end of segment

}  // namespace

extern "C" int zpaqhip_compress_blocks(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                                       const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                                       const uint8_t *orig, const uint64_t *orig_off, const char *const *filenames,
                                       uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                                       const zpaqhip_compress_opts *opts, zpaqhip_err *err) {
  return compress_impl(ctx, hdr, hdr_len, pcomp, pcomp_len, in, in_off, n_blocks, orig, orig_off, filenames, out, out_cap, out_len,
                       block_off, opts, nullptr, err);
}

// `pre` (the method path): block i's coded bytes are pre-processed on the device from its plaintext in[in_off[i], in_off[i+1]),
// which the size comment and SHA-1 describe; orig is then NULL.
int zh::compress_impl(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                      const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                      const uint8_t *orig, const uint64_t *orig_off, const char *const *filenames,
                      uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                      const zpaqhip_compress_opts *opts, PreStage *pre, zpaqhip_err *err) {
  if (!ctx || !hdr || !out_len || (!out && out_cap) || (n_blocks && !in_off) || (orig && !orig_off) || (pcomp_len && !pcomp) ||
      pcomp_len > 65535) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *out_len = 0;
  zpaqhip_compress_opts o;
  memset(&o, 0, sizeof o);
  if (opts) memcpy(&o, opts, std::min<size_t>(sizeof o, opts->struct_size ? opts->struct_size : sizeof o));
  else o.flags = 3;
  for (size_t i = 0; i < n_blocks; ++i)
    if (in_off[i + 1] < in_off[i] || (orig && orig_off[i + 1] < orig_off[i]) || (!in && in_off[i + 1] > in_off[i])) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, "block offsets must not decrease");
      return ZPAQHIP_E_ARG;
    }
  ZhModel M;
  std::vector<uint8_t> code;
  int rc = build_model(hdr, hdr_len, M, code, err);
  if (rc) return rc;
  if (M.n == 0) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "compress_blocks codes modelled blocks only (n >= 1)");
    return ZPAQHIP_E_ARG;
  }
  // the coded sequence starts with the post-processor's header (Compressor.postProcess, Compressor.cs:156-190)
  std::vector<uint8_t> prefix;
  if (pcomp_len) {
    prefix.push_back(1);
    prefix.push_back((uint8_t)(pcomp_len & 255));
    prefix.push_back((uint8_t)(pcomp_len >> 8));
    prefix.insert(prefix.end(), pcomp, pcomp + pcomp_len);
  } else prefix.push_back(0);
  const uint64_t np = prefix.size();
  const bool want_sha = (o.flags & 1) != 0, want_tag = (o.flags & 2) != 0;

  CtxView v = ctx_view(ctx);
  HIPCHK(hipSetDevice(v.device));
  zpaqhip_stats st{};
  st.blocks = n_blocks;
  Event ev_model;                                 // end of the model pass: init_ms times zh_enc_cm_model on its own
  HIPCHK(hipEventCreate(&ev_model.e));

  // model for the generic encoder; what the CM encoder needs of it
  DevMem d_model, d_code;
  HIPCHK(d_model.alloc(sizeof(ZhModel)));
  HIPCHK(d_code.alloc(code.size()));
  HIPCHK(hipMemcpy(d_model.p, &M, sizeof(ZhModel), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_code.p, code.data(), code.size(), hipMemcpyHostToDevice));
  uint32_t wmask = 0;
  if ((M.kind & 255u) == ZH_FAM_CM1) {
    const uint32_t K = (M.kind >> 16) & 255u;
    for (uint32_t b = 0; b < 8; ++b)             // the bits of the previous byte that survive (c << K) & mask pick the window
      if ((((1ull << (b + K)) & 0xFFFFFFFFull) & M.comp[0].cm_mask) >> 9) wmask |= 1u << b;
  }

  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t budget = (free_b > (2ull << 30) ? free_b - (1ull << 30) : free_b / 2) / std::max(1u, v.mem_share);
  const uint64_t arena_stride = align_up(M.arena_bytes, 256);

  auto coded_len = [&](size_t i) { return np + (pre ? pre->bound(i) : in_off[i + 1] - in_off[i]); };   // (an upper bound with pre)
  auto plain_len = [&](size_t i) { return orig ? orig_off[i + 1] - orig_off[i] : in_off[i + 1] - in_off[i]; };
  auto block_cost = [&](size_t i) {
    const uint64_t n = coded_len(i);
    uint64_t c = n + (o.slot_bytes ? o.slot_bytes : auto_slot(n)) + 64 + (orig && want_sha ? plain_len(i) : 0) + (pre ? pre->scratch(i) : 0);
    if (route_encode(M, o, n) == EncKernel::Cm) c += 24 * n + 4 * (ZH_ENC_CM_KEYS + 1);
    return c;
  };

  uint64_t pos = 0;                               // bytes of the stream so far
  bool any_cm = false;
  for (size_t b0 = 0; b0 < n_blocks;) {
    size_t b1 = b0 + 1;
    uint64_t cost = block_cost(b0);
    if (o.batch_blocks) b1 = std::min<size_t>(n_blocks, b0 + o.batch_blocks);
    else
      while (b1 < n_blocks && b1 - b0 < 4096 && cost + block_cost(b1) <= budget / 2) cost += block_cost(b1++);
    const size_t nb = b1 - b0;

    // the coded sequences in block order (with pre, each in room for its bound), filled from the host or on the device
    std::vector<uint64_t> boff(nb), blen(nb), sha_off;
    const uint8_t *sha_base = nullptr;
    uint64_t in_total = 0;
    for (size_t j = 0; j < nb; ++j) {
      boff[j] = in_total;
      blen[j] = coded_len(b0 + j);
      in_total += align_up(blen[j], 16);
    }
    DevMem d_in, d_slots, d_desc, d_res, d_queue, d_arena, d_la, d_lb, d_bases, d_P, d_orig, d_seg, d_dig;
    HIPCHK(d_in.alloc(in_total));
    float pre_ms = 0;
    if (pre) {
      std::vector<uint64_t> len;
      rc = pre->run(v, b0, b1, d_in.as<uint8_t>(), boff, prefix, len, &sha_base, sha_off, pre_ms, err);
      if (rc) return rc;
      for (size_t j = 0; j < nb; ++j) blen[j] = np + len[j];
      st.init_ms += pre_ms;
      st.kernel_ms += pre_ms;
    } else {
      std::vector<uint8_t> h_in(in_total);
      for (size_t j = 0; j < nb; ++j) {
        memcpy(h_in.data() + boff[j], prefix.data(), np);
        if (blen[j] > np) memcpy(h_in.data() + boff[j] + np, in + in_off[b0 + j], blen[j] - np);
      }
      HIPCHK(hipMemcpy(d_in.p, h_in.data(), in_total, hipMemcpyHostToDevice));
    }

    // layout: CM blocks first (blockIdx = index), then the generic ones (work queue)
    std::vector<size_t> order;
    for (size_t i = b0; i < b1; ++i) if (route_encode(M, o, blen[i - b0]) == EncKernel::Cm) order.push_back(i);
    const size_t n_cm = order.size();
    for (size_t i = b0; i < b1; ++i) if (route_encode(M, o, blen[i - b0]) != EncKernel::Cm) order.push_back(i);
    any_cm |= n_cm > 0;
    std::vector<ZhEncBlock> desc(nb);
    std::vector<size_t> slot_of(nb);              // batch-relative block -> index in order
    uint64_t slot_total = 0, scr_total = 0, orig_total = 0;
    for (size_t k = 0; k < nb; ++k) {
      const size_t i = order[k];
      slot_of[i - b0] = k;
      ZhEncBlock &d = desc[k];
      d.n = blen[i - b0];
      d.in_off = boff[i - b0];
      d.slot_cap = o.slot_bytes ? o.slot_bytes : auto_slot(d.n);
      d.slot_off = slot_total;
      slot_total += align_up(d.slot_cap, 256);
      d.scr_off = scr_total;
      if (k < n_cm) scr_total += align_up(d.n, 4);
      if (orig && want_sha) orig_total += align_up(plain_len(i), 16);
    }
    HIPCHK(d_slots.alloc(slot_total));
    HIPCHK(d_desc.alloc(nb * sizeof(ZhEncBlock)));
    HIPCHK(d_res.alloc(nb * sizeof(ZhEncResult)));
    HIPCHK(d_queue.alloc(256));
    HIPCHK(hipMemcpy(d_desc.p, desc.data(), nb * sizeof(ZhEncBlock), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_queue.p, 0, 256));

    ZhEncLaunch L;
    memset(&L, 0, sizeof L);
    L.in = d_in.as<uint8_t>();
    L.slots = d_slots.as<uint8_t>();
    L.model = d_model.as<ZhModel>();
    L.code = d_code.as<uint8_t>();
    L.tables = v.tables;
    L.budget = 1ull << 32;
    L.limit = (uint32_t)M.comp[0].arg[1] * 4;
    L.wmask = wmask;
    uint32_t grid = 0;
    const size_t n_gen = nb - n_cm;
    if (n_cm) {
      HIPCHK(d_la.alloc(scr_total * 4));
      HIPCHK(d_lb.alloc(scr_total * 4));
      HIPCHK(d_P.alloc(scr_total * 16));
      HIPCHK(d_bases.alloc(n_cm * (ZH_ENC_CM_KEYS + 1) * 4));
      L.list_a = d_la.as<uint32_t>(); L.list_b = d_lb.as<uint32_t>(); L.P = d_P.as<uint16_t>(); L.bases = d_bases.as<uint32_t>();
    }
    if (n_gen) {
      const uint64_t by_mem = std::max<uint64_t>(1, (budget / 4) / arena_stride);
      grid = (uint32_t)std::min<uint64_t>({(uint64_t)n_gen, 1024, by_mem});
      HIPCHK(d_arena.alloc(grid * arena_stride));
      L.arena = d_arena.as<uint8_t>();
      L.arena_stride = arena_stride;
    }

    HIPCHK(hipEventRecord(v.ev0, v.stream));
    L.blocks = d_desc.as<ZhEncBlock>(); L.res = d_res.as<ZhEncResult>(); L.n_blocks = (uint32_t)n_cm;
    HIPCHK(zh_launch_enc_cm_model(&L, (uint32_t)n_cm, v.stream));
    HIPCHK(hipEventRecord(ev_model.e, v.stream));
    if (n_cm) {
      HIPCHK(zh_launch_enc_cm_code(&L, (uint32_t)n_cm, v.stream));
      st.launches += 2;
    }
    if (n_gen) {
      L.blocks = d_desc.as<ZhEncBlock>() + n_cm; L.res = d_res.as<ZhEncResult>() + n_cm; L.n_blocks = (uint32_t)n_gen;
      L.queue = d_queue.as<uint32_t>();
      HIPCHK(zh_launch_enc_generic(&L, grid, v.stream));
      st.launches += 1;
    }
    HIPCHK(hipEventRecord(v.ev1, v.stream));

    std::vector<uint32_t> digest;
    if (want_sha) {                               // SHA-1 of what the size comment describes (Compressor.endSegment)
      std::vector<uint64_t> seg(2 * nb);
      const uint8_t *base = d_in.as<uint8_t>();
      if (pre) {
        for (size_t k = 0; k < nb; ++k) { seg[2 * k] = sha_off[order[k] - b0]; seg[2 * k + 1] = plain_len(order[k]); }
        base = sha_base;
      } else if (orig) {
        std::vector<uint8_t> h_orig(orig_total);
        uint64_t off = 0;
        for (size_t k = 0; k < nb; ++k) {
          const size_t i = order[k], len = plain_len(i);
          if (len) memcpy(h_orig.data() + off, orig + orig_off[i], len);
          seg[2 * k] = off; seg[2 * k + 1] = len;
          off += align_up(len, 16);
        }
        HIPCHK(d_orig.alloc(orig_total));
        HIPCHK(hipMemcpy(d_orig.p, h_orig.data(), orig_total, hipMemcpyHostToDevice));
        base = d_orig.as<uint8_t>();
      } else
        for (size_t k = 0; k < nb; ++k) { seg[2 * k] = desc[k].in_off + np; seg[2 * k + 1] = desc[k].n - np; }
      HIPCHK(d_seg.alloc(seg.size() * 8));
      HIPCHK(d_dig.alloc(nb * 20));
      HIPCHK(hipMemcpy(d_seg.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice));
      HIPCHK(zh_launch_sha1(base, d_seg.as<uint64_t>(), (uint32_t)nb, d_dig.as<uint32_t>(), v.stream));
      digest.resize(5 * nb);
    }
    HIPCHK(hipStreamSynchronize(v.stream));
    float ms = 0, ms_model = 0;
    HIPCHK(hipEventElapsedTime(&ms, v.ev0, v.ev1));
    HIPCHK(hipEventElapsedTime(&ms_model, v.ev0, ev_model.e));
    st.kernel_ms += ms;
    if (!pre) st.init_ms += ms_model;
    if (want_sha) HIPCHK(hipMemcpy(digest.data(), d_dig.p, nb * 20, hipMemcpyDeviceToHost));
    std::vector<ZhEncResult> res(nb);
    HIPCHK(hipMemcpy(res.data(), d_res.p, nb * sizeof(ZhEncResult), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < nb; ++k)
      if (res[k].status) {
        set_err(err, res[k].status, (int)order[k], -1);
        return res[k].status;
      }

    // overflow: the block goes again, alone in its slot, on the generic encoder with a slot that cannot overflow
    std::vector<size_t> over;
    for (size_t k = 0; k < nb; ++k) if (res[k].overflow) over.push_back(k);
    DevMem d_big, d_bdesc, d_bres, d_bqueue, d_barena;
    std::vector<ZhEncResult> bres;
    std::vector<uint64_t> big_off(nb, 0);
    std::vector<char> in_big(nb, 0);
    if (!over.empty()) {
      std::vector<ZhEncBlock> bdesc(over.size());
      uint64_t tot = 0;
      for (size_t j = 0; j < over.size(); ++j) {
        bdesc[j] = desc[over[j]];
        bdesc[j].slot_cap = worst_slot(bdesc[j].n);
        bdesc[j].slot_off = tot;
        big_off[over[j]] = tot;
        tot += align_up(bdesc[j].slot_cap, 256);
      }
      const uint32_t g2 = (uint32_t)std::min<uint64_t>({(uint64_t)over.size(), 1024, std::max<uint64_t>(1, (budget / 4) / arena_stride)});
      HIPCHK(d_big.alloc(tot));
      HIPCHK(d_bdesc.alloc(bdesc.size() * sizeof(ZhEncBlock)));
      HIPCHK(d_bres.alloc(bdesc.size() * sizeof(ZhEncResult)));
      HIPCHK(d_bqueue.alloc(256));
      HIPCHK(d_barena.alloc(g2 * arena_stride));
      HIPCHK(hipMemcpy(d_bdesc.p, bdesc.data(), bdesc.size() * sizeof(ZhEncBlock), hipMemcpyHostToDevice));
      HIPCHK(hipMemset(d_bqueue.p, 0, 256));
      ZhEncLaunch L2 = L;
      L2.slots = d_big.as<uint8_t>();
      L2.blocks = d_bdesc.as<ZhEncBlock>(); L2.res = d_bres.as<ZhEncResult>(); L2.n_blocks = (uint32_t)bdesc.size();
      L2.queue = d_bqueue.as<uint32_t>();
      L2.arena = d_barena.as<uint8_t>(); L2.arena_stride = arena_stride;
      HIPCHK(hipEventRecord(v.ev0, v.stream));
      HIPCHK(zh_launch_enc_generic(&L2, g2, v.stream));
      HIPCHK(hipEventRecord(v.ev1, v.stream));
      st.launches += 1;
      HIPCHK(hipStreamSynchronize(v.stream));
      HIPCHK(hipEventElapsedTime(&ms, v.ev0, v.ev1));
      st.kernel_ms += ms;
      bres.resize(bdesc.size());
      HIPCHK(hipMemcpy(bres.data(), d_bres.p, bres.size() * sizeof(ZhEncResult), hipMemcpyDeviceToHost));
      for (size_t j = 0; j < over.size(); ++j) {
        if (bres[j].status) { set_err(err, bres[j].status, (int)order[over[j]], -1); return bres[j].status; }
        if (bres[j].overflow) { set_err(err, ZPAQHIP_E_HIP, (int)order[over[j]], -1, "coded block exceeds its worst-case slot"); return ZPAQHIP_E_HIP; }
        res[over[j]] = bres[j];
        in_big[over[j]] = 1;
      }
    }

    // the batch's slots in one copy, unless nothing more fits in `out` (the call then only counts the bytes it needs)
    std::vector<uint8_t> h_slots;
    if (pos < out_cap) {
      h_slots.resize(slot_total);
      HIPCHK(hipMemcpy(h_slots.data(), d_slots.p, slot_total, hipMemcpyDeviceToHost));
    }
    // framing around each block's coded bytes, in block order (LibZPAQ.cs:296-323; BlockWriter::write_block)
    for (size_t i = b0; i < b1; ++i) {
      const size_t k = slot_of[i - b0];
      std::string head;
      if (want_tag) head.append((const char *)kTag, 13);
      head.append("zPQ\x01\x01", 5);
      head.append((const char *)hdr, hdr_len);
      head.push_back(1);
      if (filenames && filenames[i]) head.append(filenames[i]);
      head.push_back(0);
      head.append(std::to_string(plain_len(i)));
      head.push_back(0);
      head.push_back(0);
      std::string tail(4, '\0');
      if (want_sha) {
        tail.push_back((char)253);
        for (int w = 0; w < 5; ++w)
          for (int s = 24; s >= 0; s -= 8) tail.push_back((char)(digest[5 * k + w] >> s));
      } else tail.push_back((char)254);
      tail.push_back((char)255);
      const uint64_t clen = res[k].len, need = head.size() + clen + tail.size();
      if (block_off) block_off[i] = pos;
      if (pos + need <= out_cap) {
        memcpy(out + pos, head.data(), head.size());
        if (in_big[k]) HIPCHK(hipMemcpy(out + pos + head.size(), d_big.as<uint8_t>() + big_off[k], clen, hipMemcpyDeviceToHost));
        else if (clen) memcpy(out + pos + head.size(), h_slots.data() + desc[k].slot_off, clen);
        memcpy(out + pos + head.size() + clen, tail.data(), tail.size());
      }
      pos += need;
      st.in_bytes += plain_len(i);
    }
    b0 = b1;
  }
  if (block_off) block_off[n_blocks] = pos;
  st.out_bytes = pos;
  st.kernel_kind = any_cm ? 2 : 1;
  *v.stats = st;
  *out_len = pos;
  if (pos > out_cap) {
    set_err(err, ZPAQHIP_E_OUTPUT_FULL, -1, -1);
    return ZPAQHIP_E_OUTPUT_FULL;
  }
  return ZPAQHIP_OK;
}
