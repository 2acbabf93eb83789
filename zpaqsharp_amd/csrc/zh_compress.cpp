// zh_compress.cpp — zpaqhip_compress_blocks: Compressor.startBlock / startSegment / postProcess / compress / endSegment /
// endBlock (Compressor.cs:27-299) for a batch of blocks, one segment each (LibZPAQ.cs:296-323 framing), coded on the GPU;
// zpaqhip_compress_solid_blocks, the same with several segments per block (startSegment .. endSegment repeated);
// and what zh_compress.h shares with the method path (zh_pre.cpp).  There is one path: every call carries a segment table,
// and a block of one segment is a solid block with n_seg == 1 (the identity table).  Still one segment per block only: the
// method path (`pre`), the store layout and the window-parallel encoder.
//
// The host validates the header with the decoder's framing code and then, batch by batch (Call's steps below): plans the
// batch from the device budget, stages the coded sequences (a host copy, or the pre-processing stage on the device),
// locates the plaintext, takes the SHA-1s, picks an encoder per block (route_encode) and launches the encoders, re-encodes a block whose slot was
// too small with a worst-case slot (on the chain encoder if it ran there, else on the generic one), and writes tag, block,
// segment and end framing around each slot's bytes.  Every coded byte comes out of a HIP kernel (zh_enc_cm.hip, zh_enc_chain.hip, zh_enc_generic.hip); there is
// no CPU encoder here.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zh_compress.h"
#include "zh_ctx_view.h"
#include "zh_enc.h"
#include "zh_verify.h"

extern "C" hipError_t zh_launch_enc_generic(const ZhEncLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_enc_chain(const ZhEncLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_enc_cm_model(const ZhEncLaunch *L, uint32_t n_blocks, hipStream_t stream);
extern "C" hipError_t zh_launch_enc_cm_code(const ZhEncLaunch *L, uint32_t n_blocks, hipStream_t stream);
extern "C" hipError_t zh_launch_sha1(const uint8_t *data, const uint64_t *seg, uint32_t n_seg, uint32_t *digest, hipStream_t stream);
extern "C" hipError_t zh_launch_frame_pack(const ZhFrameLaunch *L, hipStream_t stream, uint32_t *launches);

using namespace zh;

// ---- zh_compress.h's helpers

hipError_t zh::device_budget(uint32_t mem_share, uint64_t reusable, uint64_t *budget) {
  size_t free_b = 0, total_b = 0;
  const hipError_t e = hipMemGetInfo(&free_b, &total_b);
  const uint64_t f = free_b + reusable;
  *budget = (f > (2ull << 30) ? f - (1ull << 30) : f / 2) / std::max(1u, mem_share);
  return e;
}

zpaqhip_compress_opts zh::resolve_compress_opts(const zpaqhip_compress_opts *opts) {
  zpaqhip_compress_opts o;
  memset(&o, 0, sizeof o);
  if (opts) memcpy(&o, opts, std::min<size_t>(sizeof o, opts->struct_size ? opts->struct_size : sizeof o));
  else o.flags = 3;
  return o;
}

int zh::sha1_segments(const CtxView &v, const uint8_t *d_base, const std::vector<uint64_t> &seg, std::vector<uint32_t> &digest,
                      zpaqhip_err *err) {
  const size_t n = seg.size() / 2;
  DevMem d_seg, d_dig;
  HIPCHK(d_seg.alloc(seg.size() * 8));
  HIPCHK(d_dig.alloc(n * 20));
  HIPCHK(hipMemcpy(d_seg.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(zh_launch_sha1(d_base, d_seg.as<uint64_t>(), (uint32_t)n, d_dig.as<uint32_t>(), v.stream));
  HIPCHK(hipStreamSynchronize(v.stream));
  digest.resize(5 * n);
  HIPCHK(hipMemcpy(digest.data(), d_dig.p, n * 20, hipMemcpyDeviceToHost));
  return ZPAQHIP_OK;
}

hipError_t zh::DevSink::reserve(uint64_t need, uint64_t keep, hipStream_t stream) {
  if (need <= cap) return hipSuccess;
  const uint64_t grown = std::max(need, 2 * cap);
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, grown + 16);                          // (+ 16: zh_frame.hip reads aligned 16-byte groups)
  if (e != hipSuccess) return e;
  if (keep) {
    e = hipMemcpyAsync(p, mem.p, keep, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
      (void)hipFree(p);
      return e;
    }
  }
  if (mem.p) (void)hipFree(mem.p);
  mem.p = p;
  cap = grown;
  return hipSuccess;
}

int zh::finish_call(const CtxView &v, zpaqhip_stats st, uint64_t pos, size_t n_blocks, uint64_t *off, size_t out_cap, size_t *out_len,
                    zpaqhip_err *err) {
  if (off) off[n_blocks] = pos;
  st.out_bytes = pos;
  *v.stats = st;
  *out_len = pos;
  if (pos > out_cap) {
    set_err(err, ZPAQHIP_E_OUTPUT_FULL, -1, -1);
    return ZPAQHIP_E_OUTPUT_FULL;
  }
  return ZPAQHIP_OK;
}

namespace {

// ---- which kernel encodes a block (the encode-side twin of zh_dec_plan.h's route_block): the window-parallel CM encoder for
// ZH_FAM_CM1 models with opts.kernel 0 or 2, the lane-per-component encoder for the chain families with opts.kernel 2, the
// generic encoder for everything else (and for a block too long for zh_enc_cm's 28-bit positions).  A block of several
// segments (the solid form) never goes to the window-parallel encoder, which codes one segment: its ZH_FAM_CM1 model is a
// chain of one component, so such a block takes the lane-per-component encoder with opts.kernel 2 and the generic one otherwise.
enum class EncKernel { Generic, Cm, Chain };
EncKernel route_encode(const ZhModel &m, const zpaqhip_compress_opts &o, uint64_t coded, uint64_t n_seg) {
  const bool cm1 = (m.kind & 255u) == ZH_FAM_CM1;
  if (cm1 && n_seg == 1 && (o.kernel == 0 || o.kernel == 2) && coded < ZH_ENC_CM_MAX_N) return EncKernel::Cm;
  if (o.kernel == 2 && (chain_family(m.kind & 255u) || (cm1 && n_seg > 1 && m.arena_bytes < (1ull << 32)))) return EncKernel::Chain;
  return EncKernel::Generic;
}

// The chain encoder's LDS plan for a model: its ICM / ISSE units, and the most waves of one workgroup (one per SIMD) whose
// regions fit next to the shared tables (zh_enc.h).  Models outside the chain family get no wave.
struct ChainPlan { uint32_t waves = 0, units = 0, lds_bytes = 0; };
ChainPlan plan_chain(const ZhModel &m) {
  ChainPlan p;
  if (!chain_family(m.kind & 255u)) return p;
  p.units = chain_units(m);
  p.waves = zh_enc_chain_fit(p.units);
  p.lds_bytes = p.waves ? ZH_ENC_CHAIN_TABLES + p.waves * zh_enc_chain_stride(p.units) : 0;
  return p;
}

uint64_t auto_slot(uint64_t coded) { return coded + coded / 8 + 4096; }
uint64_t worst_slot(uint64_t coded) { return 16 * coded + 4096; }    // 2 bytes per coded bit, plus the end of segment

// One launch of the encoders over blocks of a batch: what the host lays out, the device buffers, and the results
struct EncRun {
  std::vector<ZhEncBlock> desc;           // the CM blocks first (blockIdx = index), then the chain encoder's, then the generic
  std::vector<size_t> block;              // one's (a work queue each); desc[k] codes block block[k] of the call
  size_t n_cm = 0, n_chain = 0;
  uint64_t slot_total = 0, scr_total = 0;
  std::vector<ZhEncSeg> segs;             // desc[k]'s segments are segs[desc[k].seg0 ...], n_seg of them
  std::vector<ZhEncResult> res;
  std::vector<uint64_t> seg_end;          // per entry of segs, from the device
  DevMem slots, d_desc, d_res, queue, arena, chain_arena, la, lb, bases, P;   // (d_desc: desc, then segs; d_res: res, then seg_end)
};

// Where on the device the plaintext of a batch lies: segment k of the batch (in segment order) is seg[2k + 1] bytes at
// base + seg[2k], the pairs sha1_segments takes
struct PlainView {
  const uint8_t *base = nullptr;
  std::vector<uint64_t> seg;
};

struct Batch {                            // blocks [b0, b1) of the call
  size_t b0 = 0, b1 = 0;
  std::vector<uint64_t> boff, blen;       // the coded sequence of block b0 + j in d_in (store layout: its pre-processed bytes)
  uint64_t in_total = 0;
  DevMem d_in;
  PreBatch pre;
  PlainView plain;                        // what the size comments and SHA-1s describe (Call::locate)
  DevMem d_orig;                          // ... when it came from the host: the batch's range of `orig`, uploaded once
  std::vector<uint32_t> digest;           // five words per segment, in segment order
  EncRun first, redo;                     // every block with its own slot; the overflowed ones again with worst-case slots
  std::vector<size_t> slot_of;            // j -> index in `first`
  std::vector<int64_t> redo_of;           // index in `first` -> index in `redo`, or -1
  size_t nb() const { return b1 - b0; }
};

// One call of compress_impl: its arguments, what it keeps on the device for all batches, and the steps of a batch
struct Call : CompressCall {
  zpaqhip_compress_opts o;
  const bool dev_in, dev_out;             // the device form: `in` and `orig`, `out` are device memory; stage and frame differ
  DevSink *const sink;                    // the device form appends to it instead of writing to `out`
  uint32_t pack_launches = 0;             // zh_frame.hip's launches, of staging and of framing
  uint32_t verify_launches = 0;           // the verify pass's (opts.flags bit 5)
  ZhModel M;
  std::vector<uint8_t> code, sel, dev_prefix;   // the selector prefix; what of it goes in front of the bytes on the device
  bool store = false;                     // n = 0: no encoder, the store layout of the pre-processed bytes (a level 2 block)
  CtxView v{};
  Event ev_model;                         // end of the model pass: init_ms times zh_enc_cm_model on its own
  DevMem d_model, d_code;
  DevMem d_tab;                           // the packing kernel's table and blob, kept across batches and grown when needed
  size_t tab_cap = 0;
  uint32_t wmask = 0;
  uint64_t budget = 0, arena_stride = 0;
  zpaqhip_stats st{};
  uint64_t pos = 0;                       // bytes of the stream so far
  bool any_cm = false, any_chain = false;
  // The segment table: block i holds the segments [seg_first[i], seg_first[i + 1]); seg_in, seg_orig (NULL without `orig`)
  // and filenames are per segment, in_off and orig_off the blocks' view of them.  The solid form brings its own; every
  // other call gets the identity, one segment per block, over its in_off and orig_off.
  std::vector<uint64_t> ident;
  const uint64_t *seg_first, *seg_in, *seg_orig;
  DevMem d_model_chain;                   // a ZH_FAM_CM1 model as the lane-per-component encoder takes it
  int cus = 0;                            // compute units: the chain encoder's LDS lets one of its workgroups live on each
  ChainPlan chain;                        // ... with this many waves at most

  explicit Call(const CompressCall &a)
      : CompressCall(a), o(resolve_compress_opts(a.opts)), dev_in(a.dev), dev_out(a.dev), sink(a.dev ? a.dev->sink : nullptr),
        seg_first(a.solid ? a.solid->seg_first : nullptr), seg_in(a.solid ? a.solid->in_off : a.in_off),
        seg_orig(a.solid ? a.solid->orig_off : a.orig_off) {
    if (sink) pos = sink->used;
    if (!solid) {
      ident.resize(n_blocks + 1);
      for (size_t i = 0; i <= n_blocks; ++i) ident[i] = i;
      seg_first = ident.data();
    }
  }
  bool want_sha() const { return (o.flags & 1) != 0; }
  bool want_verify() const { return (o.flags & kFlagVerify) != 0; }
  size_t seg_lo(size_t i) const { return seg_first[i]; }
  size_t n_seg(size_t i) const { return seg_first[i + 1] - seg_first[i]; }
  uint64_t seg_plain(size_t s) const { return seg_orig ? seg_orig[s + 1] - seg_orig[s] : seg_in[s + 1] - seg_in[s]; }
  uint64_t in_len(size_t i) const { return in_off[i + 1] - in_off[i]; }
  uint64_t plain_len(size_t i) const { return orig ? orig_off[i + 1] - orig_off[i] : in_len(i); }
  uint64_t coded_len(size_t i) const { return dev_prefix.size() + (pre ? pre->bound(i) : in_len(i)); }   // (an upper bound with pre)
  uint64_t slot_cap(uint64_t n) const { return o.slot_bytes ? o.slot_bytes : auto_slot(n); }
  uint64_t block_cost(size_t i) const {
    const uint64_t vc = want_verify() ? 2 * plain_len(i) + (store ? pre->bound(i) : 0) : 0;   // post-processed bytes, plaintext, staged copy
    if (store) return pre->bound(i) + pre->scratch(i) + vc;
    const uint64_t n = coded_len(i);
    uint64_t c = n + slot_cap(n) + 64 + (orig && want_sha() ? plain_len(i) : 0) + (pre ? pre->scratch(i) : 0) + vc;
    if (route_encode(M, o, n, n_seg(i)) == EncKernel::Cm) c += 24 * n + 4 * (ZH_ENC_CM_KEYS + 1);
    return c + 24 * n_seg(i);
  }

  int open();
  int plan(Batch &B, size_t b0) const;
  int stage(Batch &B);
  int locate(Batch &B) const;
  int digests(Batch &B) const;
  int verify(Batch &B);
  int encode(const Batch &B, EncRun &r);
  int encode_batch(Batch &B);
  int retry(Batch &B);
  int pack(const FrameTable &T, const Batch &B, uint8_t *d_dst, float *ms);
  int frame(Batch &B);
};

// the device, the model for the generic encoder and what the CM encoder needs of it, the budget
int Call::open() {
  v = ctx_view(ctx);
  if (dev && dev->stream) v.stream = dev->stream;
  HIPCHK(hipSetDevice(v.device));
  st.blocks = n_blocks;
  if (!store) {
    HIPCHK(hipEventCreate(&ev_model.e));
    HIPCHK(d_model.alloc(sizeof(ZhModel)));
    HIPCHK(d_code.alloc(code.size()));
    HIPCHK(hipMemcpy(d_model.p, &M, sizeof(ZhModel), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_code.p, code.data(), code.size(), hipMemcpyHostToDevice));
    if ((M.kind & 255u) == ZH_FAM_CM1) {
      const uint32_t K = (M.kind >> 16) & 255u;
      for (uint32_t b = 0; b < 8; ++b)             // the bits of the previous byte that survive (c << K) & mask pick the window
        if ((((1ull << (b + K)) & 0xFFFFFFFFull) & M.comp[0].cm_mask) >> 9) wmask |= 1u << b;
    }
  }
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, v.device));
  HIPCHK(device_budget(v.mem_share, 0, &budget));
  arena_stride = align_up(M.arena_bytes, 256);
  chain = plan_chain(M);
  if (solid && (M.kind & 255u) == ZH_FAM_CM1) {
    // a single CM is a chain of one component without ICM / ISSE units; that encoder reads a translated HCOMP's id from
    // bits 8-15 of the kind, where this family keeps something else: 0 there has it interpret the program
    ZhModel Mc = M;
    Mc.kind = ZH_FAM_CHAIN;
    HIPCHK(d_model_chain.alloc(sizeof(ZhModel)));
    HIPCHK(hipMemcpy(d_model_chain.p, &Mc, sizeof(ZhModel), hipMemcpyHostToDevice));
    chain.units = 0;
    chain.waves = zh_enc_chain_fit(0);
    chain.lds_bytes = ZH_ENC_CHAIN_TABLES + chain.waves * zh_enc_chain_stride(0);
  }
  return ZPAQHIP_OK;
}

// the batch's blocks and room for their coded sequences in block order (with pre, each in room for its bound)
int Call::plan(Batch &B, size_t b0) const {
  B.b0 = b0;
  B.b1 = batch_end(b0, n_blocks, o.batch_blocks, budget, [&](size_t i) { return block_cost(i); });
  B.boff.resize(B.nb());
  B.blen.resize(B.nb());
  for (size_t j = 0; j < B.nb(); ++j) {
    B.boff[j] = B.in_total;
    B.blen[j] = coded_len(b0 + j);
    B.in_total += align_up(B.blen[j], 16);
  }
  HIPCHK(B.d_in.alloc(B.in_total));
  return ZPAQHIP_OK;
}

// the coded sequences, filled from the host or on the device
int Call::stage(Batch &B) {
  const size_t np = dev_prefix.size();
  if (pre) {
    const int rc = pre->run(v, B.b0, B.b1, B.d_in.as<uint8_t>(), B.boff, dev_prefix, B.pre, err);
    if (rc) return rc;
    for (size_t j = 0; j < B.nb(); ++j) B.blen[j] = np + B.pre.len[j];
    st.init_ms += B.pre.ms;
    st.kernel_ms += B.pre.ms;
    return ZPAQHIP_OK;
  }
  if (dev_in) {                           // device to device: prefix || block at its aligned place, by the packing kernel
    FrameTable T;
    T.blob = dev_prefix;
    for (size_t j = 0; j < B.nb(); ++j) {
      ZhFrameEntry e;
      memset(&e, 0, sizeof e);
      e.dst_off = B.boff[j];
      e.head_len = (uint32_t)np;
      e.src = ZH_FRAME_SRC_INPUT;
      e.src_off = in_off[B.b0 + j];
      e.body_len = B.blen[j] - np;
      T.entry.push_back(e);
      T.pieces = (uint32_t)std::max<uint64_t>(T.pieces, (e.body_len + ZH_FRAME_PIECE - 1) / ZH_FRAME_PIECE);
    }
    float ms = 0;
    return pack(T, B, B.d_in.as<uint8_t>(), &ms);
  }
  std::vector<uint8_t> h_in(B.in_total);
  for (size_t j = 0; j < B.nb(); ++j) {
    memcpy(h_in.data() + B.boff[j], dev_prefix.data(), np);
    if (B.blen[j] > np) memcpy(h_in.data() + B.boff[j] + np, in + in_off[B.b0 + j], B.blen[j] - np);
  }
  HIPCHK(hipMemcpy(B.d_in.p, h_in.data(), B.in_total, hipMemcpyHostToDevice));
  return ZPAQHIP_OK;
}

// Where the plaintext is that the size comments and SHA-1s of the batch describe (Compressor.endSegment), decided once for
// digests and verify: the plaintext the pre-processing left on the device, the coded bytes behind the prefix (a block's
// segments lie back to back there), `orig` where the caller has it on the device, or the batch's range of a host `orig`,
// uploaded here as it is.  The segments then start wherever the caller's offsets put them: zh_sha1_dev.hip and the verify
// pass take unaligned starts, as the device form has always given them.  (zh_sha1_dev.hip loads 16 bytes at a time only
// from a 4-byte aligned start and single bytes otherwise: a host `orig`, which an earlier form of this upload aligned
// block by block, now mostly takes the byte path.  Correct either way; the kernel's time on that path is not measured.)
int Call::locate(Batch &B) const {
  if (!want_sha() && !want_verify()) return ZPAQHIP_OK;
  const size_t sa = seg_first[B.b0], sb = seg_first[B.b1], np = dev_prefix.size();
  PlainView &P = B.plain;
  P.seg.resize(2 * (sb - sa));
  for (size_t s = sa; s < sb; ++s) P.seg[2 * (s - sa) + 1] = seg_plain(s);
  if (pre) {
    P.base = B.pre.plain;
    for (size_t s = sa; s < sb; ++s) P.seg[2 * (s - sa)] = seg_in[s] - seg_in[sa];
  } else if (!orig) {
    P.base = B.d_in.as<uint8_t>();
    for (size_t j = 0; j < B.nb(); ++j)
      for (size_t s = seg_lo(B.b0 + j); s < seg_lo(B.b0 + j + 1); ++s)
        P.seg[2 * (s - sa)] = B.boff[j] + np + (seg_in[s] - seg_in[seg_lo(B.b0 + j)]);
  } else if (dev_in) {
    P.base = orig;
    for (size_t s = sa; s < sb; ++s) P.seg[2 * (s - sa)] = seg_orig[s];
  } else {
    const uint64_t base = seg_orig[sa], bytes = seg_orig[sb] - base;
    HIPCHK(B.d_orig.alloc(bytes + 16));
    if (bytes) HIPCHK(hipMemcpy(B.d_orig.p, orig + base, bytes, hipMemcpyHostToDevice));
    P.base = B.d_orig.as<uint8_t>();
    for (size_t s = sa; s < sb; ++s) P.seg[2 * (s - sa)] = seg_orig[s] - base;
  }
  return ZPAQHIP_OK;
}

// a SHA-1 per segment of the batch
int Call::digests(Batch &B) const {
  return want_sha() ? sha1_segments(v, B.plain.base, B.plain.seg, B.digest, err) : ZPAQHIP_OK;
}

// opts.flags bit 5 (Compressor.setVerify): the batch's coded sequences through the block's own post-processor, against the
// plaintext the size comment and SHA-1 describe; the lowest failing block ends the call.  (One segment per block: the
// solid entry points refuse the flag.)
int Call::verify(Batch &B) {
  if (!want_verify()) return ZPAQHIP_OK;
  const size_t nb = B.nb();
  VerifyIn vin;
  DevMem d_stage;
  if (store) {                            // (the store layout keeps the selector on the host: a copy with it in front)
    if (const int rc = verify_stage(v, sel, B.d_in.as<uint8_t>(), B.boff, B.blen, d_stage, vin, &verify_launches, err)) return rc;
  } else {
    vin.d_in = B.d_in.as<uint8_t>();
    vin.off = B.boff;
    vin.len = B.blen;
  }
  vin.d_plain = B.plain.base;
  for (size_t j = 0; j < nb; ++j) {
    vin.poff.push_back(B.plain.seg[2 * j]);
    vin.plen.push_back(B.plain.seg[2 * j + 1]);
  }
  std::vector<zpaqhip_verify_result> rec;
  uint64_t wrote = 0;
  if (const int rc = verify_pass(v, M.ph, M.pm, vin, budget / 4, rec, &st.kernel_ms, &verify_launches, &wrote, err)) {
    if (err && err->block >= 0) err->block += (int32_t)B.b0;
    return rc;
  }
  for (size_t j = 0; j < nb; ++j)
    if (rec[j].status) {
      set_err(err, rec[j].status, (int)(B.b0 + j), -1);
      return rec[j].status;
    }
  return ZPAQHIP_OK;
}

// allocate what r's blocks need, upload their descriptors, launch the encoders, fetch and check the results
int Call::encode(const Batch &B, EncRun &r) {
  const size_t n = r.desc.size(), n_gen = n - r.n_cm - r.n_chain;
  HIPCHK(r.slots.alloc(r.slot_total));
  const size_t desc_b = n * sizeof(ZhEncBlock), segs_b = r.segs.size() * sizeof(ZhEncSeg), res_b = n * sizeof(ZhEncResult);
  std::vector<uint8_t> up(desc_b + segs_b);
  memcpy(up.data(), r.desc.data(), desc_b);
  memcpy(up.data() + desc_b, r.segs.data(), segs_b);
  HIPCHK(r.d_desc.alloc(up.size()));
  HIPCHK(r.d_res.alloc(res_b + r.segs.size() * 8));
  HIPCHK(hipMemcpy(r.d_desc.p, up.data(), up.size(), hipMemcpyHostToDevice));
  ZhEncLaunch L;
  memset(&L, 0, sizeof L);
  L.segs = reinterpret_cast<const ZhEncSeg *>(r.d_desc.as<uint8_t>() + desc_b);
  L.seg_end = reinterpret_cast<uint64_t *>(r.d_res.as<uint8_t>() + res_b);
  L.in = B.d_in.as<uint8_t>();
  L.slots = r.slots.as<uint8_t>();
  L.model = d_model.as<ZhModel>();
  L.code = d_code.as<uint8_t>();
  L.tables = v.tables;
  L.budget = 1ull << 32;
  L.limit = (uint32_t)M.comp[0].arg[1] * 4;
  L.wmask = wmask;
  uint32_t grid = 0, chain_grid = 0, chain_waves = 1;
  if (r.n_cm) {
    HIPCHK(r.la.alloc(r.scr_total * 4));
    HIPCHK(r.lb.alloc(r.scr_total * 4));
    HIPCHK(r.P.alloc(r.scr_total * 16));
    HIPCHK(r.bases.alloc(r.n_cm * (ZH_ENC_CM_KEYS + 1) * 4));
    L.list_a = r.la.as<uint32_t>(); L.list_b = r.lb.as<uint32_t>(); L.P = r.P.as<uint16_t>(); L.bases = r.bases.as<uint32_t>();
  }
  // an arena slot per resident wave; the two queue heads share one buffer
  if (n_gen || r.n_chain) {
    HIPCHK(r.queue.alloc(256));
    HIPCHK(hipMemset(r.queue.p, 0, 256));
    L.arena_stride = arena_stride;
  }
  if (n_gen) {
    const uint64_t by_mem = std::max<uint64_t>(1, (budget / 4) / arena_stride);
    grid = (uint32_t)std::min<uint64_t>({(uint64_t)n_gen, 1024, by_mem});
    HIPCHK(r.arena.alloc(grid * arena_stride));
  }
  if (r.n_chain) {
    // (half the budget for these arenas: a batch's own buffers are planned within the other half, and max's 22 tables
    // would otherwise leave most compute units without a wave).  The blocks spread over the compute units first; only a
    // launch with more blocks than units puts a second, third and fourth wave into a workgroup, as many as the model's
    // LDS plan, opts.enc_waves and the blocks per workgroup allow; where memory is short of an arena slot per wave the
    // waves go before the workgroups.
    const uint64_t chain_mem = std::max<uint64_t>(1, (budget / 2) / arena_stride);
    chain_grid = (uint32_t)std::min<uint64_t>((uint64_t)r.n_chain, (uint64_t)std::max(1, cus));
    const uint32_t cap = o.enc_waves ? std::min(o.enc_waves, chain.waves) : chain.waves;
    chain_waves = (uint32_t)std::min<uint64_t>(std::max(1u, cap), (r.n_chain + chain_grid - 1) / chain_grid);
    while (chain_waves > 1 && (uint64_t)chain_grid * chain_waves > chain_mem) --chain_waves;
    chain_grid = (uint32_t)std::min<uint64_t>(chain_grid, chain_mem);
    HIPCHK(r.chain_arena.alloc((uint64_t)chain_grid * chain_waves * arena_stride));
    st.concurrent = std::max(st.concurrent, (uint32_t)std::min<uint64_t>(r.n_chain, (uint64_t)chain_grid * chain_waves));
  }

  HIPCHK(hipEventRecord(v.ev0, v.stream));
  if (r.n_cm) {
    L.blocks = r.d_desc.as<ZhEncBlock>(); L.res = r.d_res.as<ZhEncResult>(); L.n_blocks = (uint32_t)r.n_cm;
    HIPCHK(zh_launch_enc_cm_model(&L, (uint32_t)r.n_cm, v.stream));
    HIPCHK(hipEventRecord(ev_model.e, v.stream));
    HIPCHK(zh_launch_enc_cm_code(&L, (uint32_t)r.n_cm, v.stream));
    st.launches += 2;
  }
  if (r.n_chain) {
    L.blocks = r.d_desc.as<ZhEncBlock>() + r.n_cm; L.res = r.d_res.as<ZhEncResult>() + r.n_cm; L.n_blocks = (uint32_t)r.n_chain;
    L.queue = r.queue.as<uint32_t>() + 16; L.arena = r.chain_arena.as<uint8_t>();
    L.waves = chain_waves; L.lds_pool = chain.units * 1024u; L.lds_stride = zh_enc_chain_stride(chain.units);
    if (d_model_chain.p) L.model = d_model_chain.as<ZhModel>();
    HIPCHK(zh_launch_enc_chain(&L, chain_grid, v.stream));
    L.model = d_model.as<ZhModel>();
    st.launches += 1;
  }
  if (n_gen) {
    const size_t g0 = r.n_cm + r.n_chain;
    L.blocks = r.d_desc.as<ZhEncBlock>() + g0; L.res = r.d_res.as<ZhEncResult>() + g0; L.n_blocks = (uint32_t)n_gen;
    L.queue = r.queue.as<uint32_t>(); L.arena = r.arena.as<uint8_t>();
    HIPCHK(zh_launch_enc_generic(&L, grid, v.stream));
    st.launches += 1;
  }
  HIPCHK(hipEventRecord(v.ev1, v.stream));
  HIPCHK(hipStreamSynchronize(v.stream));
  float ms = 0, ms_model = 0;
  HIPCHK(hipEventElapsedTime(&ms, v.ev0, v.ev1));
  st.kernel_ms += ms;
  if (r.n_cm && !pre) {
    HIPCHK(hipEventElapsedTime(&ms_model, v.ev0, ev_model.e));
    st.init_ms += ms_model;
  }
  std::vector<uint8_t> down(res_b + r.segs.size() * 8);
  HIPCHK(hipMemcpy(down.data(), r.d_res.p, down.size(), hipMemcpyDeviceToHost));
  r.res.resize(n);
  r.seg_end.resize(r.segs.size());
  memcpy(r.res.data(), down.data(), res_b);
  memcpy(r.seg_end.data(), down.data() + res_b, r.segs.size() * 8);
  for (size_t k = 0; k < r.n_cm; ++k) r.seg_end[r.desc[k].seg0] = r.res[k].len;   // zh_enc_cm keeps no such record: one segment
  for (size_t k = 0; k < n; ++k)
    if (r.res[k].status) {
      set_err(err, r.res[k].status, (int)r.block[k], -1);
      return r.res[k].status;
    }
  return ZPAQHIP_OK;
}

// every block of the batch on its encoder, with the slot the options give it
int Call::encode_batch(Batch &B) {
  EncRun &r = B.first;
  auto take = [&](EncKernel k) {
    for (size_t i = B.b0; i < B.b1; ++i) if (route_encode(M, o, B.blen[i - B.b0], n_seg(i)) == k) r.block.push_back(i);
  };
  take(EncKernel::Cm);
  r.n_cm = r.block.size();
  take(EncKernel::Chain);
  r.n_chain = r.block.size() - r.n_cm;
  take(EncKernel::Generic);
  any_cm |= r.n_cm > 0;
  any_chain |= r.n_chain > 0;
  r.desc.resize(B.nb());
  B.slot_of.resize(B.nb());
  for (size_t k = 0; k < B.nb(); ++k) {
    const size_t j = r.block[k] - B.b0;
    B.slot_of[j] = k;
    ZhEncBlock &d = r.desc[k];
    d.n = B.blen[j];
    d.in_off = B.boff[j];
    d.slot_cap = slot_cap(d.n);
    d.slot_off = r.slot_total;
    r.slot_total += align_up(d.slot_cap, 256);
    d.scr_off = r.scr_total;
    if (k < r.n_cm) r.scr_total += align_up(d.n, 4);
    // its segments, back to back with the prefix in the first; with pre a block is one segment of the length the
    // pre-processing gave it
    const size_t i = r.block[k];
    d.seg0 = (uint32_t)r.segs.size();
    d.n_seg = (uint32_t)n_seg(i);
    uint64_t at = d.in_off;
    for (size_t s = seg_lo(i); s < seg_lo(i + 1); ++s) {
      const uint64_t len = pre ? d.n : seg_in[s + 1] - seg_in[s] + (s == seg_lo(i) ? dev_prefix.size() : 0);
      r.segs.push_back({at, len});
      at += len;
    }
  }
  return encode(B, r);
}

// overflow: the block goes again with a slot that cannot overflow, on the chain encoder if it ran there, else on the
// generic one
int Call::retry(Batch &B) {
  EncRun &r = B.redo;
  B.redo_of.assign(B.nb(), -1);
  const size_t c0 = B.first.n_cm, c1 = c0 + B.first.n_chain;
  for (int pass = 0; pass < 2; ++pass)
  for (size_t k = 0; k < B.nb(); ++k)
    if (B.first.res[k].overflow && (pass == 0) == (k >= c0 && k < c1)) {
      ZhEncBlock d = B.first.desc[k];
      d.slot_cap = worst_slot(d.n);
      d.slot_off = r.slot_total;
      r.slot_total += align_up(d.slot_cap, 256);
      r.segs.insert(r.segs.end(), B.first.segs.begin() + d.seg0, B.first.segs.begin() + d.seg0 + d.n_seg);
      d.seg0 = (uint32_t)(r.segs.size() - d.n_seg);
      B.redo_of[k] = (int64_t)r.desc.size();
      r.desc.push_back(d);
      r.block.push_back(B.first.block[k]);
      r.n_chain += pass == 0;
    }
  if (r.desc.empty()) return ZPAQHIP_OK;
  const int rc = encode(B, r);
  if (rc) return rc;
  for (size_t j = 0; j < r.desc.size(); ++j)
    if (r.res[j].overflow) {
      set_err(err, ZPAQHIP_E_HIP, (int)r.block[j], -1, "coded block exceeds its worst-case slot");
      return ZPAQHIP_E_HIP;
    }
  return ZPAQHIP_OK;
}

// zh_frame.hip over a table: uploads it with its blob and packs into d_dst from the batch's buffers and the caller's input
int Call::pack(const FrameTable &T, const Batch &B, uint8_t *d_dst, float *ms) {
  if (T.entry.empty()) return ZPAQHIP_OK;
  const size_t tb = T.entry.size() * sizeof(ZhFrameEntry);
  std::vector<uint8_t> up(tb + T.blob.size());
  memcpy(up.data(), T.entry.data(), tb);
  if (!T.blob.empty()) memcpy(up.data() + tb, T.blob.data(), T.blob.size());
  if (up.size() + 16 > tab_cap) {         // (+ 16: the kernel reads the blob in aligned 16-byte groups)
    HIPCHK(d_tab.alloc(2 * up.size() + 16));
    tab_cap = 2 * up.size() + 16;
  }
  HIPCHK(hipMemcpy(d_tab.p, up.data(), up.size(), hipMemcpyHostToDevice));
  ZhFrameLaunch L;
  memset(&L, 0, sizeof L);
  L.table = d_tab.as<ZhFrameEntry>();
  L.blob = d_tab.as<uint8_t>() + tb;
  L.src[ZH_FRAME_SRC_FIRST] = B.first.slots.as<uint8_t>();
  L.src[ZH_FRAME_SRC_REDO] = B.redo.slots.as<uint8_t>();
  L.src[ZH_FRAME_SRC_PRE] = B.d_in.as<uint8_t>();
  L.src[ZH_FRAME_SRC_INPUT] = in;
  L.out = d_dst;
  L.sel_len = T.sel_len;
  L.n = (uint32_t)T.entry.size();
  L.pieces = T.pieces;
  HIPCHK(hipEventRecord(v.ev0, v.stream));
  HIPCHK(zh_launch_frame_pack(&L, v.stream, &pack_launches));
  HIPCHK(hipEventRecord(v.ev1, v.stream));
  HIPCHK(hipStreamSynchronize(v.stream));
  HIPCHK(hipEventElapsedTime(ms, v.ev0, v.ev1));
  return ZPAQHIP_OK;
}

// framing around each block's coded bytes, in block order: an entry of the frame table per segment, cut out of the
// block's slot at the ends the encoder recorded (the retry's when the block went again; store layout: the block's
// pre-processed bytes, whole); the host form copies by the table, the device form hands it to the packing kernel
int Call::frame(Batch &B) {
  std::vector<TableBlock> items(B.nb());
  const size_t sa = seg_first[B.b0];
  for (size_t j = 0; j < B.nb(); ++j) {
    const size_t i = B.b0 + j, k = store ? 0 : B.slot_of[j];
    const int64_t redo = store ? -1 : B.redo_of[k];
    const EncRun &r = redo >= 0 ? B.redo : B.first;
    TableBlock &it = items[j];
    it.src = store ? ZH_FRAME_SRC_PRE : redo >= 0 ? ZH_FRAME_SRC_REDO : ZH_FRAME_SRC_FIRST;
    it.src_off = store ? B.boff[j] : r.desc[redo >= 0 ? (size_t)redo : k].slot_off;
    for (size_t s = seg_lo(i); s < seg_lo(i + 1); ++s)
      it.seg.push_back({filenames ? filenames[s] : nullptr, seg_plain(s), want_sha() ? &B.digest[5 * (s - sa)] : nullptr,
                        store ? B.blen[j] : r.seg_end[r.desc[redo >= 0 ? (size_t)redo : k].seg0 + (s - seg_lo(i))]});
    st.in_bytes += plain_len(i);
  }
  const uint64_t pos0 = pos;
  FrameTable T;
  pos = build_frame_table((o.flags & 2) != 0, store ? 2 : 1, hdr, hdr_len, items, store ? &sel : nullptr, pos0, sink ? ~0ull : out_cap, T,
                          block_off ? block_off + B.b0 : nullptr);
  if (pos == kFrameRefused) {             // (not reached: the store layout needs pre, which the solid entry points refuse)
    set_err(err, ZPAQHIP_E_ARG, (int)B.b0, -1, "the store layout takes one segment per block");
    return ZPAQHIP_E_ARG;
  }
  if (sink) {                             // room for the batch behind what the sink holds
    if (sink->reserve(pos, pos0, v.stream) != hipSuccess) {
      (void)hipGetLastError();
      set_err(err, ZPAQHIP_E_DEVICE_MEM, (int)B.b0, -1, "no device memory for the scratch stream");
      return ZPAQHIP_E_DEVICE_MEM;
    }
    out = sink->base();
  }
  if (dev_out) {
    float ms = 0;
    const int rc = pack(T, B, out, &ms);
    st.kernel_ms += ms;
    return rc;
  }
  // the batch's slots (store layout: its pre-processed bytes) in one copy, unless nothing more fits in `out` (the call
  // then only counts the bytes it needs); a retry's slot is fetched on its own
  const DevMem &d_src = store ? B.d_in : B.first.slots;
  std::vector<uint8_t> h_src;
  if (pos0 < out_cap) {
    h_src.resize(store ? B.in_total : B.first.slot_total);
    HIPCHK(hipMemcpy(h_src.data(), d_src.p, h_src.size(), hipMemcpyDeviceToHost));
  }
  for (const ZhFrameEntry &e : T.entry) {
    uint8_t *w = out + e.dst_off;
    memcpy(w, T.blob.data() + e.head_off, e.head_len);
    w += e.head_len;
    uint64_t body = e.body_len;
    if (store) {
      write_store_body(w, sel, h_src.data() + e.src_off, body);
      body = store_body_len(sel.size() + body);
    } else if (e.src == ZH_FRAME_SRC_REDO) {
      if (body) HIPCHK(hipMemcpy(w, B.redo.slots.as<uint8_t>() + e.src_off, body, hipMemcpyDeviceToHost));
    } else if (body) memcpy(w, h_src.data() + e.src_off, body);
    memcpy(w + body, T.blob.data() + e.tail_off, e.tail_len);
  }
  return ZPAQHIP_OK;
}

}  // namespace

extern "C" int zpaqhip_enc_chain_plan(const uint8_t *hdr, size_t hdr_len, uint32_t *waves, uint32_t *lds_bytes, zpaqhip_err *err) {
  if (!hdr || !waves || !lds_bytes) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  ZhModel m;
  std::vector<uint8_t> code;
  const int rc = build_model(hdr, hdr_len, m, code, err);
  if (rc) return rc;
  const ChainPlan p = plan_chain(m);
  *waves = p.waves;
  *lds_bytes = p.lds_bytes;
  return ZPAQHIP_OK;
}

extern "C" int zpaqhip_compress_blocks(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                                       const uint8_t *in, const uint64_t *in_off, size_t n_blocks,
                                       const uint8_t *orig, const uint64_t *orig_off, const char *const *filenames,
                                       uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                                       const zpaqhip_compress_opts *opts, zpaqhip_err *err) {
  CompressCall a;
  a.ctx = ctx; a.hdr = hdr; a.hdr_len = hdr_len; a.pcomp = pcomp; a.pcomp_len = pcomp_len;
  a.in = in; a.in_off = in_off; a.n_blocks = n_blocks; a.orig = orig; a.orig_off = orig_off; a.filenames = filenames;
  a.out = out; a.out_cap = out_cap; a.out_len = out_len; a.block_off = block_off; a.opts = opts; a.err = err;
  return compress_impl(a);
}

extern "C" int zpaqhip_compress_blocks_device(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp,
                                              size_t pcomp_len, const void *d_in, const uint64_t *in_off, size_t n_blocks,
                                              const void *d_orig, const uint64_t *orig_off, const char *const *filenames,
                                              void *d_out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                                              const zpaqhip_compress_opts *opts, void *hip_stream, zpaqhip_err *err) {
  const DeviceEnds dev{(hipStream_t)hip_stream};
  CompressCall a;
  a.ctx = ctx; a.hdr = hdr; a.hdr_len = hdr_len; a.pcomp = pcomp; a.pcomp_len = pcomp_len;
  a.in = (const uint8_t *)d_in; a.in_off = in_off; a.n_blocks = n_blocks; a.orig = (const uint8_t *)d_orig; a.orig_off = orig_off;
  a.filenames = filenames; a.out = (uint8_t *)d_out; a.out_cap = out_cap; a.out_len = out_len; a.block_off = block_off;
  a.opts = opts; a.err = err; a.dev = &dev;
  return compress_impl(a);
}

namespace {

// The solid entry points: the checks of the segment tables, the blocks' view of the per-segment offsets, compress_impl.
// `a` comes with the per-segment in_off and orig_off.
int solid_impl(CompressCall a, const uint64_t *seg_first) {
  zpaqhip_err *const err = a.err;
  const size_t n_blocks = a.n_blocks;
  const uint64_t *const in_off = a.in_off, *const orig_off = a.orig_off;
  if (!a.ctx || !a.hdr || !a.out_len || (!a.out && a.out_cap) || (n_blocks && (!in_off || !seg_first)) || (a.orig && !orig_off)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *a.out_len = 0;
  if (resolve_compress_opts(a.opts).flags & ~3u) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "solid blocks take bits 0 and 1 of flags only (no method opt-ins, no verify)");
    return ZPAQHIP_E_ARG;
  }
  if (n_blocks && seg_first[0] != 0) {
    set_err(err, ZPAQHIP_E_ARG, 0, -1, "seg_first[0] must be 0");
    return ZPAQHIP_E_ARG;
  }
  for (size_t i = 0; i < n_blocks; ++i) {
    if (seg_first[i + 1] <= seg_first[i] || seg_first[i + 1] > 0xFFFFFFFFull) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, seg_first[i + 1] == seg_first[i] ? "a block needs at least one segment" : "seg_first must not decrease");
      return ZPAQHIP_E_ARG;
    }
    for (uint64_t s = seg_first[i]; s < seg_first[i + 1]; ++s)
      if (in_off[s + 1] < in_off[s] || (a.orig && orig_off[s + 1] < orig_off[s])) {
        set_err(err, ZPAQHIP_E_ARG, (int)i, (int)(s - seg_first[i]), "segment offsets must not decrease");
        return ZPAQHIP_E_ARG;
      }
  }
  std::vector<uint64_t> b_in(n_blocks + 1, 0), b_orig(a.orig ? n_blocks + 1 : 0, 0);
  for (size_t i = 0; i <= n_blocks && n_blocks; ++i) {
    b_in[i] = in_off[seg_first[i]];
    if (a.orig) b_orig[i] = orig_off[seg_first[i]];
  }
  const SolidSegs solid{seg_first, in_off, a.orig ? orig_off : nullptr};
  a.in_off = b_in.data();
  a.orig_off = a.orig ? b_orig.data() : nullptr;
  a.solid = &solid;
  return compress_impl(a);
}

}  // namespace

extern "C" int zpaqhip_compress_solid_blocks(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                                             const uint8_t *in, const uint64_t *in_off, const uint64_t *seg_first, size_t n_blocks,
                                             const uint8_t *orig, const uint64_t *orig_off, const char *const *filenames,
                                             uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *block_off,
                                             const zpaqhip_compress_opts *opts, zpaqhip_err *err) {
  CompressCall a;
  a.ctx = ctx; a.hdr = hdr; a.hdr_len = hdr_len; a.pcomp = pcomp; a.pcomp_len = pcomp_len;
  a.in = in; a.in_off = in_off; a.n_blocks = n_blocks; a.orig = orig; a.orig_off = orig_off; a.filenames = filenames;
  a.out = out; a.out_cap = out_cap; a.out_len = out_len; a.block_off = block_off; a.opts = opts; a.err = err;
  return solid_impl(a, seg_first);
}

extern "C" int zpaqhip_compress_solid_blocks_device(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp,
                                                    size_t pcomp_len, const void *d_in, const uint64_t *in_off,
                                                    const uint64_t *seg_first, size_t n_blocks, const void *d_orig,
                                                    const uint64_t *orig_off, const char *const *filenames, void *d_out,
                                                    size_t out_cap, size_t *out_len, uint64_t *block_off,
                                                    const zpaqhip_compress_opts *opts, void *hip_stream, zpaqhip_err *err) {
  const DeviceEnds dev{(hipStream_t)hip_stream};
  CompressCall a;
  a.ctx = ctx; a.hdr = hdr; a.hdr_len = hdr_len; a.pcomp = pcomp; a.pcomp_len = pcomp_len;
  a.in = (const uint8_t *)d_in; a.in_off = in_off; a.n_blocks = n_blocks; a.orig = (const uint8_t *)d_orig; a.orig_off = orig_off;
  a.filenames = filenames; a.out = (uint8_t *)d_out; a.out_cap = out_cap; a.out_len = out_len; a.block_off = block_off;
  a.opts = opts; a.err = err; a.dev = &dev;
  return solid_impl(a, seg_first);
}

int zh::compress_impl(const CompressCall &a) {
  zpaqhip_err *const err = a.err;
  if (!a.ctx || !a.hdr || !a.out_len || (!a.out && a.out_cap) || (a.n_blocks && !a.in_off) || (a.orig && !a.orig_off) ||
      (a.pcomp_len && !a.pcomp) || a.pcomp_len > 65535) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  *a.out_len = 0;
  if (resolve_compress_opts(a.opts).enc_waves > ZH_ENC_CHAIN_MAX_WAVES) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "enc_waves is 0 (automatic) or 1 to 4");
    return ZPAQHIP_E_ARG;
  }
  for (size_t i = 0; i < a.n_blocks; ++i)
    if (a.in_off[i + 1] < a.in_off[i] || (a.orig && a.orig_off[i + 1] < a.orig_off[i]) || (!a.in && a.in_off[i + 1] > a.in_off[i])) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, "block offsets must not decrease");
      return ZPAQHIP_E_ARG;
    }
  Call c(a);
  int rc = build_model(a.hdr, a.hdr_len, c.M, c.code, err);
  if (rc) return rc;
  c.store = c.M.n == 0;
  if (c.store && !a.pre) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1, "compress_blocks codes modelled blocks only (n >= 1)");
    return ZPAQHIP_E_ARG;
  }
  // The store layout splices the selector in on the host: the pre-processing then launches no prefix kernel, which
  // st.launches would count on this path.
  c.sel = selector_prefix(a.pcomp, a.pcomp_len);
  if (!c.store) c.dev_prefix = c.sel;
  if ((rc = c.open())) return rc;
  for (size_t b0 = 0; b0 < a.n_blocks;) {
    Batch B;
    if ((rc = c.plan(B, b0)) || (rc = c.stage(B)) || (rc = c.locate(B)) || (rc = c.digests(B)) || (rc = c.verify(B))) return rc;
    if (!c.store && ((rc = c.encode_batch(B)) || (rc = c.retry(B)))) return rc;
    if ((rc = c.frame(B))) return rc;
    b0 = B.b1;
  }
  // A known wart, kept for zpaqhip_last_stats' sake: the store layout counts the pre-processing launches, the encoders' path
  // counts its own only.
  if (c.store) c.st.launches = a.pre->launches;
  c.st.launches += c.pack_launches + c.verify_launches;
  c.st.kernel_kind = c.store ? 0 : c.any_chain ? 3 : c.any_cm ? 2 : 1;
  if (c.sink) c.sink->used = c.pos;
  return finish_call(c.v, c.st, c.pos, a.n_blocks, a.block_off, c.sink ? ~(size_t)0 : a.out_cap, a.out_len, err);
}
