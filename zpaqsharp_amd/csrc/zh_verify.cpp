// zh_verify.cpp — the verify pass (zh_verify.h) and zpaqhip_verify_blocks[_device].
//
// A round of the pass gives every block a place for what its post-processor writes, launches zh_verify_lz.hip (the decoder's
// wave-wide post-processors over raw bytes, one workgroup per block from a work queue), hands the blocks that kernel does
// not take to zh_verify_vm.hip (the translated programs and the ZPAQL VM), and then hashes (zh_sha1_dev.hip) and compares
// (zh_verify_k.hip) what was written.  The size of a post-processor's output is not known before it ran: a block gets the
// plaintext's length when there is one, else four times its input, and the kernels count past that; a block that wrote more
// goes through a second round with exactly the room it asked for.  Post-processed bytes never leave the device.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "zh_verify.h"

extern "C" hipError_t zh_launch_verify_store(const ZhLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_verify_generic(const ZhLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_verify_compare(const uint8_t *A, const uint8_t *B, const ZhVerifyCmp *blocks, uint32_t n_blocks, uint32_t *queue,
                                               uint64_t *first_diff, hipStream_t stream);
extern "C" hipError_t zh_launch_sha1(const uint8_t *data, const uint64_t *seg, uint32_t n_seg, uint32_t *digest, hipStream_t stream);
extern "C" hipError_t zh_launch_frame_pack(const ZhFrameLaunch *L, hipStream_t stream, uint32_t *launches);

using namespace zh;

static_assert(sizeof(zpaqhip_verify_result) == 48, "zpaqhip_verify_result is 48 bytes");

namespace {

constexpr uint32_t kVerifyBlocks = 256;   // blocks in flight: one per compute unit, as the decoders'

// time between ev0 and ev1 of a finished stream, added to *ms
int add_elapsed(const CtxView &v, double *ms, zpaqhip_err *err) {
  HIPCHK(hipStreamSynchronize(v.stream));
  float t = 0;
  HIPCHK(hipEventElapsedTime(&t, v.ev0, v.ev1));
  *ms += t;
  return ZPAQHIP_OK;
}

}  // namespace

int zh::verify_stage(const CtxView &v, const std::vector<uint8_t> &sel, const uint8_t *d_src, const std::vector<uint64_t> &src_off,
                     const std::vector<uint64_t> &src_len, DevMem &dst, VerifyIn &in, uint32_t *launches, zpaqhip_err *err) {
  const size_t n = src_off.size();
  FrameTable T;
  T.blob = sel;
  in.off.resize(n);
  in.len.resize(n);
  uint64_t total = 0;
  for (size_t j = 0; j < n; ++j) {
    ZhFrameEntry e;
    memset(&e, 0, sizeof e);
    e.dst_off = in.off[j] = total;
    e.head_len = (uint32_t)sel.size();
    e.src = ZH_FRAME_SRC_INPUT;
    e.src_off = src_off[j];
    e.body_len = src_len[j];
    in.len[j] = sel.size() + src_len[j];
    total += align_up(in.len[j], 16);
    T.entry.push_back(e);
    T.pieces = (uint32_t)std::max<uint64_t>(T.pieces, (e.body_len + ZH_FRAME_PIECE - 1) / ZH_FRAME_PIECE);
  }
  HIPCHK(dst.alloc(total + 16));
  in.d_in = dst.as<uint8_t>();
  if (!n) return ZPAQHIP_OK;
  const size_t tb = n * sizeof(ZhFrameEntry);
  std::vector<uint8_t> up(tb + T.blob.size());
  memcpy(up.data(), T.entry.data(), tb);
  memcpy(up.data() + tb, T.blob.data(), T.blob.size());
  DevMem d_tab;
  HIPCHK(d_tab.alloc(up.size() + 16));                  // (+ 16: the kernel reads the blob in aligned 16-byte groups)
  HIPCHK(hipMemcpy(d_tab.p, up.data(), up.size(), hipMemcpyHostToDevice));
  ZhFrameLaunch L;
  memset(&L, 0, sizeof L);
  L.table = d_tab.as<ZhFrameEntry>();
  L.blob = d_tab.as<uint8_t>() + tb;
  L.src[ZH_FRAME_SRC_INPUT] = d_src;
  L.out = dst.as<uint8_t>();
  L.n = (uint32_t)n;
  L.pieces = T.pieces;
  HIPCHK(zh_launch_frame_pack(&L, v.stream, launches));
  HIPCHK(hipStreamSynchronize(v.stream));
  return ZPAQHIP_OK;
}

int zh::verify_pass(const CtxView &v, uint8_t ph, uint8_t pm, const VerifyIn &in, uint64_t mem_budget,
                    std::vector<zpaqhip_verify_result> &rec, double *ms, uint32_t *launches, uint64_t *out_bytes, zpaqhip_err *err) {
  const size_t n = in.off.size();
  const bool cmp = in.d_plain != nullptr;
  zpaqhip_verify_result none;
  memset(&none, 0, sizeof none);
  none.first_diff = ~0ull;
  rec.assign(n, none);
  *out_bytes = 0;
  if (!n) return ZPAQHIP_OK;

  // the post-processor's memories in an arena slot laid out like a decoder's for a block without a model
  const uint8_t hdr[9] = {7, 0, 0, 0, ph, pm, 0, 0, 0};
  ZhModel M;
  std::vector<uint8_t> code;
  if (const int rc = build_model(hdr, sizeof hdr, M, code, err)) return rc;
  const uint64_t stride = align_up(M.arena_bytes, 256);
  if (mem_budget < stride) {
    set_err(err, ZPAQHIP_E_DEVICE_MEM, -1, -1, "Out of memory");
    return ZPAQHIP_E_DEVICE_MEM;
  }
  const uint32_t slots = (uint32_t)std::min<uint64_t>({(uint64_t)n, kVerifyBlocks, mem_budget / stride});

  std::vector<ZhSegDesc> sd(n);
  uint64_t in_end = 0;
  for (size_t i = 0; i < n; ++i) {
    sd[i].in_off = in.off[i];
    sd[i].in_len = in.len[i];
    in_end = std::max(in_end, in.off[i] + in.len[i]);
  }
  DevMem d_model, d_code, d_sd, d_bd, d_res, d_queue, d_arena;
  HIPCHK(d_model.alloc(sizeof(ZhModel)));
  HIPCHK(d_code.alloc(code.size() + 16));
  HIPCHK(d_sd.alloc(n * sizeof(ZhSegDesc)));
  HIPCHK(d_bd.alloc(n * sizeof(ZhBlockDesc)));
  HIPCHK(d_res.alloc(n * sizeof(ZhSegResult)));
  HIPCHK(d_queue.alloc(256));
  HIPCHK(d_arena.alloc((uint64_t)slots * stride));
  HIPCHK(hipMemcpy(d_model.p, &M, sizeof(ZhModel), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_code.p, code.data(), code.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_sd.p, sd.data(), n * sizeof(ZhSegDesc), hipMemcpyHostToDevice));

  ZhLaunch L;
  memset(&L, 0, sizeof L);
  L.in = in.d_in;
  L.in_total = in_end;
  L.models = d_model.as<ZhModel>();
  L.code = d_code.as<uint8_t>();
  L.blocks = d_bd.as<ZhBlockDesc>();
  L.segs = d_sd.as<ZhSegDesc>();
  L.results = d_res.as<ZhSegResult>();
  L.arena = d_arena.as<uint8_t>();
  L.arena_stride = stride;
  L.tables = v.tables;
  L.queue = d_queue.as<uint32_t>();
  L.budget = 1ull << 32;
  L.flags = ZH_LAUNCH_STORE_E8;

  // blocks to run, the longest first (the work queue then balances the tail), and the room each gets
  std::vector<size_t> todo(n);
  std::iota(todo.begin(), todo.end(), (size_t)0);
  std::stable_sort(todo.begin(), todo.end(), [&](size_t a, size_t b) { return in.len[a] > in.len[b]; });
  std::vector<uint64_t> cap(n);
  for (size_t i = 0; i < n; ++i) cap[i] = cmp ? in.plen[i] : 4 * in.len[i] + 4096;

  std::vector<ZhSegResult> res(n);
  for (int round = 0; !todo.empty(); ++round) {
    const size_t nt = todo.size();
    // ---- places: on the plaintext's 16-byte phase, so that the compare reads both in aligned groups
    std::vector<ZhBlockDesc> bd(nt);
    uint64_t total = 0;
    for (size_t k = 0; k < nt; ++k) {
      const size_t i = todo[k];
      const uint64_t phase = cmp ? (uint64_t)((uintptr_t)(in.d_plain + in.poff[i]) & 15) : 0;
      memset(&bd[k], 0, sizeof bd[k]);
      bd[k].first_seg = (uint32_t)i;
      bd[k].n_seg = 1;
      bd[k].out_off = total + phase;
      bd[k].out_cap = cap[i];
      total += align_up(phase + cap[i] + 16, 256);
    }
    DevMem d_out;
    if (d_out.alloc(total + 256) != hipSuccess) {
      (void)hipGetLastError();
      set_err(err, ZPAQHIP_E_DEVICE_MEM, (int)todo[0], -1, "no device memory for the post-processed bytes");
      return ZPAQHIP_E_DEVICE_MEM;
    }
    L.out = d_out.as<uint8_t>();
    HIPCHK(hipMemcpyAsync(d_bd.p, bd.data(), nt * sizeof(ZhBlockDesc), hipMemcpyHostToDevice, v.stream));
    HIPCHK(hipMemsetAsync(d_res.p, 0xff, n * sizeof(ZhSegResult), v.stream));
    HIPCHK(hipMemsetAsync(d_queue.p, 0, 256, v.stream));
    L.n_blocks = (uint32_t)nt;
    HIPCHK(hipEventRecord(v.ev0, v.stream));
    HIPCHK(zh_launch_verify_store(&L, std::min<uint32_t>(slots, L.n_blocks), v.stream));
    HIPCHK(hipEventRecord(v.ev1, v.stream));
    HIPCHK(hipMemcpyAsync(res.data(), d_res.p, n * sizeof(ZhSegResult), hipMemcpyDeviceToHost, v.stream));
    if (const int rc = add_elapsed(v, ms, err)) return rc;
    ++*launches;
    // ---- what the wave-wide kernel handed back: the same places, the complete implementation
    std::vector<ZhBlockDesc> redo;
    for (size_t k = 0; k < nt; ++k)
      if (res[todo[k]].status == ZH_E_RETRY) redo.push_back(bd[k]);
    if (!redo.empty()) {
      HIPCHK(hipMemcpyAsync(d_bd.p, redo.data(), redo.size() * sizeof(ZhBlockDesc), hipMemcpyHostToDevice, v.stream));
      HIPCHK(hipMemsetAsync(d_queue.p, 0, 256, v.stream));
      L.n_blocks = (uint32_t)redo.size();
      HIPCHK(hipEventRecord(v.ev0, v.stream));
      HIPCHK(zh_launch_verify_generic(&L, std::min<uint32_t>(slots, L.n_blocks), v.stream));
      HIPCHK(hipEventRecord(v.ev1, v.stream));
      HIPCHK(hipMemcpyAsync(res.data(), d_res.p, n * sizeof(ZhSegResult), hipMemcpyDeviceToHost, v.stream));
      if (const int rc = add_elapsed(v, ms, err)) return rc;
      ++*launches;
    }
    // ---- the blocks that had room are final; the others go again with what they asked for
    std::vector<size_t> fin, fin_k, again;
    for (size_t k = 0; k < nt; ++k) {
      const size_t i = todo[k];
      if (res[i].out_len > cap[i] && round < 2) { cap[i] = res[i].out_len; again.push_back(i); }
      else { fin.push_back(i); fin_k.push_back(k); }
    }
    const size_t nf = fin.size();
    if (nf) {
      std::vector<uint64_t> seg(2 * nf);
      std::vector<ZhVerifyCmp> cm(nf);
      for (size_t f = 0; f < nf; ++f) {
        const size_t i = fin[f];
        const uint64_t got = std::min(res[i].out_len, cap[i]);
        seg[2 * f] = bd[fin_k[f]].out_off;
        seg[2 * f + 1] = got;
        cm[f] = ZhVerifyCmp{bd[fin_k[f]].out_off, got, cmp ? in.poff[i] : 0, cmp ? in.plen[i] : 0};
      }
      DevMem d_seg, d_dig, d_cm, d_diff;
      HIPCHK(d_seg.alloc(seg.size() * 8));
      HIPCHK(d_dig.alloc(nf * 20));
      HIPCHK(hipMemcpyAsync(d_seg.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice, v.stream));
      std::vector<uint32_t> digest(5 * nf);
      std::vector<uint64_t> diff(nf, ~0ull);
      if (cmp) {
        HIPCHK(d_cm.alloc(nf * sizeof(ZhVerifyCmp)));
        HIPCHK(d_diff.alloc(nf * 8));
        HIPCHK(hipMemcpyAsync(d_cm.p, cm.data(), nf * sizeof(ZhVerifyCmp), hipMemcpyHostToDevice, v.stream));
        HIPCHK(hipMemsetAsync(d_queue.p, 0, 256, v.stream));
      }
      HIPCHK(hipEventRecord(v.ev0, v.stream));
      HIPCHK(zh_launch_sha1(d_out.as<uint8_t>(), d_seg.as<uint64_t>(), (uint32_t)nf, d_dig.as<uint32_t>(), v.stream));
      ++*launches;
      if (cmp) {
        HIPCHK(zh_launch_verify_compare(d_out.as<uint8_t>(), in.d_plain, d_cm.as<ZhVerifyCmp>(), (uint32_t)nf, d_queue.as<uint32_t>(),
                                        d_diff.as<uint64_t>(), v.stream));
        ++*launches;
      }
      HIPCHK(hipEventRecord(v.ev1, v.stream));
      HIPCHK(hipMemcpyAsync(digest.data(), d_dig.p, nf * 20, hipMemcpyDeviceToHost, v.stream));
      if (cmp) HIPCHK(hipMemcpyAsync(diff.data(), d_diff.p, nf * 8, hipMemcpyDeviceToHost, v.stream));
      if (const int rc = add_elapsed(v, ms, err)) return rc;
      for (size_t f = 0; f < nf; ++f) {
        const size_t i = fin[f];
        zpaqhip_verify_result &r = rec[i];
        r.status = res[i].status == ZH_E_OUTPUT_FULL ? ZPAQHIP_OK : res[i].status;
        r.out_len = res[i].out_len;
        for (int w = 0; w < 5; ++w)
          for (int b = 0; b < 4; ++b) r.sha1[4 * w + b] = (uint8_t)(digest[5 * f + w] >> (24 - 8 * b));
        if (res[i].out_len > cap[i]) {                   // (a post-processor whose output grew between two rounds: never seen)
          set_err(err, ZPAQHIP_E_HIP, (int)i, -1, "post-processed block exceeds the room it asked for");
          return ZPAQHIP_E_HIP;
        }
        if (cmp) {
          r.first_diff = diff[f];
          if (r.status == ZPAQHIP_OK && diff[f] != ~0ull) r.status = ZPAQHIP_E_VERIFY;
        }
        *out_bytes += r.out_len;
      }
    }
    todo.swap(again);
  }
  return ZPAQHIP_OK;
}

namespace {

int verify_entry(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len, const uint8_t *in,
                 const uint64_t *in_off, size_t n_blocks, const uint8_t *orig, const uint64_t *orig_off, zpaqhip_verify_result *results,
                 bool dev, hipStream_t stream, zpaqhip_err *err) {
  if (!ctx || !hdr || (n_blocks && (!in_off || !results)) || (orig && !orig_off) || (pcomp_len && !pcomp) || pcomp_len > 65535) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  for (size_t i = 0; i < n_blocks; ++i)
    if (in_off[i + 1] < in_off[i] || (orig && orig_off[i + 1] < orig_off[i]) || (!in && in_off[i + 1] > in_off[i])) {
      set_err(err, ZPAQHIP_E_ARG, (int)i, -1, "block offsets must not decrease");
      return ZPAQHIP_E_ARG;
    }
  ZhModel M;
  std::vector<uint8_t> code;
  if (const int rc = build_model(hdr, hdr_len, M, code, err)) return rc;
  CtxView v = ctx_view(ctx);
  if (stream) v.stream = stream;
  HIPCHK(hipSetDevice(v.device));
  zpaqhip_stats st{};
  st.blocks = n_blocks;
  uint64_t budget = 0;
  HIPCHK(device_budget(v.mem_share, 0, &budget));
  const std::vector<uint8_t> sel = selector_prefix(pcomp, pcomp_len);

  // batches as the compressing calls size them: the staged copy, the post-processed bytes and the plaintext of a block
  auto cost = [&](size_t i) {
    const uint64_t a = in_off[i + 1] - in_off[i];
    return 2 * a + (orig ? 2 * (orig_off[i + 1] - orig_off[i]) : 4 * a) + 8192;
  };
  for (size_t b0 = 0; b0 < n_blocks;) {
    const size_t b1 = batch_end(b0, n_blocks, 0, budget, cost), nb = b1 - b0;
    std::vector<uint64_t> so(nb), sl(nb);
    DevMem d_src, d_stage, d_orig;
    const uint8_t *src = in;
    for (size_t j = 0; j < nb; ++j) { so[j] = in_off[b0 + j]; sl[j] = in_off[b0 + j + 1] - in_off[b0 + j]; }
    if (!dev) {                                          // the batch's bytes go up as they lie
      const uint64_t base = in_off[b0], bytes = in_off[b1] - base;
      HIPCHK(d_src.alloc(bytes + 16));
      if (bytes) HIPCHK(hipMemcpy(d_src.p, in + base, bytes, hipMemcpyHostToDevice));
      src = d_src.as<uint8_t>();
      for (size_t j = 0; j < nb; ++j) so[j] -= base;
    }
    VerifyIn vin;
    if (const int rc = verify_stage(v, sel, src, so, sl, d_stage, vin, &st.launches, err)) return rc;
    if (orig) {
      vin.poff.resize(nb);
      vin.plen.resize(nb);
      for (size_t j = 0; j < nb; ++j) { vin.poff[j] = orig_off[b0 + j]; vin.plen[j] = orig_off[b0 + j + 1] - orig_off[b0 + j]; }
      vin.d_plain = orig;
      if (!dev) {
        const uint64_t base = orig_off[b0], bytes = orig_off[b1] - base;
        HIPCHK(d_orig.alloc(bytes + 16));
        if (bytes) HIPCHK(hipMemcpy(d_orig.p, orig + base, bytes, hipMemcpyHostToDevice));
        vin.d_plain = d_orig.as<uint8_t>();
        for (size_t j = 0; j < nb; ++j) vin.poff[j] -= base;
      }
    }
    std::vector<zpaqhip_verify_result> rec;
    uint64_t wrote = 0;
    if (const int rc = verify_pass(v, M.ph, M.pm, vin, budget / 4, rec, &st.kernel_ms, &st.launches, &wrote, err)) {
      if (err && err->block >= 0) err->block += (int32_t)b0;
      return rc;
    }
    std::copy(rec.begin(), rec.end(), results + b0);
    st.in_bytes += in_off[b1] - in_off[b0];
    st.out_bytes += wrote;
    b0 = b1;
  }
  *v.stats = st;
  return ZPAQHIP_OK;
}

}  // namespace

extern "C" int zpaqhip_verify_blocks(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                                     const uint8_t *in, const uint64_t *in_off, size_t n_blocks, const uint8_t *orig,
                                     const uint64_t *orig_off, zpaqhip_verify_result *results, zpaqhip_err *err) {
  return verify_entry(ctx, hdr, hdr_len, pcomp, pcomp_len, in, in_off, n_blocks, orig, orig_off, results, false, nullptr, err);
}

extern "C" int zpaqhip_verify_blocks_device(zpaqhip_ctx *ctx, const uint8_t *hdr, size_t hdr_len, const uint8_t *pcomp, size_t pcomp_len,
                                            const void *d_in, const uint64_t *in_off, size_t n_blocks, const void *d_orig,
                                            const uint64_t *orig_off, zpaqhip_verify_result *results, void *hip_stream,
                                            zpaqhip_err *err) {
  return verify_entry(ctx, hdr, hdr_len, pcomp, pcomp_len, (const uint8_t *)d_in, in_off, n_blocks, (const uint8_t *)d_orig, orig_off,
                      results, true, (hipStream_t)hip_stream, err);
}
