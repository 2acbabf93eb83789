// zh_api.cpp — C-ABI entry points of libzpaqhip.so (include/zpaqhip.h) and the
// host driver that turns a block table into kernel launches.
//
// There is deliberately no CPU decode path in this file or library: every
// decoded byte comes out of a HIP kernel, and every entry point that needs a
// GPU fails with ZPAQHIP_E_NO_DEVICE when none is usable.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "zh_compress.h"
#include "zh_ctx_view.h"
#include "zh_dec_plan.h"
#include "zh_frame.h"
#include "zh_host.h"
#include "zh_scan.h"
#include "zh_stream_plan.h"
#include "zh_zpaql_native.h"

extern "C" hipError_t zh_launch_generic(const ZhLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_cm(const ZhLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_cm_x2(const ZhLaunch *L, uint32_t grid, hipStream_t stream);   // two blocks per workgroup
extern "C" hipError_t zh_launch_sha1(const uint8_t *data, const uint64_t *seg, uint32_t n_seg, uint32_t *digest, hipStream_t stream);
extern "C" hipError_t zh_launch_chain(const ZhLaunch *L, uint32_t grid, hipStream_t stream, uint32_t spec, int prof, int pcall);
extern "C" hipError_t zh_launch_chain_mw(const ZhLaunch *L, const ZhChainWaves *V, uint32_t grid, hipStream_t stream, int pcall);
extern "C" hipError_t zh_launch_cm_prof(const ZhLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_chain2(const ZhLaunch *L, uint32_t grid, hipStream_t stream, uint32_t spec, int prof);
extern "C" int zh_chain2_has(uint32_t spec);
extern "C" hipError_t zh_launch_nibble(const ZhLaunch *L, uint32_t grid, hipStream_t stream, uint32_t spec, int prof);
extern "C" int zh_nibble_has(uint32_t spec);
extern "C" hipError_t zh_launch_store(const ZhLaunch *L, uint32_t grid, hipStream_t stream);
extern "C" hipError_t zh_launch_frame_pack(const ZhFrameLaunch *L, hipStream_t stream, uint32_t *launches);


using namespace zh;

namespace {

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

struct zpaqhip_ctx {
  int device = 0;
  int cus = 0;                            // compute units: a several-waves launch of zh_chain puts one workgroup on each
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DevBuf tables, arena, models, code, bdesc, sdesc, results, queue, in, out;
  // whole-stream pipeline (created on first use): copy streams, double-buffered device input / staging / second-pass
  // buffers, pinned chunks for the Writer callback
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_pin[2] = {nullptr, nullptr}, ev_h0 = nullptr, ev_h1 = nullptr;
  hipEvent_t ev_d[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // D2H of a batch slot: first copy enqueued / last copy done
  bool d_pending[2] = {false, false};
  float d2h_acc = 0;
  DevBuf in2[2], out2[2], out_fix[2];
  uint8_t *pin[2] = {nullptr, nullptr};
  zpaqhip_stats stats{};
  uint32_t mem_share = 1;                 // contexts of this process that share the device (zpaqhip_decompress_multi): divides the memory budgets
  // a launch whose blocks need several kernel families (an archive that mixes models): one stream per family, forked from
  // and joined to the launch stream, each family with its own region of the arena
  hipStream_t fam_stream[ZH_NFAM_HOST] = {};
  hipEvent_t fam_ev[ZH_NFAM_HOST] = {};
  hipEvent_t fork_ev = nullptr;
  // zpaqhip_scan_device: per-piece counts with totals and result, the lists, the per-hit records, the block and segment tables;
  // zpaqhip_decompress_device: the table of the packing kernel
  DevBuf scan_cnt, scan_list, scan_rec, scan_blk, scan_seg, pack_tab;
  std::vector<uint32_t> raw_pp;           // last decode: per segment pp_state | PCOMP length << 8, as the kernels report it
};

namespace {

constexpr size_t kQueueBytes = 512, kDebugBytes = 128;    // work-queue heads (32 B per family) and the *_prof kernels' sums
constexpr uint64_t kPpOnlyMagic = 0x5A50505F4F4E4C59ull;   // internal: zpaqhip_block_pcomp -> decode_blocks_device ("ZPP_ONLY")

zpaqhip_opts resolve_opts(const zpaqhip_opts *o) {
  zpaqhip_opts r;
  memset(&r, 0, sizeof r);
  if (o) memcpy(&r, o, std::min<size_t>(sizeof r, o->struct_size ? o->struct_size : sizeof r));
  if (!r.zpaql_budget) r.zpaql_budget = 1ull << 32;
  if (r.dec_waves > ZH_DEC_CHAIN_MAX_WAVES) r.dec_waves = ZH_DEC_CHAIN_MAX_WAVES;
  return r;
}

const ZhKernelHas kKernelHas = {zh_nibble_has, zh_chain2_has};   // route_block: what the kernels are built with

}  // namespace

extern "C" {

int zpaqhip_version(void) { return ZPAQHIP_ABI_VERSION; }

const char *zpaqhip_strerror(int status) { return status_message(status); }

int zpaqhip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int zpaqhip_ctx_create(int device, zpaqhip_ctx **out, zpaqhip_err *err) {
  if (!out) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  *out = nullptr;
  if (!host_tables_ok()) {
    set_err(err, ZPAQHIP_E_NO_DEVICE, -1, -1, "model tables failed their reference checksums");
    return ZPAQHIP_E_NO_DEVICE;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    set_err(err, ZPAQHIP_E_NO_DEVICE, -1, -1);
    return ZPAQHIP_E_NO_DEVICE;
  }
  HIPCHK(hipSetDevice(device));
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  zpaqhip_ctx *c = new zpaqhip_ctx();
  c->device = device;
  c->cus = std::max(1, cus);
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess ||
      (e = c->tables.reserve(sizeof(ZhTables) + sizeof(ZhTablesX))) != hipSuccess ||
      (e = hipMemcpy(c->tables.p, &host_tables(), sizeof(ZhTables), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy((uint8_t *)c->tables.p + sizeof(ZhTables), &host_tables_x(), sizeof(ZhTablesX), hipMemcpyHostToDevice)) != hipSuccess) {
    char m[112];
    snprintf(m, sizeof m, "HIP: %s (context setup)", hipGetErrorString(e));
    set_err(err, ZPAQHIP_E_HIP, -1, -1, m);
    zpaqhip_ctx_destroy(c);
    return ZPAQHIP_E_HIP;
  }
  *out = c;
  return ZPAQHIP_OK;
}

void zpaqhip_ctx_destroy(zpaqhip_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (DevBuf *b : {&c->tables, &c->arena, &c->models, &c->code, &c->bdesc, &c->sdesc, &c->results, &c->queue, &c->in, &c->out,
                    &c->in2[0], &c->in2[1], &c->out2[0], &c->out2[1], &c->out_fix[0], &c->out_fix[1], &c->scan_cnt, &c->scan_list, &c->scan_rec,
                    &c->scan_blk, &c->scan_seg, &c->pack_tab})
    b->release();
  for (int i = 0; i < 2; ++i) {
    if (c->pin[i]) (void)hipHostFree(c->pin[i]);
    if (c->ev_in[i]) (void)hipEventDestroy(c->ev_in[i]);
    if (c->ev_pin[i]) (void)hipEventDestroy(c->ev_pin[i]);
    for (int k = 0; k < 2; ++k) if (c->ev_d[i][k]) (void)hipEventDestroy(c->ev_d[i][k]);
  }
  if (c->ev_h0) (void)hipEventDestroy(c->ev_h0);
  if (c->ev_h1) (void)hipEventDestroy(c->ev_h1);
  if (c->s_in) (void)hipStreamDestroy(c->s_in);
  if (c->s_out) (void)hipStreamDestroy(c->s_out);
  for (uint32_t g = 0; g < ZH_NFAM_HOST; ++g) {
    if (c->fam_ev[g]) (void)hipEventDestroy(c->fam_ev[g]);
    if (c->fam_stream[g]) (void)hipStreamDestroy(c->fam_stream[g]);
  }
  if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int zpaqhip_last_stats(const zpaqhip_ctx *c, zpaqhip_stats *out) {
  if (!c || !out) return ZPAQHIP_E_ARG;
  *out = c->stats;
  return ZPAQHIP_OK;
}

int zpaqhip_scan(const uint8_t *in, size_t in_len, zpaqhip_block *blocks, size_t block_cap, size_t *n_blocks,
                 zpaqhip_segment *segs, size_t seg_cap, size_t *n_segs, zpaqhip_err *err) {
  if ((!in && in_len) || !n_blocks || !n_segs) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  ScanOut so;
  zpaqhip_err e2{};
  const int rc = scan_stream(in, in_len, so, &e2);
  // On a framing error the blocks before the damage are still handed back (counts and tables), with the error code:
  // the reference's Decompresser delivers them too and only fails on reaching the damaged block.
  *n_blocks = so.blocks.size();
  *n_segs = so.segs.size();
  if (so.blocks.size() > block_cap || so.segs.size() > seg_cap) {
    if (block_cap || seg_cap) { set_err(err, ZPAQHIP_E_ARG, -1, -1, "block/segment table too small"); return ZPAQHIP_E_ARG; }
    if (rc && err) *err = e2;
    return rc;
  }
  if (blocks && !so.blocks.empty()) memcpy(blocks, so.blocks.data(), so.blocks.size() * sizeof(zpaqhip_block));
  if (segs && !so.segs.empty()) memcpy(segs, so.segs.data(), so.segs.size() * sizeof(zpaqhip_segment));
  if (rc && err) *err = e2;
  return rc;
}

int zpaqhip_read_device_tables(zpaqhip_ctx *c, uint16_t *squash, int16_t *stretch, int32_t *dt, int32_t *dt2k,
                               uint8_t *ns, zpaqhip_err *err) {
  if (!c) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint8_t> buf(sizeof(ZhTables));
  HIPCHK(hipMemcpy(buf.data(), c->tables.p, sizeof(ZhTables), hipMemcpyDeviceToHost));
  const ZhTables *t = reinterpret_cast<const ZhTables *>(buf.data());
  if (squash) memcpy(squash, t->squash, sizeof t->squash);
  if (stretch) memcpy(stretch, t->stretch, sizeof t->stretch);
  if (dt) memcpy(dt, t->dt, sizeof t->dt);
  if (dt2k) memcpy(dt2k, t->dt2k, sizeof t->dt2k);
  if (ns) memcpy(ns, t->ns, sizeof t->ns);
  return ZPAQHIP_OK;
}

}  // extern "C"

// `h_hdrs`: the block headers are needed on the host to build the model
// descriptors; they are fetched from the device stream (a few hundred bytes per
// distinct model) so the ABI stays a pure device-buffer interface.
// The call has two halves so that the whole-stream forms can keep the host busy (callbacks, scanning, copies of the
// neighbouring batches) while a batch's kernels run: decode_launch() enqueues everything on `stream` and returns,
// decode_finish() waits for the stream and turns the device results into zpaqhip_seg_result records.  One launch may be
// outstanding per context (the descriptor / result / arena buffers belong to the context).
static size_t pool_trim_device(int device, size_t keep);   // idle contexts of zpaqhip_decompress_multi's pool (below)

struct GroupLaunch {                      // what one kernel group of a launch was started with
  ZhLaunch L{};                           // (L.n_blocks: the group's blocks)
  size_t base = 0;                        // its first descriptor in bd_sorted
  uint32_t slots = 0;
};

struct zh_pending {
  std::vector<uint32_t> sel;
  const zpaqhip_block *blocks = nullptr;
  const zpaqhip_segment *segs = nullptr;
  size_t n_segs = 0;
  hipStream_t stream = nullptr;
  uint64_t total_in = 0, total_model = 0;
  bool active = false;
  // sources of the launch's asynchronous H2D copies: they must outlive decode_launch (the API does not promise that a
  // pageable hipMemcpyAsync has read its source when it returns)
  std::vector<ZhModel> models;
  std::vector<uint8_t> code;
  std::vector<ZhSegDesc> sd;
  DecPlan plan;                                         // (its bd_sorted)
  // zh_store.hip hands blocks it does not take (ZH_E_RETRY) back: they run on the generic kernel in decode_finish
  bool has_store = false;
  GroupLaunch store;
  bool e8_wave = false;                                 // a launch had ZH_LAUNCH_MODEL_E8: word 1 of its work-queue head counts segments
};

// Step 1 of decode_launch: the headers of the selected blocks read, one model per distinct header built (P.models, P.code),
// and per block its descriptor and weight (coded bytes), per segment its descriptor (P.sd); the totals of the statistics.
static int collect_models(const void *d_in, const uint8_t *h_in, size_t in_len, const uint64_t *out_off, const uint64_t *out_cap,
                          zh_pending &P, std::vector<ZhBlockDesc> &bd, std::vector<uint64_t> &weight, zpaqhip_err *err) {
  const std::vector<uint32_t> &sel = P.sel;
  const zpaqhip_block *blocks = P.blocks;
  const zpaqhip_segment *segs = P.segs;
  const size_t n_segs = P.n_segs;
  std::map<std::string, uint32_t> model_of;
  std::vector<ZhModel> &models = P.models;
  std::vector<uint8_t> &code = P.code;
  bd.assign(sel.size(), ZhBlockDesc{});
  std::vector<ZhSegDesc> &sd = P.sd;
  sd.assign(n_segs, ZhSegDesc{});
  std::vector<uint8_t> hdr;
  uint64_t &total_in = P.total_in, &total_model = P.total_model;
  for (size_t k = 0; k < sel.size(); ++k) {
    const zpaqhip_block &b = blocks[sel[k]];
    if (b.hdr_off + b.hdr_len > in_len || (uint64_t)b.first_seg + b.n_seg > n_segs) {
      set_err(err, ZPAQHIP_E_ARG, (int)sel[k], -1, "block table does not match the stream");
      return ZPAQHIP_E_ARG;
    }
    hdr.resize(b.hdr_len);
    if (h_in) memcpy(hdr.data(), h_in + b.hdr_off, b.hdr_len);
    else HIPCHK(hipMemcpy(hdr.data(), (const uint8_t *)d_in + b.hdr_off, b.hdr_len, hipMemcpyDeviceToHost));
    std::string key((const char *)hdr.data(), hdr.size());
    auto it = model_of.find(key);
    if (it == model_of.end()) {
      ZhModel m;
      int rc = build_model(hdr.data(), hdr.size(), m, code, err);
      if (rc) { if (err) err->block = (int)sel[k]; return rc; }
      it = model_of.emplace(key, (uint32_t)models.size()).first;
      models.push_back(m);
    }
    const ZhModel &m = models[it->second];
    total_model += m.arena_bytes;
    bd[k].model = it->second;
    bd[k].first_seg = b.first_seg;
    bd[k].n_seg = b.n_seg;
    bd[k].out_off = out_off ? out_off[k] : 0;
    bd[k].out_cap = out_cap ? out_cap[k] : 0;
    for (uint32_t s = 0; s < b.n_seg; ++s) {
      const zpaqhip_segment &sg = segs[b.first_seg + s];
      if (sg.data_off + sg.data_len > in_len) {
        set_err(err, ZPAQHIP_E_ARG, (int)sel[k], (int)(b.first_seg + s), "segment table does not match the stream");
        return ZPAQHIP_E_ARG;
      }
      sd[b.first_seg + s].in_off = sg.data_off;
      sd[b.first_seg + s].in_len = sg.data_len;
      total_in += sg.data_len;
    }
  }
  weight.assign(sel.size(), 0);
  for (size_t k = 0; k < sel.size(); ++k)
    for (uint32_t i = 0; i < bd[k].n_seg; ++i) weight[k] += sd[bd[k].first_seg + i].in_len;
  return ZPAQHIP_OK;
}

// Step 4 of decode_launch: the kernel of one group (plan_decode chose it and its shape), launched on `stream`.
static int launch_group(zh_pending &P, const DecPlan &plan, const DecGroup &g, const ZhLaunch &L, hipStream_t stream, zpaqhip_err *err) {
  const ZhRoute &r = g.route;
  switch (r.kernel) {
    case ZhKernel::Generic: HIPCHK(zh_launch_generic(&L, g.grid(), stream)); break;
    case ZhKernel::Store:
      HIPCHK(zh_launch_store(&L, g.grid(), stream));
      P.has_store = true; P.store = {L, g.base, g.slots};
      break;
    case ZhKernel::Cm:
      if (plan.prof) HIPCHK(zh_launch_cm_prof(&L, g.grid(), stream));
      else if (g.cm_x2) HIPCHK(zh_launch_cm_x2(&L, g.grid(), stream));
      else HIPCHK(zh_launch_cm(&L, g.grid(), stream));
      break;
    case ZhKernel::Chain:
      if (g.mw.waves > 1) HIPCHK(zh_launch_chain_mw(&L, &g.mw, g.grid(), stream, g.pcall));
      else HIPCHK(zh_launch_chain(&L, g.grid(), stream, r.spec, plan.prof, g.pcall));
      break;
    case ZhKernel::Chain2: HIPCHK(zh_launch_chain2(&L, g.grid(), stream, r.spec, plan.prof)); break;   // per-model bit loop
    case ZhKernel::Nibble: HIPCHK(zh_launch_nibble(&L, g.grid(), stream, r.spec, plan.prof)); break;   // a nibble at a time
  }
  P.e8_wave |= (r.flags & ZH_LAUNCH_MODEL_E8) != 0;
  return ZPAQHIP_OK;
}

// Four steps: collect_models; plan_decode (zh_dec_plan.h: every decision about slots, waves, workgroups and the arena); the
// buffers reserved and the tables and descriptors uploaded; launch_group for every group of the plan.
static int decode_launch(zpaqhip_ctx *c, const void *d_in, const uint8_t *h_in, size_t in_len,
                                 const zpaqhip_block *blocks,
                                 size_t n_blocks, const zpaqhip_segment *segs, size_t n_segs, const uint32_t *ids,
                                 size_t n_ids, void *d_out, const uint64_t *out_off, const uint64_t *out_cap,
                                 const zpaqhip_opts &opts, hipStream_t stream, zh_pending &P,
                                 zpaqhip_err *err) {
  P = zh_pending();
  P.blocks = blocks; P.segs = segs; P.n_segs = n_segs; P.stream = stream;
  HIPCHK(hipSetDevice(c->device));
  memset(&c->stats, 0, sizeof c->stats);

  std::vector<uint32_t> &sel = P.sel;
  if (ids) sel.assign(ids, ids + n_ids);
  else { sel.resize(n_blocks); std::iota(sel.begin(), sel.end(), 0u); }
  if (sel.empty()) return ZPAQHIP_OK;
  for (uint32_t b : sel)
    if (b >= n_blocks) { set_err(err, ZPAQHIP_E_ARG, (int)b, -1, "block id out of range"); return ZPAQHIP_E_ARG; }

  // ---- 1. models: one per distinct header
  std::vector<ZhBlockDesc> bd;
  std::vector<uint64_t> weight;
  if (int rc = collect_models(d_in, h_in, in_len, out_off, out_cap, P, bd, weight, err)) return rc;
  const std::vector<ZhModel> &models = P.models;
  const std::vector<uint8_t> &code = P.code;
  const std::vector<ZhSegDesc> &sd = P.sd;

  // ---- 2. the plan
  const bool pp_only = opts.reserved[0] == kPpOnlyMagic;        // the library's own use of the reserved word (zpaqhip_block_pcomp)
  const bool prof = getenv("ZPAQHIP_PROF") != nullptr;   // diagnostic build with in-kernel stamps
  std::vector<DecGroup> groups = group_blocks(models, bd, opts, pp_only, kKernelHas);
  uint64_t mem_budget = 0;
  HIPCHK(device_budget(c->mem_share, c->arena.cap, &mem_budget));     // our own cached arena is reusable
  // Idle contexts zpaqhip_decompress_multi has pooled on this device keep their arenas (tens of GB for the larger models).
  // If this launch could not give every block (up to kDecBlocks) its slot, they are released first and the budget taken again
  // (multi([0,0,0,0]) followed by a max-model decode on a context of one's own saw a quarter of the memory).
  if (arena_wish(groups, opts) > mem_budget && pool_trim_device(c->device, 0))
    HIPCHK(device_budget(c->mem_share, c->arena.cap, &mem_budget));
  DecPlan &plan = P.plan;
  if (int rc = plan_decode(std::move(groups), models, bd, weight, opts, prof, (uint32_t)c->cus, mem_budget,
                           getenv("ZPAQHIP_SERIAL_FAMILIES") != nullptr, plan, err))
    return rc;

  // ---- 3. buffers, tables and descriptors
  HIPCHK(c->models.reserve(models.size() * sizeof(ZhModel)));
  HIPCHK(c->code.reserve(code.size() + 16));
  HIPCHK(c->bdesc.reserve(sel.size() * sizeof(ZhBlockDesc)));
  HIPCHK(c->sdesc.reserve(sd.size() * sizeof(ZhSegDesc)));
  HIPCHK(c->results.reserve(n_segs * sizeof(ZhSegResult)));
  static_assert(32 * ZH_NFAM_HOST <= kQueueBytes, "one 32-byte work-queue head per kernel family");
  HIPCHK(c->queue.reserve(kQueueBytes + kDebugBytes));   // [heads | diagnostic cycle sums]: the two never overlap
  HIPCHK(hipMemcpyAsync(c->models.p, models.data(), models.size() * sizeof(ZhModel), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(c->code.p, code.data(), code.size(), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(c->sdesc.p, sd.data(), sd.size() * sizeof(ZhSegDesc), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(c->results.p, 0xff, n_segs * sizeof(ZhSegResult), stream));
  HIPCHK(hipMemsetAsync(c->queue.p, 0, kQueueBytes + kDebugBytes, stream));

  HIPCHK(c->arena.reserve((size_t)plan.arena_bytes));
  if (plan.side_by_side && !c->fork_ev) HIPCHK(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
  HIPCHK(hipMemcpyAsync(c->bdesc.p, plan.bd_sorted.data(), plan.bd_sorted.size() * sizeof(ZhBlockDesc), hipMemcpyHostToDevice, stream));

  // ---- 4. one launch per group: on the launch stream one after the other, or side by side on the families' own streams,
  // forked from the launch stream and joined to it
  HIPCHK(hipEventRecord(c->ev0, stream));
  if (plan.side_by_side) HIPCHK(hipEventRecord(c->fork_ev, stream));      // the tables and descriptors above are on `stream`
  for (const DecGroup &g : plan.groups) {
    const uint32_t f = g.route.group;
    hipStream_t gs = stream;
    if (plan.side_by_side) {
      if (!c->fam_stream[f]) {
        HIPCHK(hipStreamCreateWithFlags(&c->fam_stream[f], hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->fam_ev[f], hipEventDisableTiming));
      }
      gs = c->fam_stream[f];
      HIPCHK(hipStreamWaitEvent(gs, c->fork_ev, 0));
    }
    ZhLaunch L;
    memset(&L, 0, sizeof L);
    L.in = (const uint8_t *)d_in;
    L.in_total = in_len;
    L.models = (const ZhModel *)c->models.p;
    L.code = (const uint8_t *)c->code.p;
    L.blocks = (const ZhBlockDesc *)c->bdesc.p + g.base;
    L.segs = (const ZhSegDesc *)c->sdesc.p;
    L.results = (ZhSegResult *)c->results.p;
    L.out = (uint8_t *)d_out;
    L.arena = (uint8_t *)c->arena.p + g.arena_off;
    L.arena_stride = g.stride;
    L.tables = (const ZhTables *)c->tables.p;
    L.queue = (uint32_t *)c->queue.p + 8 * f;           // one work-queue head per launch
    L.n_blocks = (uint32_t)g.blocks.size();
    L.budget = opts.zpaql_budget;
    L.flags = (pp_only ? ZH_LAUNCH_PP_ONLY : 0u) | g.route.flags;
    if (prof) L.debug = (uint64_t *)((uint8_t *)c->queue.p + kQueueBytes);
    if (int rc = launch_group(P, plan, g, L, gs, err)) return rc;
    if (plan.side_by_side) {                             // join: the launch stream goes on when every family is done
      HIPCHK(hipEventRecord(c->fam_ev[f], gs));
      HIPCHK(hipStreamWaitEvent(stream, c->fam_ev[f], 0));
    }
  }
  HIPCHK(hipEventRecord(c->ev1, stream));
  P.active = true;
  return ZPAQHIP_OK;
}

static int decode_finish(zpaqhip_ctx *c, zh_pending &P, zpaqhip_seg_result *results, zpaqhip_err *err) {
  if (!P.active) return ZPAQHIP_OK;                     // nothing was selected
  P.active = false;
  const std::vector<uint32_t> &sel = P.sel;
  const zpaqhip_block *blocks = P.blocks;
  const zpaqhip_segment *segs = P.segs;
  const size_t n_segs = P.n_segs;
  hipStream_t stream = P.stream;
  const uint64_t total_in = P.total_in, total_model = P.total_model;
  const uint32_t launches = P.plan.launches, slots = P.plan.concurrent, kind_used = P.plan.kernel_kind;
  if (P.plan.prof) {
    uint64_t dbg[16];
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(dbg, (uint8_t *)c->queue.p + kQueueBytes, kDebugBytes, hipMemcpyDeviceToHost));
    fprintf(stderr, "ZPAQHIP_PROF cycles:");
    for (int i = 0; i < 16; ++i) fprintf(stderr, " %llu", (unsigned long long)dbg[i]);
    fprintf(stderr, "\n");
  }
  std::vector<ZhSegResult> res(n_segs);
  c->raw_pp.assign(n_segs, 0);
  HIPCHK(hipMemcpyAsync(res.data(), c->results.p, n_segs * sizeof(ZhSegResult), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  uint32_t extra_launches = 0;
  if (P.has_store) {
    // blocks the store kernel handed back (programs other than the reference's LZ77 ones, damaged chunks): the generic
    // kernel is the complete implementation.  Same arena slots, same output places.
    std::vector<ZhBlockDesc> redo;
    for (size_t k = 0; k < P.store.L.n_blocks; ++k) {
      const ZhBlockDesc &b = P.plan.bd_sorted[P.store.base + k];
      if (b.n_seg && res[b.first_seg].status == ZH_E_RETRY) redo.push_back(b);
    }
    if (!redo.empty()) {
      ZhLaunch L = P.store.L;
      HIPCHK(hipMemcpyAsync((void *)L.blocks, redo.data(), redo.size() * sizeof(ZhBlockDesc), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemsetAsync(L.queue, 0, 32, stream));
      L.n_blocks = (uint32_t)redo.size();
      HIPCHK(hipEventRecord(c->ev0, stream));
      HIPCHK(zh_launch_generic(&L, std::min<uint32_t>(P.store.slots, L.n_blocks), stream));
      HIPCHK(hipEventRecord(c->ev1, stream));
      HIPCHK(hipMemcpyAsync(res.data(), c->results.p, n_segs * sizeof(ZhSegResult), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      float ms2 = 0;
      HIPCHK(hipEventElapsedTime(&ms2, c->ev0, c->ev1));
      ms += ms2;
      ++extra_launches;
    }
  }

  int first_bad = ZPAQHIP_OK;
  uint64_t total_out = 0;
  for (size_t k = 0; k < sel.size(); ++k) {
    const zpaqhip_block &b = blocks[sel[k]];
    for (uint32_t s = 0; s < b.n_seg; ++s) {
      const uint32_t si = b.first_seg + s;
      if (res[si].status == ZH_E_STOPPED) res[si].status = ZPAQHIP_OK, res[si].in_used = segs[si].data_len;   // ended on request
      results[si].status = res[si].status;
      results[si].pp_state = res[si].pp_state & 255u;
      c->raw_pp[si] = res[si].pp_state;
      results[si].out_off = res[si].out_off;
      results[si].out_len = res[si].out_len;
      results[si].in_used = res[si].in_used;
      // A decoder that stopped anywhere but at the scanned end of the coded data means a
      // damaged stream: the reference would now read its end-of-segment marker from the
      // wrong place (Decompresser.cs:163-194).
      if (res[si].status == ZPAQHIP_OK && res[si].in_used != segs[si].data_len) results[si].status = res[si].status = ZPAQHIP_E_SEGEND;
      total_out += res[si].out_len;
      if (res[si].status != ZPAQHIP_OK && res[si].status != ZPAQHIP_E_OUTPUT_FULL && first_bad == ZPAQHIP_OK &&
          res[si].status != ZH_E_SKIPPED) {
        first_bad = res[si].status;
        set_err(err, first_bad, (int)sel[k], (int)si);
      }
    }
  }
  c->stats.kernel_ms = ms;
  c->stats.blocks = sel.size();
  c->stats.in_bytes = total_in;
  c->stats.out_bytes = total_out;
  c->stats.model_bytes = total_model;
  c->stats.launches = launches + extra_launches;
  c->stats.concurrent = slots;
  c->stats.kernel_kind = kind_used;
  if (P.e8_wave) {                                      // (the heads of launches of other kernels keep their word 1 at zero)
    uint32_t heads[kQueueBytes / 4];
    HIPCHK(hipMemcpyAsync(heads, c->queue.p, kQueueBytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (size_t g = 0; g < kQueueBytes / 32; ++g) c->stats.e8_wave_segs += heads[8 * g + 1];
  }
  return first_bad;
}

extern "C" int zpaqhip_decode_blocks_device(zpaqhip_ctx *c, const void *d_in, const uint8_t *h_in, size_t in_len,
                                 const zpaqhip_block *blocks,
                                 size_t n_blocks, const zpaqhip_segment *segs, size_t n_segs, const uint32_t *ids,
                                 size_t n_ids, void *d_out, const uint64_t *out_off, const uint64_t *out_cap,
                                 zpaqhip_seg_result *results, const zpaqhip_opts *opts_in, void *hip_stream,
                                 zpaqhip_err *err) {
  if (!c || !blocks || !segs || !results || (!d_in && in_len) || (ids == nullptr && n_ids != 0 && n_ids != n_blocks)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  const zpaqhip_opts opts = resolve_opts(opts_in);
  zh_pending P;
  int rc = decode_launch(c, d_in, h_in, in_len, blocks, n_blocks, segs, n_segs, ids, n_ids, d_out, out_off, out_cap, opts,
                         hip_stream ? (hipStream_t)hip_stream : c->stream, P, err);
  if (rc) return rc;
  return decode_finish(c, P, results, err);
}


// ---------------------------------------------------------------------------
// Whole-stream forms: a three-stage pipeline over batches of whole blocks
//
//   source (caller's buffer, or Reader-shaped callback read incrementally)
//     -> scan a batch (>= 512 blocks when the stream has them)            host
//     -> H2D of the batch's bytes                                         stream s_in
//     -> decode kernels (zh_* families)                                   stream c->stream
//     -> D2H of the plaintext, block by block, into stream order          stream s_out
//   sink (caller's buffer, or Writer-shaped callback fed from pinned chunks)
//
// While the kernels of batch k run, the host drains the output of batch k-1 and reads / scans / uploads batch k+1
// (double-buffered device input and staging buffers).  Blocks whose plaintext size is unknown (no decimal size in the
// segment comment, LICENSE:57-58) get a provisional staging slot and are decoded ONCE; only a block that overflows its
// slot is decoded a second time, alone, with the exact size it reported.
// ---------------------------------------------------------------------------
namespace {

// Staging slots of `blocks` in out2[slot]: plan_slots (zh_stream_plan.h) within a quarter of the free memory, to which
// `reusable` counts (the staging buffers the caller is free to grow).
int plan_staging(zpaqhip_ctx *c, int slot, size_t reusable, const std::vector<zpaqhip_block> &blocks, const std::vector<zpaqhip_segment> &segs,
                 std::vector<uint64_t> &cap, std::vector<uint64_t> &off, zpaqhip_err *err) {
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  free_b += reusable;
  const uint64_t budget = free_b / 4 / std::max(1u, c->mem_share);   // per staging buffer; the arena needs the rest
  const uint64_t pos = plan_slots(blocks, segs, budget, cap, off);
  if (c->out2[slot].reserve((size_t)pos + 16) != hipSuccess) {      // not even that: everything count-only, exact second pass
    (void)hipGetLastError();
    count_only_slots(cap, off);
    HIPCHK(c->out2[slot].reserve(16));
  }
  return ZPAQHIP_OK;
}

// SHA-1 of the table's segments (offsets from `base`), computed ON THE DEVICE (zh_sha1_dev.hip) on `stream` while the
// plaintext is still there; the segments whose digest differs from the stored one (Decompresser.cs:183-191) are added to `bad`.
int sha1_check(zpaqhip_ctx *c, hipStream_t stream, const uint8_t *base, const Sha1Table &t, const zpaqhip_segment *segs,
               std::vector<uint32_t> &bad, zpaqhip_err *err) {
  if (t.which.empty()) return ZPAQHIP_OK;
  const size_t tab_bytes = t.pairs.size() * 8, dig_bytes = t.which.size() * 20;
  HIPCHK(c->sdesc.reserve(tab_bytes + dig_bytes + 64));          // the descriptors of the finished decode are not needed any more
  uint8_t *d_tab = (uint8_t *)c->sdesc.p, *d_dig = d_tab + ((tab_bytes + 15) & ~(size_t)15);
  HIPCHK(hipMemcpyAsync(d_tab, t.pairs.data(), tab_bytes, hipMemcpyHostToDevice, stream));
  HIPCHK(zh_launch_sha1(base, (const uint64_t *)d_tab, (uint32_t)t.which.size(), (uint32_t *)d_dig, stream));
  std::vector<uint32_t> dig(t.which.size() * 5);
  HIPCHK(hipMemcpyAsync(dig.data(), d_dig, dig_bytes, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (size_t k = 0; k < t.which.size(); ++k) {
    uint8_t d[20];
    for (int i = 0; i < 5; ++i) {
      const uint32_t v = dig[5 * k + i];
      d[4 * i] = (uint8_t)(v >> 24); d[4 * i + 1] = (uint8_t)(v >> 16); d[4 * i + 2] = (uint8_t)(v >> 8); d[4 * i + 3] = (uint8_t)v;
    }
    if (memcmp(d, segs[t.which[k]].sha1, 20) != 0) bad.push_back(t.which[k]);
  }
  return ZPAQHIP_OK;
}

// ... of every decoded segment of a batch that stores one: first those in the staging buffer, then those in the
// second-pass buffer
int sha1_mismatches(zpaqhip_ctx *c, const Batch &bt, std::vector<uint32_t> &bad, zpaqhip_err *err) {
  for (int where = 0; where < 2; ++where) {
    Sha1Table t;
    for (size_t b = 0; b < bt.so.blocks.size(); ++b) {
      if ((int)(bt.off[b] >> 63) != where) continue;
      const zpaqhip_block &B = bt.so.blocks[b];
      for (uint32_t i = 0; i < B.n_seg; ++i) t.add(bt.so.segs[B.first_seg + i], bt.res[B.first_seg + i], B.first_seg + i, bt.res[B.first_seg + i].out_off);
    }
    const uint8_t *base = where ? (const uint8_t *)c->out_fix[bt.slot].p : (const uint8_t *)c->out2[bt.slot].p;
    if (int rc = sha1_check(c, c->stream, base, t, bt.so.segs.data(), bad, err)) return rc;
  }
  return ZPAQHIP_OK;
}

// After decode_finish: plaintext sizes, and a second decode of the blocks that did not fit their staging slot.
int settle_batch(zpaqhip_ctx *c, Batch &bt, const zpaqhip_opts &opts, zpaqhip_stats &acc, zpaqhip_err *err) {
  const SecondPass sp = plan_second_pass(bt);
  if (sp.redo.empty()) return ZPAQHIP_OK;
  // exact sizes are known now: these blocks go to a buffer of their own
  HIPCHK(c->out_fix[bt.slot].reserve((size_t)sp.bytes + 16));
  zh_pending P;
  int rc = decode_launch(c, c->in2[bt.slot].p, bt.h, bt.len, bt.so.blocks.data(), bt.so.blocks.size(), bt.so.segs.data(), bt.so.segs.size(),
                         sp.redo.data(), sp.redo.size(), c->out_fix[bt.slot].p, sp.off2.data(), sp.cap2.data(), opts, c->stream, P, err);
  if (!rc) rc = decode_finish(c, P, bt.res.data(), err);
  add_kernel_stats(acc, c->stats);
  if (rc && !data_error(rc)) return rc;
  for (size_t k = 0; k < sp.redo.size(); ++k) {         // mark: lives in out_fix
    bt.off[sp.redo[k]] = sp.off2[k] | kInFix;
    bt.cap[sp.redo[k]] = sp.cap2[k];
  }
  return ZPAQHIP_OK;
}

// D2H time of a batch slot's last drain (memory and placed forms), added to c->d2h_acc once the copies are done
int harvest_d2h(zpaqhip_ctx *c, int slot, zpaqhip_err *err) {
  if (!c->d_pending[slot]) return ZPAQHIP_OK;
  c->d_pending[slot] = false;
  HIPCHK(hipEventSynchronize(c->ev_d[slot][1]));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev_d[slot][0], c->ev_d[slot][1]));
  c->d2h_acc += ms;
  return ZPAQHIP_OK;
}

// Deliver the first `upto_blocks` blocks (plus `partial` bytes of the next one) of a decoded batch to the sink, in order:
// the copies of plan_delivery (zh_stream_plan.h) on s_out.
int drain_batch(zpaqhip_ctx *c, const Batch &bt, size_t upto_blocks, uint64_t partial, Sinkk &sink, zpaqhip_err *err) {
  const bool timed = !sink.writer();
  if (timed) {
    int hrc = harvest_d2h(c, bt.slot, err);
    if (hrc) return hrc;
    HIPCHK(hipEventRecord(c->ev_d[bt.slot][0], c->s_out));
  }
  const Delivery d = plan_delivery(bt, upto_blocks, partial, sink);
  auto src_of = [&](const Copy &cp) { return (const uint8_t *)(cp.fix ? c->out_fix[bt.slot].p : c->out2[bt.slot].p) + cp.src_off; };
  if (timed) {                                          // memory and placed forms
    for (const Copy &cp : d.copies) {
      uint8_t *dst = sink.mem + cp.dst;
      if (cp.spill >= 0) {
        std::vector<uint8_t> &sp = (*sink.spill)[(size_t)cp.spill];
        sp.resize((size_t)cp.n);
        dst = sp.data();
      }
      HIPCHK(hipMemcpyAsync(dst, src_of(cp), (size_t)cp.n, hipMemcpyDeviceToHost, c->s_out));
    }
    sink.total = d.total;
    HIPCHK(hipEventRecord(c->ev_d[bt.slot][1], c->s_out));
    c->d_pending[bt.slot] = true;
    return ZPAQHIP_OK;
  }
  // Writer form: pinned double buffer; the copy of chunk i+1 runs while write_fn consumes chunk i
  for (int i = 0; i < 2; ++i)
    if (!c->pin[i]) HIPCHK(hipHostMalloc((void **)&c->pin[i], kPinChunk, hipHostMallocDefault));
  int cur = 0;
  uint64_t fill[2] = {0, 0};
  bool inflight[2] = {false, false};
  auto flush = [&](int i) -> int {
    if (!inflight[i]) return ZPAQHIP_OK;
    HIPCHK(hipEventSynchronize(c->ev_pin[i]));
    inflight[i] = false;
    for (uint64_t p = 0; p < fill[i];) {
      const int n = (int)std::min<uint64_t>(fill[i] - p, 1u << 30);
      if (sink.wr(sink.user, c->pin[i] + p, n) < 0) { set_err(err, ZPAQHIP_E_CALLBACK, -1, -1); return ZPAQHIP_E_CALLBACK; }
      p += (uint64_t)n;
    }
    sink.total += fill[i];
    fill[i] = 0;
    return ZPAQHIP_OK;
  };
  for (const Copy &cp : d.copies) {
    for (uint64_t done = 0; done < cp.n;) {
      const uint64_t n = std::min<uint64_t>(cp.n - done, kPinChunk - fill[cur]);
      HIPCHK(hipMemcpyAsync(c->pin[cur] + fill[cur], src_of(cp) + done, (size_t)n, hipMemcpyDeviceToHost, c->s_out));
      fill[cur] += n; done += n;
      if (fill[cur] == kPinChunk) {
        HIPCHK(hipEventRecord(c->ev_pin[cur], c->s_out));
        inflight[cur] = true;
        cur ^= 1;
        int rc = flush(cur);                            // the other buffer must be free before it is refilled
        if (rc) return rc;
      }
    }
  }
  if (fill[cur]) { HIPCHK(hipEventRecord(c->ev_pin[cur], c->s_out)); inflight[cur] = true; }
  int rc = flush(cur ^ 1);
  if (!rc) rc = flush(cur);
  return rc;
}

// The pipeline.  `tolerate`: per-segment data errors do not end the call (zpaqhip_decompress_segments).
// *stream_error: the returned code describes the stream (damage behind the delivered blocks), not a failure of the call.
int run_pipeline_impl(zpaqhip_ctx *c, Source &src, Sinkk &sink, const zpaqhip_opts &opts, bool tolerate, SegSink *segsink,
                      zpaqhip_err *err, bool *stream_error);
// Every exit with an error leaves nothing in flight: copies on s_out / s_in may still be writing caller-owned (pageable) host
// memory or reading staging the caller is about to free (the multi-device worker destroyed its spill vectors and
// the context right after an early return).
int run_pipeline(zpaqhip_ctx *c, Source &src, Sinkk &sink, const zpaqhip_opts &opts, bool tolerate, SegSink *segsink,
                 zpaqhip_err *err, bool *stream_error = nullptr) {
  const int rc = run_pipeline_impl(c, src, sink, opts, tolerate, segsink, err, stream_error);
  if (rc) {
    if (c->s_out) (void)hipStreamSynchronize(c->s_out);
    if (c->s_in) (void)hipStreamSynchronize(c->s_in);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
  }
  return rc;
}
int run_pipeline_impl(zpaqhip_ctx *c, Source &src, Sinkk &sink, const zpaqhip_opts &opts, bool tolerate, SegSink *segsink,
                      zpaqhip_err *err, bool *stream_error) {
  if (stream_error) *stream_error = false;
  HIPCHK(hipSetDevice(c->device));
  if (!c->s_in) {
    HIPCHK(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      HIPCHK(hipEventCreate(&c->ev_in[i])); HIPCHK(hipEventCreate(&c->ev_pin[i]));
      HIPCHK(hipEventCreate(&c->ev_d[i][0])); HIPCHK(hipEventCreate(&c->ev_d[i][1]));
    }
    HIPCHK(hipEventCreate(&c->ev_h0)); HIPCHK(hipEventCreate(&c->ev_h1));
  }
  zpaqhip_stats acc{};
  c->d2h_acc = 0; c->d_pending[0] = c->d_pending[1] = false;
  Batch bt[2];
  zh_pending P;
  int final_rc = ZPAQHIP_OK;
  zpaqhip_err final_err{};
  float h2d_ms = 0;

  // ---- the steps of a batch
  // fetch: the next batch of the source (global indices from blk0 / seg0), its bytes on their way to device slot `slot`
  auto fetch = [&](int slot, size_t blk0, size_t seg0) -> int {
    Batch &b = bt[slot];
    if (int rc = next_batch(src, b, blk0, seg0, (size_t)opts.batch_blocks, (size_t)opts.dec_waves, err)) return rc;
    b.slot = slot;
    if (b.so.blocks.empty()) return ZPAQHIP_OK;
    HIPCHK(c->in2[slot].reserve(b.len + 16));
    HIPCHK(hipEventRecord(c->ev_h0, c->s_in));
    HIPCHK(hipMemcpyAsync(c->in2[slot].p, b.h, b.len, hipMemcpyHostToDevice, c->s_in));
    HIPCHK(hipEventRecord(c->ev_h1, c->s_in));
    HIPCHK(hipEventRecord(c->ev_in[slot], c->s_in));
    return ZPAQHIP_OK;
  };
  auto add_h2d_time = [&] {                              // of the last upload
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev_h0, c->ev_h1) == hipSuccess) h2d_ms += ms; else (void)hipGetLastError();
  };
  // launch: the batch's kernels enqueued behind its upload, writing to its staging buffer
  auto launch = [&](Batch &B) -> int {
    B.res.assign(B.so.segs.size(), zpaqhip_seg_result{});
    B.real.assign(B.so.blocks.size(), 0);
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_in[B.slot], 0));
    return decode_launch(c, c->in2[B.slot].p, B.h, B.len, B.so.blocks.data(), B.so.blocks.size(), B.so.segs.data(),
                         B.so.segs.size(), nullptr, 0, c->out2[B.slot].p, B.off.data(), B.cap.data(), opts, c->stream, P, err);
  };
  // finish: the kernels waited for, the blocks that overflowed their slot decoded again, the checksums compared
  auto finish = [&](Batch &B) -> int {
    int rc = decode_finish(c, P, B.res.data(), err);
    add_kernel_stats(acc, c->stats);
    add_block_stats(acc, c->stats);
    if (rc && !data_error(rc)) { rebase_err(err, B); return rc; }
    rc = settle_batch(c, B, opts, acc, err);
    if (rc) { rebase_err(err, B); return rc; }
    if (opts.verify_sha1) {
      std::vector<uint32_t> bad;
      rc = sha1_mismatches(c, B, bad, err);
      if (rc) return rc;
      for (uint32_t s2 : bad) B.res[s2].status = ZPAQHIP_E_SHA1;
    }
    return ZPAQHIP_OK;
  };
  auto end_of_stream = [&](const Batch &B) {             // a framing error behind the last block: reported when all is delivered
    if (B.rc_after) { final_rc = B.rc_after; final_err = B.err_after; rebase_err(&final_err, B); }
  };

  int rc = fetch(0, 0, 0);
  if (rc) return rc;
  bool have_prev = false;
  for (int cur = 0;; cur ^= 1) {
    Batch &B = bt[cur], &prev = bt[cur ^ 1];
    const bool have = !B.so.blocks.empty();
    if (have && (rc = plan_staging(c, B.slot, c->out2[0].cap + c->out2[1].cap, B.so.blocks, B.so.segs, B.cap, B.off, err))) return rc;
    if (have && (rc = launch(B))) {                      // (device memory, HIP): what is already decoded is delivered first
      rebase_err(err, B);
      if (have_prev) { zpaqhip_err e3{}; (void)drain_batch(c, prev, prev.so.blocks.size(), 0, sink, &e3); (void)hipStreamSynchronize(c->s_out); }
      return rc;
    }
    // ---- while the kernels run: deliver the previous batch, fetch and upload the next one
    if (have_prev && (rc = drain_batch(c, prev, prev.so.blocks.size(), 0, sink, err))) return rc;
    have_prev = false;
    const bool more = have && !B.last;
    if (more) {
      add_h2d_time();
      HIPCHK(hipStreamSynchronize(c->s_out));          // prev's device buffers are about to be reused
      if ((rc = fetch(cur ^ 1, B.blk0 + B.so.blocks.size(), B.seg0 + B.so.segs.size()))) return rc;
    }
    if (!have) { end_of_stream(B); break; }
    if ((rc = finish(B))) return rc;
    const FirstBad bad = tolerate ? FirstBad() : first_failure(B);
    if (segsink) append_segment_records(B, sink.total, *segsink);
    if (bad.found) {                                     // everything before the failed segment, then its error
      final_rc = bad.rc; final_err = bad.err;
      if ((rc = drain_batch(c, B, bad.ok_blocks, bad.partial, sink, err))) return rc;
      break;
    }
    if (!more) {
      if ((rc = drain_batch(c, B, B.so.blocks.size(), 0, sink, err))) return rc;
      end_of_stream(B);
      break;
    }
    have_prev = true;
  }
  add_h2d_time();
  HIPCHK(hipStreamSynchronize(c->s_out));
  for (int i = 0; i < 2; ++i) { int hrc = harvest_d2h(c, i, err); if (hrc) return hrc; }
  c->stats = acc;
  c->stats.h2d_ms = h2d_ms;
  c->stats.d2h_ms = c->d2h_acc;                          // copy-stream time of the plaintext (memory forms; it overlaps the kernels)
  c->stats.out_bytes = sink.total;
  if (final_rc) { if (err) *err = final_err; if (stream_error) *stream_error = true; return final_rc; }
  return ZPAQHIP_OK;
}

}  // namespace

extern "C" {

int zpaqhip_decompress(zpaqhip_ctx *c, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, size_t *out_len,
                       const zpaqhip_opts *opts_in, zpaqhip_err *err) {
  if (!c || (!in && in_len) || !out_len || (!out && out_cap)) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  const zpaqhip_opts opts = resolve_opts(opts_in);
  Source src; src.mem = in ? in : (const uint8_t *)""; src.mem_len = in_len;
  Sinkk sink; sink.mem = out; sink.cap = out_cap;
  *out_len = 0;
  int rc = run_pipeline(c, src, sink, opts, false, nullptr, err);
  *out_len = (size_t)sink.total;
  if (rc) return rc;
  if (sink.total > out_cap) { set_err(err, ZPAQHIP_E_OUTPUT_FULL, -1, -1); return ZPAQHIP_E_OUTPUT_FULL; }
  return ZPAQHIP_OK;
}

// Estimated decode cost of every block: plaintext bytes (the decimal size in the comments when it is plausible, else
// 4 x the coded bytes) x the cycles per plaintext byte of the kernel the block's header selects (measured, profiles/r03;
// a block's decode time is its bit count x the depth of its model, not its coded size).  Host-side only.
static constexpr uint64_t kCm1Marker = ~0ull;
int zpaqhip_block_costs(const uint8_t *in, size_t in_len, const zpaqhip_block *blocks, size_t n_blocks,
                        const zpaqhip_segment *segs, size_t n_segs, uint64_t *cost, zpaqhip_err *err) {
  if ((!in && in_len) || (!blocks && n_blocks) || (!segs && n_segs) || (!cost && n_blocks)) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  std::map<std::string, uint64_t> per_byte;
  for (size_t b = 0; b < n_blocks; ++b) {
    const zpaqhip_block &B = blocks[b];
    if (B.hdr_off + B.hdr_len > in_len || (uint64_t)B.first_seg + B.n_seg > n_segs) {
      set_err(err, ZPAQHIP_E_ARG, (int)b, -1, "block table does not match the stream");
      return ZPAQHIP_E_ARG;
    }
    std::string key((const char *)in + B.hdr_off, B.hdr_len);
    auto it = per_byte.find(key);
    if (it == per_byte.end()) {
      ZhModel m;
      std::vector<uint8_t> code;
      zpaqhip_err e2{};
      uint64_t w = 6000;                                  // a header the model builder refuses costs nothing real; keep it finite
      if (build_model(in + B.hdr_off, B.hdr_len, m, code, &e2) == ZPAQHIP_OK) {
        const ZhRoute r = route_block(m, resolve_opts(nullptr), false, kKernelHas);
        const bool pcomp = (m.ph | m.pm) != 0;
        // measured cycles of the owning workgroup per plaintext byte (profiles/r03: 256 x 4 MiB, one block per CU), rounded;
        // estimates for the fallback kernels
        switch (r.kernel) {
          case ZhKernel::Store: w = pcomp ? 120u : 30u; break;          // zh_store.hip: wave-wide copy / LZ77 / inverse BWT
          case ZhKernel::Cm: w = kCm1Marker; break;                      // zh_cm.hip: by coded / plain ratio, below
          case ZhKernel::Nibble: w = r.spec == 2 ? 6800u : r.spec == 5 ? 7000u : 3800u; break;   // zh_nibble.hip: mid, mid8; min, min1 (profiles/r05)
          case ZhKernel::Chain2: w = 16600u; break;                      // zh_chain2.hip: max (profiles/r05)
          case ZhKernel::Chain: w = 4000u + 2200u * m.n; break;          // zh_chain.hip: level walk at run time
          case ZhKernel::Generic: w = 10000u + 16000u * m.n; break;      // zh_generic.hip: one lane, tables in HBM
        }
        if (pcomp && r.kernel != ZhKernel::Store) w += w == kCm1Marker ? (uint64_t)-1 : 1500u;   // (marker - 1: single CM with a post-processor)
      }
      it = per_byte.emplace(key, w).first;
    }
    uint64_t coded = 0;
    for (uint32_t i = 0; i < B.n_seg; ++i) coded += segs[B.first_seg + i].data_len;
    const bool hinted = plausible_hint(B.usize_hint);
    const uint64_t plain = hinted ? B.usize_hint : coded * 4;
    uint64_t w = it->second;
    if (w >= kCm1Marker - 1) {
      const uint64_t pp = w == kCm1Marker ? 0u : 1500u;
      // zh_cm.hip: the byte loop costs the same on any data, a window miss ~1 400 cycles more, and the miss rate of an
      // order-1 context follows the data's entropy — which the block shows as coded / plain.  Measured at 256 blocks per GPU
      // (profiles/r04): text 0.45 -> 920 cycles per byte, x86-like 0.75 -> 1 250, random 1.03 -> 2 020; piecewise linear
      // between them (a block without a size hint counts as text)
      const double rho = hinted && plain ? (double)coded / (double)plain : 0.45;
      w = pp + (rho <= 0.45 ? 920u : rho <= 0.75 ? 920u + (uint64_t)((rho - 0.45) * 1100.0) : 1250u + (uint64_t)((std::min(rho, 1.1) - 0.75) * 2750.0));
    }
    cost[b] = std::max<uint64_t>(1, plain) * w;
  }
  return ZPAQHIP_OK;
}

// Contexts zpaqhip_decompress_multi has used stay alive between calls (the arena of a context is tens of GB for the larger
// models: allocating and faulting it in on every call cost more than the decode of a small archive): a device thread takes
// one of its device's from this pool, or makes one, and puts it back.  zpaqhip_multi_trim() destroys the idle ones.
namespace {
std::mutex g_pool_mu;
std::map<int, std::vector<zpaqhip_ctx *>> g_pool;
zpaqhip_ctx *pool_take(int device, int *rc, zpaqhip_err *err) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto &v = g_pool[device];
    if (!v.empty()) { zpaqhip_ctx *c = v.back(); v.pop_back(); *rc = ZPAQHIP_OK; return c; }
  }
  zpaqhip_ctx *c = nullptr;
  *rc = zpaqhip_ctx_create(device, &c, err);
  return *rc ? nullptr : c;
}
void pool_give(zpaqhip_ctx *c) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  g_pool[c->device].push_back(c);
}
}  // namespace
// Destroys the idle pooled contexts of `device` beyond the first `keep`; returns how many went.
static size_t pool_trim_device(int device, size_t keep) {
  std::vector<zpaqhip_ctx *> gone;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool.find(device);
    if (it == g_pool.end()) return 0;
    while (it->second.size() > keep) { gone.push_back(it->second.back()); it->second.pop_back(); }
  }
  for (zpaqhip_ctx *c : gone) zpaqhip_ctx_destroy(c);
  return gone.size();
}

extern "C" void zpaqhip_multi_trim(void) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (auto &kv : g_pool) for (zpaqhip_ctx *c : kv.second) zpaqhip_ctx_destroy(c);
  g_pool.clear();
}

// Several GPUs of one node: one context and one host thread per entry of `devices`, all pulling from ONE work queue.
//   queue   the blocks sorted by estimated cost (zpaqhip_block_costs) are dealt into K = ceil(n / queue_blocks) chunks,
//           chunk k = every K-th block of that order starting at k (each chunk is a cross-section of the cost
//           distribution; queue_blocks defaults to min(256 — one block per CU —, a quarter of a device's share)); a device thread takes the
//           next chunk (one atomic counter) whenever it has finished one, so a GPU that is faster, or whose chunks
//           turned out cheaper than estimated, simply takes more of them
//   placing block b goes to out + (sum of the plausible comment sizes before it); a block whose comment carries no
//           plausible size, or the wrong one, is kept whole in a host buffer by the thread that decoded it and only
//           THAT block (and the blocks behind it, by memmove) is put in place when all sizes are known — nothing is
//           decoded twice
//   errors  a damaged block ends its chunk there; the other chunks go on, so that every block before the first damaged
//           one of the stream is delivered, *out_len says how many bytes that is, and the call returns that block's error
int zpaqhip_decompress_multi_stats(const int *devices, size_t n_dev, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                   size_t *out_len, const zpaqhip_opts *opts_in, zpaqhip_stats *per_device, zpaqhip_err *err) {
  if (!devices || !n_dev || (!in && in_len) || !out_len || (!out && out_cap)) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  zpaqhip_opts opts = resolve_opts(opts_in);
  *out_len = 0;
  if (per_device) memset(per_device, 0, n_dev * sizeof(zpaqhip_stats));
  ScanOut so;
  zpaqhip_err scan_err{};
  const int scan_rc = scan_stream(in ? in : (const uint8_t *)"", in_len, so, &scan_err);   // blocks before damage are decoded
  const size_t nb = so.blocks.size();
  if (!nb) { if (scan_rc && err) *err = scan_err; return scan_rc; }
  // ---- the queue: the blocks by cost, dealt into K chunks
  std::vector<uint64_t> cost(nb, 0);
  { int rc = zpaqhip_block_costs(in, in_len, so.blocks.data(), nb, so.segs.data(), so.segs.size(), cost.data(), err); if (rc) return rc; }
  const std::vector<size_t> order = queue_order(cost);
  size_t chunk_blocks = (size_t)opts.queue_blocks;      // blocks per pull: what the caller says, or default_chunk_blocks
  if (!chunk_blocks) {
    bool all_cm1 = true;
    for (size_t b = 0; b < nb; ++b) all_cm1 = all_cm1 && so.blocks[b].n_comp == 1;
    chunk_blocks = default_chunk_blocks(nb, n_dev, all_cm1);
  }
  const size_t K = (nb + chunk_blocks - 1) / chunk_blocks;
  std::atomic<size_t> next_chunk{0};
  std::atomic<bool> abort_all{false};
  // ---- slots
  std::vector<uint64_t> slot_off, slot_cap, real(nb, 0);
  place_slots(so.blocks, out_cap, slot_off, slot_cap);
  std::vector<std::vector<uint8_t>> spill(nb);
  std::vector<uint8_t> done(nb, 0);
  {  // idle pooled contexts beyond what this call uses on a device give their memory back before the workers size their arenas
    std::map<int, size_t> use;
    for (size_t r = 0; r < n_dev; ++r) ++use[devices[r]];
    for (auto &kv : use) pool_trim_device(kv.first, kv.second);
  }
  // ---- workers
  std::vector<MultiJob> jobs(n_dev);
  auto worker = [&](size_t r) {
    MultiJob &J = jobs[r];
    zpaqhip_ctx *c = pool_take(devices[r], &J.rc, &J.err);
    if (!c) { abort_all = true; return; }
    c->mem_share = 1;
    for (size_t k = 0; k < n_dev; ++k) c->mem_share += k != r && devices[k] == devices[r];
    std::vector<uint8_t> sub;
    std::vector<size_t> ids;
    std::vector<uint64_t> place, cap, sizes;
    std::vector<std::vector<uint8_t>> sp;
    while (!abort_all) {
      const size_t k = next_chunk.fetch_add(1);
      if (k >= K) break;
      const bool run = queue_chunk(order, k, K, ids);
      sub.clear(); place.clear(); cap.clear();
      for (size_t b : ids) {
        if (!run) sub.insert(sub.end(), in + so.blocks[b].tag_off, in + so.blocks[b].end_off);
        place.push_back(slot_off[b]); cap.push_back(slot_cap[b]);
      }
      sizes.assign(ids.size(), 0);
      sp.assign(ids.size(), std::vector<uint8_t>());
      Source src;
      if (run) { src.mem = in + so.blocks[ids.front()].tag_off; src.mem_len = (size_t)(so.blocks[ids.back()].end_off - so.blocks[ids.front()].tag_off); }
      else { src.mem = sub.data(); src.mem_len = sub.size(); }
      Sinkk sink;
      sink.mem = out; sink.cap = out_cap; sink.place = place.data(); sink.place_cap = cap.data(); sink.sizes = &sizes; sink.spill = &sp;
      zpaqhip_err e2{};
      bool stream_error = false;
      const int rc = run_pipeline(c, src, sink, opts, false, nullptr, &e2, &stream_error);
      add_block_stats(J.st, c->stats);
      J.st.kernel_ms += c->stats.kernel_ms; J.st.h2d_ms += c->stats.h2d_ms; J.st.d2h_ms += c->stats.d2h_ms;
      J.st.out_bytes += c->stats.out_bytes; J.st.launches += 1; J.st.e8_wave_segs += c->stats.e8_wave_segs;   // (launches: chunks taken)
      bool call_failed = false;
      const size_t good = note_chunk(J, ids, rc, e2, stream_error, &call_failed);
      if (call_failed) { abort_all = true; break; }
      for (size_t j = 0; j < good; ++j) { real[ids[j]] = sizes[j]; spill[ids[j]].swap(sp[j]); done[ids[j]] = 1; }
    }
    if (J.rc && J.bad < 0) zpaqhip_ctx_destroy(c);       // a failure of the call itself (HIP, memory): do not keep that context
    else pool_give(c);
  };
  {
    std::vector<std::thread> th;
    for (size_t r = 0; r < n_dev; ++r) th.emplace_back(worker, r);
    for (auto &t : th) t.join();
  }
  if (per_device) for (size_t r = 0; r < n_dev; ++r) per_device[r] = jobs[r].st;
  // ---- merge: a failure of the call itself first; else the first damaged block of the stream
  const MultiOutcome oc = merge_jobs(jobs, nb);
  if (oc.rc) { if (err) *err = oc.err; return oc.rc; }
  for (size_t b = 0; b < oc.limit; ++b)
    if (!done[b]) { set_err(err, ZPAQHIP_E_HIP, (int)b, -1, "multi-device queue: a block was left undecoded"); return ZPAQHIP_E_HIP; }
  // ---- put the blocks whose size was not the promised one in place
  if (int rc = settle_places(out, out_cap, oc.limit, slot_off, slot_cap, real, spill, out_len)) { set_err(err, rc, -1, -1); return rc; }
  if (oc.data_rc) { if (err) *err = oc.data_err; return oc.data_rc; }
  if (scan_rc) { if (err) *err = scan_err; return scan_rc; }
  return ZPAQHIP_OK;
}

int zpaqhip_decompress_multi(const int *devices, size_t n_dev, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                             size_t *out_len, const zpaqhip_opts *opts_in, zpaqhip_err *err) {
  return zpaqhip_decompress_multi_stats(devices, n_dev, in, in_len, out, out_cap, out_len, opts_in, nullptr, err);
}

int zpaqhip_decompress_segments(zpaqhip_ctx *c, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                                size_t *out_len, zpaqhip_seg_result *results, size_t result_cap, size_t *n_results,
                                const zpaqhip_opts *opts_in, zpaqhip_err *err) {
  if (!c || (!in && in_len) || !out_len || !n_results || (!out && out_cap) || (!results && result_cap)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  const zpaqhip_opts opts = resolve_opts(opts_in);
  Source src; src.mem = in ? in : (const uint8_t *)""; src.mem_len = in_len;
  Sinkk sink; sink.mem = out; sink.cap = out_cap;
  SegSink ss;
  *out_len = 0; *n_results = 0;
  bool stream_error = false;
  int rc = run_pipeline(c, src, sink, opts, true, &ss, err, &stream_error);
  *out_len = (size_t)sink.total;
  *n_results = ss.res.size();
  if (rc && !stream_error) return rc;                    // the call itself failed (device, arguments, callback)
  const int frame_rc = rc;                               // a framing error after the last good block: reported below
  if (ss.res.size() > result_cap) { set_err(err, ZPAQHIP_E_ARG, -1, -1, "result table too small"); return ZPAQHIP_E_ARG; }
  if (!ss.res.empty()) memcpy(results, ss.res.data(), ss.res.size() * sizeof(zpaqhip_seg_result));
  if (sink.total > out_cap) { set_err(err, ZPAQHIP_E_OUTPUT_FULL, -1, -1); return ZPAQHIP_E_OUTPUT_FULL; }
  return frame_rc;
}

// Decompresser.pcomp (Decompresser.cs:155-158 -> ZPAQL.write(out, true), ZPAQL.cs:158-179): the PCOMP program a block's
// first segment carries, as "length lo, length hi, program bytes"; *out_len = 0 when the block has none.  The program
// travels inside the coded data, so the start of the block is decoded (the generic kernel stops once the post-processor
// header is complete) and the program is read back from the arena slot.
int zpaqhip_block_pcomp(zpaqhip_ctx *c, const uint8_t *in, size_t in_len, uint32_t block, uint8_t *out, size_t out_cap,
                        size_t *out_len, zpaqhip_err *err) {
  if (!c || (!in && in_len) || !out_len || (!out && out_cap)) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  *out_len = 0;
  ScanOut so;
  int rc = scan_stream(in, in_len, so, err);
  if (rc) return rc;
  if (block >= so.blocks.size()) { set_err(err, ZPAQHIP_E_ARG, (int)block, -1, "block id out of range"); return ZPAQHIP_E_ARG; }
  const zpaqhip_block &b = so.blocks[block];
  if (b.n_seg == 0) return ZPAQHIP_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(c->in.reserve(in_len + 16));
  HIPCHK(hipMemcpy(c->in.p, in, in_len, hipMemcpyHostToDevice));
  HIPCHK(c->out.reserve(16));
  zpaqhip_opts o;
  memset(&o, 0, sizeof o);
  o.struct_size = sizeof o;
  o.max_concurrent = 1;                                  // the block runs in arena slot 0
  o.kernel = 1;                                          // the generic kernel knows how to stop after the header
  o.reserved[0] = kPpOnlyMagic;
  std::vector<zpaqhip_seg_result> res(so.segs.size());
  const uint32_t id = block;
  const uint64_t off0 = 0, cap0 = 0;                     // count-only: nothing is written
  rc = zpaqhip_decode_blocks_device(c, c->in.p, in, in_len, so.blocks.data(), so.blocks.size(), so.segs.data(), so.segs.size(),
                                    &id, 1, c->out.p, &off0, &cap0, res.data(), &o, c->stream, err);
  const uint32_t raw = c->raw_pp.size() > b.first_seg ? c->raw_pp[b.first_seg] : 0;
  const uint32_t state = raw & 255u, hsize = raw >> 8;
  if (state < 5) {                                       // PASS, or the stream broke before the program was complete
    const int st0 = res[b.first_seg].status;
    if (rc && st0 != ZPAQHIP_OK && st0 != ZPAQHIP_E_OUTPUT_FULL) return rc;
    return ZPAQHIP_OK;
  }
  *out_len = (size_t)hsize + 2;
  if (*out_len > out_cap) { set_err(err, ZPAQHIP_E_OUTPUT_FULL, (int)block, (int)b.first_seg); return ZPAQHIP_E_OUTPUT_FULL; }
  std::vector<uint8_t> code;
  ZhModel m;
  rc = build_model(in + b.hdr_off, b.hdr_len, m, code, err);
  if (rc) return rc;
  out[0] = (uint8_t)(hsize & 255);
  out[1] = (uint8_t)(hsize >> 8);
  HIPCHK(hipMemcpy(out + 2, (const uint8_t *)c->arena.p + m.pz_off + ZH_CODE_PAD, hsize, hipMemcpyDeviceToHost));
  return ZPAQHIP_OK;
}

// zh_chain.hip's several-waves plan for a block header: host only
int zpaqhip_dec_chain_plan(const uint8_t *hdr, size_t hdr_len, uint32_t *waves, uint32_t *lds_bytes, zpaqhip_err *err) {
  if (!hdr || !waves || !lds_bytes) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  *waves = *lds_bytes = 0;
  ZhModel m;
  std::vector<uint8_t> code;
  const int rc = build_model(hdr, hdr_len, m, code, err);
  if (rc) return rc;
  const DecChainPlan p = plan_dec_chain(m);
  *waves = p.waves;
  *lds_bytes = p.lds_bytes;
  return ZPAQHIP_OK;
}

int zpaqhip_decompress_cb(zpaqhip_ctx *c, zpaqhip_read_fn read_fn, zpaqhip_write_fn write_fn, void *user,
                          const zpaqhip_opts *opts_in, zpaqhip_err *err) {
  if (!c || !read_fn || !write_fn) { set_err(err, ZPAQHIP_E_ARG, -1, -1); return ZPAQHIP_E_ARG; }
  const zpaqhip_opts opts = resolve_opts(opts_in);
  Source src; src.rd = read_fn; src.user = user;
  Sinkk sink; sink.wr = write_fn; sink.user = user;
  return run_pipeline(c, src, sink, opts, false, nullptr, err);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Device-resident streams: the framing scan on the GPU (zh_scan.hip, zh_scan_walk.h) and the whole-stream form over it
// ---------------------------------------------------------------------------
namespace {

struct DevScan {
  ZhScanLists L{};                        // the lists, in c->scan_list
  ZhScanResult R{};
  float ms = 0;                           // HIP-event time of the kernels
  uint32_t launches = 0;
};

// The kernels of a timed phase are enqueued by `enqueue`; waits for them
template <class F>
int timed_phase(zpaqhip_ctx *c, hipStream_t stream, float &total_ms, zpaqhip_err *err, F enqueue) {
  HIPCHK(hipEventRecord(c->ev0, stream));
  if (int rc = enqueue()) return rc;
  HIPCHK(hipEventRecord(c->ev1, stream));
  HIPCHK(hipStreamSynchronize(stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  total_ms += ms;
  return ZPAQHIP_OK;
}

// Lists, per-hit records and the chain: S.R says how many blocks and segments the stream has and how the scan ended; the
// chosen blocks are in c->scan_blk.  Three words of totals and the result record are all that crosses the bus.
int scan_device_chain(zpaqhip_ctx *c, const uint8_t *d_in, size_t n, hipStream_t stream, DevScan &S, zpaqhip_err *err) {
  HIPCHK(hipSetDevice(c->device));
  const uint64_t np = zh_scan_pieces(n);
  HIPCHK(c->scan_cnt.reserve((size_t)(3 * np + 8) * 8 + sizeof(ZhScanResult)));
  uint64_t *d_cnt = (uint64_t *)c->scan_cnt.p, *d_total = d_cnt + 3 * np;
  ZhScanResult *d_res = (ZhScanResult *)(d_total + 8);
  uint64_t total[3] = {0, 0, 0};
  int rc = timed_phase(c, stream, S.ms, err, [&]() -> int {
    HIPCHK(zh_launch_scan_count(d_in, n, d_cnt, d_total, stream));
    HIPCHK(hipMemcpyAsync(total, d_total, sizeof total, hipMemcpyDeviceToHost, stream));
    return ZPAQHIP_OK;
  });
  if (rc) return rc;
  S.launches += 2;
  if (total[1] != total[2]) { set_err(err, ZPAQHIP_E_HIP, -1, -1, "framing scan: zero-run starts and ends differ"); return ZPAQHIP_E_HIP; }
  const uint64_t n_tag = total[0], n_run = total[1];
  HIPCHK(c->scan_list.reserve((size_t)(n_tag + 2 * n_run) * 8 + 16));
  HIPCHK(c->scan_rec.reserve((size_t)n_tag * sizeof(ZhScanRec) + 16));
  uint64_t *d_tag = (uint64_t *)c->scan_list.p;
  S.L = ZhScanLists{d_tag, d_tag + n_tag, d_tag + n_tag + n_run, n_tag, n_run};
  for (int pass = 0; pass < 2; ++pass) {                // (a second time only for more blocks than tag hits and a few: bare "zPQ" blocks)
    const uint64_t cap = pass ? S.R.n_blocks : n_tag + 64;
    HIPCHK(c->scan_blk.reserve((size_t)cap * sizeof(zpaqhip_block) + 16));
    rc = timed_phase(c, stream, S.ms, err, [&]() -> int {
      if (!pass) {
        HIPCHK(zh_launch_scan_fill(d_in, n, d_cnt, d_tag, d_tag + n_tag, d_tag + n_tag + n_run, n_tag, n_run, stream));
        HIPCHK(zh_launch_scan_parse(d_in, n, &S.L, (ZhScanRec *)c->scan_rec.p, stream));
        S.launches += n_tag ? 2 : 1;
      }
      HIPCHK(zh_launch_scan_chain(d_in, n, &S.L, (const ZhScanRec *)c->scan_rec.p, (zpaqhip_block *)c->scan_blk.p, cap, d_res, stream));
      ++S.launches;
      HIPCHK(hipMemcpyAsync(&S.R, d_res, sizeof S.R, hipMemcpyDeviceToHost, stream));
      return ZPAQHIP_OK;
    });
    if (rc) return rc;
    if (S.R.n_blocks <= cap) break;
  }
  return ZPAQHIP_OK;
}

// The tables of the chain's blocks to the host
int scan_device_tables(zpaqhip_ctx *c, const uint8_t *d_in, size_t n, hipStream_t stream, DevScan &S, zpaqhip_block *blocks,
                       zpaqhip_segment *segs, zpaqhip_err *err) {
  const uint64_t nb = S.R.n_blocks, ns = S.R.n_segs;
  if (!nb) return ZPAQHIP_OK;
  HIPCHK(c->scan_seg.reserve((size_t)ns * sizeof(zpaqhip_segment) + 16));
  return timed_phase(c, stream, S.ms, err, [&]() -> int {
    HIPCHK(zh_launch_scan_segments(d_in, n, &S.L, (const zpaqhip_block *)c->scan_blk.p, nb, (zpaqhip_segment *)c->scan_seg.p, ns, stream));
    ++S.launches;
    HIPCHK(hipMemcpyAsync(blocks, c->scan_blk.p, (size_t)nb * sizeof(zpaqhip_block), hipMemcpyDeviceToHost, stream));
    if (ns) HIPCHK(hipMemcpyAsync(segs, c->scan_seg.p, (size_t)ns * sizeof(zpaqhip_segment), hipMemcpyDeviceToHost, stream));
    return ZPAQHIP_OK;
  });
}

void scan_device_err(const DevScan &S, zpaqhip_err *e) {
  set_err(e, S.R.status, S.R.err_block, S.R.err_seg, zh_scan_message(S.R.msg));
}

// zh_frame.hip over entries without head and tail: bodies from staging (FIRST), the second-pass buffer (REDO) or d_out
// (INPUT), copied to `dst`
int pack_bodies(zpaqhip_ctx *c, hipStream_t stream, const std::vector<ZhFrameEntry> &tab, const uint8_t *d_out, uint8_t *dst, float &ms,
                uint32_t &launches, zpaqhip_err *err) {
  if (tab.empty()) return ZPAQHIP_OK;
  const size_t tb = tab.size() * sizeof(ZhFrameEntry);
  HIPCHK(c->pack_tab.reserve(tb + 32));
  HIPCHK(hipMemcpyAsync(c->pack_tab.p, tab.data(), tb, hipMemcpyHostToDevice, stream));
  ZhFrameLaunch L;
  memset(&L, 0, sizeof L);
  L.table = (const ZhFrameEntry *)c->pack_tab.p;
  L.blob = (const uint8_t *)c->pack_tab.p + tb;
  L.src[ZH_FRAME_SRC_FIRST] = (const uint8_t *)c->out2[0].p;
  L.src[ZH_FRAME_SRC_REDO] = (const uint8_t *)c->out_fix[0].p;
  L.src[ZH_FRAME_SRC_INPUT] = d_out;
  L.out = dst;
  L.n = (uint32_t)tab.size();
  uint64_t longest = 0;
  for (const ZhFrameEntry &e : tab) longest = std::max(longest, e.body_len);
  L.pieces = (uint32_t)std::max<uint64_t>(1, (longest + ZH_FRAME_PIECE - 1) / ZH_FRAME_PIECE);
  return timed_phase(c, stream, ms, err, [&]() -> int {
    HIPCHK(zh_launch_frame_pack(&L, stream, &launches));
    return ZPAQHIP_OK;
  });
}

bool device_stream_ok(const void *d_in, size_t in_len) { return (d_in || !in_len) && ((uintptr_t)d_in & 3u) == 0; }

}  // namespace

extern "C" int zpaqhip_scan_device(zpaqhip_ctx *c, const void *d_in, size_t in_len, zpaqhip_block *blocks, size_t block_cap,
                                   size_t *n_blocks, zpaqhip_segment *segs, size_t seg_cap, size_t *n_segs, void *hip_stream,
                                   zpaqhip_err *err) {
  if (!c || !device_stream_ok(d_in, in_len) || !n_blocks || !n_segs || (!blocks && block_cap) || (!segs && seg_cap)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : c->stream;
  DevScan S;
  if (int rc = scan_device_chain(c, (const uint8_t *)d_in, in_len, stream, S, err)) return rc;
  const int rc = S.R.status;
  zpaqhip_err e2{};
  if (rc) scan_device_err(S, &e2);
  *n_blocks = (size_t)S.R.n_blocks;
  *n_segs = (size_t)S.R.n_segs;
  memset(&c->stats, 0, sizeof c->stats);
  c->stats.blocks = S.R.n_blocks;
  c->stats.in_bytes = in_len;
  auto done = [&](int r) { c->stats.kernel_ms = c->stats.init_ms = S.ms; c->stats.launches = S.launches; return r; };
  if (S.R.n_blocks > block_cap || S.R.n_segs > seg_cap) {      // zpaqhip_scan's rules: count only, or a table too small
    if (block_cap || seg_cap) { set_err(err, ZPAQHIP_E_ARG, -1, -1, "block/segment table too small"); return done(ZPAQHIP_E_ARG); }
    if (rc && err) *err = e2;
    return done(rc);
  }
  if (int rc2 = scan_device_tables(c, (const uint8_t *)d_in, in_len, stream, S, blocks, segs, err)) return rc2;
  if (rc && err) *err = e2;
  return done(rc);
}

extern "C" int zpaqhip_decompress_device(zpaqhip_ctx *c, const void *d_in, size_t in_len, void *d_out, size_t out_cap,
                                         size_t *out_len, zpaqhip_seg_result *results, size_t result_cap, size_t *n_results,
                                         const zpaqhip_opts *opts_in, void *hip_stream, zpaqhip_err *err) {
  if (!c || !device_stream_ok(d_in, in_len) || !out_len || (!d_out && out_cap) || (!results && result_cap)) {
    set_err(err, ZPAQHIP_E_ARG, -1, -1);
    return ZPAQHIP_E_ARG;
  }
  const zpaqhip_opts opts = resolve_opts(opts_in);
  hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : c->stream;
  const uint8_t *in = (const uint8_t *)d_in;
  *out_len = 0;
  if (n_results) *n_results = 0;

  // ---- scan: the tables, and what ends the stream behind the last good block
  DevScan S;
  if (int rc = scan_device_chain(c, in, in_len, stream, S, err)) return rc;
  DevPlan p;
  p.blocks.resize((size_t)S.R.n_blocks);
  p.segs.resize((size_t)S.R.n_segs);
  if (int rc = scan_device_tables(c, in, in_len, stream, S, p.blocks.data(), p.segs.data(), err)) return rc;
  int after_rc = S.R.status;
  zpaqhip_err after_err{};
  if (after_rc) scan_device_err(S, &after_err);
  zpaqhip_stats acc{};
  acc.kernel_ms = acc.init_ms = S.ms;
  acc.launches = S.launches;

  // ---- cut in front of the first block whose model is refused.  (One copy and one wait per header, as ever: fetching
  // all headers in one copy is a change of speed, not of shape, and is left to a change of its own.)
  ModelCut cut;
  std::vector<uint8_t> hdr;
  const int cut_rc = first_bad_model(p.blocks, [&](size_t b, const uint8_t *&h) -> int {
    hdr.resize(p.blocks[b].hdr_len);
    HIPCHK(hipMemcpyAsync(hdr.data(), in + p.blocks[b].hdr_off, hdr.size(), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    h = hdr.data();
    return ZPAQHIP_OK;
  }, cut);
  if (cut_rc) return cut_rc;
  if (cut.rc) { after_rc = cut.rc; after_err = cut.err; }
  p.cut(cut.nb);

  bool first_time = true;
  auto decode = [&](const DevDecode &d, void *to) -> int {
    if (d.ids.empty()) return ZPAQHIP_OK;
    zh_pending P;
    zpaqhip_err e2{};
    int rc = decode_launch(c, in, nullptr, in_len, p.blocks.data(), p.blocks.size(), p.segs.data(), p.segs.size(), d.ids.data(), d.ids.size(),
                           to, d.off.data(), d.cap.data(), opts, stream, P, &e2);
    if (!rc) rc = decode_finish(c, P, p.res.data(), &e2);
    add_kernel_stats(acc, c->stats);
    if (first_time) add_block_stats(acc, c->stats);
    if (rc && !data_error(rc)) { if (err) *err = e2; return rc; }
    note_decoded(p, d.ids);
    return ZPAQHIP_OK;
  };
  float pack_ms = 0;
  uint32_t pack_launches = 0;
  auto pack = [&](const std::vector<ZhFrameEntry> &tab, void *to) {
    return pack_bodies(c, stream, tab, (const uint8_t *)d_out, (uint8_t *)to, pack_ms, pack_launches, err);
  };

  // ---- first decode: straight to d_out what has a place there, the rest to staging
  if (int rc = decode(plan_direct(p, out_cap), d_out)) return rc;
  if (p.bad.limit > p.k) {
    const std::vector<zpaqhip_block> rest(p.blocks.begin() + (ptrdiff_t)p.k, p.blocks.end());
    std::vector<uint64_t> cap, off;
    if (int rc = plan_staging(c, 0, c->out2[0].cap, rest, p.segs, cap, off, err)) return rc;
    if (int rc = decode(plan_staged(p, cap, off), c->out2[0].p)) return rc;
  }
  first_time = false;

  // ---- second decode: whole blocks in a wrong place out of the way, then what outgrew its room with its exact size
  const DevSecond second = plan_device_second(p);
  if (second.fix_bytes) HIPCHK(c->out_fix[0].reserve((size_t)second.fix_bytes + 16));
  if (int rc = pack(second.move, c->out_fix[0].p)) return rc;
  if (int rc = decode(second.redo, c->out_fix[0].p)) return rc;

  // ---- checksums, on the device, where the plaintext lies
  if (opts.verify_sha1) {
    const uint8_t *const base[3] = {(const uint8_t *)d_out, (const uint8_t *)c->out2[0].p, (const uint8_t *)c->out_fix[0].p};
    for (DevWhere w : {DevWhere::kOut, DevWhere::kStaging, DevWhere::kFix}) {
      std::vector<uint32_t> bad;
      if (int rc = sha1_check(c, stream, base[(int)w], device_sha1_table(p, w), p.segs.data(), bad, err)) return rc;
      for (uint32_t s : bad) p.res[s].status = ZPAQHIP_E_SHA1;
    }
    lowest_failed_block(p.blocks, p.res, p.bad);
  }

  // ---- gather: every delivered block that is not in its place yet, in one launch
  const DevGather g = plan_gather(p, out_cap);
  if (int rc = pack(g.entries, d_out)) return rc;
  *out_len = (size_t)g.out_len();

  // ---- report
  const size_t n_res = device_result_count(p);
  if (n_results) *n_results = n_res;
  c->stats = acc;
  c->stats.kernel_ms += pack_ms;
  c->stats.launches += pack_launches;
  c->stats.out_bytes = g.out_len();
  if (results || result_cap) {
    if (n_res > result_cap) { set_err(err, ZPAQHIP_E_ARG, -1, -1, "result table too small"); return ZPAQHIP_E_ARG; }
    device_results(p, g, results);
  }
  if (p.bad.rc) { if (err) *err = p.bad.err; return p.bad.rc; }
  if (after_rc) { if (err) *err = after_err; return after_rc; }
  if (g.out_len() > out_cap) { set_err(err, ZPAQHIP_E_OUTPUT_FULL, -1, -1); return ZPAQHIP_E_OUTPUT_FULL; }
  return ZPAQHIP_OK;
}

// zh_compress.cpp works on a context through this view (zh_ctx_view.h)
zh::CtxView zh::ctx_view(zpaqhip_ctx *c) {
  return zh::CtxView{c->device, c->stream, c->ev0, c->ev1, (const ZhTables *)c->tables.p, &c->stats, c->mem_share};
}
