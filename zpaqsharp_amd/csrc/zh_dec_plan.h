// zh_dec_plan.h — the decode driver's launch plan: which kernel decodes a block, and how many arena slots, waves and workgroups
// each kernel group of a launch gets.  Host C++ only (no HIP): zh_api.cpp's decode_launch enqueues what plan_decode returns,
// tests/native/dec_plan_main.cpp prints it without a GPU.
#pragma once
#include <algorithm>
#include <vector>

#include "zh_host.h"
#include "zh_zpaql_native.h"

namespace zh {

// ---- which kernel decodes a block (the table is include/zpaqhip.h's): the one place that reads opts.kernel, but for zh_cm's
// one / two blocks per workgroup, decided in plan_decode where the group's size is known.  `group` is the block's family
// after opts.kernel's overrides (its work-queue head, arena region, stream and launch order); `spec` the kernel's specialisation
enum class ZhKernel { Generic, Store, Cm, Chain, Chain2, Nibble };
struct ZhRoute { uint32_t group; ZhKernel kernel; uint32_t spec; uint32_t flags = 0; };   // flags: ZH_LAUNCH_* of the launch
// the specialisations zh_nibble.hip and zh_chain2.hip are built with (zh_nibble_has, zh_chain2_has: defined next to the kernels)
struct ZhKernelHas { int (*nibble)(uint32_t spec); int (*chain2)(uint32_t spec); };

inline ZhRoute route_block(const ZhModel &m, const zpaqhip_opts &o, bool pp_only, const ZhKernelHas &has) {
  const uint32_t K = o.kernel, hk = (m.kind >> 8) & 255u;
  uint32_t f = m.kind & 255u;
  // the method models of min's / mid's shape (zh_framing.cpp) are known to zh_nibble.hip only: the older kernels of these
  // families carry the built-in HCOMP programs
  const bool method = hk == ZH_NATIVE_HCOMP_M4 || hk == ZH_NATIVE_HCOMP_M3 || hk == ZH_NATIVE_HCOMP_M2 || hk == ZH_NATIVE_HCOMP_M2E;
  if (K == 1 || (f == ZH_FAM_STORE && pp_only)) f = ZH_FAM_GENERIC;
  if (K == 3 && f == ZH_FAM_CM1) f = ZH_FAM_CHAIN;
  if (K == 4 && f > ZH_FAM_CHAIN) f = ZH_FAM_CHAIN;                  // stored blocks included
  if ((K == 5 || K == 9) && ((f > ZH_FAM_CHAIN && f < ZH_FAM_STORE && method) || f == ZH_FAM_CHAIN_MID8 || f == ZH_FAM_CHAIN_MIN1))
    f = ZH_FAM_CHAIN;
  const uint32_t nb_flags = K == 11 ? ZH_LAUNCH_MODEL_E8 : 0u;         // zh_nibble.hip: lzpre / bwtrle with E8E9 wave-wide
  switch (f) {
    case ZH_FAM_GENERIC: return {f, ZhKernel::Generic, 0};
    case ZH_FAM_CM1: return {f, ZhKernel::Cm, 0};
    case ZH_FAM_STORE: return {f, ZhKernel::Store, 0, K == 10 || K == 11 ? ZH_LAUNCH_STORE_E8 : 0u};   // the E8E9 forms of lazy2 / lzpre stay on it
    case ZH_FAM_CHAIN_MID8: return {f, ZhKernel::Nibble, 5, nb_flags};  // mid's shape, eight mixer inputs
    case ZH_FAM_CHAIN_MIN1: return {f, ZhKernel::Nibble, 6, nb_flags};  // one ICM on min's loop
  }
  const uint32_t spec = f - ZH_FAM_CHAIN;                              // 0: level walk at run time; 1 / 2 / 3: min / mid / max
  if (spec && has.nibble(spec) && K != 5 && K != 9) return {f, ZhKernel::Nibble, spec, nb_flags};   // 9: the bit-at-a-time form
  if (spec && has.chain2(spec) && K != 5) return {f, ZhKernel::Chain2, spec};
  return {f, ZhKernel::Chain, spec};
}

constexpr uint32_t kDecBlocks = 256;      // blocks in flight a launch asks for without opts.max_concurrent: one per CU

// One kernel group of a launch: the blocks of one route, its region of the arena and the shape of its launch.
struct DecGroup {
  ZhRoute route{};
  std::vector<uint32_t> blocks;           // indices into the launch's block descriptors; LPT order once planned
  uint64_t stride = 256;                  // arena bytes per slot: the largest of the group's models
  uint32_t slots = 0;                     // arena slots = blocks in flight
  bool cm_x2 = false;                     // zh_decode_cm_x2: two blocks per workgroup
  ZhChainWaves mw{};                      // waves > 1: the group runs on zh_decode_chain_mw, mw_grid workgroups of that many waves
  uint32_t mw_grid = 0;
  bool pcall = false;                     // any model with PCOMP memory: zh_chain's variant with translated post-processors
  uint64_t arena_off = 0;
  size_t base = 0;                        // the group's first descriptor in DecPlan::bd_sorted
  uint32_t grid() const { return cm_x2 ? slots / 2 : mw.waves > 1 ? mw_grid : slots; }   // workgroups of the launch
};

struct DecPlan {
  std::vector<DecGroup> groups;           // non-empty, in family order: one launch each
  bool side_by_side = false;              // every group on a stream and an arena region of its own
  bool prof = false;
  uint64_t arena_bytes = 0;
  std::vector<ZhBlockDesc> bd_sorted;     // the descriptors group by group, each group in LPT order
  uint32_t launches = 0, concurrent = 0, kernel_kind = 0;   // zpaqhip_stats
};

// The blocks grouped by route (route_block): one group, one kernel.  Non-empty groups in family order, blocks in input order.
inline std::vector<DecGroup> group_blocks(const std::vector<ZhModel> &models, const std::vector<ZhBlockDesc> &bd,
                                          const zpaqhip_opts &opts, bool pp_only, const ZhKernelHas &has) {
  std::vector<DecGroup> fam(ZH_NFAM_HOST);
  for (size_t k = 0; k < bd.size(); ++k) {
    const ZhModel &m = models[bd[k].model];
    const ZhRoute r = route_block(m, opts, pp_only, has);
    DecGroup &g = fam[r.group];
    g.route = r;
    g.blocks.push_back((uint32_t)k);
    g.stride = std::max<uint64_t>(g.stride, m.arena_bytes);
    g.pcall |= (m.ph | m.pm) != 0;
  }
  fam.erase(std::remove_if(fam.begin(), fam.end(), [](const DecGroup &g) { return g.blocks.empty(); }), fam.end());
  return fam;
}

// The arena that gives every block (up to kDecBlocks per group, or opts.max_concurrent) its slot.
inline uint64_t arena_wish(const std::vector<DecGroup> &groups, const zpaqhip_opts &opts) {
  uint64_t wish = 0;
  for (const DecGroup &g : groups)
    wish += g.stride * std::min<uint64_t>(g.blocks.size(), opts.max_concurrent ? opts.max_concurrent : kDecBlocks);
  return wish;
}

// Slots, waves, workgroups and arena region of every group of group_blocks, for `mem_budget` bytes of arena on a device of
// `cus` compute units.  `weight`: per block, what orders a group (coded bytes).  `prof`: the diagnostic build with in-kernel
// stamps.  ZPAQHIP_E_DEVICE_MEM when a group's model does not get one slot.
inline int plan_decode(std::vector<DecGroup> groups, const std::vector<ZhModel> &models, const std::vector<ZhBlockDesc> &bd,
                       const std::vector<uint64_t> &weight, const zpaqhip_opts &opts, bool prof, uint32_t cus,
                       uint64_t mem_budget, bool serial_families, DecPlan &plan, zpaqhip_err *err) {
  plan = DecPlan();
  plan.prof = prof;
  // arena: one region per kernel family when all of them fit at once (the families then run side by side: an archive
  // that mixes models fills the GPU with whatever blocks it has), else one region sized for the most demanding family,
  // used by one family after the other
  uint64_t arena_need = 0, arena_sum = 0;
  for (DecGroup &g : groups) {
    const uint64_t n = g.blocks.size(), max_slots = mem_budget / g.stride;
    if (max_slots == 0) { set_err(err, ZPAQHIP_E_DEVICE_MEM, -1, -1, "Out of memory"); return ZPAQHIP_E_DEVICE_MEM; }
    uint32_t want = opts.max_concurrent ? opts.max_concurrent : kDecBlocks;
    // single-CM blocks beyond one per CU: two per workgroup (zh_decode_cm_x2: 32 LDS windows each instead of 64), so a stream
    // of many blocks uses all four SIMDs of a CU; opts.kernel == 6 forces that form, 2 the one-block form (A/B runs, tests)
    g.cm_x2 = g.route.kernel == ZhKernel::Cm && !prof && opts.kernel != 2 &&
              (opts.kernel == 6 || (!opts.max_concurrent && n > kDecBlocks));
    if (g.cm_x2) want = opts.max_concurrent ? opts.max_concurrent : 2 * kDecBlocks;
    g.slots = (uint32_t)std::min<uint64_t>({(uint64_t)want, max_slots, n});
    if (g.cm_x2) {
      g.slots = (g.slots + 1u) & ~1u;                   // a slot for the second block of the last workgroup
      if (g.slots > max_slots) {                        // ... which memory does not have: whole pairs, or the one-block form
        g.slots = (uint32_t)(max_slots & ~1ull);
        g.cm_x2 = g.slots >= 2;
        if (!g.cm_x2) g.slots = 1;
      }
    }
    // opts.dec_waves >= 2, blocks on zh_chain's run-time level walk: several decoder waves per workgroup, an arena slot
    // each.  The blocks spread over the compute units first; a second, third and fourth wave come with more blocks than
    // workgroups, as many as the LDS plan of the group's models (the smallest: one launch, its pool sized for the largest
    // chain), opts.dec_waves and the blocks per workgroup allow; where memory (or opts.max_concurrent) is short of a slot
    // per wave the waves go before the workgroups.  One wave left: the launch is the one-wave kernel's, as without the option.
    if (g.route.kernel == ZhKernel::Chain && g.route.spec == 0 && !prof && opts.dec_waves >= 2) {
      uint32_t fit = ZH_DEC_CHAIN_MAX_WAVES, units = 0;
      for (uint32_t k : g.blocks) {
        const DecChainPlan p = plan_dec_chain(models[bd[k].model]);
        fit = std::min(fit, p.waves);
        units = std::max(units, p.units);
      }
      const uint32_t grid = std::min<uint32_t>(g.slots, cus);
      const uint64_t room = std::min<uint64_t>(max_slots, opts.max_concurrent ? opts.max_concurrent : UINT32_MAX);
      uint32_t w = (uint32_t)std::min<uint64_t>({(uint64_t)fit, opts.dec_waves, (n + grid - 1) / grid});
      while (w > 1 && (uint64_t)grid * w > room) --w;
      if (w > 1) {
        g.mw.waves = w;
        g.mw.lds_pool = units * 1024u;
        g.mw.lds_stride = zh_dec_chain_stride(units);
        g.mw_grid = grid;
        g.slots = grid * w;                             // one arena slot per resident wave
      }
    }
    arena_need = std::max<uint64_t>(arena_need, g.slots * g.stride);
    g.arena_off = arena_sum;
    arena_sum += (g.slots * g.stride + 255) & ~255ull;
  }
  plan.side_by_side = groups.size() > 1 && arena_sum <= mem_budget && !serial_families;
  plan.arena_bytes = plan.side_by_side ? arena_sum : arena_need;
  plan.bd_sorted.reserve(bd.size());
  for (DecGroup &g : groups) {
    if (!plan.side_by_side) g.arena_off = 0;
    // Longest block first: the work queue then balances the tail (LPT order).
    std::stable_sort(g.blocks.begin(), g.blocks.end(), [&](uint32_t a, uint32_t b) { return weight[a] > weight[b]; });
    g.base = plan.bd_sorted.size();
    for (uint32_t k : g.blocks) plan.bd_sorted.push_back(bd[k]);
    ++plan.launches;
    // (a several-waves launch: the blocks in flight are its waves with a block)
    plan.concurrent = std::max(plan.concurrent, g.mw.waves > 1 ? (uint32_t)std::min<uint64_t>(g.slots, g.blocks.size()) : g.slots);
    const ZhKernel k = g.route.kernel;
    plan.kernel_kind = std::max(plan.kernel_kind, k == ZhKernel::Generic || k == ZhKernel::Store ? 1u : k == ZhKernel::Cm ? 2u : 3u);
  }
  plan.groups = std::move(groups);
  return ZPAQHIP_OK;
}

}  // namespace zh
