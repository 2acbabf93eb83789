// zh_enc_chain.hip — lane-per-component ENCODER for gfx950: component chains of up to 64 components and 4 mixers
// (ZH_FAM_CHAIN and its specialisations: min / mid / max, the method models `ci1`, `ci1,1,1,1,2am`, `c0,0,511i2`, ...).
//
// The shape of zh_chain.hip's run-time level walk (its ZhSpec_generic form), turned round: one wavefront owns one block at
// a time and pulls blocks from the work queue of ZhEncLaunch; lane i owns component i of the model; the dependent
// components are resolved level by level from ZhModel's levels; the final probability goes through v_readlane to the
// scalar unit, which runs Encoder.encode (Encoder.cs:87-103) inline on wave-uniform values and writes the coded bytes
// through zh_dev.h's OutBuf into the block's slot (counted past the slot, never written past it).  No P scratch, no second
// pass.  The file repeats what it needs of zh_chain.hip (the decoders stay byte for byte what they were).
//
// A workgroup holds up to four such wavefronts, one per SIMD (ZhEncLaunch::waves is the launch's block size / 64): they share
// the model-independent tables in LDS and nothing else.  Each has its own LDS region (the model's ICM / ISSE pool, then
// EncWaveLds; zh_enc.h's layout), its own arena slot and pulls its own blocks, so the waves of a workgroup run different
// numbers of blocks: the ONE workgroup barrier of the kernel follows the table fill, before the loop, and inside the loop
// a wave orders its lanes' stores and loads against each other with wave_sync() only.
//
// What an encoder knows and a decoder does not, as used here:
//  * the bit: update() takes y from the coded sequence, nothing is fetched two ways or selected;
//  * the byte: both nibbles' contexts (h[i] + 16 * c8, h[i] ^ hmap4) are known when the byte starts, so the hash rows / CM
//    line of the SECOND nibble are requested at their exact addresses before the first bit is predicted and are in
//    registers when the nibble boundary comes (the first nibble's are requested at the previous byte's boundary, before
//    the MATCH search, as in the decoder).  A row the first nibble's write-back has changed meanwhile is taken from
//    the lane's LDS copy instead (small tables: the two nibbles' candidate rows can coincide);
//  * PCOMP is not run: it is only bytes of the coded sequence.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zh_core.h"
#include "zh_dev.h"
#include "zh_enc.h"
#include "zh_model.h"
#include "zh_zpaql_native.h"

using namespace zhcore;
using namespace zhdev;

#pragma clang diagnostic ignored "-Wint-to-pointer-cast"

namespace {

constexpr int kHWords = 512;              // HCOMP H kept in LDS when 2^hh <= 512 (the method models have hh = 9)
constexpr int kMBytes = 4096;             // HCOMP M kept in LDS when 2^hm <= 4096
constexpr int kMaxMix = 4;
constexpr int kCodeBytes = 2048;          // HCOMP program window kept in LDS when it fits

struct alignas(16) EncWaveLds {           // what a wave keeps per block, behind its ICM (256 words) / ISSE (512 words) pool
  uint8_t slot[64][64];                   // per-lane nibble cache (hash row or CM line)
  uint32_t dummy[64];                     // per-lane sink for the stores of lanes a branch-free step does not concern
  uint32_t hreg[kHWords];
  uint8_t mreg[kMBytes];
  uint32_t r[256];
  uint8_t code[kCodeBytes];
  Vm hz;
};
struct alignas(16) EncChainLds {
  ZhTables t;                             // one copy for the workgroup, read-only after the fill
  uint8_t waves[ZH_ENC_CHAIN_LDS - sizeof(ZhTables)];   // region w at w * ZhEncLaunch::lds_stride: pool, then EncWaveLds
};
static_assert(sizeof(EncWaveLds) == ZH_ENC_CHAIN_WAVE_FIXED, "zh_enc.h plans with this size");
static_assert(sizeof(ZhTables) == ZH_ENC_CHAIN_TABLES && sizeof(ZhTables) % 16 == 0, "zh_enc.h plans with this size");
static_assert(sizeof(EncChainLds) == ZH_ENC_CHAIN_LDS && ZH_ENC_CHAIN_LDS <= 163840, "LDS budget");
static_assert(ZH_ENC_CHAIN_TABLES + 64 * 1024 + ZH_ENC_CHAIN_WAVE_FIXED <= ZH_ENC_CHAIN_LDS, "the largest chain (64 units) fits one wave");

// Orders what the lanes of THIS wave stored (LDS and the arena in global memory) before what they load next: the waits of a
// workgroup fence and a scheduling fence, no s_barrier (the other waves of the workgroup are at other blocks).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int clampk(int x, int lo, int hi) { return x < lo ? lo : x > hi ? hi : x; }
typedef __attribute__((address_space(3))) uint8_t *lds_u8_p;
typedef __attribute__((address_space(3))) uint16_t *lds_u16_p;
typedef __attribute__((address_space(3))) uint32_t *lds_u32_p;
__device__ __forceinline__ uint32_t lds_off(const void *p) { return (uint32_t)(uintptr_t)p; }

struct Lane {
  uint32_t type, a0, a1, a2, a3, a4, level;
  uint32_t cmo, hto;                      // arena offsets of the tables (the arena is < 4 GiB for this family)
  uint32_t cm_mask, ht_mask;
  uint32_t sbase;                         // word offset of the ICM/ISSE table in S.small
  uint32_t limit, cxt, a, b, c;           // Component state
  uint32_t h;                             // h[i]
  int p, pj, pk;                          // own prediction and the inputs it was computed from
  int w0, w1;                             // ISSE weights / MIX2 weight / SSE entry of this bit
  uint32_t mbyte, mcur;                   // MATCH: predicted byte, byte being assembled
  int mw[kMaxMix];                        // weights of this lane in each mixer row
  uint32_t memb;                          // bit q set: this lane feeds mixer q
  bool rowvalid;                          // slot holds a row/line that must be written back
};

struct Enc { uint32_t low, high; };

// Encoder.encode (Encoder.cs:87-103) on wave-uniform values; ps = p << 16, so (range * p) >> 16 == mulhi(range, ps)
__device__ __forceinline__ void encode(Enc &e, OutBuf &o, uint32_t y, uint32_t ps, uint32_t lane) {
  const uint32_t mid = uni(e.low + __umulhi(e.high - e.low, ps));
  if (y) e.high = mid; else e.low = mid + 1;
  while (UNLIKELY((e.high ^ e.low) < 0x1000000u)) {
    out_put(o, e.high >> 24, lane);
    e.high = e.high << 8 | 255;
    e.low = e.low << 8;
    e.low += (e.low == 0);
  }
}

// the translated HCOMP programs (tools/gen_zpaql_native.py), by the id build_model put into bits 8-15 of ZhModel::kind:
// the built-in models' with H and M in LDS (typed ds_* accesses), the method models' (hm = 16) with M in the arena
#define ZH_ENC_NAT(name, M_, H_) rc = zh_native_hcomp_##name(ha, hb, hc, hd, hf, c, M_, hz.mmask, H_, hmask, S.r, (Sink *)nullptr, L.budget)
#define ZH_ENC_HCOMP_LDS(id)                                          \
  switch (id) {                                                       \
    case ZH_NATIVE_HCOMP_MIN: ZH_ENC_NAT(min, lds_m, lds_h); break;   \
    case ZH_NATIVE_HCOMP_MID: ZH_ENC_NAT(mid, lds_m, lds_h); break;   \
    case ZH_NATIVE_HCOMP_MAX: ZH_ENC_NAT(max, lds_m, lds_h); break;   \
    default: rc = vm_run(hz, c, nullptr, L.budget); break;            \
  }
#define ZH_ENC_HCOMP_MEM(id)                                          \
  switch (id) {                                                       \
    case ZH_NATIVE_HCOMP_M4: ZH_ENC_NAT(m4, Mptr, Hptr); break;       \
    case ZH_NATIVE_HCOMP_M4W: ZH_ENC_NAT(m4w, Mptr, Hptr); break;     \
    case ZH_NATIVE_HCOMP_M3: ZH_ENC_NAT(m3, Mptr, Hptr); break;       \
    case ZH_NATIVE_HCOMP_M2: ZH_ENC_NAT(m2, Mptr, Hptr); break;       \
    case ZH_NATIVE_HCOMP_M2E: ZH_ENC_NAT(m2e, Mptr, Hptr); break;     \
    case ZH_NATIVE_HCOMP_M2S: ZH_ENC_NAT(m2s, Mptr, Hptr); break;     \
    case ZH_NATIVE_HCOMP_M2SE: ZH_ENC_NAT(m2se, Mptr, Hptr); break;   \
    default: rc = vm_run(hz, c, nullptr, L.budget); break;            \
  }

}  // namespace

extern "C" __global__ __launch_bounds__(256) void zh_enc_chain(ZhEncLaunch L) {
  __shared__ EncChainLds T;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = uni(threadIdx.x >> 6);

  {  // model-independent tables -> LDS, by every wave of the workgroup
    const uint4 *src = reinterpret_cast<const uint4 *>(L.tables);
    uint4 *dst = reinterpret_cast<uint4 *>(&T.t);
    for (uint32_t i = threadIdx.x; i < sizeof(ZhTables) / 16; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();                                     // the kernel's only workgroup barrier: every wave reaches it

  // this wave's LDS region and arena slot
  uint8_t *const region = T.waves + wave * uni(L.lds_stride);
  uint32_t *const small = reinterpret_cast<uint32_t *>(region);
  EncWaveLds &S = *reinterpret_cast<EncWaveLds *>(region + uni(L.lds_pool));
  uint8_t *slot_mem = L.arena + ((uint64_t)blockIdx.x * uni(L.waves) + wave) * L.arena_stride;
  uint8_t *myslot = &S.slot[lane][0];
  const ZhModel *M = L.model;
  const uint32_t n = uni(M->n), depth = uni(M->depth);
  const uint32_t hh = uni(M->hh), hmb = uni(M->hm);

  for (;;) {
    uint32_t bi = 0;
    if (lane == 0) bi = atomicAdd(L.queue, 1u);
    bi = uni((uint32_t)__shfl((int)bi, 0));
    if (bi >= L.n_blocks) break;                       // every wave leaves here, each at its own time

    const ZhEncBlock *bdp = &L.blocks[bi];
    const uint64_t b_n = uni64(bdp->n);                // all of the block's coded bytes, over its segments
    const uint32_t seg0 = uni(bdp->seg0), seg1 = uni(seg0 + uni(bdp->n_seg));

    // ---- Predictor.init (Predictor.cs:82-171): arena tables by all lanes, component by component.  The same initial
    // state as zh_enc_generic.hip's init_slot, with the ICM / ISSE bit-history tables in LDS (below) instead of the arena.
    for (uint32_t i = 0; i < n; ++i) {
      const ZhComp &cp = M->comp[i];
      const uint32_t type = uni(cp.type);
      uint8_t *cm = slot_mem + uni64(cp.cm_off), *ht = slot_mem + uni64(cp.ht_off);
      const uint64_t cmb = uni64(cp.cm_bytes), htb = uni64(cp.ht_bytes);
      uint4 pat = make_uint4(0, 0, 0, 0);
      bool fill_cm = false;
      if (type == ZH_CM) { pat = make_uint4(0x80000000u, 0x80000000u, 0x80000000u, 0x80000000u); fill_cm = true; }
      else if (type == ZH_MATCH) fill_cm = true;
      else if (type == ZH_MIX2) { pat = make_uint4(0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u); fill_cm = true; }
      else if (type == ZH_MIX) { const uint32_t w = 65536u / uni(cp.arg[2]); pat = make_uint4(w, w, w, w); fill_cm = true; }
      if (fill_cm) { uint4 *q = reinterpret_cast<uint4 *>(cm); for (uint64_t k = lane; k < cmb / 16; k += 64) q[k] = pat; }
      if (type == ZH_SSE) {                              // squash((j&31)*64-992)<<17 | start, period 32 entries
        const uint32_t start = uni(cp.arg[2]);
        uint4 *q = reinterpret_cast<uint4 *>(cm);
        for (uint64_t k = lane; k < cmb / 16; k += 64) {
          const uint32_t j = (uint32_t)(k * 4) & 31;
          uint4 v;
          v.x = (uint32_t)T.t.squash[(j + 0) * 64 - 992 + 2048] << 17 | start;
          v.y = (uint32_t)T.t.squash[(j + 1) * 64 - 992 + 2048] << 17 | start;
          v.z = (uint32_t)T.t.squash[(j + 2) * 64 - 992 + 2048] << 17 | start;
          v.w = (uint32_t)T.t.squash[(j + 3) * 64 - 992 + 2048] << 17 | start;
          q[k] = v;
        }
      }
      if (type == ZH_ICM || type == ZH_ISSE || type == ZH_MATCH) {
        uint4 *q = reinterpret_cast<uint4 *>(ht);
        for (uint64_t k = lane; k < htb / 16; k += 64) q[k] = make_uint4(0, 0, 0, 0);
      }
    }
    {  // HCOMP memories: H and M in the arena zeroed; LDS copies zeroed
      const uint64_t h_off = uni64(M->h_off), tail = uni64(M->ph_off) - h_off;
      uint4 *z = reinterpret_cast<uint4 *>(slot_mem + h_off);
      for (uint64_t i = lane; i < tail / 16; i += 64) z[i] = make_uint4(0, 0, 0, 0);
      for (uint32_t i = lane; i < 256; i += 64) S.r[i] = 0;
      for (uint32_t i = lane; i < kHWords; i += 64) S.hreg[i] = 0;
      for (uint32_t i = lane; i < kMBytes / 4; i += 64) reinterpret_cast<uint32_t *>(S.mreg)[i] = 0;
    }

    wave_sync();
    // ---- this lane's component
    Lane me;
    {
      const bool act = lane < n;
      const ZhComp *cp = &M->comp[act ? lane : 0];
      me.type = act ? cp->type : (uint32_t)ZH_NONE;
      me.a0 = cp->arg[0]; me.a1 = cp->arg[1]; me.a2 = cp->arg[2]; me.a3 = cp->arg[3]; me.a4 = cp->arg[4];
      me.level = cp->level;
      me.cmo = (uint32_t)cp->cm_off; me.hto = (uint32_t)cp->ht_off;
      me.cm_mask = cp->cm_mask; me.ht_mask = cp->ht_mask;
      me.sbase = (uint32_t)cp->small_unit * 256u;
      me.limit = me.cxt = me.a = me.b = me.c = 0; me.h = 0;
      me.p = me.pj = me.pk = 0; me.w0 = me.w1 = 0; me.mbyte = me.mcur = 0; me.memb = 0; me.rowvalid = false;
      for (int q = 0; q < kMaxMix; ++q) me.mw[q] = 0;
      switch (me.type) {                                 // scalar parts of Predictor.init
        case ZH_CONS: me.p = ((int)me.a0 - 128) * 4; break;
        case ZH_CM: me.limit = me.a1 * 4; break;
        case ZH_ICM:
          me.limit = 1023;
          for (uint32_t j = 0; j < 256; ++j) {
            const uint32_t n0 = T.t.ns[j * 4 + 2], n1 = T.t.ns[j * 4 + 3];
            small[me.sbase + j] = ((n1 * 2 + 1) << 22) / (n0 + n1 + 1);                 // StateTable.cminit
          }
          break;
        case ZH_ISSE:
          for (uint32_t j = 0; j < 256; ++j) {
            const uint32_t n0 = T.t.ns[j * 4 + 2], n1 = T.t.ns[j * 4 + 3];
            const uint32_t ci = ((n1 * 2 + 1) << 22) / (n0 + n1 + 1);
            small[me.sbase + 2 * j] = 1u << 15;
            small[me.sbase + 2 * j + 1] = (uint32_t)clamp512k(T.t.stretch[ci >> 8] * 1024);
          }
          break;
        case ZH_MATCH: (slot_mem + me.hto)[0] = 1; break;
        case ZH_MIX2: case ZH_MIX: me.c = me.cm_mask + 1; break;
        case ZH_SSE: me.limit = me.a3 * 4; break;
        default: break;
      }
    }
    // mixers (wave-uniform) and which of them each lane feeds
    uint32_t nmix = 0;
    uint32_t mx_lane[kMaxMix] = {0, 0, 0, 0}, mx_j0[kMaxMix] = {0, 0, 0, 0}, mx_m[kMaxMix] = {0, 0, 0, 0}, mx_lv[kMaxMix] = {0, 0, 0, 0};
    uint32_t mx_off[kMaxMix] = {0, 0, 0, 0};
    {
      const uint64_t mm = __ballot(me.type == ZH_MIX);
#pragma unroll
      for (int q = 0; q < kMaxMix; ++q) {
        uint64_t rest = mm;
        for (int k = 0; k < q; ++k) rest &= rest - 1;             // drop the q lowest set bits
        if (!rest) break;
        const uint32_t ml = (uint32_t)__builtin_ctzll(rest);
        mx_lane[q] = ml; mx_j0[q] = rdlane(me.a1, ml); mx_m[q] = rdlane(me.a2, ml); mx_lv[q] = rdlane(me.level, ml);
        mx_off[q] = rdlane(me.cmo, ml);
        if (lane >= mx_j0[q] && lane < mx_j0[q] + mx_m[q]) me.memb |= 1u << q;
        nmix = (uint32_t)q + 1;
      }
    }
    // Level descriptors, one per level, held in lane `level` of lvl_desc:
    //   bits 0-6  : the lane of the level's only non-MIX component, 64 = several, 65 = none
    //   bits 8-11 : its type      bits 12-14 : 1 + index of the mixer evaluated at this level (0 = none, 7 = several)
    //   bits 16-21: first input   bits 24-29 : second input
    uint32_t lvl_desc = 65;
    for (uint32_t lv = 1; lv <= depth && lv < 64; ++lv) {
      const uint64_t at = __ballot(me.level == lv && me.type != ZH_MIX && lane < n);
      uint32_t dsc = at ? 64u : 65u;
      if (__builtin_popcountll(at) == 1) {
        const uint32_t cl = (uint32_t)__builtin_ctzll(at);
        const uint32_t sj = rdlane(me.type == ZH_AVG ? me.a0 : me.a1, cl), sk = rdlane(me.type == ZH_AVG ? me.a1 : me.a2, cl);
        dsc = cl | rdlane(me.type, cl) << 8 | (sj & 63) << 16 | (sk & 63) << 24;
      }
#pragma unroll
      for (int q = 0; q < kMaxMix; ++q)
        if ((uint32_t)q < nmix && mx_lv[q] == lv && !(dsc >> 12 & 7)) dsc |= (uint32_t)(q + 1) << 12;
      uint32_t cnt = 0;
#pragma unroll
      for (int q = 0; q < kMaxMix; ++q) cnt += (uint32_t)q < nmix && mx_lv[q] == lv;
      if (cnt > 1) dsc |= 7u << 12;
      if (lane == lv) lvl_desc = dsc;
    }
    wave_sync();

    // per-lane constants of the branch-free ICM / ISSE steps
    const bool is_icm = me.type == ZH_ICM, is_isse = me.type == ZH_ISSE, is_ii = is_icm || is_isse, is_match = me.type == ZH_MATCH;
    const bool is_cm = me.type == ZH_CM;
    const uint32_t ii_tab = lds_off(&small[0]) + me.sbase * 4;
    const uint32_t ii_sh = is_isse ? 3u : 2u;
    const uint32_t slot_off = lds_off(myslot), dummy_off = lds_off(&S.dummy[lane]), ns_off = lds_off(&T.t.ns[0]);
    int pm0 = 0, pm1 = 0;                                             // MATCH: stretch of +-dt2k[len] for this byte

    // HCOMP machine (ZPAQL.cs:1010-1026): H and M in LDS when they fit
    Vm &hz = S.hz;
    hz.a = hz.b = hz.c = hz.d = hz.f = 0;
    hz.len = uni(M->hcomp_len);
    {
      const uint8_t *gcode = L.code + uni(M->code_off);            // padded window: PAD | program | PAD
      const uint32_t win = hz.len + 2 * ZH_CODE_PAD;
      if (win <= (uint32_t)kCodeBytes) {
        for (uint32_t i = lane; i < win; i += 64) S.code[i] = gcode[i];
        hz.prog = S.code + ZH_CODE_PAD;
      } else hz.prog = gcode + ZH_CODE_PAD;
    }
    hz.hmask = (uint32_t)((1ull << hh) - 1); hz.mmask = (uint32_t)((1ull << hmb) - 1);
    hz.h = hh < 31 && (1u << hh) <= (uint32_t)kHWords ? S.hreg : reinterpret_cast<uint32_t *>(slot_mem + uni64(M->h_off));
    hz.m = hmb < 31 && (1u << hmb) <= (uint32_t)kMBytes ? S.mreg : slot_mem + uni64(M->m_off);
    hz.r = S.r;
    uint32_t *const Hptr = hz.h;
    uint8_t *const Mptr = hz.m;
    const uint32_t hmask = hz.hmask;
    const bool h_in_lds = hz.h == S.hreg;
    const bool hm_lds = h_in_lds && hz.m == S.mreg;
    const uint32_t hnative = (uni(M->kind) >> 8) & 255;              // ahead-of-time translated HCOMP, if known
    uint32_t ha = 0, hb = 0, hc = 0, hd = 0, hf = 0;                  // HCOMP registers A B C D F (wave-uniform)
    const lds_u8_p lds_m = (lds_u8_p)lds_off(S.mreg);
    const lds_u32_p lds_h = (lds_u32_p)lds_off(S.hreg);

    Enc e{1u, 0xFFFFFFFFu};
    OutBuf ob;
    ob.base = L.slots + uni64(bdp->slot_off); ob.cap = uni64(bdp->slot_cap); ob.len = 0; ob.stored = 0; ob.word = 0; ob.park = 0;
    out_room(ob);
    wave_sync();

    // ---- the rows of a nibble (Predictor.find, Predictor.cs:550-567; a CM's 64-byte line), in three steps so that the
    // loads can be put in flight long before they are used: write the lane's row / line back, request the rows of the
    // nibble that starts with (c8x, hmap4x), and select among them into the lane's LDS slot.
    auto row_writeback = [&]() __attribute__((always_inline)) {
      if (is_ii && me.rowvalid) *reinterpret_cast<uint4 *>(slot_mem + me.hto + me.c) = *reinterpret_cast<const uint4 *>(myslot);
      if (is_cm && me.rowvalid) {
        uint4 *g = reinterpret_cast<uint4 *>(slot_mem + me.cmo) + (size_t)me.c * 4;
        const uint4 *l = reinterpret_cast<const uint4 *>(myslot);
        g[0] = l[0]; g[1] = l[1]; g[2] = l[2]; g[3] = l[3];
      }
    };
    // every lane requests three rows (lanes of other types read the first bytes of the arena slot and ignore them): no
    // divergent region, the probes leave back to back
    auto rows_load = [&](uint32_t c8x, uint32_t hmap4x, uint4 &r0, uint4 &r1, uint4 &r2, uint4 &r3, uint32_t &h0) __attribute__((always_inline)) {
      const uint32_t cxt = me.h + 16u * c8x;
      h0 = is_ii ? (cxt * 16u) & (me.ht_mask - 15u) : 0u;
      const uint8_t *tb = slot_mem + (is_ii ? me.hto : 0u);
      r0 = *reinterpret_cast<const uint4 *>(tb + h0);
      r1 = *reinterpret_cast<const uint4 *>(tb + (h0 ^ 16));
      r2 = *reinterpret_cast<const uint4 *>(tb + (h0 ^ 32));
      if (is_cm) {
        h0 = ((me.h ^ hmap4x) & me.cm_mask) >> 4;      // 16-entry line of this nibble
        const uint4 *g = reinterpret_cast<const uint4 *>(slot_mem + me.cmo) + (size_t)h0 * 4;
        r0 = g[0]; r1 = g[1]; r2 = g[2]; r3 = g[3];
      }
    };
    // rows requested BEFORE the lane's last write-back: the row / line that write-back stored (me.c, still in the LDS
    // slot) replaces its stale copy
    auto rows_patch = [&](uint4 &r0, uint4 &r1, uint4 &r2, uint4 &r3, uint32_t h0) __attribute__((always_inline)) {
      const uint4 *l = reinterpret_cast<const uint4 *>(myslot);
      if (is_ii && me.rowvalid) {
        const uint4 cur = l[0];
        if (h0 == me.c) r0 = cur;
        if ((h0 ^ 16) == me.c) r1 = cur;
        if ((h0 ^ 32) == me.c) r2 = cur;
      }
      if (is_cm && me.rowvalid && h0 == me.c) { r0 = l[0]; r1 = l[1]; r2 = l[2]; r3 = l[3]; }
    };
    auto rows_finish = [&](uint32_t c8x, const uint4 &r0, const uint4 &r1, const uint4 &r2, const uint4 &r3, uint32_t h0) __attribute__((always_inline)) {
      const uint32_t chk = ((me.h + 16u * c8x) >> (me.a0 + 2)) & 255;
      const bool m0 = (r0.x & 255) == chk, m1 = (r1.x & 255) == chk, m2 = (r2.x & 255) == chk;
      const uint32_t p0 = (r0.x >> 8) & 255, p1 = (r1.x >> 8) & 255, p2 = (r2.x >> 8) & 255;
      const uint32_t victim = (p0 <= p1 && p0 <= p2) ? h0 : p1 < p2 ? h0 ^ 16 : h0 ^ 32;
      const uint32_t sel = m0 ? h0 : m1 ? h0 ^ 16 : m2 ? h0 ^ 32 : victim;
      const uint4 fresh = make_uint4(chk, 0, 0, 0);
      const uint4 row = m0 ? r0 : m1 ? r1 : m2 ? r2 : fresh;
      if (is_ii) {
        *reinterpret_cast<uint4 *>(myslot) = row;
        me.c = sel;
        me.rowvalid = true;
      }
      if (is_cm) {
        uint4 *l = reinterpret_cast<uint4 *>(myslot);
        l[0] = r0; l[1] = r1; l[2] = r2; l[3] = r3;
        me.c = h0;
        me.rowvalid = true;
      }
    };

    int status = 0;
    if (b_n) {                                           // first nibble of the block (h[] = 0)
      uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0, a2 = a0, a3 = a0;
      uint32_t ah = 0;
      rows_load(1u, 1u, a0, a1, a2, a3, ah);
      rows_finish(1u, a0, a1, a2, a3, ah);
    }

    // The block's segments (Compressor.startSegment .. endSegment, repeated): the model, the rows in flight, the coder and
    // the output buffer carry over a boundary; a segment adds its end-of-segment bit and the record of where it ended.
    // seg0, seg1 and every segment's place and length are wave-uniform, so every lane takes the same trips.
    for (uint32_t sg = seg0; sg < seg1 && !status; ++sg) {
      const uint64_t s_n = uni64(L.segs[sg].n);
      const uint8_t *in = L.in + uni64(L.segs[sg].in_off);
      // 64 bytes of the coded sequence per step, a byte per lane; the next 64 are loaded meanwhile
      uint32_t cv = lane < s_n ? in[lane] : 0u;
      for (uint64_t base = 0; base < s_n && !status; base += 64) {
        const uint64_t ni = base + 64 + lane;
        const uint32_t cnx = ni < s_n ? in[ni] : 0u;
        const uint64_t left = s_n - base;
        const uint32_t cnt = uni(left < 64 ? (uint32_t)left : 64u);
        for (uint32_t l = 0; l < cnt; ++l) {               // Encoder.compress(c), Encoder.cs:39-60: one byte per iteration
          const uint32_t c = rdlane(cv, l);
          e.low = uni(e.low); e.high = uni(e.high);
          encode(e, ob, 0, 0, lane);                       // the EOS flag
          // the second nibble's rows, at their exact addresses: in flight during the first nibble's four bits
          uint4 nr0 = make_uint4(0, 0, 0, 0), nr1 = nr0, nr2 = nr0, nr3 = nr0;
          uint32_t nh0 = 0;
          const uint32_t c8b = 16u | c >> 4, hmap4b = c8b << 4 | 1u;
          rows_load(c8b, hmap4b, nr0, nr1, nr2, nr3, nh0);
          uint32_t c8 = 1, hmap4 = 1;                      // Predictor.cs:20-21
          for (int bit = 0; bit < 8; ++bit) {
            c8 = uni(c8); hmap4 = uni(hmap4);
            const uint32_t y = (c >> (7 - bit)) & 1u;
            const uint32_t hm15 = hmap4 & 15;
            // ================= predict, level 0 (Predictor.cs:259-343) =================
            uint32_t rows[kMaxMix] = {0, 0, 0, 0};
  #pragma unroll
            for (uint32_t q = 0; q < (uint32_t)kMaxMix; ++q) {      // mixer rows: every input lane loads its own weight
              if (q >= nmix) break;
              const uint32_t rowv = ((me.h + (c8 & me.a4)) & (me.c - 1)) * mx_m[q];    // valid in the mixer lane
              rows[q] = rdlane(rowv, mx_lane[q]);
              const uint32_t *mrow = reinterpret_cast<const uint32_t *>(slot_mem + mx_off[q]) + (lane - mx_j0[q]);
              if (me.memb >> q & 1) me.mw[q] = (int)mrow[rows[q]];
            }
            uint32_t pv = 0, pns = 0;
            int pdt = 0;
            if (is_cm) {
              me.cxt = (me.h ^ hmap4) & 15;
              pv = reinterpret_cast<const uint32_t *>(myslot)[me.cxt];
              me.p = T.t.stretch[pv >> 17];
              pdt = T.t.dt[pv & 0x3ff];
            }
            uint32_t ii_a = 0;
            {
              // every lane walks the same three dependent LDS reads (row byte -> table entry -> stretch);
              // lanes of other types read harmless locations and keep nothing
              const uint32_t sw = *(lds_u32_p)(slot_off + (hm15 & 12));
              const uint32_t st = (sw >> ((hm15 & 3) * 8)) & 255;               // the bit history of this context
              ii_a = ii_tab + (st << ii_sh);
              const uint32_t w_x = *(lds_u32_p)ii_a, w_y = *(lds_u32_p)(ii_a + 4);
              const uint32_t nsv = *(lds_u16_p)(ns_off + st * 4);               // next(state, 0) | next(state, 1) << 8
              const int stv = T.t.stretch[is_icm ? w_x >> 8 : 0];
              if (is_ii) { me.cxt = st; pns = nsv; pv = w_x; me.w0 = (int)w_x; me.w1 = (int)w_y; }
              if (is_icm) me.p = stv;
            }
            {
              const uint32_t cbit = (me.mbyte >> (7 - (me.cxt & 7))) & 1;
              if (is_match) { me.c = me.a ? cbit : me.c; me.p = me.a ? (cbit ? pm1 : pm0) : 0; }
            }
            if (me.type == ZH_MIX2) {
              me.cxt = (me.h + (c8 & me.a4)) & (me.c - 1);
              me.w0 = reinterpret_cast<const uint16_t *>(slot_mem + me.cmo)[me.cxt];
            }
            // ================= predict, dependent levels =================
            for (uint32_t lv = 1; lv <= depth; ++lv) {
              const uint32_t desc = rdlane(lvl_desc, lv & 63);
              const uint32_t one = desc & 127, typ = (desc >> 8) & 15;
              if (LIKELY(one < 64)) {
                // a single component at this level: wave-uniform control flow, operands by v_readlane,
                // every lane computes, only lane `one` keeps the result
                const int pj = (int)rdlane((uint32_t)me.p, (desc >> 16) & 63);
                const bool mine = lane == one;
                if (LIKELY(typ == ZH_ISSE)) {
                  const int v = clamp2k((__mul24(me.w0, pj) + me.w1 * 64) >> 16);
                  me.p = mine ? v : me.p; me.pj = mine ? pj : me.pj;
                } else if (typ == ZH_MIX2) {
                  const int pk = (int)rdlane((uint32_t)me.p, (desc >> 24) & 63);
                  const int v = (__mul24(me.w0, pj) + __mul24(65536 - me.w0, pk)) >> 16;
                  me.p = mine ? v : me.p; me.pj = mine ? pj : me.pj; me.pk = mine ? pk : me.pk;
                } else if (typ == ZH_AVG) {
                  const int pk = (int)rdlane((uint32_t)me.p, (desc >> 24) & 63);
                  const int v = (pj * (int)me.a2 + pk * (256 - (int)me.a2)) >> 8;
                  me.p = mine ? v : me.p;
                } else if (mine) {                       // SSE (Predictor.cs:327-340)
                  me.pj = pj;
                  me.cxt = (me.h + c8) * 32u;
                  int pq = clampk(pj + 992, 0, 1983);
                  const int wt = pq & 63;
                  pq >>= 6;
                  me.cxt += (uint32_t)pq;
                  const uint32_t *cm = reinterpret_cast<const uint32_t *>(slot_mem + me.cmo);
                  const uint32_t e0 = cm[me.cxt & me.cm_mask], e1 = cm[(me.cxt + 1) & me.cm_mask];
                  me.p = T.t.stretch[((e0 >> 10) * (uint32_t)(64 - wt) + (e1 >> 10) * (uint32_t)wt) >> 13];
                  me.cxt += (uint32_t)(wt >> 5);
                  me.w0 = (int)((wt >> 5) ? e1 : e0);    // the entry train() will update
                }
              } else if (one == 64) {
                // several components at this level: every lane gathers its own operands (ds_bpermute)
                const int pj = __shfl(me.p, (int)(me.type == ZH_AVG ? me.a0 : me.a1));
                const int pk = __shfl(me.p, (int)(me.type == ZH_AVG ? me.a1 : me.a2));
                if (me.level == lv) {
                  me.pj = pj; me.pk = pk;
                  switch (me.type) {
                    case ZH_ISSE: me.p = clamp2k((__mul24(me.w0, pj) + me.w1 * 64) >> 16); break;
                    case ZH_AVG: me.p = (pj * (int)me.a2 + pk * (256 - (int)me.a2)) >> 8; break;
                    case ZH_MIX2: me.p = (__mul24(me.w0, pj) + __mul24(65536 - me.w0, pk)) >> 16; break;
                    case ZH_SSE: {
                      me.cxt = (me.h + c8) * 32u;
                      int pq = clampk(pj + 992, 0, 1983);
                      const int wt = pq & 63;
                      pq >>= 6;
                      me.cxt += (uint32_t)pq;
                      const uint32_t *cm = reinterpret_cast<const uint32_t *>(slot_mem + me.cmo);
                      const uint32_t e0 = cm[me.cxt & me.cm_mask], e1 = cm[(me.cxt + 1) & me.cm_mask];
                      me.p = T.t.stretch[((e0 >> 10) * (uint32_t)(64 - wt) + (e1 >> 10) * (uint32_t)wt) >> 13];
                      me.cxt += (uint32_t)(wt >> 5);
                      me.w0 = (int)((wt >> 5) ? e1 : e0);
                      break;
                    }
                    default: break;
                  }
                }
              }
              const uint32_t mq = (desc >> 12) & 7;
              if (mq) {                                   // a MIX: wave reduction over its input lanes
  #pragma unroll
                for (uint32_t q = 0; q < (uint32_t)kMaxMix; ++q) {
                  if (q >= nmix) break;
                  if (mq != 7 ? mq != q + 1 : mx_lv[q] != lv) continue;
                  const int term = (me.memb >> q & 1) ? __mul24(me.mw[q] >> 8, me.p) : 0;
                  const int sum = wave_sum(term);
                  if (lane == mx_lane[q]) me.p = clamp2k(sum >> 8);
                }
              }
            }
            // ================= code the bit =================
            const int sqp = (int)T.t.squash[me.p + 2048];          // squash(p[i]) of every lane, one LDS pass
            const uint32_t pr = rdlane((uint32_t)sqp, n - 1);
            encode(e, ob, y, (pr * 2 + 1) << 16, lane);

            // ================= update (Predictor.cs:363-461) =================
            const int ey = (int)y * 32767;
            const int emix = __mul24(ey - sqp, (int)me.a3) >> 4;   // MIX error term (meaningful in mixer lanes)
  #pragma unroll
            for (uint32_t q = 0; q < (uint32_t)kMaxMix; ++q) {      // MIX: error from the mixer lane, weights in the input lanes
              if (q >= nmix) break;
              const int eq = (int)rdlane((uint32_t)emix, mx_lane[q]);
              if (me.memb >> q & 1) {
                me.mw[q] = clamp512k(me.mw[q] + ((__mul24(eq, me.p) + (1 << 12)) >> 13));
                reinterpret_cast<uint32_t *>(slot_mem + mx_off[q])[rows[q] + (lane - mx_j0[q])] = (uint32_t)me.mw[q];
              }
            }
            if (is_cm) {
              const uint32_t cnt_ = pv & 0x3ff;
              const int er = ey - (int)(pv >> 17);
              reinterpret_cast<uint32_t *>(myslot)[me.cxt] = pv + (((uint32_t)er * (uint32_t)pdt) & 0xFFFFFC00u) + (cnt_ < me.limit);
            }
            if (me.type == ZH_SSE) {
              const uint32_t v = (uint32_t)me.w0, cnt_ = v & 0x3ff;
              const int er = ey - (int)(v >> 17);
              reinterpret_cast<uint32_t *>(slot_mem + me.cmo)[me.cxt & me.cm_mask] =
                  v + (((uint32_t)er * (uint32_t)T.t.dt[cnt_]) & 0xFFFFFC00u) + (cnt_ < me.limit);
            }
            {                                              // ICM / ISSE: all lanes, stores of unconcerned lanes go to their dummy cell
              *(lds_u8_p)(is_ii ? slot_off + hm15 : dummy_off) = (uint8_t)(pns >> (y * 8));   // StateTable.next
              const int er = ey - sqp;
              const uint32_t n0 = is_icm ? pv + (uint32_t)((int)(ey - (int)(pv >> 8)) >> 2)
                                         : (uint32_t)clamp512k(me.w0 + ((__mul24(er, me.pj) + (1 << 12)) >> 13));
              const uint32_t n1 = (uint32_t)clamp512k(me.w1 + ((er + 16) >> 5));
              *(lds_u32_p)(is_ii ? ii_a : dummy_off) = n0;
              *(lds_u32_p)(is_isse ? ii_a + 4 : dummy_off) = n1;
            }
            if (is_match) {
              if (me.c != y) me.a = 0;
              me.mcur = (me.mcur * 2 + y) & 255;
              ++me.cxt;                                  // finished at the byte boundary below
            }
            if (me.type == ZH_MIX2) {
              const int er = __mul24(ey - sqp, (int)me.a3) >> 5;
              int w = me.w0 + ((er * (me.pj - me.pk) + (1 << 12)) >> 13);
              w = clampk(w, 0, 65535);
              reinterpret_cast<uint16_t *>(slot_mem + me.cmo)[me.cxt] = (uint16_t)w;
            }
            // ---- c8 / hmap4 bookkeeping (Predictor.cs:463-474)
            c8 = uni(c8 * 2 + y);
            if (bit == 3) {
              hmap4 = uni((hmap4 & 0xf) << 5 | y << 4 | 1);
              row_writeback();                             // the first nibble's row, then the rows requested at the byte's start
              rows_patch(nr0, nr1, nr2, nr3, nh0);
              rows_finish(c8, nr0, nr1, nr2, nr3, nh0);
            } else hmap4 = uni((hmap4 & 0x1f0) | (((hmap4 & 0xf) * 2 + y) & 0xf));
          }

          // ---- MATCH at the byte boundary (Predictor.cs:391-410)
          uint32_t need = 0, cmv = 0;
          if (is_match) {
            me.cxt = 0;
            (slot_mem + me.hto)[me.limit & me.ht_mask] = (uint8_t)me.mcur;   // the assembled byte; ht(0)=1 is overwritten like the reference
            me.mcur = 0;
            me.limit = (me.limit + 1) & me.ht_mask;
            uint32_t *cm = reinterpret_cast<uint32_t *>(slot_mem + me.cmo);   // still with the h[i] of the byte just coded
            cmv = cm[me.h & me.cm_mask];                 // consumed after HCOMP: the load travels meanwhile
            cm[me.h & me.cm_mask] = me.limit;
          }
          // h[] for the next byte: z.run(c), then H(i) (Predictor.cs:465-469)
          int rc;
          if (hm_lds) { ZH_ENC_HCOMP_LDS(hnative) }
          else { ZH_ENC_HCOMP_MEM(hnative) }
          rc = (int)uni((uint32_t)rc);
          if (rc) { status = rc; break; }
          me.h = h_in_lds ? lds_h[lane & hmask] : Hptr[lane & hmask];
          {                                                // rows of the next byte's first nibble: in flight during MATCH
            uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0, a2 = a0, a3 = a0;
            uint32_t ah = 0;
            row_writeback();
            rows_load(1u, 1u, a0, a1, a2, a3, ah);
            if (is_match) {
              if (me.a == 0) {
                me.b = me.limit - cmv;
                need = (me.b & me.ht_mask) != 0;
              } else me.a += me.a < 255;
            }
            uint64_t nm = __ballot(need != 0);
            while (nm) {                                   // verify candidates with the whole wave
              const uint32_t ml = (uint32_t)__builtin_ctzll(nm);
              nm &= nm - 1;
              const uint32_t lim = rdlane(me.limit, ml), off = rdlane(me.b, ml), msk = rdlane(me.ht_mask, ml);
              const uint8_t *hp = slot_mem + rdlane(me.hto, ml);
              uint32_t len = 0;
              for (uint32_t tb = 0; tb < 256; tb += 64) {
                const uint32_t t = tb + lane;
                const bool eq = t < 255 && hp[(lim - t - 1) & msk] == hp[(lim - t - off - 1) & msk];
                const uint64_t mism = __ballot(!eq);
                if (mism) { len += (uint32_t)__builtin_ctzll(mism); break; }
                len += 64;
              }
              if (lane == ml) me.a = len > 255 ? 255 : len;
            }
            if (is_match) me.mbyte = (slot_mem + me.hto)[(me.limit - me.b) & me.ht_mask];
            {                                              // the two predictions a match of this length can make (Predictor.cs:273-287)
              const int dk = T.t.dt2k[is_match ? me.a : 0];
              pm0 = T.t.stretch[dk & 32767];
              pm1 = T.t.stretch[(-dk) & 32767];
            }
            rows_finish(1u, a0, a1, a2, a3, ah);
          }
        }
        cv = cnx;
      }
      e.low = uni(e.low); e.high = uni(e.high);
      if (!status) encode(e, ob, 1, 0, lane);              // compress(-1): end of segment
      if (lane == 0) L.seg_end[sg] = ob.len;
    }
    out_flush(ob, lane);
    if (lane == 0) {
      ZhEncResult r;
      r.len = ob.len; r.status = status; r.overflow = ob.len > ob.cap;
      L.res[bi] = r;
    }
    wave_sync();
  }
}

extern "C" hipError_t zh_launch_enc_chain(const ZhEncLaunch *L, uint32_t grid, hipStream_t stream) {
  // the regions of the launch's waves lie inside the kernel's LDS block, and the pool in front of each is whole units
  if (L->waves < 1 || L->waves > ZH_ENC_CHAIN_MAX_WAVES || L->lds_pool % 1024 || L->lds_stride % 16 ||
      L->lds_stride < L->lds_pool + ZH_ENC_CHAIN_WAVE_FIXED ||
      (uint64_t)L->waves * L->lds_stride > ZH_ENC_CHAIN_LDS - ZH_ENC_CHAIN_TABLES)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(zh_enc_chain, dim3(grid), dim3(64 * L->waves), 0, stream, *L);
  return hipGetLastError();
}
