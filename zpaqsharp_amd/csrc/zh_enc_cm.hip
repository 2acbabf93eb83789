// zh_enc_cm.hip — window-parallel encoder for blocks of ZH_FAM_CM1: one direct CM whose HCOMP is "a<<= K  *d=a  halt"
// with K >= 9 and at least 2^9 entries.
//
// The entry a bit trains is (c_prev << K ^ hmap4) & mask with hmap4 < 512 (Predictor.cs:208-220,264), so all eight
// entries of a byte lie in the 512-entry window its previous byte picks: the first nibble walks entries 1..15 of the
// window, the second nibble entries 256 + 16 * hi + 1..15.  The table therefore splits into disjoint chains keyed by
// (window, nibble group); each chain starts from 0x80000000 and only the order inside a chain matters.  The plaintext is
// known, so every chain can run at once.  Two launches:
//   zh_enc_cm_model  one workgroup per block: orders the positions by window (list_a) and by (window, high nibble)
//                    (list_b), then its lanes pull chains and write predict()*2+1 of every coded bit to P;
//   zh_enc_cm_code   one wavefront per block: the arithmetic coder (Encoder.cs:39-104) over P, bytes parked in a VGPR and
//                    stored 256 bytes at a time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zh_dev.h"
#include "zh_enc.h"
#include "zh_model.h"

using namespace zhdev;

namespace {

constexpr uint32_t kWG = 256;          // model pass: threads per block
constexpr uint32_t kSortWaves = 2;     // waves that scatter (each owns a contiguous part of the block and its own offsets)

struct SortLds {
  uint32_t off_b[kSortWaves][ZH_ENC_CM_KEYS];   // counts, then the next free slot of each key in list_b
  uint32_t off_a[kSortWaves][256];              // next free slot of each window bin in list_a
  uint32_t part[kWG];
};
struct ChainLds {
  int16_t sh[16384];                            // stretch(x) for x in [16384, 32768); stretch(x) = -stretch(32767 - x) below
  uint16_t sq[4096];                            // squash
  int32_t dt[1024];
  uint32_t st[16][kWG];                         // the chain each lane runs: entries 1..15 of its nibble group
};
union ModelLds {
  SortLds s;
  ChainLds c;
};

__device__ __forceinline__ uint32_t p16_of(const ChainLds &T, uint32_t cm) {
  const uint32_t xv = cm >> 17;
  const int st = xv >= 16384 ? (int)T.sh[xv - 16384] : -(int)T.sh[16383 - xv];
  return (uint32_t)T.sq[st + 2048] * 2 + 1;
}

// Predictor.cs:486-493 in the intended form kept at Predictor.cs:1031-1036 (zh_core.h's train)
__device__ __forceinline__ uint32_t train(const ChainLds &T, uint32_t v, uint32_t limit, uint32_t y) {
  const uint32_t count = v & 0x3ff;
  const int error = (int)(y * 32767u) - (int)(v >> 17);
  return v + (((uint32_t)error * (uint32_t)T.dt[count]) & 0xFFFFFC00u) + (count < limit);
}

}  // namespace

extern "C" __global__ __launch_bounds__(kWG) void zh_enc_cm_model(ZhEncLaunch L) {
  __shared__ ModelLds S;
  __shared__ uint32_t next_chain;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ZhEncBlock bd = L.blocks[blockIdx.x];
  const uint8_t *in = L.in + bd.in_off;
  const uint32_t n = (uint32_t)bd.n;                   // < ZH_ENC_CM_MAX_N (host)
  const uint32_t wm = L.wmask;
  uint32_t *list_a = L.list_a + bd.scr_off, *list_b = L.list_b + bd.scr_off;
  uint32_t *bases = L.bases + (uint64_t)blockIdx.x * (ZH_ENC_CM_KEYS + 1);
  uint16_t *P = L.P + 8 * bd.scr_off;
  const uint32_t half = max(1u, (n + kSortWaves - 1) / kSortWaves);
  static_assert(kSortWaves == 2, "step 2 splits the counts of two parts");

  // 1. histogram of (bin, high nibble) per scatter part.  bin = window of the byte = what of c_prev survives << K & mask
  for (uint32_t k = tid; k < kSortWaves * ZH_ENC_CM_KEYS; k += kWG) (&S.s.off_b[0][0])[k] = 0;
  if (tid == 0) next_chain = 0;
  __syncthreads();
  for (uint32_t i = tid; i < n; i += kWG) {
    const uint32_t cp = i ? in[i - 1] : 0u, c = in[i];
    atomicAdd(&S.s.off_b[i / half][(cp & wm) << 4 | c >> 4], 1u);
  }
  __syncthreads();

  // 2. exclusive scan over the keys (thread t owns bin t = keys 16t..16t+15); run starts to `bases`, per-part offsets to LDS
  {
    uint32_t tot = 0, a0 = 0;
    for (uint32_t k = tid * 16; k < tid * 16 + 16; ++k) {
      a0 += S.s.off_b[0][k];
      for (uint32_t w = 0; w < kSortWaves; ++w) tot += S.s.off_b[w][k];
    }
    S.s.part[tid] = tot;
    S.s.off_a[1][tid] = a0;
    __syncthreads();
    if (tid == 0) {
      uint32_t run = 0;
      for (uint32_t t = 0; t < kWG; ++t) { const uint32_t v = S.s.part[t]; S.s.part[t] = run; run += v; }
    }
    __syncthreads();
    uint32_t run = S.s.part[tid];
    S.s.off_a[0][tid] = run;
    S.s.off_a[1][tid] += run;
    for (uint32_t k = tid * 16; k < tid * 16 + 16; ++k) {
      bases[k] = run;
      const uint32_t c0 = S.s.off_b[0][k], c1 = S.s.off_b[1][k];
      S.s.off_b[0][k] = run;
      S.s.off_b[1][k] = run + c0;
      run += c0 + c1;
    }
    if (tid == kWG - 1) bases[ZH_ENC_CM_KEYS] = run;
  }
  __syncthreads();

  // 3. stable scatter: wave w walks its part 64 positions at a time; lanes of one key take consecutive slots in lane order
  if (wave < kSortWaves) {
    const uint32_t lo = wave * half, hi = min(n, lo + half);
    for (uint32_t t0 = lo; t0 < hi; t0 += 64) {
      const uint32_t i = t0 + lane;
      const bool valid = i < hi;
      const uint32_t cp = valid && i ? in[i - 1] : 0u, c = valid ? in[i] : 0u;
      const uint32_t bin = cp & wm, kb = bin << 4 | c >> 4;
      const uint64_t below = (1ull << lane) - 1;
      uint64_t pend = __ballot(valid);
      while (pend) {
        const uint32_t k = rdlane(kb, (uint32_t)__builtin_ctzll(pend));
        const uint64_t m = __ballot(valid && kb == k);
        const uint32_t base = S.s.off_b[wave][k];
        if (valid && kb == k) list_b[base + __popcll(m & below)] = i << 4 | (c & 15);
        if (lane == 0) S.s.off_b[wave][k] = base + __popcll(m);
        pend &= ~m;
      }
      pend = __ballot(valid);
      while (pend) {
        const uint32_t b = rdlane(bin, (uint32_t)__builtin_ctzll(pend));
        const uint64_t m = __ballot(valid && bin == b);
        const uint32_t base = S.s.off_a[wave][b];
        if (valid && bin == b) list_a[base + __popcll(m & below)] = i << 4 | c >> 4;
        if (lane == 0) S.s.off_a[wave][b] = base + __popcll(m);
        pend &= ~m;
      }
    }
  }
  __threadfence();                                       // list_a / list_b / bases are read by other waves below
  __syncthreads();

  // 4. chains: the tables replace the sort's offsets in LDS; each lane pulls chains (the 256 first-nibble chains first)
  {
    const uint4 *s0 = reinterpret_cast<const uint4 *>(L.tables->stretch + 16384);
    uint4 *d0 = reinterpret_cast<uint4 *>(S.c.sh);
    for (uint32_t i = tid; i < sizeof(S.c.sh) / 16; i += kWG) d0[i] = s0[i];
    const uint4 *s1 = reinterpret_cast<const uint4 *>(L.tables->squash);
    uint4 *d1 = reinterpret_cast<uint4 *>(S.c.sq);
    for (uint32_t i = tid; i < sizeof(S.c.sq) / 16; i += kWG) d1[i] = s1[i];
    const uint4 *s2 = reinterpret_cast<const uint4 *>(L.tables->dt);
    uint4 *d2 = reinterpret_cast<uint4 *>(S.c.dt);
    for (uint32_t i = tid; i < sizeof(S.c.dt) / 16; i += kWG) d2[i] = s2[i];
  }
  __syncthreads();

  const uint32_t limit = L.limit;
  uint32_t cur = 0, end = 0, half_off = 0;
  const uint32_t *list = list_a;
  bool active = true;
  auto fetch = [&]() {
    for (;;) {
      const uint32_t ci = atomicAdd(&next_chain, 1u);
      if (ci >= ZH_ENC_CM_CHAINS) { active = false; return; }
      if (ci < 256) { cur = bases[ci * 16]; end = bases[ci * 16 + 16]; list = list_a; half_off = 0; }
      else { cur = bases[ci - 256]; end = bases[ci - 255]; list = list_b; half_off = 4; }
      if (cur < end) break;
    }
    for (uint32_t j = 1; j < 16; ++j) S.c.st[j][tid] = 0x80000000u;
  };
  fetch();
  uint32_t nxt = active ? list[cur] : 0u;
  while (__any(active)) {
    if (active) {
      const uint32_t e = nxt;
      const uint32_t pos = e >> 4, nib = e & 15;
      if (cur + 1 < end) nxt = list[cur + 1];
      const uint32_t j0 = 1, j1 = 2 | nib >> 3, j2 = 4 | nib >> 2, j3 = 8 | nib >> 1;
      const uint32_t e0 = S.c.st[j0][tid], e1 = S.c.st[j1][tid], e2 = S.c.st[j2][tid], e3 = S.c.st[j3][tid];
      S.c.st[j0][tid] = train(S.c, e0, limit, nib >> 3 & 1);
      S.c.st[j1][tid] = train(S.c, e1, limit, nib >> 2 & 1);
      S.c.st[j2][tid] = train(S.c, e2, limit, nib >> 1 & 1);
      S.c.st[j3][tid] = train(S.c, e3, limit, nib & 1);
      uint2 pv;
      pv.x = p16_of(S.c, e0) | p16_of(S.c, e1) << 16;
      pv.y = p16_of(S.c, e2) | p16_of(S.c, e3) << 16;
      *reinterpret_cast<uint2 *>(P + 8ull * pos + half_off) = pv;
      if (++cur == end) {
        fetch();
        if (active) nxt = list[cur];
      }
    }
  }
}

namespace {

struct Enc { uint32_t low, high; };

// Encoder.encode (Encoder.cs:87-103) on wave-uniform values; ps = p << 16, so (range * p) >> 16 == mulhi(range, ps)
__device__ __forceinline__ void encode(Enc &e, OutBuf &o, uint32_t y, uint32_t ps, uint32_t lane) {
  const uint32_t mid = e.low + __umulhi(e.high - e.low, ps);
  if (y) e.high = mid; else e.low = mid + 1;
  while (UNLIKELY((e.high ^ e.low) < 0x1000000u)) {
    out_put(o, e.high >> 24, lane);
    e.high = e.high << 8 | 255;
    e.low = e.low << 8;
    e.low += (e.low == 0);
  }
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void zh_enc_cm_code(ZhEncLaunch L) {
  const uint32_t lane = threadIdx.x;
  const ZhEncBlock bd = L.blocks[blockIdx.x];
  const uint8_t *in = L.in + bd.in_off;
  const uint4 *P4 = reinterpret_cast<const uint4 *>(L.P + 8 * bd.scr_off);
  const uint32_t n = (uint32_t)bd.n;
  OutBuf o;
  o.base = L.slots + bd.slot_off; o.cap = bd.slot_cap; o.len = 0; o.stored = 0; o.word = 0; o.park = 0;
  out_room(o);
  Enc e{1u, 0xFFFFFFFFu};
  // 64 coded bytes per step: lane l holds byte base + l and its eight probabilities; the next 64 are loaded meanwhile
  uint4 pv = lane < n ? P4[lane] : make_uint4(0, 0, 0, 0);
  uint32_t cv = lane < n ? in[lane] : 0u;
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t ni = base + 64 + lane;
    const uint4 pn = ni < n ? P4[ni] : make_uint4(0, 0, 0, 0);
    const uint32_t cn = ni < n ? in[ni] : 0u;
    const uint32_t cnt = min(64u, n - base);
    for (uint32_t l = 0; l < cnt; ++l) {
      const uint32_t c = rdlane(cv, l);
      const uint32_t w0 = rdlane(pv.x, l), w1 = rdlane(pv.y, l), w2 = rdlane(pv.z, l), w3 = rdlane(pv.w, l);
      encode(e, o, 0, 0, lane);                          // Encoder.compress(c): the EOS flag, then MSB first
      encode(e, o, c >> 7 & 1, w0 << 16, lane);
      encode(e, o, c >> 6 & 1, w0 & 0xFFFF0000u, lane);
      encode(e, o, c >> 5 & 1, w1 << 16, lane);
      encode(e, o, c >> 4 & 1, w1 & 0xFFFF0000u, lane);
      encode(e, o, c >> 3 & 1, w2 << 16, lane);
      encode(e, o, c >> 2 & 1, w2 & 0xFFFF0000u, lane);
      encode(e, o, c >> 1 & 1, w3 << 16, lane);
      encode(e, o, c & 1, w3 & 0xFFFF0000u, lane);
    }
    pv = pn;
    cv = cn;
  }
  encode(e, o, 1, 0, lane);                              // compress(-1)
  out_flush(o, lane);
  if (lane == 0) {
    ZhEncResult r;
    r.len = o.len; r.status = 0; r.overflow = o.len > o.cap;
    L.res[blockIdx.x] = r;
  }
}

// The two passes are launched separately so that the host can time each (zpaqhip_stats: init_ms = the model pass).
extern "C" hipError_t zh_launch_enc_cm_model(const ZhEncLaunch *L, uint32_t n_blocks, hipStream_t stream) {
  if (!n_blocks) return hipSuccess;
  hipLaunchKernelGGL(zh_enc_cm_model, dim3(n_blocks), dim3(kWG), 0, stream, *L);
  return hipGetLastError();
}

extern "C" hipError_t zh_launch_enc_cm_code(const ZhEncLaunch *L, uint32_t n_blocks, hipStream_t stream) {
  if (!n_blocks) return hipSuccess;
  hipLaunchKernelGGL(zh_enc_cm_code, dim3(n_blocks), dim3(64), 0, stream, *L);
  return hipGetLastError();
}
