// zh_enc_generic.hip — generic ZPAQ block encoder for gfx950: any modelled header, any HCOMP.
//
// The shape of zh_generic.hip: one wavefront owns one block at a time and pulls blocks from a device-scope work queue;
// all 64 lanes initialise the block's model tables in its arena slot, then lane 0 runs the bit-serial chain
//     Encoder.compress (Encoder.cs:39-104)  ->  Predictor.predict0 / update0 (Predictor.cs:245-475)  ->  ZPAQL.run0
// through zh_core.h: the loop of BlockWriter::compress_byte in ../gen/zpaqgen.cpp, on the device.  This kernel is the
// correctness floor of zpaqhip_compress_blocks (min, mid, max, the method models, arbitrary headers, and every block
// with opts.kernel == 1); the single-CM blocks of ZH_FAM_CM1 have the window-parallel encoder of zh_enc_cm.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zh_core.h"
#include "zh_enc.h"
#include "zh_model.h"

using namespace zhcore;

namespace {

__device__ void fill16(uint8_t *dst, uint64_t bytes, uint4 pat, uint32_t lane) {
  uint4 *q = reinterpret_cast<uint4 *>(dst);
  for (uint64_t i = lane; i < bytes / 16; i += 64) q[i] = pat;
}

// Predictor.init() per component (Predictor.cs:94-167) + ZPAQL.init (ZPAQL.cs:1010-1026), executed by all 64 lanes:
// the same initial state zh_generic.hip's init_slot gives a decoder (and ../gen/zpaqgen.cpp's host_init_slot the CPU
// encoder).
__device__ void init_slot(const ZhModel *M, uint8_t *slot, const GenLds *S, uint32_t lane) {
  const uint4 z4 = make_uint4(0, 0, 0, 0);
  for (uint32_t i = 0; i < M->n; ++i) {
    const ZhComp &cp = M->comp[i];
    uint8_t *cm = slot + cp.cm_off, *ht = slot + cp.ht_off;
    switch (cp.type) {
      case ZH_CM:
        fill16(cm, cp.cm_bytes, make_uint4(0x80000000u, 0x80000000u, 0x80000000u, 0x80000000u), lane);
        break;
      case ZH_ICM:
        fill16(ht, cp.ht_bytes, z4, lane);
        for (uint32_t j = lane; j < 256; j += 64) {
          uint32_t n0 = S->t.ns[j * 4 + 2], n1 = S->t.ns[j * 4 + 3];
          ((uint32_t *)cm)[j] = ((n1 * 2 + 1) << 22) / (n0 + n1 + 1);       // StateTable.cminit
        }
        break;
      case ZH_MATCH:
        fill16(cm, cp.cm_bytes, z4, lane);
        fill16(ht, cp.ht_bytes, z4, lane);
        for (uint64_t j = (cp.ht_bytes & ~15ull) + lane; j < cp.ht_bytes; j += 64) ht[j] = 0;
        break;
      case ZH_MIX2:
        fill16(cm, cp.cm_bytes, make_uint4(0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u), lane);
        for (uint64_t j = (cp.cm_bytes & ~15ull) / 2 + lane; j < cp.cm_bytes / 2; j += 64) ((uint16_t *)cm)[j] = 32768;
        break;
      case ZH_MIX: {
        uint32_t w = 65536u / cp.arg[2];
        fill16(cm, cp.cm_bytes, make_uint4(w, w, w, w), lane);
        for (uint64_t j = (cp.cm_bytes & ~15ull) / 4 + lane; j < cp.cm_bytes / 4; j += 64) ((uint32_t *)cm)[j] = w;
        break;
      }
      case ZH_ISSE:
        fill16(ht, cp.ht_bytes, z4, lane);
        for (uint32_t j = lane; j < 256; j += 64) {
          uint32_t n0 = S->t.ns[j * 4 + 2], n1 = S->t.ns[j * 4 + 3];
          uint32_t ci = ((n1 * 2 + 1) << 22) / (n0 + n1 + 1);
          ((int *)cm)[j * 2] = 1 << 15;
          ((int *)cm)[j * 2 + 1] = clamp512k(S->t.stretch[ci >> 8] * 1024);
        }
        break;
      case ZH_SSE: {
        uint32_t start = cp.arg[2];
        uint4 *q = reinterpret_cast<uint4 *>(cm);
        for (uint64_t k = lane; k < cp.cm_bytes / 16; k += 64) {
          uint32_t j = (uint32_t)(k * 4) & 31;
          uint4 v;
          v.x = (uint32_t)S->t.squash[(j + 0) * 64 - 992 + 2048] << 17 | start;
          v.y = (uint32_t)S->t.squash[(j + 1) * 64 - 992 + 2048] << 17 | start;
          v.z = (uint32_t)S->t.squash[(j + 2) * 64 - 992 + 2048] << 17 | start;
          v.w = (uint32_t)S->t.squash[(j + 3) * 64 - 992 + 2048] << 17 | start;
          q[k] = v;
        }
        break;
      }
      default: break;
    }
  }
  fill16(slot + M->h_off, M->arena_bytes - M->h_off, z4, lane);
}

struct Enc { uint32_t low, high; };

// Encoder.encode (Encoder.cs:87-103)
__device__ __forceinline__ void encode(Enc &e, Sink &out, int y, uint32_t p) {
  const uint32_t mid = e.low + (uint32_t)(((uint64_t)(e.high - e.low) * p) >> 16);
  if (y) e.high = mid; else e.low = mid + 1;
  while ((e.high ^ e.low) < 0x1000000u) {
    sink_put(out, e.high >> 24);
    e.high = e.high << 8 | 255;
    e.low = e.low << 8;
    e.low += (e.low == 0);
  }
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void zh_enc_generic(ZhEncLaunch L) {
  __shared__ GenLds S;
  const uint32_t lane = threadIdx.x;
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(L.tables);
    uint4 *dst = reinterpret_cast<uint4 *>(&S.t);
    for (uint32_t i = lane; i < sizeof(ZhTables) / 16; i += 64) dst[i] = src[i];
  }
  __syncthreads();

  uint8_t *slot = L.arena + (uint64_t)blockIdx.x * L.arena_stride;
  const ZhModel *M = L.model;
  const uint32_t n = M->n;

  for (;;) {
    uint32_t bi = 0;
    if (lane == 0) bi = atomicAdd(L.queue, 1u);
    bi = __shfl(bi, 0);
    if (bi >= L.n_blocks) break;
    const ZhEncBlock bd = L.blocks[bi];

    init_slot(M, slot, &S, lane);
    for (uint32_t i = lane; i < 256; i += 64) {
      S.p[i] = 0; S.h[i] = 0; S.r[i] = 0; S.pr[i] = 0;
      S.cs[i] = CompSt{0, 0, 0, 0, 0};
    }
    if (n <= ZH_MAX_LDS_COMP)
      for (uint32_t i = lane; i < n; i += 64) S.cd[i] = M->comp[i];
    __syncthreads();

    if (lane == 0) {
      Pred P;
      P.S = &S;
      P.cd = n <= ZH_MAX_LDS_COMP ? S.cd : M->comp;
      P.slot = slot;
      P.n = n;
      P.c8 = 1; P.hmap4 = 1;
      P.z.a = P.z.b = P.z.c = P.z.d = P.z.f = 0;
      P.z.prog = L.code + M->code_off + ZH_CODE_PAD;
      P.z.len = M->hcomp_len;
      P.z.m = slot + M->m_off; P.z.mmask = (uint32_t)((1ull << M->hm) - 1);
      P.z.h = (uint32_t *)(slot + M->h_off); P.z.hmask = (uint32_t)((1ull << M->hh) - 1);
      P.z.r = S.r;
      for (uint32_t i = 0; i < n; ++i) {               // scalar parts of Predictor.init
        const ZhComp &cp = P.cd[i];
        switch (cp.type) {
          case ZH_CONS: S.p[i] = ((int)cp.arg[0] - 128) * 4; break;
          case ZH_CM: S.cs[i].limit = (uint32_t)cp.arg[1] * 4; break;
          case ZH_ICM: S.cs[i].limit = 1023; break;
          case ZH_MATCH: (slot + cp.ht_off)[0] = 1; break;
          case ZH_MIX2: case ZH_MIX: S.cs[i].c = cp.cm_mask + 1; break;
          case ZH_SSE: S.cs[i].limit = (uint32_t)cp.arg[3] * 4; break;
          default: break;
        }
      }
      Sink &out = S.sink;
      out.out = L.slots + bd.slot_off; out.cap = bd.slot_cap; out.len = 0;
      Enc e{1u, 0xFFFFFFFFu};
      int status = 0;
      // the block's segments (Compressor.startSegment .. endSegment, repeated): model, coder and output carry over
      for (uint32_t s = bd.seg0; s < bd.seg0 + bd.n_seg && !status; ++s) {
        const ZhEncSeg sg = L.segs[s];
        const uint8_t *in = L.in + sg.in_off;
        for (uint64_t i = 0; i < sg.n && !status; ++i) {   // Encoder.compress(c), Encoder.cs:39-60
          const int c = in[i];
          encode(e, out, 0, 0);
          for (int k = 7; k >= 0; --k) {
            const uint32_t p = (uint32_t)predict(P) * 2 + 1;
            const int y = c >> k & 1;
            encode(e, out, y, p);
            status = update(P, y, L.budget);
            if (status) break;
          }
        }
        if (!status) encode(e, out, 1, 0);              // compress(-1): end of segment
        L.seg_end[s] = out.len;
      }
      ZhEncResult r;
      r.len = out.len; r.status = status; r.overflow = out.len > out.cap;
      L.res[bi] = r;
    }
    __syncthreads();
  }
}

extern "C" hipError_t zh_launch_enc_generic(const ZhEncLaunch *L, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(zh_enc_generic, dim3(grid), dim3(64), 0, stream, *L);
  return hipGetLastError();
}
