// zh_scan.hip — the framing scan of a device-resident stream (zpaqhip_scan_device; the rules are zh_scan_walk.h's).
//
// zh_scan_pass is the streaming kernel: one wave per ZH_SCAN_PIECE bytes, four steps of one aligned 16-byte group per lane,
// the group in front of it (the halo) from the lane below.  Positions 0 .. n are covered, n included: a zero run that
// reaches the end of the stream ends there.  Per group a lane makes three 16-bit masks:
//   tag hits     bit j: the 16 bytes that end with byte j of the group have findBlock's hashes.  The first hash is kept
//                rolling over halo and group (shifts and adds: x12 = x8 + x4); the other three are computed only where it
//                matches, from the bytes themselves.
//   run starts   bit j: byte j is the fourth zero byte of a run (the byte in front of the four is not zero)
//   run ends     bit j: byte j is the first byte behind at least four zero bytes (or lies at n)
// from a dword compare mask of the zero bytes (20 bits: the halo's last four bytes and the group).  Bytes at and behind n
// count as non-zero.  The k-th start and the k-th end of the stream are the same run.
// The lists are made in two passes of that kernel with an exclusive scan between them (zh_scan_offsets): counts per piece,
// then the fill at each piece's offset, in position order — no capacity is guessed and no atomic is needed, since a piece
// belongs to one wave; within a wave the lanes' places come from ballot / mbcnt where every lane has at most one hit (the
// usual case: a hit is rare), else from a shuffle scan.
// The loads never touch a byte at or behind n rounded up to a multiple of 4: whole groups as one 16-byte load where the
// stream is 16-byte aligned, the last group and a 4-byte aligned stream dword by dword.
//
// zh_scan_parse runs zh_scan_parse_block with one lane per tag hit; zh_scan_chain is the serial pass over their records
// (one lane); zh_scan_segments writes the segment records of the chosen blocks, one lane per block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zh_scan.h"

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
static_assert(ZH_SCAN_PIECE == 64 * 16 * 4, "a wave takes four steps of 64 groups");

// the zero bytes of a dword as 4 bits
__device__ __forceinline__ uint32_t zero_bits(uint32_t w) {
  uint32_t t = (w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  t = ~(t | w | 0x7F7F7F7Fu);                                    // 0x80 in every zero byte, exactly
  if (t == 0) return 0;
  return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

// group g of the stream (16 bytes at in + g); dwords at or behind n rounded up to 4 are not read and hold no zero byte
__device__ __forceinline__ void load_group(const uint8_t *in, uint64_t g, uint64_t nr, bool al16, uint32_t w[4]) {
  if (al16 && g + 16 <= nr) {
    const uint4 v = *reinterpret_cast<const uint4 *>(in + g);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = g + 4 * k < nr ? *reinterpret_cast<const uint32_t *>(in + g + 4 * k) : 0xFFFFFFFFu;
  }
}

// One list's share of a step: `mask` has this lane's hits (bit j = position pos0 + j).  FILL: they are written at
// out[base ..] in lane order; base moves on by the wave's hits either way.
template <bool FILL>
__device__ __forceinline__ void emit(uint32_t mask, uint64_t pos0, uint32_t lane, uint64_t &base, uint64_t *out, uint64_t cap) {
  const uint32_t c = __popc(mask);
  const unsigned long long any = __ballot(c != 0);
  if (any == 0) return;
  uint32_t before, total;
  if (__ballot(c > 1) == 0) {
    before = __builtin_amdgcn_mbcnt_hi((uint32_t)(any >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)any, 0u));
    total = (uint32_t)__popcll(any);
  } else {
    uint32_t incl = c;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    before = incl - c;
    total = __shfl(incl, 63);
  }
  if (FILL) {
    uint64_t o = base + before;
    while (mask) {
      const uint32_t j = (uint32_t)__ffs(mask) - 1u;
      mask &= mask - 1u;
      if (o < cap) out[o] = pos0 + j;
      ++o;
    }
  }
  base += total;
}

}  // namespace

// cnt[k * n_pieces + piece], k = 0 tags, 1 run starts, 2 run ends: written by the count pass, read (as offsets) by the fill
template <bool FILL>
__global__ __launch_bounds__(256) void zh_scan_pass(const uint8_t *in, uint64_t n, uint64_t n_pieces, uint64_t *cnt,
                                                    uint64_t *tag, uint64_t *run_start, uint64_t *run_end, uint64_t tag_cap,
                                                    uint64_t run_cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t piece = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (piece >= n_pieces) return;                                 // (the whole wave)
  uint64_t base[3] = {0, 0, 0};
  if (FILL) {
#pragma unroll
    for (int k = 0; k < 3; ++k) base[k] = cnt[k * n_pieces + piece];
  }
  const uint64_t nr = (n + 3) & ~3ull;
  const bool al16 = ((uintptr_t)in & 15u) == 0;
#pragma unroll 1
  for (uint32_t step = 0; step < 4; ++step) {
    const uint64_t g = piece * ZH_SCAN_PIECE + step * 1024u + lane * 16u;
    uint32_t w[4], p[4];
    load_group(in, g, nr, al16, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = __shfl_up(w[k], 1);
    if (lane == 0) {
      if (g >= 16) load_group(in, g - 16, nr, al16, p);
      else p[0] = p[1] = p[2] = p[3] = 0xFFFFFFFFu;             // in front of the stream: no zero byte, no tag
    }
    // ---- zero bytes: 4 of the halo, 16 of the group; positions at and behind n do not count
    const uint32_t vc = n > g ? (uint32_t)(n - g < 16 ? n - g : 16) : 0u;
    const uint32_t vp = g >= 4 && n > g - 4 ? (uint32_t)(n - (g - 4) < 4 ? n - (g - 4) : 4) : 0u;
    const uint32_t zc = (zero_bits(w[0]) | zero_bits(w[1]) << 4 | zero_bits(w[2]) << 8 | zero_bits(w[3]) << 12) & ((1u << vc) - 1u);
    const uint32_t zp = zero_bits(p[3]) & ((1u << vp) - 1u);
    const uint32_t z = zp | zc << 4;
    const uint32_t r4 = z & z >> 1 & z >> 2 & z >> 3;            // bit k: four zero bytes from bit k on
    const uint32_t starts = (r4 >> 1) & ~z & 0xFFFFu;            // bit j: the run's fourth byte is byte j
    const uint32_t ends = r4 & ~(z >> 4) & 0xFFFFu;              // bit j: the run ends in front of byte j
    // ---- tag hits: the first hash over halo and group, the rest where it matches
    uint32_t h = 0, cand = 0;
#pragma unroll
    for (int i = 1; i < 16; ++i) h = (h << 3) + (h << 2) + ((p[i >> 2] >> (8 * (i & 3))) & 255u);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      h = (h << 3) + (h << 2) + ((w[i >> 2] >> (8 * (i & 3))) & 255u);
      cand |= (h == 0xB16B88F1u ? 1u : 0u) << i;
    }
    uint32_t tags = 0;
    while (cand) {                                               // (rare)
      const uint32_t j = (uint32_t)__ffs(cand) - 1u;
      cand &= cand - 1u;
      const uint64_t q = g + j + 1;
      if (q >= 16 && q <= n && zh_scan_tag_at(in, q)) tags |= 1u << j;
    }
    emit<FILL>(tags, g + 1, lane, base[0], tag, tag_cap);
    emit<FILL>(starts, g - 3, lane, base[1], run_start, run_cap);
    emit<FILL>(ends, g, lane, base[2], run_end, run_cap);
  }
  if (!FILL && lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) cnt[k * n_pieces + piece] = base[k];
  }
}

// Exclusive scan of each of the three rows of cnt in place; total[k] = the row's sum.  One workgroup.
__global__ __launch_bounds__(1024) void zh_scan_offsets(uint64_t *cnt, uint64_t n_pieces, uint64_t *total) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t per = (n_pieces + 1023) / 1024, lo = t * per, hi = lo + per < n_pieces ? lo + per : n_pieces;
  for (int k = 0; k < 3; ++k) {
    uint64_t *row = cnt + k * n_pieces;
    uint64_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += row[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
      const uint64_t v = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    uint64_t run = part[t] - s;
    if (t == 1023) total[k] = part[t];
    for (uint64_t i = lo; i < hi; ++i) { const uint64_t c = row[i]; row[i] = run; run += c; }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void zh_scan_parse(const uint8_t *in, uint64_t n, ZhScanLists L, ZhScanRec *recs) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < L.n_tag) zh_scan_parse_block(in, n, L, L.tag[i], recs[i], nullptr, 0, 0);
}

__global__ __launch_bounds__(64) void zh_scan_chain_k(const uint8_t *in, uint64_t n, ZhScanLists L, const ZhScanRec *recs,
                                                      zpaqhip_block *blocks, uint64_t block_cap, ZhScanResult *res) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ZhScanResult R;
  zh_scan_chain(in, n, L, recs, blocks, block_cap, R);
  *res = R;
}

__global__ __launch_bounds__(256) void zh_scan_segments(const uint8_t *in, uint64_t n, ZhScanLists L, const zpaqhip_block *blocks,
                                                        uint64_t n_blocks, zpaqhip_segment *segs, uint64_t seg_cap) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n_blocks) zh_scan_fill_segments(in, n, L, blocks[i], (uint32_t)i, segs, seg_cap);
}

static uint32_t grid_for(uint64_t items, uint64_t per) { return (uint32_t)((items + per - 1) / per); }

extern "C" hipError_t zh_launch_scan_count(const uint8_t *in, uint64_t n, uint64_t *cnt, uint64_t *total, hipStream_t stream) {
  const uint64_t np = zh_scan_pieces(n);
  hipLaunchKernelGGL(zh_scan_pass<false>, dim3(grid_for(np, kWaves)), dim3(kThreads), 0, stream, in, n, np, cnt, nullptr, nullptr,
                     nullptr, 0, 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(zh_scan_offsets, dim3(1), dim3(1024), 0, stream, cnt, np, total);
  return hipGetLastError();
}

extern "C" hipError_t zh_launch_scan_fill(const uint8_t *in, uint64_t n, uint64_t *cnt, uint64_t *tag, uint64_t *run_start,
                                          uint64_t *run_end, uint64_t n_tag, uint64_t n_run, hipStream_t stream) {
  const uint64_t np = zh_scan_pieces(n);
  hipLaunchKernelGGL(zh_scan_pass<true>, dim3(grid_for(np, kWaves)), dim3(kThreads), 0, stream, in, n, np, cnt, tag, run_start,
                     run_end, n_tag, n_run);
  return hipGetLastError();
}

extern "C" hipError_t zh_launch_scan_parse(const uint8_t *in, uint64_t n, const ZhScanLists *L, ZhScanRec *recs, hipStream_t stream) {
  if (!L->n_tag) return hipSuccess;
  hipLaunchKernelGGL(zh_scan_parse, dim3(grid_for(L->n_tag, kThreads)), dim3(kThreads), 0, stream, in, n, *L, recs);
  return hipGetLastError();
}

extern "C" hipError_t zh_launch_scan_chain(const uint8_t *in, uint64_t n, const ZhScanLists *L, const ZhScanRec *recs,
                                           zpaqhip_block *blocks, uint64_t block_cap, ZhScanResult *res, hipStream_t stream) {
  hipLaunchKernelGGL(zh_scan_chain_k, dim3(1), dim3(64), 0, stream, in, n, *L, recs, blocks, block_cap, res);
  return hipGetLastError();
}

extern "C" hipError_t zh_launch_scan_segments(const uint8_t *in, uint64_t n, const ZhScanLists *L, const zpaqhip_block *blocks,
                                              uint64_t n_blocks, zpaqhip_segment *segs, uint64_t seg_cap, hipStream_t stream) {
  if (!n_blocks) return hipSuccess;
  hipLaunchKernelGGL(zh_scan_segments, dim3(grid_for(n_blocks, kThreads)), dim3(kThreads), 0, stream, in, n, *L, blocks, n_blocks,
                     segs, seg_cap);
  return hipGetLastError();
}
