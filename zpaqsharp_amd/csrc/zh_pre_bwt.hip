// zh_pre_bwt.hip — LZBuffer's level 3 on the GPU (LZBuffer.cs:205-240): the Burrows-Wheeler transform of every block of a
// batch, from a suffix array built by prefix doubling.  The reference sorts with divsufsort; a suffix array is unique, so
// the bytes are the same whatever builds it.  The end of a block sorts below every byte.
//
// All blocks of a launch share one slot space: block b owns the slots starts[b] .. starts[b + 1] - 1, a suffix is named
// by the slot number of its first byte, and rank[] holds the first slot of a suffix's group, so a rank carries the block
// as its leading bits and every pass runs over all slots of the launch at once, whatever the block sizes.
//
//   zh_bwt_init      slot order = each block's positions from its end down; key = 4 bytes, zero-padded past the end
//   zh_bwt_hist /    one pass of a stable least-significant-digit radix sort of (key, position), 8 bits per pass: a
//   zh_bwt_scatter   wave owns a tile of 4096 pairs; equal digits among its 64 lanes are found with eight ballots, so
//                    the cost of a pass does not depend on the data; the digit counts of all tiles are scanned in between
//   zh_bwt_scan_*    grid-wide scan (sum or max) of 32-bit words in three launches
//   zh_bwt_blockkey  key = the block of a position: the last passes of the first sort put the blocks in order
//   zh_bwt_flags     1st sort: a group starts where the 4 bytes change;  round h: where (rank[i], rank[i + h]) changes.
//                    A suffix of at most h bytes always starts a group: among equal zero-padded keys the order of the
//                    slots (shorter first) is already the right one
//   zh_bwt_rank      rank[position] = first slot of its group (a max-scan of the flags); counts groups of two or more
//   zh_bwt_build     round h: the array is sorted by h bytes, so position - h, read in slot order, is sorted by
//                    rank[i + h]; the h slots per block this leaves free take the block's last h positions, which are
//                    groups of their own already.  One stable sort by rank[i] then orders by 2h bytes
//   zh_bwt_emit      one thread per output byte: out[1 + slot] = in[sa[slot] - 1] (255 and idx where sa[slot] = 0)
//
// The rounds stop when every group is a single suffix, after at most log2(max block) rounds (h = 4, 8, ...): the host
// reads one counter per round.  Every store is a plain C++ store or an atomicAdd on the vector unit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "zh_pre.h"

namespace {

constexpr uint32_t kTile = 4096;          // pairs per wave and radix pass
constexpr uint32_t kChunk = 4096;         // words per workgroup of a scan

__device__ __forceinline__ uint32_t key4(const uint8_t *p, uint32_t l, uint32_t n) {
  uint32_t k = 0;
  for (uint32_t t = 0; t < 4; ++t) k = k << 8 | (l + t < n ? p[l + t] : 0u);
  return k;
}

// the lanes whose digit equals this lane's (active lanes only)
__device__ __forceinline__ uint64_t match8(uint32_t d, bool act) {
  uint64_t m = __ballot(act);
  for (uint32_t b = 0; b < 8; ++b) {
    const uint64_t bal = __ballot((d >> b) & 1);
    m &= ((d >> b) & 1) ? bal : ~bal;
  }
  return m;
}

template <bool MAX> __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return MAX ? max(a, b) : a + b; }

// inclusive scan over the 256 threads of a workgroup (0 is the identity of both operations)
template <bool MAX> __device__ __forceinline__ uint32_t wg_scan(uint32_t v, uint32_t *wt, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d);
    if (lane >= d) v = op<MAX>(v, o);
  }
  if (lane == 63) wt[w] = v;
  __syncthreads();
  uint32_t pre = 0;
  for (uint32_t q = 0; q < w; ++q) pre = op<MAX>(pre, wt[q]);
  total = op<MAX>(op<MAX>(wt[0], wt[1]), op<MAX>(wt[2], wt[3]));
  __syncthreads();
  return op<MAX>(pre, v);
}

}  // namespace

// ---- grid-wide scan ------------------------------------------------------------------------------------------------
template <bool MAX> __global__ __launch_bounds__(256) void zh_bwt_scan_reduce(const uint32_t *p, uint32_t len, uint32_t *sums) {
  __shared__ uint32_t wt[4];
  const uint64_t base = (uint64_t)blockIdx.x * kChunk;
  uint32_t v = 0;
  for (uint32_t t = 0; t < kChunk / 256; ++t) {
    const uint64_t i = base + t * 256 + threadIdx.x;
    if (i < len) v = op<MAX>(v, p[i]);
  }
  uint32_t total;
  wg_scan<MAX>(v, wt, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// pre[c] = everything before chunk c; one workgroup, 256 chunk sums per step
template <bool MAX> __global__ __launch_bounds__(256) void zh_bwt_scan_mid(const uint32_t *sums, uint32_t nchunks, uint32_t *pre) {
  __shared__ uint32_t wt[4];
  uint32_t carry = 0;
  if (threadIdx.x == 0) pre[0] = 0;
  for (uint32_t base = 0; base < nchunks; base += 256) {
    const uint32_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t incl = wg_scan<MAX>(i < nchunks ? sums[i] : 0u, wt, total);
    if (i < nchunks) pre[i + 1] = op<MAX>(carry, incl);
    carry = op<MAX>(carry, total);
  }
}

// in place: the inclusive maximum, or the exclusive sum
template <bool MAX> __global__ __launch_bounds__(256) void zh_bwt_scan_down(uint32_t *p, uint32_t len, const uint32_t *pre) {
  __shared__ uint32_t wt[4];
  const uint64_t base = (uint64_t)blockIdx.x * kChunk;
  uint32_t carry = pre ? pre[blockIdx.x] : 0u;
  for (uint32_t t = 0; t < kChunk / 256; ++t) {
    const uint64_t i = base + t * 256 + threadIdx.x;
    if (base + t * 256 >= len) break;
    const uint32_t v = i < len ? p[i] : 0u;
    uint32_t total;
    const uint32_t incl = wg_scan<MAX>(v, wt, total);
    if (i < len) p[i] = MAX ? op<MAX>(carry, incl) : carry + incl - v;
    carry = op<MAX>(carry, total);
  }
}

// ---- one radix pass --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void zh_bwt_hist(const uint32_t *key, uint32_t n, uint32_t shift, uint32_t nt, uint32_t *counts) {
  __shared__ uint32_t cnt[256];
  const uint32_t lane = threadIdx.x, tile = blockIdx.x;
  for (uint32_t q = 0; q < 4; ++q) cnt[lane + 64 * q] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)tile * kTile;
  for (uint32_t s = 0; s < kTile / 64 && base + s * 64 < n; ++s) {
    const uint64_t i = base + s * 64 + lane;
    const bool act = i < n;
    const uint32_t d = act ? (key[i] >> shift) & 255u : 0u;
    const uint64_t m = match8(d, act);
    if (act && lane == 63u - (uint32_t)__clzll((long long)m)) cnt[d] += (uint32_t)__popcll(m);
    __syncthreads();
  }
  for (uint32_t q = 0; q < 4; ++q) counts[(uint64_t)(lane + 64 * q) * nt + tile] = cnt[lane + 64 * q];
}

// counts[] now holds, per digit and tile, the first output slot.  The wave places 64 pairs per step: a pair goes behind the
// pairs of its digit that earlier steps and lower lanes placed, which keeps the sort stable.
__global__ __launch_bounds__(64) void zh_bwt_scatter(const uint32_t *key, const uint32_t *val, uint32_t *key_out, uint32_t *val_out,
                                                     uint32_t n, uint32_t shift, uint32_t nt, const uint32_t *counts) {
  __shared__ uint32_t off[256];
  const uint32_t lane = threadIdx.x, tile = blockIdx.x;
  for (uint32_t q = 0; q < 4; ++q) off[lane + 64 * q] = counts[(uint64_t)(lane + 64 * q) * nt + tile];
  __syncthreads();
  const uint64_t below = (1ull << lane) - 1;
  const uint64_t base = (uint64_t)tile * kTile;
  for (uint32_t s0 = 0; s0 < kTile / 64 && base + s0 * 64 < n; s0 += 4) {
    uint32_t k[4], v[4];
    for (uint32_t u = 0; u < 4; ++u) {              // four steps' loads in flight
      const uint64_t i = base + (s0 + u) * 64 + lane;
      k[u] = i < n ? key[i] : 0u;
      v[u] = i < n ? val[i] : 0u;
    }
    for (uint32_t u = 0; u < 4; ++u) {
      const uint64_t i = base + (s0 + u) * 64 + lane;
      const bool act = i < n;
      const uint32_t d = (k[u] >> shift) & 255u;
      const uint64_t m = match8(d, act);
      const uint32_t at = off[d] + (uint32_t)__popcll(m & below);
      __syncthreads();
      if (act && lane == 63u - (uint32_t)__clzll((long long)m)) off[d] = at + 1;
      __syncthreads();
      if (act && at < n) {
        key_out[at] = k[u];
        val_out[at] = v[u];
      }
    }
  }
}

// ---- the element-wise passes ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zh_bwt_init(ZhBwtLaunch L) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= L.n) return;
  const uint32_t b = block_of(L.starts, L.n_blocks, (uint32_t)j), s = L.starts[b], nb = L.starts[b + 1] - s;
  const uint32_t l = nb - 1 - ((uint32_t)j - s);
  L.val[0][j] = s + l;
  L.key[0][j] = key4(L.src + L.blocks[b].in_off, l, nb);
}

__global__ __launch_bounds__(256) void zh_bwt_blockkey(ZhBwtLaunch L, uint32_t c) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= L.n) return;
  L.key[c][j] = block_of(L.starts, L.n_blocks, L.val[c][j]);
}

__global__ __launch_bounds__(256) void zh_bwt_build(ZhBwtLaunch L, uint32_t c, uint32_t h) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= L.n) return;
  const uint32_t b = block_of(L.starts, L.n_blocks, (uint32_t)j), s = L.starts[b], nb = L.starts[b + 1] - s;
  const uint32_t l = L.val[c][j] - s;
  const uint32_t i = l >= h ? l - h : nb >= h ? nb - h + l : l;
  L.val[c][j] = s + i;
  L.key[c][j] = L.rank[s + i];
}

// key[c][j] = j where slot j starts a group, else 0 (the keys of the finished sort are not needed any more)
__global__ __launch_bounds__(256) void zh_bwt_flags(ZhBwtLaunch L, uint32_t c, uint32_t h, uint32_t first) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= L.n) return;
  const uint32_t b = block_of(L.starts, L.n_blocks, (uint32_t)j), s = L.starts[b], nb = L.starts[b + 1] - s;
  bool head = j == s;
  if (!head) {
    const uint32_t a = L.val[c][j], p = L.val[c][j - 1];
    const uint64_t la = a - s, lp = p - s;
    if (la + h >= nb || lp + h >= nb) head = true;
    else if (first) {
      const uint8_t *d = L.src + L.blocks[b].in_off;
      head = key4(d, (uint32_t)la, nb) != key4(d, (uint32_t)lp, nb);
    } else head = L.rank[a] != L.rank[p] || L.rank[a + h] != L.rank[p + h];
  }
  L.key[c][j] = head ? (uint32_t)j : 0u;
}

__global__ __launch_bounds__(256) void zh_bwt_rank(ZhBwtLaunch L, uint32_t c) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool multi = false;
  if (j < L.n) {
    const uint32_t g = L.key[c][j];
    L.rank[L.val[c][j]] = g;
    multi = g != j || (j + 1 < L.n && L.key[c][j + 1] != j + 1);
  }
  const uint64_t bal = __ballot(multi);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(L.multi, (uint32_t)__popcll(bal));
}

__global__ __launch_bounds__(256) void zh_bwt_emit(ZhBwtLaunch L, uint32_t c) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < L.n) {
    const uint32_t b = block_of(L.starts, L.n_blocks, (uint32_t)j), s = L.starts[b];
    const ZhPreBlock B = L.blocks[b];
    const uint32_t l = L.val[c][j] - s;
    const uint64_t slot = j - s;
    uint8_t *out = L.out + B.out_off;
    if (1 + slot < B.out_cap) out[1 + slot] = l && l <= B.n ? L.src[B.in_off + l - 1] : (uint8_t)255;
    if (!l)
      for (uint32_t t = 0; t < 4; ++t)
        if (B.n + 1 + t < B.out_cap) out[B.n + 1 + t] = (uint8_t)((slot + 1) >> (8 * t));
  } else if (j < (uint64_t)L.n + L.n_blocks) {
    const uint32_t b = (uint32_t)(j - L.n);
    const ZhPreBlock B = L.blocks[b];
    uint8_t *out = L.out + B.out_off;
    if (B.out_cap) out[0] = B.n ? L.src[B.in_off + B.n - 1] : (uint8_t)255;
    if (!B.n)
      for (uint32_t t = 1; t < 5; ++t)
        if (t < B.out_cap) out[t] = 0;
    L.out_len[b] = B.n + 5;
  }
}

namespace {

struct Run {
  const ZhBwtLaunch &L;
  hipStream_t stream;
  uint32_t launches = 0;
  hipError_t e = hipSuccess;
  uint32_t grid() const { return (uint32_t)(((uint64_t)L.n + 255) / 256); }
  bool ok() {
    if (e == hipSuccess) e = hipGetLastError();
    ++launches;
    return e == hipSuccess;
  }
  template <bool MAX> bool scan(uint32_t *p, uint32_t len) {
    const uint32_t nchunks = (len + kChunk - 1) / kChunk;
    uint32_t *pre = nullptr;
    if (nchunks > 1) {
      pre = L.sums + nchunks;
      hipLaunchKernelGGL(zh_bwt_scan_reduce<MAX>, dim3(nchunks), dim3(256), 0, stream, p, len, L.sums);
      if (!ok()) return false;
      hipLaunchKernelGGL(zh_bwt_scan_mid<MAX>, dim3(1), dim3(256), 0, stream, L.sums, nchunks, pre);
      if (!ok()) return false;
    }
    hipLaunchKernelGGL(zh_bwt_scan_down<MAX>, dim3(nchunks), dim3(256), 0, stream, p, len, pre);
    return ok();
  }
  bool sort(uint32_t &c, uint32_t bits) {           // stable, by the low `bits` bits of key[c]; the result is in key / val[c]
    const uint32_t nt = (L.n + kTile - 1) / kTile;
    for (uint32_t shift = 0; shift < bits; shift += 8) {
      hipLaunchKernelGGL(zh_bwt_hist, dim3(nt), dim3(64), 0, stream, L.key[c], L.n, shift, nt, L.counts);
      if (!ok()) return false;
      if (!scan<false>(L.counts, 256 * nt)) return false;
      hipLaunchKernelGGL(zh_bwt_scatter, dim3(nt), dim3(64), 0, stream, L.key[c], L.val[c], L.key[c ^ 1], L.val[c ^ 1], L.n, shift, nt,
                         L.counts);
      if (!ok()) return false;
      c ^= 1;
    }
    return true;
  }
  bool regroup(uint32_t c, uint32_t h, uint32_t first, uint32_t &multi) {
    hipLaunchKernelGGL(zh_bwt_flags, dim3(grid()), dim3(256), 0, stream, L, c, h, first);
    if (!ok()) return false;
    if (!scan<true>(L.key[c], L.n)) return false;
    if ((e = hipMemsetAsync(L.multi, 0, 4, stream)) != hipSuccess) return false;
    hipLaunchKernelGGL(zh_bwt_rank, dim3(grid()), dim3(256), 0, stream, L, c);
    if (!ok()) return false;
    if ((e = hipMemcpyAsync(&multi, L.multi, 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return false;
    return (e = hipStreamSynchronize(stream)) == hipSuccess;
  }
};

uint32_t bits_of(uint32_t x) {
  uint32_t b = 0;
  while (x) { ++b; x >>= 1; }
  return b;
}

}  // namespace

namespace {

// The suffix sort of all blocks of the launch: afterwards val[c] is the suffix array and rank[] its inverse, both in slots.
bool sort_suffixes(Run &R, uint32_t &c, uint32_t *rounds) {
  const ZhBwtLaunch *L = &R.L;
  hipStream_t stream = R.stream;
  hipLaunchKernelGGL(zh_bwt_init, dim3(R.grid()), dim3(256), 0, stream, *L);
  if (!R.ok() || !R.sort(c, 32)) return false;
  if (L->n_blocks > 1) {
    hipLaunchKernelGGL(zh_bwt_blockkey, dim3(R.grid()), dim3(256), 0, stream, *L, c);
    if (!R.ok() || !R.sort(c, bits_of(L->n_blocks - 1))) return false;
  }
  uint32_t multi = 0;
  if (!R.regroup(c, 4, 1, multi)) return false;
  const uint32_t bits = bits_of(L->n - 1);
  for (uint64_t h = 4; multi && h < L->max_n; h *= 2) {      // at most 29 rounds: max_n < 2^31
    hipLaunchKernelGGL(zh_bwt_build, dim3(R.grid()), dim3(256), 0, stream, *L, c, (uint32_t)h);
    if (!R.ok() || !R.sort(c, bits) || !R.regroup(c, (uint32_t)h, 0, multi)) return false;
    if (rounds) ++*rounds;
  }
  return true;
}

}  // namespace

// The BWT of L->n_blocks blocks (L->n <= 2^31 - 1 bytes together).  *launches grows by the kernels launched, *rounds by the
// doubling rounds after the first sort.
extern "C" hipError_t zh_launch_pre_bwt(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *rounds) {
  if (!L->n_blocks) return hipSuccess;
  Run R{*L, stream};
  uint32_t c = 0;
  if (L->n && !sort_suffixes(R, c, rounds)) return R.e;
  const uint64_t threads = (uint64_t)L->n + L->n_blocks;
  hipLaunchKernelGGL(zh_bwt_emit, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, stream, *L, c);
  R.ok();
  if (launches) *launches += R.launches;
  return R.e;
}

// The suffix sort alone (zh_pre_lzsa.hip searches it): L->val[*c] is the suffix array, L->rank the slot of every position.
extern "C" hipError_t zh_launch_pre_sufsort(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *c) {
  *c = 0;
  if (!L->n_blocks || !L->n) return hipSuccess;
  Run R{*L, stream};
  sort_suffixes(R, *c, nullptr);
  if (launches) *launches += R.launches;
  return R.e;
}

// The radix passes alone (zh_pre_lzht.hip sorts positions by hash slot with them): see zh_pre.h.
extern "C" hipError_t zh_launch_pre_sort(const ZhBwtLaunch *L, hipStream_t stream, uint32_t *launches, uint32_t *c, uint32_t bits) {
  if (!L->n) return hipSuccess;
  Run R{*L, stream};
  R.sort(*c, bits);
  if (launches) *launches += R.launches;
  return R.e;
}
