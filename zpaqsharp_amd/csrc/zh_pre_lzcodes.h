// zh_pre_lzcodes.h — LZBuffer's code writers for levels 1 and 2 (write_literal LZBuffer.cs:387-419, write_match :422-485),
// the only copy: the greedy parse (zh_pre_lz.hip) and the walk over a search's decisions (zh_pre_lzwalk.h) write through
// it.  One wave per block; every lane holds the same state, the stores are plain C++ stores bounded by `cap`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ int lg(uint64_t x) { return x ? 64 - __clzll((long long)x) : 0; }   // LZBuffer.cs:116-126

// the bit writer of LZBuffer level 1 (LSB first, LZBuffer.cs:50-63); every lane holds the same state, lane 0 stores
struct Bits {
  uint8_t *out;
  uint64_t cap, pos;
  uint64_t acc;
  int n;
  __device__ void put(uint64_t x, int k) {
    if (k == 0) return;
    x &= (1ull << k) - 1;
    acc |= x << n;
    n += k;
    while (n > 7) {
      if (threadIdx.x == 0 && pos < cap) out[pos] = (uint8_t)acc;
      ++pos;
      acc >>= 8;
      n -= 8;
    }
  }
};

// The codes of one block: level 1 bits, level 2 bytes; m = args[2], rb as in ZhPreLaunch.  Bytes are counted past cap.
struct LzCodes {
  Bits w;                                         // level 1 writer; level 2 uses w.pos only
  uint32_t level;
  int m, rb;
  __device__ LzCodes(uint8_t *out, uint64_t cap, uint32_t level, int m, int rb) : w{out, cap, 0, 0, 0}, level(level), m(m), rb(rb) {}

  __device__ __forceinline__ void literals(const uint8_t *d, int64_t a, int64_t b) {   // write_literal of d[a .. b)
    if (b <= a) return;
    const int lane = threadIdx.x;
    if (level == 1) {
      const uint64_t lit = (uint64_t)(b - a);
      int ll = lg(lit);
      w.put(0, 2);
      --ll;
      while (ll > 0) {
        --ll;
        w.put(1, 1);
        w.put((lit >> ll) & 1, 1);
      }
      w.put(0, 1);
      for (int64_t s = a; s < b; s += 64) {       // whole bytes at a bit offset of w.n
        const int cnt = (int)min((int64_t)64, b - s);
        const uint32_t v = lane < cnt ? d[s + lane] : 0;
        const uint32_t lo = __shfl(v, lane > 0 ? lane - 1 : 0);
        const uint32_t byte = ((v << w.n) | (lane == 0 ? (uint32_t)w.acc : lo >> (8 - w.n))) & 255;
        if (lane < cnt && w.pos + lane < w.cap) w.out[w.pos + lane] = (uint8_t)byte;
        w.acc = __shfl(v, cnt - 1) >> (8 - w.n);
        w.pos += cnt;
      }
    } else {
      for (int64_t s = a; s < b; s += 64) {       // 64-byte chunks, each after its length - 1
        const int cnt = (int)min((int64_t)64, b - s);
        if (lane == 0 && w.pos < w.cap) w.out[w.pos] = (uint8_t)(cnt - 1);
        if (lane < cnt && w.pos + 1 + lane < w.cap) w.out[w.pos + 1 + lane] = d[s + lane];
        w.pos += cnt + 1;
      }
    }
  }

  __device__ __forceinline__ void match(uint64_t ln, uint64_t off) {   // write_match; offsets stay below 2^24
    if (level == 1) {
      int ll = lg(ln) - 1;
      off += (1ull << rb) - 1;
      const int lo = lg(off) - 1 - rb;
      w.put((uint64_t)(lo + 8) >> 3, 2);
      w.put((uint64_t)lo & 7, 3);
      while (ll > 2) {
        --ll;
        w.put(1, 1);
        w.put((ln >> ll) & 1, 1);
      }
      w.put(0, 1);
      w.put(ln & 3, 2);
      w.put(off, rb);
      w.put(off >> rb, lo);
    } else {
      --off;
      while (ln > 0) {
        const uint64_t len1 = ln > (uint64_t)(2 * m + 63) ? (uint64_t)(m + 63) : ln > (uint64_t)(m + 63) ? ln - m : ln;
        uint8_t c[4];
        int nc;
        if (off < (1u << 16)) {
          c[0] = (uint8_t)(64 + len1 - m); c[1] = (uint8_t)(off >> 8); c[2] = (uint8_t)off; nc = 3;
        } else {
          c[0] = (uint8_t)(128 + len1 - m); c[1] = (uint8_t)(off >> 16); c[2] = (uint8_t)(off >> 8); c[3] = (uint8_t)off; nc = 4;
        }
        if (threadIdx.x == 0)
          for (int t = 0; t < nc; ++t)
            if (w.pos + t < w.cap) w.out[w.pos + t] = c[t];
        w.pos += nc;
        ln -= len1;
      }
    }
  }

  __device__ __forceinline__ uint64_t finish() {  // the level 1 flush; returns the bytes of the block
    if (level == 1 && w.n > 0) {
      if (threadIdx.x == 0 && w.pos < w.cap) w.out[w.pos] = (uint8_t)w.acc;
      ++w.pos;
    }
    return w.pos;
  }
};

}  // namespace
