// zh_lzcopy.h — the chunk schedule of a wave-wide LZ77 match copy inside the program's M array (lzpre, LibZPAQ.cs:625-631:
// `a=*c *b=a c++ b++`, n times, with c = b - off - 1 and M addressed modulo its size).  Plain integer code without any memory
// access: zh_nibble.hip's drain runs it on the scalar unit, tests/test_lz_edges.py compiles it for the host and plays a wave
// over it (all lanes of a chunk load, then all store) against the bytewise copy.
//
// The program copies a byte at a time, so a match that overlaps its source repeats what the copy itself wrote: cell
// pb + i takes the value of cell pb + i - d for i = 0 .. n-1, where d is the distance REDUCED MODULO |M| — the program's
// `c` is only ever used as an address, and addresses wrap.  Two distances have no chunk schedule of their own:
//   d == 0      (the encoded offset is |M| - 1 modulo |M|, e.g. FF FF FF FF): every cell is copied onto itself.  The cells
//               already in M[pb ..] are what the program writes out; nothing is stored.
//   d >= 64     one chunk of 64 never reaches its own output.
// Below 64 a chunk is as wide as the span `back` that the lanes look back, a multiple of d; once the bytes written so far
// and the d cells in front of them cover twice that span, it doubles (the region is periodic with d by then).
//
// In every chunk lane l < width reads cell (pb + done + l - back) & mm and writes cell (pb + done + l) & mm.  The width never
// exceeds back, so no lane reads what a lane of the same chunk writes, nor |M| - back, so that this also holds for the cells
// taken modulo |M| and no chunk overwrites a cell of the first period that a later chunk still reads.  (|M| - back only
// matters for an M of a few hundred cells; it costs one scalar minimum.)  A chunk is at least one cell wide: n chunks at most.
#pragma once
#include <stdint.h>

// the distance the copy really has: dist modulo |M| (mm = |M| - 1); 0 = self-copy
__device__ __forceinline__ uint32_t zh_lz_reduce(uint32_t dist, uint32_t mm) { return dist & mm; }

// width of the chunk that starts `done` cells into a copy of n; back = how far its lanes look back (0: the self-copy)
__device__ __forceinline__ uint32_t zh_lz_width(uint32_t back, uint32_t mm, uint32_t n, uint32_t done) {
  uint32_t m = n - done;
  m = m < 64u ? m : 64u;
  if (back == 0u) return m;
  m = m < back ? m : back;
  const uint32_t wrap = mm + 1u - back;                // (back <= mm: a reduced distance, doubled only while under 64 <= |M| / 2)
  return m < wrap ? m : wrap;
}

// `back` for the next chunk, after `done` cells of the copy (d: the reduced distance, not 0)
__device__ __forceinline__ uint32_t zh_lz_grow(uint32_t d, uint32_t back, uint32_t done, uint32_t mm) {
  return (back < 64u && 2u * back <= done + d && 2u * back <= mm) ? 2u * back : back;
}
