"""The end-of-segment E8E9 pass (zh_e8e9_wave.h, zh_e8e9_round.h) built for the host: the one harness of tests/test_store_e8.py,
tests/test_model_e8.py and tools/store_e8_rate.py.  It plays the 64 lanes of a wave one after the other with the functions
the kernels' driver (zh_e8e9_pass.h) calls — zh_e8w_load, zh_e8w_first, zh_e8w_retake, zh_e8w_store; its own is only what
the driver does with a shuffle, a ballot and a readlane."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every lane takes the outgoing state of the lane before it from the SAME pass (the snapshot `prev`), as lanes in lockstep
# do; lane 0 gets its own, as from __shfl_up.  The flat buffers are read and written in dwords where they are aligned and in
# bytes elsewhere, as zh_nibble.hip's nb_e8_pass does (zh_store.hip's e8_pass: aligned, dst == src).
SOURCE = r"""
#include <stdint.h>
#include <string.h>
#define ZH_E8W_FN static inline
#include "%s/zpaqsharp_amd/csrc/zh_e8e9_round.h"
extern "C" void e8w_sizes(uint32_t *s) { s[0] = kZhE8wSlice; s[1] = kZhE8wLanes; s[2] = kZhE8wRound; }
extern "C" void e8w_regs(uint32_t *r) { for (int i = 0; i < 7; ++i) r[i] = 77u; zh_e8w_regs_after(r[0], r[1], r[2], r[3], r[4], r[5], r[6]); }
// The pass over src[0 .. d): final bytes to dst[0 .. d) (may be src, or null) and, below room, to out (may be src too).
// stat[0] = rounds, [1] = walk passes over all rounds, [2] = most in a round, [3] = positions walked.  -1: a round was left
// unsettled after kZhE8wLanes + 1 times through step 2 (the bound of the driver's loop)
extern "C" int e8w_pass(const uint8_t *src, uint8_t *dst, uint8_t *out, uint64_t room, uint32_t d, uint64_t *stat) {
  static uint32_t in_w[kZhE8wBuf / 4], fin_w[kZhE8wBuf / 4];
  uint8_t *in = (uint8_t *)in_w, *fin = (uint8_t *)fin_w;
  const bool src_dw = ((uintptr_t)src & 3u) == 0u, dst_dw = ((uintptr_t)dst & 3u) == 0u;
  const auto rd = [&](uint32_t p, uint32_t k) -> uint32_t {
    if (p + k > d || k < 1u || k > 4u) __builtin_trap();
    uint32_t v = 0;
    if (src_dw && k == 4u) memcpy(&v, src + p, 4); else for (uint32_t t = 0; t < k; ++t) v |= (uint32_t)src[p + t] << (8u * t);
    return v;
  };
  const auto wr = [&](uint32_t p, uint32_t k, uint32_t v) {
    if (p + k > d || k < 1u || k > 4u) __builtin_trap();
    if (dst_dw && k == 4u) memcpy(dst + p, &v, 4); else for (uint32_t t = 0; t < k; ++t) dst[p + t] = (uint8_t)(v >> (8u * t));
  };
  uint32_t carry = kZhE8wNone;
  stat[0] = stat[1] = stat[2] = stat[3] = 0;
  for (uint32_t base = 0; base < d; base += kZhE8wRound) {
    const uint32_t nr = zh_e8w_round_len(base, d);
    memset(in, 0xAA, kZhE8wBuf); memset(fin, 0x55, kZhE8wBuf);      // (what a lane without positions finds in its slot does not matter)
    for (uint32_t l = 0; l < kZhE8wLanes; ++l) zh_e8w_load(rd, in_w, base, d, l);
    ZhE8wLane lanes[kZhE8wLanes];
    uint32_t prev[kZhE8wLanes], steps = 0;
    for (uint32_t l = 0; l < kZhE8wLanes; ++l) zh_e8w_first(lanes[l], in, fin, base, l, d, carry, &steps);
    bool any = true;
    uint64_t passes = 1;
    for (uint32_t pass = 0; pass <= kZhE8wLanes; ++pass) {
      for (uint32_t l = 0; l < kZhE8wLanes; ++l) prev[l] = lanes[l ? l - 1u : 0u].ost;
      any = false;
      for (uint32_t l = 0; l < kZhE8wLanes; ++l) any |= zh_e8w_retake(lanes[l], in, fin, base, l, d, prev[l], &steps);
      if (!any) break;
      ++passes;
    }
    if (any) return -1;
    carry = lanes[kZhE8wLanes - 1u].ost;
    if (dst) for (uint32_t l = 0; l < kZhE8wLanes; ++l) zh_e8w_store(wr, fin_w, base, d, l);
    for (uint32_t j = 0; j < nr; ++j) if (base + j < room) out[base + j] = fin[zh_e8w_slot(j)];
    stat[0] += 1; stat[1] += passes; stat[3] += steps;
    if (passes > stat[2]) stat[2] = passes;
  }
  return 0;
}
#ifdef E8W_MAIN
#include <stdio.h>
#include <stdlib.h>
int main() {                                             // for a sanitizer build: every length around two rounds, every misalignment
  uint64_t stat[4];
  for (uint32_t d = 0; d < 2u * kZhE8wRound + 70u; d += (d < 80u || d > 2u * kZhE8wRound - 8u) ? 1u : 61u)
    for (uint32_t mis = 0; mis < 4u; ++mis) {
      uint8_t *a = (uint8_t *)malloc(d + mis + 1u), *m = (uint8_t *)malloc(d + 1u), *o = (uint8_t *)malloc(d + 1u), *s = (uint8_t *)malloc(d + 1u);
      for (uint32_t i = 0; i < d; ++i) s[i] = a[mis + i] = (i %% 7u == 0u) ? 0xE8 : (i %% 7u == 4u) ? 0xFF : (uint8_t)(i * 31u);
      if (e8w_pass(a + mis, m, o, d > 7u ? d - 7u : 0u, d, stat) < 0) return 1;       // to M and the Writer, seven bytes short
      if (e8w_pass(a + mis, nullptr, a + mis, d, d, stat) < 0) return 1;              // in place
      if (d > 7u && memcmp(a + mis, m, d - 7u)) return 2;
      if (d > 7u && memcmp(o, m, d - 7u)) return 3;
      if (e8w_pass(s, s, o, d, d, stat) < 0) return 1;                                // M onto itself, aligned: the store kernel's call
      if (memcmp(s, m, d) || memcmp(o, m, d)) return 4;
      free(a); free(m); free(o); free(s);
    }
  puts("ok");
  return 0;
}
#endif
"""


def compile_lib(directory, opt="-O1"):
    """The harness as a shared library in `directory`: (the library, its C++ file)."""
    src, so = os.path.join(str(directory), "e8w.cpp"), os.path.join(str(directory), "e8w.so")
    with open(src, "w") as f:
        f.write(SOURCE % ROOT)
    subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    lib.e8w_pass.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    return lib, src


@pytest.fixture(scope="module")
def e8w(tmp_path_factory):
    """run(data, mis, m_in_place, in_place, short) -> (bytes written out, M afterwards or None, stat): the pass over `data`
    lying `mis` bytes into an aligned buffer.  By default M's final bytes go to a buffer of their own and the bytes written
    out to another, whose capacity is `short` bytes less than needed; m_in_place: M's go back over `data`; in_place: there is
    no M and the bytes written out go over `data`."""
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    lib, src = compile_lib(tmp_path_factory.mktemp("e8w"))
    sizes = (ctypes.c_uint32 * 3)()
    lib.e8w_sizes(sizes)

    def run(data: bytes, mis: int = 0, m_in_place: bool = False, in_place: bool = False, short: int = 0):
        n = len(data)
        buf = (ctypes.c_uint8 * (n + 8))()                 # ctypes arrays are aligned well beyond 4 bytes
        ctypes.memmove(ctypes.addressof(buf) + mis, data, n)
        m, out = (ctypes.c_uint8 * (n + 1))(), (ctypes.c_uint8 * (n + 1))()
        stat = (ctypes.c_uint64 * 4)()
        at = ctypes.addressof(buf) + mis
        rc = lib.e8w_pass(at, None if in_place else at if m_in_place else ctypes.addressof(m), at if in_place else ctypes.addressof(out),
                          max(0, n - short), n, stat)
        assert rc == 0 and stat[2] <= sizes[1] + 1, (rc, tuple(stat))
        there = bytes(buf[mis:mis + n])
        return (there, None, tuple(stat)) if in_place else (bytes(out[:n]), there if m_in_place else bytes(m[:n]), tuple(stat))
    run.lib, run.src = lib, src
    run.slice, run.lanes, run.round = tuple(sizes)
    return run
