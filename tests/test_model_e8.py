"""opts.kernel == KERNEL_MODEL_E8 without a GPU: the constant, the stats field, and zh_e8e9_round.h — a round of the
end-of-segment E8E9 pass in and out of its slot buffers as zh_nibble.hip's nb_e8_pass does it — played on the host as 64
lanes against the oracle's run of the reference's lzpre and bwtrle programs with E8E9."""
import ctypes
import os
import shutil
import subprocess

import pytest

import oracle
import zpaqsharp_amd as z
from tests import model_e8_cases as mc
from tests import store_e8_cases as cases
from tools import methods
from zpaqsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_stats_field_and_opts():
    assert z.KERNEL_MODEL_E8 == 11 and "KERNEL_MODEL_E8" in z.__all__
    assert _lib.Stats.e8_wave_segs.offset == _lib.Stats.kernel_kind.offset + 4 and _lib.Stats.e8_wave_segs.size == 4
    assert not hasattr(_lib.Stats, "reserved")
    assert ctypes.sizeof(_lib.Stats) == _lib.Stats.e8_wave_segs.offset + 4          # the last field: the size has not changed
    o = z.make_opts(kernel=z.KERNEL_MODEL_E8, verify_sha1=True)
    assert (o.kernel, o.verify_sha1, o.struct_size) == (11, 1, ctypes.sizeof(_lib.Opts))


# nb_e8_pass, lane by lane: the flat buffer begins `mis` bytes into an aligned one (the Writer's region begins anywhere), is read
# in dwords where it can be and in bytes elsewhere, and `dst` / `out` are the same place or two (M and the Writer).
HARNESS = r"""
#include <stdint.h>
#include <string.h>
#define ZH_E8W_FN static inline
#include "%s/zpaqsharp_amd/csrc/zh_e8e9_round.h"
extern "C" void e8r_regs(uint32_t *r) { for (int i = 0; i < 7; ++i) r[i] = 77u; zh_e8w_regs_after(r[0], r[1], r[2], r[3], r[4], r[5], r[6]); }
// the pass over src[0 .. d): final bytes to dst[0 .. d) (may be src) and, below room, to out (may be src too)
extern "C" int e8r_pass(const uint8_t *src, uint8_t *dst, uint8_t *out, uint32_t room, uint32_t d) {
  static uint32_t in_w[kZhE8wBuf / 4], fin_w[kZhE8wBuf / 4];
  uint8_t *in = (uint8_t *)in_w, *fin = (uint8_t *)fin_w;
  const bool dw = ((uintptr_t)src & 3u) == 0u;
  uint32_t carry = kZhE8wNone;
  int most = 0;
  for (uint32_t base = 0; base < d; base += kZhE8wRound) {
    const uint32_t nr = zh_e8w_round_len(base, d);
    memset(in, 0xAA, kZhE8wBuf); memset(fin, 0x55, kZhE8wBuf);
    auto rd = [&](uint32_t p, uint32_t k) -> uint32_t {
      if (p + k > d || k < 1u || k > 4u) __builtin_trap();
      uint32_t v = 0;
      if (dw && k == 4u) memcpy(&v, src + p, 4); else for (uint32_t t = 0; t < k; ++t) v |= (uint32_t)src[p + t] << (8u * t);
      return v;
    };
    auto wr = [&](uint32_t p, uint32_t k, uint32_t v) {
      if (p + k > d || k < 1u || k > 4u) __builtin_trap();
      for (uint32_t t = 0; t < k; ++t) dst[p + t] = (uint8_t)(v >> (8u * t));
    };
    for (uint32_t l = 0; l < kZhE8wLanes; ++l) zh_e8w_load(rd, in_w, base, d, l);
    uint32_t ist[kZhE8wLanes], ost[kZhE8wLanes], prev[kZhE8wLanes], steps = 0;
    for (uint32_t l = 0; l < kZhE8wLanes; ++l) {
      ist[l] = l == 0u && carry != kZhE8wNone ? carry : zh_e8w_clean(in + l * kZhE8wSlot);
      ost[l] = zh_e8w_walk(in + l * kZhE8wSlot, fin + l * kZhE8wSlot, base + l * kZhE8wSlice, zh_e8w_count(base, l, d), d, ist[l], kZhE8wNone, &steps);
    }
    int pass = 0;
    for (; pass <= (int)kZhE8wLanes; ++pass) {           // nb_e8_pass's bound
      memcpy(prev, ost, sizeof prev);
      bool any = false;
      for (uint32_t l = 1; l < kZhE8wLanes; ++l) {
        const uint32_t nin = prev[l - 1u];
        if (nin == ist[l]) continue;
        any = true;
        const uint32_t o = zh_e8w_walk(in + l * kZhE8wSlot, fin + l * kZhE8wSlot, base + l * kZhE8wSlice, zh_e8w_count(base, l, d), d, nin, ist[l], &steps);
        if (o != kZhE8wNone) ost[l] = o;
        ist[l] = nin;
      }
      if (!any) break;
    }
    if (pass > (int)kZhE8wLanes) return -1;              // left unsettled
    if (pass > most) most = pass;
    carry = ost[kZhE8wLanes - 1u];
    if (dst) for (uint32_t l = 0; l < kZhE8wLanes; ++l) zh_e8w_store(wr, fin_w, base, d, l);
    for (uint32_t j = 0; j < nr; ++j) if (base + j < room) out[base + j] = fin[zh_e8w_slot(j)];
  }
  return most;
}
#ifdef E8R_MAIN
#include <stdio.h>
#include <stdlib.h>
int main() {                                             // for a sanitizer build: every length around two rounds, every misalignment
  for (uint32_t d = 0; d < 2u * kZhE8wRound + 70u; d += (d < 80u || d > 2u * kZhE8wRound - 8u) ? 1u : 61u)
    for (uint32_t mis = 0; mis < 4u; ++mis) {
      uint8_t *a = (uint8_t *)malloc(d + mis + 1u), *m = (uint8_t *)malloc(d + 1u), *o = (uint8_t *)malloc(d + 1u);
      for (uint32_t i = 0; i < d; ++i) a[mis + i] = (i %% 7u == 0u) ? 0xE8 : (i %% 7u == 4u) ? 0xFF : (uint8_t)(i * 31u);
      if (e8r_pass(a + mis, m, o, d > 7u ? d - 7u : 0u, d) < 0) return 1;
      if (e8r_pass(a + mis, nullptr, a + mis, d, d) < 0) return 1;
      if (d > 7u && memcmp(a + mis, m, d - 7u)) return 2;
      if (d > 7u && memcmp(o, m, d - 7u)) return 3;
      free(a); free(m); free(o);
    }
  puts("ok");
  return 0;
}
#endif
"""


@pytest.fixture(scope="module")
def e8r(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("e8r")
    src = d / "e8r.cpp"
    src.write_text(HARNESS % ROOT)
    so = d / "e8r.so"
    subprocess.run(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.e8r_pass.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]

    def run(data: bytes, mis: int = 0, in_place: bool = False, short: int = 0):
        n = len(data)
        buf = (ctypes.c_uint8 * (n + 8))()                 # ctypes arrays are aligned well beyond 4 bytes
        ctypes.memmove(ctypes.addressof(buf) + mis, data, n)
        m, out = (ctypes.c_uint8 * (n + 1))(), (ctypes.c_uint8 * (n + 1))()
        at = ctypes.addressof(buf) + mis
        most = lib.e8r_pass(at, None if in_place else ctypes.addressof(m), at if in_place else ctypes.addressof(out), max(0, n - short), n)
        assert 0 <= most <= 64
        return (bytes(buf[mis:mis + n]), None) if in_place else (bytes(out[:n]), bytes(m[:n]))
    run.lib, run.src = lib, src
    return run


def test_registers_after_the_pass(e8r):
    """a b c d f r1 r2 as the program's loop and reset line leave them: the translated program's own run says so."""
    r = (ctypes.c_uint32 * 7)()
    e8r.lib.e8r_regs(r)
    assert list(r) == [0, 0, 0, 0, 1, 0, 0]
    # the oracle, through a second segment: after the reset the program starts a code byte (d = 0) at b = 0, so the two
    # literals of segment 2 land in M[0], M[1] and the loop writes just them out
    model, args = methods.model_of("x0,6,1,0,7,16")
    got = oracle.decompress(cases.store_block(model, [cases.literals(args, b"abcdefgh"), cases.literals(args, b"XY")]), cap=64)
    assert got == b"abcdefghXY"


@pytest.mark.parametrize("method", [mc.LZ3, mc.BWT])
def test_rounds_in_and_out_of_the_slots_are_the_reference_program(e8r, method):
    """The 165 and 182 programs on the oracle (as unmodelled blocks: the program is the same, no coder in the way) over every
    pass input, against the schedule fed and emptied by zh_e8e9_round.h: from an aligned and an unaligned flat buffer, to M and
    the Writer with a capacity 7 bytes short (lzpre's call), and in place (bwtrle's)."""
    model, _ = methods.model_of(method)
    plain = methods.model_of(method.split("c")[0].rstrip(","))[0] if "c" in method else model
    assert plain.pcomp == model.pcomp                        # the unmodelled method carries the same program
    for i, (name, x) in enumerate(cases.pass_inputs(64, 4096).items()):
        if method == mc.BWT and len(x) < 2:
            continue                                       # (n_in < 6: not this pass's business)
        pre = mc.pre_of(method, x)
        want = oracle.decompress(cases.store_block(plain, [pre]), cap=len(x) + 64)
        assert len(want) == len(x), name
        if method == mc.BWT:
            assert e8r(x, mis=i & 3, in_place=True)[0] == want, name
        else:
            out, m = e8r(x, mis=i & 3, short=7)
            assert m == want, name                           # (the byte written out at b is the final M[b])
            assert out[:max(0, len(x) - 7)] == want[:max(0, len(x) - 7)] and out[max(0, len(x) - 7):] == bytes(min(7, len(x))), name


def test_harness_under_a_sanitizer(e8r, tmp_path):
    """The same harness as a stand-alone program with AddressSanitizer and UBSan: every length around two rounds, every
    misalignment of the flat buffer, to two places and in place."""
    exe = tmp_path / "e8r_asan"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-DE8R_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), str(e8r.src)], capture_output=True, text=True)
    if r.returncode:
        pytest.skip("no sanitizer runtime for g++ here: " + r.stderr[-200:])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
