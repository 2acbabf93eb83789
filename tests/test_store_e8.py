"""zh_e8e9_wave.h — the end-of-segment E8E9 pass of `lazy2` / `lzpre` with E8E9 as a schedule for a wave — played on the
host as 64 lanes against the oracle's interpreter running the reference's program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from tests import store_e8_cases as cases
from tools import methods

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The wave, lane by lane: what zh_store.hip's e8_pass does with shuffles and a ballot is done here with arrays.  Every lane
# takes the outgoing state of the lane before it from the SAME pass (the snapshot `prev`), as lanes in lockstep do.
HARNESS = r"""
#include <stdint.h>
#include <string.h>
#define ZH_E8W_FN static inline
#include "%s/zpaqsharp_amd/csrc/zh_e8e9_wave.h"
extern "C" void e8w_sizes(uint32_t *s) { s[0] = kZhE8wSlice; s[1] = kZhE8wLanes; s[2] = kZhE8wRound; }
// M[0 .. d) in place, the bytes written out to `out`; stat[0] = rounds, [1] = walk passes over all rounds, [2] = most in a round,
// [3] = positions walked
extern "C" void e8w_pass(uint8_t *M, uint32_t d, uint8_t *out, uint64_t *stat) {
  static uint8_t in[kZhE8wBuf], fin[kZhE8wBuf];
  uint32_t carry = kZhE8wNone;
  stat[0] = stat[1] = stat[2] = stat[3] = 0;
  for (uint32_t base = 0; base < d; base += kZhE8wRound) {
    const uint32_t nr = d - base < kZhE8wRound ? d - base : kZhE8wRound;
    memset(in, 0xAA, sizeof in);                        // (what a lane without positions finds in its slot does not matter)
    for (uint32_t r = 0; r < nr + 4u; ++r) {
      const uint8_t v = base + r < d ? M[base + r] : 0;
      const uint32_t l = r / kZhE8wSlice, i = r %% kZhE8wSlice;
      if (l < kZhE8wLanes) in[l * kZhE8wSlot + i] = v;
      if (i < 4u && l > 0u) in[(l - 1u) * kZhE8wSlot + kZhE8wSlice + i] = v;
    }
    uint32_t ist[kZhE8wLanes], ost[kZhE8wLanes], prev[kZhE8wLanes], steps = 0;
    uint64_t passes = 1;
    for (uint32_t l = 0; l < kZhE8wLanes; ++l) {
      ist[l] = l == 0u && carry != kZhE8wNone ? carry : zh_e8w_clean(in + l * kZhE8wSlot);
      ost[l] = zh_e8w_walk(in + l * kZhE8wSlot, fin + l * kZhE8wSlot, base + l * kZhE8wSlice, zh_e8w_count(base, l, d), d, ist[l], kZhE8wNone, &steps);
    }
    for (;;) {
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
      ++passes;
    }
    carry = ost[kZhE8wLanes - 1u];
    for (uint32_t r = 0; r < nr; ++r) out[base + r] = M[base + r] = fin[zh_e8w_slot(r)];
    stat[0] += 1; stat[1] += passes; stat[3] += steps;
    if (passes > stat[2]) stat[2] = passes;
  }
}
"""

METHOD = "x0,6,1,0,7,16"                                  # lzpre + E8E9, matches from one byte: |M| = 2^20


@pytest.fixture(scope="module")
def wave(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("e8w")
    src = d / "e8w.cpp"
    src.write_text(HARNESS % ROOT)
    so = d / "e8w.so"
    subprocess.run(["g++", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    lib = ctypes.CDLL(str(so))
    sizes = (ctypes.c_uint32 * 3)()
    lib.e8w_sizes(sizes)

    def run(data: bytes):
        m = (ctypes.c_uint8 * max(1, len(data))).from_buffer_copy(data if data else b"\0")
        out = (ctypes.c_uint8 * max(1, len(data)))()
        stat = (ctypes.c_uint64 * 4)()
        lib.e8w_pass(m, len(data), out, stat)
        return bytes(out[:len(data)]), bytes(m[:len(data)]), tuple(stat)
    run.slice, run.lanes, run.round = tuple(sizes)
    return run


def test_header_needs_only_stdint(tmp_path):
    """The header compiles for the host with nothing but <stdint.h> before it (the harness above adds <string.h> for itself)."""
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    src = tmp_path / "only.cpp"
    src.write_text(f'#define ZH_E8W_FN static inline\n#include "{ROOT}/zpaqsharp_amd/csrc/zh_e8e9_wave.h"\n'
                   'int main() { uint8_t a[8] = {0xE8, 1, 2, 3, 0xFF, 0, 0, 0}, o[4]; uint32_t s = 0;\n'
                   '  return (int)zh_e8w_walk(a, o, 0u, 1u, 8u, zh_e8w_clean(a), kZhE8wNone, &s) & 0; }\n')
    subprocess.run(["g++", "-Wall", "-Werror", "-std=c++14", "-o", str(tmp_path / "only"), str(src)], check=True)


def _oracle_two_segments(model, args, data: bytes):
    """The reference's program on the oracle: segment 1 writes `data` into M as literals and runs the loop at its end; segment
    2 copies M[0 .. d) onto itself (distance 0 modulo |M|: the program reads and rewrites every cell as it is) and runs the
    loop again.  Returns (bytes of segment 1, bytes of segment 2)."""
    d = len(data)
    pres = [cases.literals(args, data), cases.self_copy(args, d, 1 << model.header[5])]
    got = oracle.decompress(cases.store_block(model, pres), cap=2 * d + 64)
    assert len(got) == 2 * d
    return got[:d], got[d:]


def test_wave_schedule_is_the_reference_program(wave):
    """`out` and the final M of the schedule against the oracle's interpreter running lzpre with E8E9 (LibZPAQ.cs:581-601).
    The oracle shows M only through a program, so M is compared through the next segment: it writes out the loop's result
    over M[0 .. d) as segment 1 left it.  The loop is invertible (a trigger at b leaves M[b] and M[b+4], its own condition,
    alone, so the encoder's pass undoes it from the end backwards): equal bytes in segment 2 mean equal M after segment 1.
    The harness plays that too: its second run starts from the M its first run left."""
    model, args = methods.model_of(METHOD)
    inputs = cases.pass_inputs(wave.slice, wave.round)
    assert wave.round == wave.slice * wave.lanes
    from tests import test_gpu_store_e8
    assert (test_gpu_store_e8.SLICE, test_gpu_store_e8.ROUND) == (wave.slice, wave.round)      # the GPU test builds the same inputs
    # the constructed chains are chains: nearly every trigger is one that the bytes before the pass do not show
    for name in ("chain", "chain_round"):
        data = inputs[name]
        _, hits = cases.pass_model(data)
        before = [b for b in range(len(data) - 4) if (data[b] & 254) == 232 and ((data[b + 4] + 1) & 254) == 0]
        assert len(before) == 1 and len(hits) >= wave.slice + 10, (name, len(before), len(hits))
        assert hits[-1] - hits[0] >= (3 * wave.slice if name == "chain" else wave.slice), name
    assert len(cases.pass_model(inputs["tail_d-5"])[1]) == 1 and len(cases.pass_model(inputs["tail_d-4"])[1]) == 0
    most = 0
    for name, data in inputs.items():
        want1, want2 = _oracle_two_segments(model, args, data)
        out1, m1, stat = wave(data)
        assert out1 == want1, name
        assert m1 == out1, name                             # (the byte written out at b is the final M[b])
        out2, _, _ = wave(m1)
        assert out2 == want2, name
        most = max(most, stat[2])
        if name.startswith("chain"):
            assert stat[2] >= 4, (name, stat)                # a chain is walked a slice per pass
    assert most <= wave.lanes + 1


def test_wave_schedule_on_lazy2(wave):
    """The same loop at the end of lazy2 with E8E9 (LibZPAQ.cs:441-462: d = r4 instead of b), on the dense and chain inputs."""
    model, args = methods.model_of("x0,5,4,0,3,16")
    inputs = cases.pass_inputs(wave.slice, wave.round)
    for name in ("len5", "len6", "dense", "chain", "boundary-1", "tail_d-5", "tail_d-4"):
        data = inputs[name]
        s = cases.store_block(model, [cases.literals(args, data)])
        assert wave(data)[0] == oracle.decompress(s, cap=len(data) + 64), name
