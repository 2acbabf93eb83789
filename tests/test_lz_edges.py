"""The LZ77 post-processors at distances and lengths that only a crafted or damaged code stream contains (CPU side).

tests/lzcodes.py writes lzpre / lazy2 codes token by token and models their expansion independently of the programs;
here its writers are pinned against tools.methods' encoders, the model against the oracle on the whole edge catalogue and
the seeded sweep — with NO ZPAQL budget: every case must terminate on the reference's own terms —, and the chunk schedule
of zh_nibble.hip's wave-wide match copy (zh_lzcopy.h) is compiled for the host and played lane by lane against the
bytewise copy.  tests/test_gpu_lz_edges.py sends the same catalogue through the kernels."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from tests import lzcodes, util
from tools import methods

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tokens_of(data: bytes, info: lzcodes.Info):
    """tools.methods' own parse of `data` as writer tokens."""
    if info.lazy:
        parse = methods._matches(data, max(4, info.args[2]), 1 << 16, (1 << 23) - 1)
    else:
        parse = methods._matches(data, max(info.args[2], 3), info.args[2] + 63 + 4 * 64, (1 << 24) - 1)
    return [("lit", data[t[1]:t[2]]) if t[0] == "lit" else ("match", t[1], t[2]) for t in parse]


@pytest.mark.parametrize("method", lzcodes.METHODS)
def test_writers_reproduce_the_encoders_on_well_formed_data(method):
    info = lzcodes.Info(method)
    rng = np.random.default_rng(5)
    for data in (util.text(30000, seed=2), b"ab" * 5000 + util.x86ish(8000, 3), bytes(rng.integers(0, 256, 3000, dtype=np.uint8)) * 3, b"q" * 70000, b"z"):
        d = methods.e8e9_forward(data) if info.e8 else data
        toks = _tokens_of(d, info)
        feed = lzcodes.feed_of(info, toks)
        assert feed == (methods.lz77_level1(d, info.args) if info.lazy else methods.lz77_level2(d, info.args)), len(data)
        assert lzcodes.expand(info, [feed]) == data, len(data)


def _oracle_agrees(info, feeds, want, what):
    m = info.model
    if len(feeds) == 1:
        assert oracle.run_pcomp(m.pcomp, feeds[0], m.header[4], m.header[5], cap=len(want) + 4096) == want, what
    assert oracle.decompress(lzcodes.block_of(info, feeds, plain=want), cap=len(want) + 4096) == want, what


@pytest.mark.parametrize("method", lzcodes.METHODS)
def test_edge_catalogue_model_and_oracle_agree(method):
    """The plain-Python expander, oracle.run_pcomp of the method's own PCOMP and oracle.decompress of the framed block on every
    catalogue case; no budget is set, so a case the reference would not finish hangs this test rather than passing it."""
    info = lzcodes.Info(method)
    cat = lzcodes.catalogue(method)
    names = [n for n, _ in cat]
    assert len(set(names)) == len(names)
    if not info.lazy:
        assert any("FFFFFFFF" in n for n in names)
    for name, segs in cat:
        feeds = [lzcodes.feed_of(info, t) for t in segs]
        _oracle_agrees(info, feeds, lzcodes.expand(info, feeds), (method, name))


@pytest.mark.parametrize("method", lzcodes.METHODS)
def test_seeded_sweep_model_and_oracle_agree(method):
    info = lzcodes.Info(method)
    streams = lzcodes.sweep(method)
    assert len(streams) == lzcodes.SWEEP_STREAMS
    for i, toks in enumerate(streams):
        feed = lzcodes.feed_of(info, toks)
        want = lzcodes.expand(info, [feed])
        assert len(want) <= lzcodes.SWEEP_MAX_OUT
        _oracle_agrees(info, [feed], want, (method, i))


# ---- the drain's chunk schedule on the host ---------------------------------------------------------------------------------
_SIM = r'''
#include <stdint.h>
#include <string.h>
#define __device__
#define __forceinline__ inline
#include "%s"
// One match of n cells at distance `dist` (unreduced, as the code stream gives it) into M (mm = |M| - 1) at pb, played as a wave
// plays it: in every chunk all lanes load, then all store.  Returns the number of chunks; -1: a lane read a cell that a lane of
// the same chunk writes; -2: the schedule did not end within n chunks.  out: what the copy writes out.
extern "C" int lz_sim(uint8_t *M, uint32_t mm, uint32_t pb, uint32_t dist, uint32_t n, uint8_t *out) {
  const uint32_t d = zh_lz_reduce(dist, mm);
  uint32_t done = 0, back = d;
  int chunks = 0;
  while (done < n) {
    if ((uint32_t)chunks == n) return -2;
    const uint32_t m = zh_lz_width(back, mm, n, done);
    uint8_t v[64];
    for (uint32_t l = 0; l < 64 && l < m; ++l) v[l] = M[(pb + done + l - back) & mm];
    if (d) {
      for (uint32_t l = 0; l < 64 && l < m; ++l)
        for (uint32_t w = 0; w < 64 && w < m; ++w)
          if (((pb + done + l - back) & mm) == ((pb + done + w) & mm)) return -1;
      for (uint32_t l = 0; l < 64 && l < m; ++l) M[(pb + done + l) & mm] = v[l];
    }
    for (uint32_t l = 0; l < 64 && l < m; ++l) out[done + l] = v[l];
    if (m > 64) return -2;
    done += m;
    ++chunks;
    if (d) back = zh_lz_grow(d, back, done, mm);
  }
  return chunks;
}
// the whole sweep for one M size: every dist in 0 .. 3|M| + 70 and 2^32 (= 0), every n in n_lo .. n_hi, the given pb; the
// first failure as (dist, n, pb, code): code -1 / -2 from lz_sim, -3 the cells differ from the bytewise copy, -4 the output
extern "C" int lz_sweep(uint32_t pm, uint32_t n_lo, uint32_t n_hi, const uint32_t *pbs, uint32_t npb, const uint8_t *init, int64_t *fail) {
  const uint32_t size = 1u << pm, mm = size - 1u;
  static uint8_t A[1 << 12], B[1 << 12], oa[256], ob[256];
  for (uint64_t dd = 0; dd <= 3ull * size + 71; ++dd) {
    const uint32_t dist = dd == 3ull * size + 71 ? 0xFFFFFFFFu + 1u : (uint32_t)dd;
    for (uint32_t n = n_lo; n <= n_hi; ++n)
      for (uint32_t i = 0; i < npb; ++i) {
        const uint32_t pb = pbs[i];
        memcpy(A, init, size); memcpy(B, init, size);
        for (uint32_t k = 0; k < n; ++k) { B[(pb + k) & mm] = B[(pb + k - dist) & mm]; ob[k] = B[(pb + k) & mm]; }   // the program
        int rc = lz_sim(A, mm, pb, dist, n, oa);
        if (rc >= 0 && memcmp(A, B, size)) rc = -3;
        if (rc >= 0 && memcmp(oa, ob, n)) rc = -4;
        if (rc < 0) { fail[0] = (int64_t)dd; fail[1] = n; fail[2] = pb; fail[3] = rc; return 1; }
      }
  }
  return 0;
}
'''


def build_schedule_sim(tmp_path, header=None):
    """The simulation above over `header` (default: the tree's zh_lzcopy.h) as a shared library."""
    header = header or os.path.join(ROOT, "zpaqsharp_amd", "csrc", "zh_lzcopy.h")
    src = tmp_path / "lzsim.cpp"
    src.write_text(_SIM % header)
    so = tmp_path / "lzsim.so"
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.lz_sweep.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def run_schedule_sweep(lib):
    """None, or the first (|M| bits, dist, n, pb, code) at which the wave's copy is not the bytewise one."""
    rng = np.random.default_rng(3)
    for pm in (8, 12):
        size = 1 << pm
        init = rng.integers(0, 256, size, dtype=np.uint8)
        # pb: the start, mid-array, so close to the end that the copy wraps, past the end (the program's b is not reduced), 2^32 - 5
        pbs = np.array([0, 5, size // 2 + 3, size - 70, size - 1, size + 9, 3 * size - 20, 0xFFFFFFFB], np.uint32)
        fail = np.zeros(4, np.int64)
        # every n a code can hold: minlen .. minlen + 63 for a minimum match of 1 .. 64
        if lib.lz_sweep(pm, 1, 127, pbs.ctypes.data, len(pbs), init.ctypes.data, fail.ctypes.data):
            return (pm,) + tuple(int(x) for x in fail)
    return None


def test_drain_chunk_schedule_is_the_bytewise_copy(tmp_path):
    """zh_lzcopy.h on the host, a wave of 64 lanes simulated over an M of 2^8 and of 2^12 cells: every distance in 0 .. 3|M| + 70
    and 2^32, every length 1 .. 127, write positions that wrap — the cells and the output equal the program's bytewise copy, no
    lane reads a cell written in the same chunk, and the schedule ends within n chunks.  (Fed the schedule the drain had before
    — chunk width and period from the unreduced distance — run_schedule_sweep reports |M| = 2^8, dist = 0, n = 1: does not end; with
    that one case given a width, |M| = 2^8, dist = 193, n = 64: a lane reads a cell that a lane of the same chunk writes.)"""
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    assert run_schedule_sweep(build_schedule_sim(tmp_path)) is None
