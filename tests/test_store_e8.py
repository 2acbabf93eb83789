"""zh_e8e9_wave.h — the end-of-segment E8E9 pass of `lazy2` / `lzpre` with E8E9 as a schedule for a wave — played on the
host as 64 lanes against the oracle's interpreter running the reference's program."""
import os
import shutil
import subprocess

import pytest

import oracle
from tests import store_e8_cases as cases
from tests.e8w_harness import e8w  # noqa: F401  (the fixture)
from tools import methods

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

METHOD = "x0,6,1,0,7,16"                                  # lzpre + E8E9, matches from one byte: |M| = 2^20


@pytest.fixture(scope="module")
def wave(e8w):
    """zh_store.hip's call: M[0 .. d) in place and aligned, the bytes written out to a buffer of their own.
    -> (bytes written out, M afterwards, stat)"""
    def run(data: bytes):
        return e8w(data, m_in_place=True)
    run.slice, run.lanes, run.round = e8w.slice, e8w.lanes, e8w.round
    return run


def test_header_needs_only_stdint(tmp_path):
    """The header compiles for the host with nothing but <stdint.h> before it (the harness of tests/e8w_harness.py adds <string.h> for itself)."""
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
