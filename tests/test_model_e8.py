"""opts.kernel == KERNEL_MODEL_E8 without a GPU: the constant, the stats field, and zh_e8e9_round.h — a round of the
end-of-segment E8E9 pass in and out of its slot buffers as zh_nibble.hip's nb_e8_pass does it — played on the host as 64
lanes (tests/e8w_harness.py) against the oracle's run of the reference's lzpre and bwtrle programs with E8E9."""
import ctypes
import subprocess

import pytest

import oracle
import zpaqsharp_amd as z
from tests import model_e8_cases as mc
from tests import store_e8_cases as cases
from tests.e8w_harness import e8w  # noqa: F401  (the fixture)
from tools import methods
from zpaqsharp_amd import _lib


def test_constant_stats_field_and_opts():
    assert z.KERNEL_MODEL_E8 == 11 and "KERNEL_MODEL_E8" in z.__all__
    assert _lib.Stats.e8_wave_segs.offset == _lib.Stats.kernel_kind.offset + 4 and _lib.Stats.e8_wave_segs.size == 4
    assert not hasattr(_lib.Stats, "reserved")
    assert ctypes.sizeof(_lib.Stats) == _lib.Stats.e8_wave_segs.offset + 4          # the last field: the size has not changed
    o = z.make_opts(kernel=z.KERNEL_MODEL_E8, verify_sha1=True)
    assert (o.kernel, o.verify_sha1, o.struct_size) == (11, 1, ctypes.sizeof(_lib.Opts))


@pytest.fixture(scope="module")
def e8r(e8w):
    """zh_nibble.hip's calls: the flat buffer begins `mis` bytes into an aligned one (the Writer's region begins anywhere), and
    `dst` / `out` are two places (M and the Writer, whose capacity is `short` bytes less than needed) or, in place, the one the
    bytes are read from.  -> (bytes written out, M afterwards or None)"""
    def run(data: bytes, mis: int = 0, in_place: bool = False, short: int = 0):
        return e8w(data, mis=mis, in_place=in_place, short=short)[:2]
    run.lib, run.src = e8w.lib, e8w.src
    return run


def test_registers_after_the_pass(e8r):
    """a b c d f r1 r2 as the program's loop and reset line leave them: the translated program's own run says so."""
    r = (ctypes.c_uint32 * 7)()
    e8r.lib.e8w_regs(r)
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
    misalignment of the flat buffer, to two places, in place, and aligned with M written onto itself (zh_store.hip's call)."""
    exe = tmp_path / "e8w_asan"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++14", "-DE8W_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), str(e8r.src)], capture_output=True, text=True)
    if r.returncode:
        pytest.skip("no sanitizer runtime for g++ here: " + r.stderr[-200:])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
