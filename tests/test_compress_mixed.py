"""zpaqhip_compress_mixed_blocks_device and zpaqhip_gap_hist_blocks_device without a GPU: their declarations and ctypes
mirrors, the argument errors they return before touching the device, the Python wrappers' refusals, and two stand-alone C++
programs built with -fsanitize=address,undefined: the gather table (tests/native/gather_table_main.cpp over
zh_frame_table.cpp) and the load rule of the analysis kernel (tests/native/gap_walk_main.cpp over zh_analyze.h)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from zpaqsharp_amd import _lib, api, method

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zpaqsharp_amd", "csrc")
E_ARG = -25
NAMES = ("zpaqhip_compress_mixed_blocks_device", "zpaqhip_gap_hist_blocks_device")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the stand-alone checks"
    return cxx


def test_exports_declarations_and_the_struct(tmp_path):
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "zpaqhip.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
        decl = text[text.index("int " + name + "("):]
        decl = decl[:decl.index(";")]
        assert decl.rstrip(")").split(",")[-2].strip() == "void *hip_stream" and "const void *d_in" in decl
        assert getattr(L, name).argtypes[-2] is C.c_void_p and getattr(L, name).argtypes[-1] is L.zpaqhip_gap_hist_blocks.argtypes[-1]
    assert len(L.zpaqhip_compress_mixed_blocks_device.argtypes) == 15 and len(L.zpaqhip_gap_hist_blocks_device.argtypes) == 7
    assert "#define ZPAQHIP_ABI_VERSION 1\n" in text and L.zpaqhip_version() == 1
    # sizeof(zpaqhip_method) and its offsets, as a compiled C program sees the header
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zpaqhip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(zpaqhip_method), offsetof(zpaqhip_method, reserved),\n'
                   '  offsetof(zpaqhip_method, hdr), offsetof(zpaqhip_method, hdr_len), offsetof(zpaqhip_method, pcomp),\n'
                   '  offsetof(zpaqhip_method, pcomp_len)); return 0; }\n')
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler is needed to measure the struct"
    exe = str(tmp_path / "size")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    M = _lib.Method
    assert got == [C.sizeof(M), M.reserved.offset, M.hdr.offset, M.hdr_len.offset, M.pcomp.offset, M.pcomp_len.offset]


class _Fake:
    """A context handle that is not NULL: the argument checks return before anything reads it."""

    def __init__(self):
        self.buf = (C.c_uint8 * 4096)()
        self.h = C.addressof(self.buf)


SOME = 0x10000                     # stands for a device address: never dereferenced on these paths


def _table(strings, reserved=()):
    keep, t = [], (_lib.Method * max(1, len(strings)))()
    for g, m in enumerate(strings):
        mod = method.model_of(m)[0]
        hdr = np.frombuffer(mod.header, np.uint8)
        pc = np.frombuffer(mod.pcomp, np.uint8) if mod.pcomp else None
        keep += [hdr, pc]
        t[g].args = (C.c_int32 * 9)(*method.parse_args(m)[1])
        t[g].reserved = 1 if g in reserved else 0
        t[g].hdr, t[g].hdr_len = hdr.ctypes.data, hdr.size
        t[g].pcomp, t[g].pcomp_len = (pc.ctypes.data, pc.size) if pc is not None else (None, 0)
    return t, keep


def _mixed(h, strings, method_of, in_off, *, d_in=SOME, d_out=SOME, out_cap=16, flags=7, reserved=(), n_methods=None):
    L = _lib.load()
    t, keep = _table(strings, reserved)
    which = np.asarray(method_of, np.uint32)
    off = np.asarray(in_off, np.uint64)
    o = _lib.CompressOpts()
    o.struct_size, o.flags = C.sizeof(_lib.CompressOpts), flags
    err, got = _lib.Err(), C.c_size_t(77)
    err.block = -7
    rc = L.zpaqhip_compress_mixed_blocks_device(h, t, len(strings) if n_methods is None else n_methods, which.ctypes.data, d_in,
                                                off.ctypes.data, off.size - 1, None, d_out, out_cap, C.byref(got), None, C.byref(o),
                                                None, C.byref(err))
    del keep
    return rc, err


LZ, BWT, STORE = "x0,1,4,0,3,16", "x0,3ci1", "x0,0"


def test_argument_errors_come_back_before_the_device_is_touched():
    f = _Fake()
    assert _mixed(None, [LZ], [0], [0, 4])[0] == E_ARG                             # no context
    assert _mixed(f.h, [LZ], [0], [0, 4], d_out=None)[0] == E_ARG                  # no output buffer with a capacity
    rc, err = _mixed(f.h, [LZ], [0, 0], [0, 8, 4])
    assert rc == E_ARG and err.block == 1 and b"decrease" in err.msg
    assert _mixed(f.h, [LZ], [0], [0, 4], n_methods=0)[0] == E_ARG                 # blocks, but no method
    rc, err = _mixed(f.h, [LZ, STORE], [0, 1, 2, 0], [0, 4, 8, 12, 16])
    assert rc == E_ARG and err.block == 2                                          # method_of[2] names no method
    assert _mixed(f.h, [LZ, STORE], [0, 0], [0, 4, 8], reserved=(1,))[0] == E_ARG  # reserved is checked for every entry
    # what the method form refuses, with the block's index in the call: BWT without its opt-in, at its first block
    rc, err = _mixed(f.h, [LZ, BWT], [0, 0, 1, 0], [0, 4, 8, 12, 16], flags=3)
    assert rc == E_ARG and err.block == 2
    # a method refused for one block's length: the third of five blocks is longer than the post-processor's M; its group's
    # other blocks (the first and the last) are fine, and so is a block of that length under another method
    M = 1 << 20
    off = np.cumsum([0, 4, M + 1, M + 1, 4, 4]).tolist()
    rc, err = _mixed(f.h, [STORE, LZ], [1, 0, 1, 0, 1], off)
    assert rc == E_ARG and err.block == 2 and b"longer" in err.msg
    # a method that no block takes is checked against nothing: the same list passes the checks when the long blocks take
    # "x0,0" (the call then goes on to the device; here it is stopped at the next check, a decreasing offset behind them)
    rc, err = _mixed(f.h, [STORE, LZ, BWT], [0, 0, 0, 0, 0, 0], off + [off[-1] - 1], flags=3)
    assert rc == E_ARG and err.block == 5 and b"decrease" in err.msg


def test_python_wrappers_refuse_before_the_device_is_touched():
    class NoDevice(api.Context):
        def __init__(self):                                # no zpaqhip_ctx_create
            self._L, self._h = _lib.load(), None

    ctx = NoDevice()
    with pytest.raises(ValueError):
        ctx.compress_level_device("x3", SOME, [0, 10], SOME, 100)                  # not a digit
    with pytest.raises(ValueError):
        ctx.compress_level_device("", SOME, [0, 10], SOME, 100)
    with pytest.raises(ValueError):
        ctx.compress_level_device("1", SOME, [0, 10, 20], SOME, 100, filenames=["a"])
    with pytest.raises(ValueError):
        ctx.compress_mixed_device([LZ], [0, 0], SOME, [0, 10, 20], SOME, 100, filenames=["a", "b", "c"])
    with pytest.raises(ValueError):
        ctx.compress_mixed_device([LZ, STORE], [0, 2], SOME, [0, 10, 20], SOME, 100)     # method_of out of range
    with pytest.raises(ValueError):
        ctx.compress_mixed_device([LZ], [0], SOME, [0, 10, 20], SOME, 100)               # one entry per block
    with pytest.raises(ValueError):
        ctx.compress_mixed_device([LZ, BWT], [0, 1], SOME, [0, 10, 20], SOME, 100)       # level 3 without bwt=True
    with pytest.raises(ValueError):                                                      # too long for the method its block takes
        ctx.compress_mixed_device([STORE, LZ], [0, 1], SOME, [0, 10, 10 + (1 << 20) + 1], SOME, 100)
    # ... and not checked against a method its block does not take: the library's own NULL-context error comes back instead
    with pytest.raises(api.ZpaqError) as e:
        ctx.compress_mixed_device([STORE, LZ], [1, 0], SOME, [0, 10, 10 + (1 << 20) + 1], SOME, 100)
    assert e.value.code == E_ARG
    with pytest.raises(api.ZpaqError) as e:
        ctx.gap_hist_blocks_device(SOME, [0, 10])
    assert e.value.code == E_ARG
    with pytest.raises(ValueError):
        ctx.gap_hist_blocks_device(SOME, [0, 1 << 31])


def _sanitized(tmp_path, main, *sources):
    cxx = _cxx()
    exe = str(tmp_path / main.replace(".cpp", ""))
    # the sanitizers' runtime inside the program, so that it runs as it is wherever it is started; GCC and clang spell it differently
    about = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = "-static-libsan" if "clang" in about else "-static-libasan"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", static,
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", main)] + [os.path.join(CSRC, s) for s in sources] +
                          ["-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split("\n")


def test_gather_table_in_a_sanitized_program(tmp_path):
    lines = _sanitized(tmp_path, "gather_table_main.cpp", "zh_frame_table.cpp")
    assert lines[:3] == ["ok order", "ok output_full", "ok empty"] and lines[3].startswith("ok ")


def test_load_rule_of_the_analysis_kernel_in_a_sanitized_program(tmp_path):
    lines = _sanitized(tmp_path, "gap_walk_main.cpp")
    assert lines[0] == "ok load_rule" and lines[1].startswith("ok ")
