"""The device forms of the compressing entry points without a GPU: their ctypes signatures, the argument errors they return
before touching the device, and the host-side frame table (zh_frame_table.cpp) in a stand-alone C++ program built with
-fsanitize=address,undefined (tests/native/frame_table_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from zpaqsharp_amd import _lib, api, method, models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zpaqsharp_amd", "csrc")
E_ARG = -25


def test_exports_and_argument_lists():
    L = _lib.load()
    for name in ("zpaqhip_compress_blocks_device", "zpaqhip_compress_method_blocks_device"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    host, dev = L.zpaqhip_compress_blocks.argtypes, L.zpaqhip_compress_blocks_device.argtypes
    assert len(dev) == 18 and list(dev[:16]) == list(host[:16]) and dev[16] is C.c_void_p and dev[17] is host[16]
    host, dev = L.zpaqhip_compress_method_blocks.argtypes, L.zpaqhip_compress_method_blocks_device.argtypes
    assert len(dev) == 17 and list(dev[:15]) == list(host[:15]) and dev[15] is C.c_void_p and dev[16] is host[15]
    # the header declares both with hip_stream in front of err, and the ABI version stays (an added export does not bump it)
    text = open(os.path.join(ROOT, "include", "zpaqhip.h")).read()
    for name in ("zpaqhip_compress_blocks_device", "zpaqhip_compress_method_blocks_device"):
        decl = text[text.index("int " + name + "("):]
        decl = decl[:decl.index(";")]
        assert decl.rstrip(")").split(",")[-2].strip() == "void *hip_stream" and "void *d_out" in decl and "const void *d_in" in decl
    assert "#define ZPAQHIP_ABI_VERSION 1\n" in text and L.zpaqhip_version() == 1
    assert C.sizeof(_lib.CompressOpts) == 48


class _Fake:
    """A context handle that is not NULL: the argument checks return before anything reads it."""

    def __init__(self):
        self.buf = (C.c_uint8 * 4096)()
        self.h = C.addressof(self.buf)


def _call_blocks(L, h, m, d_in, in_off, n, d_out, out_cap, pcomp_len=None, d_orig=None, orig_off=None):
    hdr = np.frombuffer(m.header, np.uint8)
    pc = np.zeros(8, np.uint8)
    err, got = _lib.Err(), C.c_size_t(77)
    off = np.asarray(in_off, np.uint64)
    ooff = np.asarray(orig_off, np.uint64) if orig_off is not None else None
    rc = L.zpaqhip_compress_blocks_device(h, hdr.ctypes.data, hdr.size, pc.ctypes.data if pcomp_len else None, pcomp_len or 0, d_in,
                                          off.ctypes.data, n, d_orig, ooff.ctypes.data if ooff is not None else None, None, d_out,
                                          out_cap, C.byref(got), None, None, None, C.byref(err))
    return rc, err


def test_argument_errors_come_back_before_the_device_is_touched():
    L, f, m = _lib.load(), _Fake(), models.get("min")
    some = 0x10000                                         # stands for a device address: never dereferenced on these paths
    # no output buffer with a capacity, no context, too long a PCOMP, offsets that decrease, data without a pointer
    assert _call_blocks(L, f.h, m, some, [0, 4], 1, None, 16)[0] == E_ARG
    assert _call_blocks(L, None, m, some, [0, 4], 1, some, 16)[0] == E_ARG
    assert _call_blocks(L, f.h, m, some, [0, 4], 1, some, 16, pcomp_len=65536)[0] == E_ARG
    rc, err = _call_blocks(L, f.h, m, some, [0, 8, 4], 2, some, 16)
    assert rc == E_ARG and err.block == 1 and b"decrease" in err.msg
    rc, err = _call_blocks(L, f.h, m, some, [0, 4, 8], 2, some, 16, d_orig=some, orig_off=[0, 9, 3])
    assert rc == E_ARG and err.block == 1
    assert _call_blocks(L, f.h, m, None, [0, 4], 1, some, 16)[0] == E_ARG
    # the method form: the same checks, and the method's own refusals
    hdr = np.frombuffer(method.model_of("x0,1,4,0,3,16")[0].header, np.uint8)

    def meth(args, in_off, d_out=some, out_cap=16, pcomp_len=0, flags=3):
        err, got = _lib.Err(), C.c_size_t(0)
        off = np.asarray(in_off, np.uint64)
        o = _lib.CompressOpts()
        o.struct_size, o.flags = C.sizeof(_lib.CompressOpts), flags
        pc = np.zeros(8, np.uint8)
        return L.zpaqhip_compress_method_blocks_device(f.h, (C.c_int32 * 9)(*args), hdr.ctypes.data, hdr.size,
                                                       pc.ctypes.data if pcomp_len else None, pcomp_len, some, off.ctypes.data,
                                                       off.size - 1, None, d_out, out_cap, C.byref(got), None, C.byref(o), None,
                                                       C.byref(err))
    a = method.parse_args("x0,1,4,0,3,16")[1]
    assert meth(a, [0, 4], d_out=None) == E_ARG
    assert meth(a, [0, 4], pcomp_len=65536) == E_ARG
    assert meth(a, [0, 8, 4]) == E_ARG
    assert meth(a, [0, (1 << 20) + 1]) == E_ARG            # longer than the post-processor's M
    assert meth(method.parse_args("x0,3ci1")[1], [0, 4]) == E_ARG        # BWT without the opt-in


def test_python_wrappers_refuse_before_the_device_is_touched():
    class NoDevice(api.Context):
        def __init__(self):                                # no zpaqhip_ctx_create
            self._L, self._h = _lib.load(), None

    ctx = NoDevice()
    with pytest.raises(ValueError):
        ctx.compress_method_device("x0,3ci1", 0x10000, [0, 10], 0x20000, 100)             # level 3 without bwt=True
    with pytest.raises(ValueError):
        ctx.compress_method_device("x0,1,4,0,3,16", 0x10000, [0, (1 << 20) + 1], 0x20000, 100)
    with pytest.raises(ValueError):
        ctx.compress_blocks_device("min", 0x10000, [0, 10], 0x20000, 100, filenames=["a", "b"])
    # a NULL context is an argument error of the library, raised as one
    with pytest.raises(api.ZpaqError) as e:
        ctx.compress_blocks_device("min", 0x10000, [0, 10], 0x20000, 100)
    assert e.value.code == E_ARG


def test_frame_table_in_a_sanitized_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the stand-alone check of the frame table"
    exe = str(tmp_path / "frame_table")
    # the sanitizers' runtime inside the program, so that it runs as it is wherever it is started; GCC and clang spell it differently
    about = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = "-static-libsan" if "clang" in about else "-static-libasan"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           static,
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "frame_table_main.cpp"),
                           os.path.join(CSRC, "zh_frame_table.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[:4] == ["ok block_frame", "ok running_sum", "ok output_full", "ok store_layout"] and lines[4].startswith("ok ")
