"""The verify pass's interface without a GPU: the result record as the C compiler and ctypes see it, the status text, and
the way from the Python keywords to bit 5 of zpaqhip_compress_opts.flags (tests/test_gpu_verify.py runs the pass)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import zpaqsharp_amd as z
from zpaqsharp_amd import _lib, api, compressor
from zpaqsharp_amd.decompresser import Reader, Writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["status", "reserved", "out_len", "first_diff", "sha1", "reserved2"]
VERIFY = 32


def test_result_record_layout_matches_the_header(tmp_path):
    src = tmp_path / "vr.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zpaqhip.h"\nint main(void){printf("%zu", sizeof(zpaqhip_verify_result));\n'
                   + "".join(f'printf(" %zu", offsetof(zpaqhip_verify_result, {f}));\n' for f in FIELDS)
                   + 'printf(" %d %d\\n", (int)ZPAQHIP_E_VERIFY, ZPAQHIP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "vr"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 48 == C.sizeof(_lib.VerifyResult)
    assert got[1:7] == [getattr(_lib.VerifyResult, f).offset for f in FIELDS] == [0, 4, 8, 16, 24, 44]
    assert got[7:] == [-28, 1]


def test_no_other_struct_changed_size():
    assert C.sizeof(_lib.CompressOpts) == 48 and C.sizeof(_lib.Stats) == 80 and C.sizeof(_lib.Err) == 128


def test_strerror_has_the_references_wording():
    assert z.strerror(-28) == "Pre/post-processor test failed"


@pytest.mark.reference
def test_strerror_is_the_string_in_the_reference():
    with open("/root/reference/ZPAQSharp/LibZPAQ.cs") as f:
        line = f.read().splitlines()[319]
    assert 'error("' + z.strerror(-28) + '")' in line


def test_the_library_exports_the_entry_points():
    L = _lib.load()
    for name in ("zpaqhip_verify_blocks", "zpaqhip_verify_blocks_device"):
        assert name in _lib.SYMBOLS and hasattr(L, name)


def test_compress_flags():
    assert api.compress_flags() == 3
    assert api.compress_flags(verify=True) == 3 | VERIFY
    assert api.compress_flags(False, False, True, True, True, True) == 4 | 8 | 16 | VERIFY


class _FakeLib:
    """Stands in for libzpaqhip.so under a Context: every entry point succeeds with an empty stream and notes the flags of the
    zpaqhip_compress_opts it was given."""

    def __init__(self):
        self.flags = []

    def __getattr__(self, name):
        def call(*args):
            for a in args:
                o = getattr(a, "_obj", None)
                if isinstance(o, _lib.CompressOpts):
                    self.flags.append((name, int(o.flags)))
            return 0
        return call


def _fake_ctx():
    ctx = object.__new__(api.Context)
    ctx._L, ctx._h = _FakeLib(), None
    return ctx


@pytest.mark.parametrize("verify", [False, True])
def test_every_compressing_keyword_reaches_bit_5(verify):
    ctx = _fake_ctx()
    blocks = [b"abc" * 50, b"defg" * 40]
    off = [0, 150, 310]
    lz = "x0,2,12,0,7,21,1c0,0,511"
    ctx.compress_blocks("l1", blocks, verify=verify)
    ctx.compress_method(lz, blocks, verify=verify)
    ctx.compress_level("1,128,0", blocks, verify=verify)
    ctx.compress_blocks_device("l1", 4096, off, 8192, 1 << 16, verify=verify)
    ctx.compress_method_device(lz, 4096, off, 8192, 1 << 16, verify=verify)
    ctx.compress_mixed_device([lz, "x0,0ci1"], [0, 1], 4096, off, 8192, 1 << 16, verify=verify)
    ctx.compress_level_device("1,128,0", 4096, off, 8192, 1 << 16, verify=verify)
    names = [n for n, _ in ctx._L.flags]
    assert names == ["zpaqhip_compress_blocks", "zpaqhip_compress_method_blocks", "zpaqhip_compress_method_blocks",
                     "zpaqhip_compress_blocks_device", "zpaqhip_compress_method_blocks_device",
                     "zpaqhip_compress_mixed_blocks_device", "zpaqhip_compress_mixed_blocks_device"]
    assert all(bool(f & VERIFY) == verify for _, f in ctx._L.flags), ctx._L.flags
    assert all(f & 3 == 3 for _, f in ctx._L.flags)


def test_the_default_is_no_verify():
    ctx = _fake_ctx()
    ctx.compress_blocks("l1", [b"x" * 10])
    assert ctx._L.flags == [("zpaqhip_compress_blocks", 3)]


def test_compress_level_names_the_failing_block_of_the_call():
    """compress_level codes its blocks in groups of one method each; a group's error (a verify failure, say) comes back as a
    ZpaqError with the block's index in the call and the group's message."""
    ctx = _fake_ctx()
    blocks = [np.zeros(10, np.uint8), np.zeros(2_000_000, np.uint8), np.zeros(20, np.uint8), np.zeros(30, np.uint8)]
    seen = []

    def failing(method, group, *a):
        seen.append((method, [b.size for b in group]))
        if len(group) == 3:
            raise z.ZpaqError(-28, 1, -1, "from the group")
        return b"", np.zeros(len(group) + 1, np.uint64)

    ctx._compress_method = failing
    with pytest.raises(z.ZpaqError) as e:
        ctx.compress_level("1,128,0", blocks, verify=True)
    assert (e.value.code, e.value.block, e.value.segment, str(e.value)) == (-28, 2, -1, "from the group")
    assert ([10, 20, 30] in [s for _, s in seen]) and len({m for m, _ in seen}) == len(seen)


class _Bytes(Reader):
    def __init__(self, data):
        self.data, self.pos = data, 0

    def read(self, n):
        b = self.data[self.pos:self.pos + n]
        self.pos += len(b)
        return b


class _Sink(Writer):
    def write(self, buf):
        pass


@pytest.mark.parametrize("how", ["model", "method", "level"])
def test_compressor_passes_verify_on(how):
    ctx = _fake_ctx()
    kw = {"model": dict(model="l1"), "method": dict(method="x0,2,12,0,7,21,1c0,0,511"), "level": dict(level="1,128,0")}[how]
    compressor.compress(_Bytes(b"hello " * 100), _Sink(), context=ctx, block_size=256, verify=True, **kw)
    assert ctx._L.flags and all(f & VERIFY for _, f in ctx._L.flags)
    ctx._L.flags.clear()
    compressor.compress(_Bytes(b"hello " * 100), _Sink(), context=ctx, block_size=256, **kw)
    assert ctx._L.flags and not any(f & VERIFY for _, f in ctx._L.flags)


def test_verify_records_are_plain_values():
    rec = (_lib.VerifyResult * 2)()
    rec[1].status, rec[1].out_len, rec[1].first_diff = -28, 7, 3
    rec[1].sha1[:] = list(range(20))
    got = api.Context._verify_records(rec, 2)
    assert got[0] == {"status": 0, "out_len": 0, "first_diff": 0, "sha1": bytes(20)}
    assert got[1] == {"status": -28, "out_len": 7, "first_diff": 3, "sha1": bytes(range(20))}
    assert np.uint64(_lib.UINT64_MAX) == np.uint64(2**64 - 1)
