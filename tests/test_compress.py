"""Compression surface that needs no GPU: the zpaqhip_compress_opts mirror and the product-side forward E8E9 transform."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import util
from zpaqsharp_amd import _lib, e8e9, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compress_opts_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in _lib.CompressOpts._fields_]
    src = tmp_path / "co.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zpaqhip.h"\nint main(void){printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(zpaqhip_compress_opts)'
                   + "".join(f", offsetof(zpaqhip_compress_opts, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "co"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.CompressOpts)] + [getattr(_lib.CompressOpts, f).offset for f in fields]


def test_library_exports_compress_blocks():
    assert "zpaqhip_compress_blocks" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "zpaqhip_compress_blocks")


def _cases():
    rng = np.random.default_rng(11)
    yield util.x86ish(60000)
    yield synth.plain("X", 3, 50000).tobytes()
    yield rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    # dense E8 / E9 runs: operands of one candidate overlap the next one's
    yield bytes(rng.choice(np.array([0xE8, 0xE9, 0x00, 0xFF], np.uint8), 5000))
    for n in range(0, 12):
        yield bytes(rng.choice(np.array([0xE8, 0x00, 0xFF, 0x12], np.uint8), n))


@pytest.mark.parametrize("k", range(16))
def test_forward_e8e9_matches_oracle_and_writer(k):
    data = list(_cases())[k]
    got = e8e9.forward(data).tobytes()
    assert got == bytes(oracle.e8e9(data))
    assert got == synth.e8e9(np.frombuffer(data, np.uint8)).tobytes()
