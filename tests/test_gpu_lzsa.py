"""LZBuffer's suffix-array match search on the GPU (zh_pre_lzsa.hip): Context.lzsa_blocks / zpaqhip_lzsa_blocks equal the
literal port tools.methods.preprocess(..., sa=True) byte for byte on the catalogue of tests/lzsa_cases.py, at levels 1 and
2, with and without E8E9; Context.compress_method(sa=True) writes the streams of tools.methods.compress_block(sa=True),
which the GPU decoder and the oracle read back; without the keyword nothing changes; the numeric levels take the keyword;
the C ABI's capacity contract."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import lzsa_cases as cases
from tools import methods
from zpaqsharp_amd import _lib, method

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m", cases.METHODS)
def test_lzsa_blocks_equal_the_port_on_the_catalogue(ctx, m):
    blocks, want = cases.blocks_for(m), cases.want(m)
    got = ctx.lzsa_blocks(m, blocks)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (m, i, len(blocks[i]), len(g), len(w))
    st = ctx.stats()
    assert st.blocks == len(blocks) and st.launches > 0 and st.kernel_ms == st.init_ms > 0
    assert ctx.lzsa_blocks(m, blocks[-5:]) == list(want[-5:])          # one call: 0, 1, 777, 4 097 and 20 000 bytes
    assert ctx.lzsa_blocks(m, []) == []


def test_bucket_sizes_and_look_ahead_on_text(ctx):
    d = cases.text()
    for m in cases.knob_methods():
        assert ctx.lzsa_blocks(m, [d, d[:3000]]) == [methods.preprocess(b, method.parse_args(m)[1], sa=True) for b in (d, d[:3000])], m


def test_other_methods_are_refused_by_lzsa_blocks(ctx):
    for m in ("x0,1,4,0,3,20", "x0,3", "x0,0", "x4,2,12,0,7,24,1"):
        with pytest.raises(ValueError):
            ctx.lzsa_blocks(m, [b"abcabcabc"])
    with pytest.raises(ValueError):
        ctx.lzsa_blocks("x0,1,3,0,3,21", [b"abcabcabc"])             # level 1 below 4 (LZBuffer.cs:198-199)


def _stream_blocks(m):
    args = method.parse_args(m)[1]
    r = bytes(np.random.default_rng(3).integers(0, 256, 5000, dtype=np.uint8))
    return cases.small(args[2]) + [cases.text(), cases.x86(), cases.phrases(), r + r[:100], b"ab" * 2048 + b"a"]


@pytest.mark.parametrize("m", cases.METHODS + ("x0,2,12,0,7,21,1", "x0,1,4,0,7,21,1ci1"))
def test_compress_method_sa_matches_the_cpu_writer_and_round_trips(ctx, m):
    blocks = _stream_blocks(m)
    names = [f"f{i}" for i in range(len(blocks))]
    want = b"".join(methods.compress_block(m, b, names[i].encode(), sa=True) for i, b in enumerate(blocks))
    got = ctx.compress_method(m, blocks, filenames=names, sa=True, kernel=2)
    assert got == want, m
    assert ctx.stats().init_ms > 0
    plain = b"".join(blocks)
    assert ctx.decompress(got, verify_sha1=True).tobytes() == plain
    assert oracle.decompress(got, cap=len(plain) + 64) == plain
    # without the keyword: today's parse
    old = b"".join(methods.compress_block(m, b, names[i].encode()) for i, b in enumerate(blocks))
    assert ctx.compress_method(m, blocks, filenames=names, kernel=2) == old
    assert old != want


def test_the_keyword_has_no_effect_on_other_methods(ctx):
    blocks = [cases.text(), cases.x86(3000)]
    for m in ("x0,1,4,0,3,20", "x0,2,12,0,7,20,1", "x0,0ci1", "x0,4"):
        assert ctx.compress_method(m, blocks, sa=True) == ctx.compress_method(m, blocks) == b"".join(methods.compress_block(m, b) for b in blocks)
    assert ctx.compress_method("x0,3ci1", blocks, sa=True, bwt=True) == b"".join(methods.compress_block("x0,3ci1", b) for b in blocks)


@pytest.mark.parametrize("level", ["2,128,0", "3,128,0"])
def test_numeric_levels_take_the_keyword(ctx, level):
    blocks = [cases.text(20000, 21), cases.x86(9000, 22), cases.text(4097, 23)]
    s = ctx.compress_level(level, blocks, sa=True)
    assert all(method.uses_sa(method.parse_args(m)[1]) for m in ctx.level_methods), ctx.level_methods
    assert s == b"".join(methods.compress_block(m, b, sa=True) for m, b in zip(ctx.level_methods, blocks))
    assert ctx.decompress(s, verify_sha1=True).tobytes() == b"".join(blocks)
    assert s != ctx.compress_level(level, blocks)


def test_capacity_through_the_c_abi(ctx):
    L = _lib.load()
    m = cases.L2
    a = (C.c_int32 * 9)(*method.parse_args(m)[1])
    blocks = [cases.text(5000, i) for i in range(3)]
    want = [methods.preprocess(b, method.parse_args(m)[1], sa=True) for b in blocks]
    total = sum(map(len, want))
    d = np.frombuffer(b"".join(blocks), np.uint8)
    offs = np.array([0, 5000, 10000, 15000], np.uint64)
    for cap in (total, total - 1, 10):
        out, n, err = np.empty(cap, np.uint8), C.c_size_t(0), _lib.Err()
        oo = np.zeros(4, np.uint64)
        rc = L.zpaqhip_lzsa_blocks(ctx._h, a, d.ctypes.data, offs.ctypes.data, 3, out.ctypes.data, cap, C.byref(n), oo.ctypes.data, C.byref(err))
        assert n.value == total and list(oo) == list(np.cumsum([0] + [len(w) for w in want]))
        assert rc == (0 if cap == total else -20)               # ZPAQHIP_E_OUTPUT_FULL
        if rc == 0:
            assert out.tobytes() == b"".join(want)
            st = ctx.stats()
            assert st.kernel_ms == st.init_ms > 0 and st.in_bytes == 15000 and st.out_bytes == total
    # another method: ZPAQHIP_E_ARG
    b = (C.c_int32 * 9)(*method.parse_args("x0,1,4,0,3,20")[1])
    out, n, err = np.empty(64, np.uint8), C.c_size_t(0), _lib.Err()
    assert L.zpaqhip_lzsa_blocks(ctx._h, b, d.ctypes.data, offs.ctypes.data, 3, out.ctypes.data, 64, C.byref(n), None, C.byref(err)) == -25
