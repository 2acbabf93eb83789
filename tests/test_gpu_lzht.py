"""LZBuffer's hash-table match search on the GPU (zh_pre_lzht.hip): Context.lzht_blocks / zpaqhip_lzht_blocks equal the port
tools.methods.preprocess(..., ht=True) byte for byte on the catalogue of tests/lzht_cases.py, at levels 1 and 2, with and
without E8E9; Context.compress_method(ht=True) writes the streams of tools.methods.compress_block(ht=True), which the GPU
decoder and the oracle read back; without the keyword nothing changes; the numeric levels take the keyword; the C ABI's
capacity contract; both searches over several batches of one call."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import lzht_cases as cases
from tools import methods
from zpaqsharp_amd import _lib, method, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m", cases.METHODS + (cases.M_MARGINAL1, cases.M_MARGINAL2))
def test_lzht_blocks_equal_the_port_on_the_catalogue(ctx, m):
    blocks, want = cases.blocks_for(m), cases.want(m)
    got = ctx.lzht_blocks(m, blocks)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (m, i, len(blocks[i]), len(g), len(w))
    st = ctx.stats()
    assert st.blocks == len(blocks) and st.launches > 0 and st.kernel_ms == st.init_ms > 0
    assert ctx.lzht_blocks(m, blocks[-5:]) == list(want[-5:])          # one call: 0, 1, 777, 4 097 and 20 000 bytes
    assert ctx.lzht_blocks(m, []) == []


def test_table_sizes_buckets_and_match_lengths_on_text(ctx):
    d = cases.text()
    for m in cases.knob_methods():
        blocks = [d, d[:3000], cases.invisible(0), cases.invisible(1)]
        assert ctx.lzht_blocks(m, blocks) == [methods.preprocess(b, method.parse_args(m)[1], ht=True) for b in blocks], m


def test_a_megabyte_of_one_value_against_the_cpp_twin(ctx):
    d = bytes(1 << 20)                                                   # every lane stops comparing at 256 bytes; the walk extends
    for m in (cases.L1, "x0,2,4,0,3,20"):
        assert ctx.lzht_blocks(m, [d]) == [synth.preprocess(method.parse_args(m)[1], d, ht=True)], m


def test_other_methods_are_refused_by_lzht_blocks(ctx):
    for m in ("x0,1,4,0,7,21,1", "x0,3", "x0,0", "x4,2,12,0,7,25,1", "x0,1,4,1,3,20", "x0,1,4,0,3,20,1", "x0,1,3,0,3,20", "x0,2,1,0,3,20",
              "x0,2,256,0,3,20", "x12,1,4,0,3,20", "x0,1,4,0,4,3", "x0,1,4,0,7,20"):
        with pytest.raises(ValueError):
            ctx.lzht_blocks(m, [b"abcabcabcabcabc"])


def _stream_blocks(m):
    args = method.parse_args(m)[1]
    r = bytes(np.random.default_rng(3).integers(0, 256, 5000, dtype=np.uint8))
    return cases.small(args[2]) + [cases.text(), cases.x86(), cases.phrases(), r + r[:100], b"ab" * 2048 + b"a"]


@pytest.mark.parametrize("m", cases.METHODS + ("x0,1,4,0,3,20ci1",))
def test_compress_method_ht_matches_the_cpu_writer_and_round_trips(ctx, m):
    blocks = _stream_blocks(m)
    names = [f"f{i}" for i in range(len(blocks))]
    want = b"".join(methods.compress_block(m, b, names[i].encode(), ht=True) for i, b in enumerate(blocks))
    got = ctx.compress_method(m, blocks, filenames=names, ht=True, kernel=2)
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
    for m in ("x0,1,4,0,7,21,1", "x0,0", "x0,0ci1", "x0,4"):
        assert ctx.compress_method(m, blocks, ht=True) == ctx.compress_method(m, blocks) == b"".join(methods.compress_block(m, b) for b in blocks)
    assert ctx.compress_method("x0,3ci1", blocks, ht=True, bwt=True) == b"".join(methods.compress_block("x0,3ci1", b) for b in blocks)
    m = "x0,1,4,0,7,21,1"
    assert ctx.compress_method(m, blocks, sa=True, ht=True) == b"".join(methods.compress_block(m, b, sa=True) for b in blocks)
    with pytest.raises(ValueError):
        ctx.compress_method("x0,1,4,1,3,20", blocks, ht=True)
    # the C ABI refuses what the route does not take, and takes the same string without the bit
    a = (C.c_int32 * 9)(*method.parse_args("x0,1,4,0,7,21,1")[1])
    d = np.frombuffer(blocks[0], np.uint8)
    offs = np.array([0, d.size], np.uint64)
    out, n, err = np.empty(64, np.uint8), C.c_size_t(0), _lib.Err()
    assert _lib.load().zpaqhip_lzht_blocks(ctx._h, a, d.ctypes.data, offs.ctypes.data, 1, out.ctypes.data, 64, C.byref(n), None, C.byref(err)) == -25


@pytest.mark.parametrize("m", ["x4,6,12,0,7,25,1", cases.L1])        # the suffix-array search behind E8E9, the hash-table search
def test_batches_of_one_call_reuse_the_sort_arena(ctx, m):
    # batches of 20 000 + 0, 1 + 4 097 and 777 slots: the arena is laid out anew for each
    blocks = [cases.text(20000, 9), b"", b"q", cases.x86(4097, 8), cases.text(777, 7)]
    got = ctx.compress_method(m, blocks, sa=True, ht=True, batch_blocks=2)
    assert got == ctx.compress_method(m, blocks, sa=True, ht=True)
    assert got == b"".join(methods.compress_block(m, b, sa=True, ht=True) for b in blocks)


@pytest.mark.parametrize("level", ["1", "1,128,0", "2,40,0", "3,30,0", "2,10,0", "3,6,0", "4,4,0"])
def test_numeric_levels_take_the_keyword(ctx, level):
    # (levels 2 to 4 write the hash-table strings for blocks of low redundancy only: "2,10,0", "3,6,0", "4,4,0"; "2,40,0" and
    # "3,30,0" get suffix-array strings, which the other keyword covers)
    blocks = [cases.text(20000, 21), cases.x86(9000, 22), cases.text(4097, 23)]
    s = ctx.compress_level(level, blocks, sa=True, ht=True)
    want_ht = level not in ("2,40,0", "3,30,0")
    assert all(method.uses_ht(method.parse_args(m)[1]) == want_ht and method.uses_sa(method.parse_args(m)[1]) != want_ht
               for m in ctx.level_methods), ctx.level_methods
    assert s == b"".join(methods.compress_block(m, b, sa=True, ht=True) for m, b in zip(ctx.level_methods, blocks))
    assert ctx.decompress(s, verify_sha1=True).tobytes() == b"".join(blocks)
    assert s != ctx.compress_level(level, blocks)


def test_level_2_at_high_redundancy_still_takes_the_sa_route(ctx):
    blocks = [cases.text(20000, 21), cases.text(4097, 23)]
    s = ctx.compress_level("2,128,0", blocks, sa=True, ht=True)
    assert all(method.uses_sa(method.parse_args(m)[1]) for m in ctx.level_methods), ctx.level_methods
    assert s == ctx.compress_level("2,128,0", blocks, sa=True) == b"".join(methods.compress_block(m, b, sa=True) for m, b in zip(ctx.level_methods, blocks))


def test_capacity_through_the_c_abi(ctx):
    L = _lib.load()
    m = "x0,2,4,0,3,20"
    a = (C.c_int32 * 9)(*method.parse_args(m)[1])
    blocks = [cases.text(5000, i) for i in range(3)]
    want = [methods.preprocess(b, method.parse_args(m)[1], ht=True) for b in blocks]
    total = sum(map(len, want))
    d = np.frombuffer(b"".join(blocks), np.uint8)
    offs = np.array([0, 5000, 10000, 15000], np.uint64)
    for cap in (total, total - 1, 10):
        out, n, err = np.empty(cap, np.uint8), C.c_size_t(0), _lib.Err()
        oo = np.zeros(4, np.uint64)
        rc = L.zpaqhip_lzht_blocks(ctx._h, a, d.ctypes.data, offs.ctypes.data, 3, out.ctypes.data, cap, C.byref(n), oo.ctypes.data, C.byref(err))
        assert n.value == total and list(oo) == list(np.cumsum([0] + [len(w) for w in want]))
        assert rc == (0 if cap == total else -20)               # ZPAQHIP_E_OUTPUT_FULL
        if rc == 0:
            assert out.tobytes() == b"".join(want)
            st = ctx.stats()
            assert st.kernel_ms == st.init_ms > 0 and st.in_bytes == 15000 and st.out_bytes == total
    # what the route refuses: ZPAQHIP_E_ARG
    for bad in ("x0,1,4,0,7,21,1", "x0,1,4,1,3,20", "x0,2,1,0,3,20"):
        b = (C.c_int32 * 9)(*method.parse_args(bad)[1])
        out, n, err = np.empty(64, np.uint8), C.c_size_t(0), _lib.Err()
        assert L.zpaqhip_lzht_blocks(ctx._h, b, d.ctypes.data, offs.ctypes.data, 3, out.ctypes.data, 64, C.byref(n), None, C.byref(err)) == -25
