"""Context.preprocess_blocks / compress_method (zpaqhip_preprocess_blocks, zpaqhip_compress_method_blocks) on the GPU:
the pre-processed bytes equal tools.methods.preprocess, the stream equals tools.methods.compress_block, large blocks
round-trip through the GPU decoder and the oracle, the output capacity contract, the refusals through the C ABI, the
streaming compressor and a seeded random sweep."""
import ctypes as C
import io

import numpy as np
import pytest

import oracle
from tests import util
from tools import methods
from zpaqsharp_amd import _lib, compressor, decompresser, method, synth

pytestmark = pytest.mark.gpu

PRE_METHODS = ["x0,1,4,0,3,16", "x6,1,4,0,3,24", "x0,1,12,0,3,16", "x0,5,4,0,3,16", "x0,2,12,0,7,16", "x0,2,3,0,7,16",
               "x0,2,1,0,7,16", "x0,2,64,0,7,16", "x0,6,5,0,3,16c0,0,511", "x0,4ci1,1,1,1,2am"]
SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 255, 4097, 65536)


def _data(kind, n, seed):
    return synth.plain(kind, seed, n).tobytes()


def _special():
    rng = np.random.default_rng(7)
    e8 = bytearray()
    for _ in range(400):                            # runs of E8 / E9 ending in 00 / FF: the E8E9 candidates chain
        e8 += bytes(rng.choice([0xE8, 0xE9], int(rng.integers(1, 9)))) + bytes(rng.choice([0, 0xFF], int(rng.integers(1, 5))))
        e8 += bytes(rng.integers(0, 256, int(rng.integers(0, 4)), dtype=np.uint8))
    return [bytes(300_000), b"ab" * 50_000, bytes(e8), b"\xe8" * 2000 + b"\0" * 10, b"\xe9\xe8\xe8\xe8\xe8\xff\xff\xff\xff"]


@pytest.mark.parametrize("m", PRE_METHODS)
def test_preprocess_matches_the_reference_preprocessor(ctx, m):
    args = method.parse_args(m)[1]
    blocks = [_data(k, n, 11 * n + i) for i, k in enumerate("TXR") for n in SIZES] + _special()
    want = [methods.preprocess(b, args) for b in blocks]
    got = ctx.preprocess_blocks(m, blocks)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (m, i, len(blocks[i]))
    assert ctx.preprocess_blocks(m, blocks[:12]) == want[:12]


@pytest.mark.parametrize("m", ["x0,1,4,0,3,16", "x0,2,12,0,7,16", "x0,5,4,0,3,16"])
def test_preprocess_of_a_mib_of_text(ctx, m):
    d = util.text(1 << 20, seed=9)
    assert ctx.preprocess_blocks(m, [d]) == [methods.preprocess(d, method.parse_args(m)[1])]


@pytest.mark.parametrize("m", PRE_METHODS + ["x0,2,12,0,7,16,1c0,0,511i2", "x0,0ci1,1,1,1,2awm"])
def test_compress_method_matches_the_cpu_writer(ctx, m):
    model, _ = method.model_of(m)
    sizes = (0, 1, 5, 300, 4097, 20000) if model.n else SIZES
    blocks = [_data(k, n, 3 * n + i) for i, k in enumerate("TR") for n in sizes]
    if not model.n:
        blocks += _special()[:3]
    names = [f"f{i}" for i in range(len(blocks))]
    want = b"".join(methods.compress_block(m, b, names[i].encode()) for i, b in enumerate(blocks))
    got = ctx.compress_method(m, blocks, filenames=names)
    assert got == want, m
    assert ctx.compress_method(m, blocks, filenames=names, batch_blocks=1) == want
    if not model.n:
        assert ctx.stats().kernel_kind == 0
    assert oracle.decompress(got, cap=sum(map(len, blocks)) + 64) == b"".join(blocks)


@pytest.mark.parametrize("m", ["x2,1,4,0,3,22", "x2,5,4,0,3,22"])
@pytest.mark.parametrize("kind", ["T", "R"])
def test_eight_4mib_blocks_round_trip(ctx, m, kind):
    blocks = [_data(kind, 4 << 20, 100 + i) for i in range(8)]
    s = ctx.compress_method(m, blocks)
    st = ctx.stats()
    assert st.blocks == 8 and st.in_bytes == 8 * (4 << 20) and st.init_ms > 0 and st.kernel_kind == 0
    plain = b"".join(blocks)
    assert ctx.decompress(s, verify_sha1=True).tobytes() == plain
    # one decode launch for lazy2; its E8E9 variant runs on the generic kernel in a second launch, as the decoder does for
    # every E8E9 LZ77 block (test_methods.test_store_kernel_hands_back_what_it_does_not_take)
    assert ctx.stats().launches == (2 if method.parse_args(m)[1][1] >= 4 else 1)
    assert oracle.decompress(s, cap=len(plain) + 64) == plain


def test_short_output_buffer_reports_the_exact_size(ctx):
    for m in ("x0,1,4,0,3,16", "x0,6,5,0,3,16c0,0,511"):
        args = method.parse_args(m)[1]
        model, _ = method.model_of(m)
        blocks = [util.text(5000, seed=i) for i in range(3)]
        got, offs, first = ctx._compress(model.header, model.pcomp, [np.frombuffer(b, np.uint8) for b in blocks], None, None, 3,
                                         0, 0, 0, out_cap=100, args=args)
        assert first == -20
        assert got == b"".join(methods.compress_block(m, b) for b in blocks)
        assert list(offs) == [0] + list(np.cumsum([len(methods.compress_block(m, b)) for b in blocks]))
    L = _lib.load()
    a = (C.c_int32 * 9)(*method.parse_args("x0,2,12,0,7,16")[1])
    d = np.frombuffer(util.text(9000, seed=2), np.uint8)
    offs = np.array([0, d.size], np.uint64)
    out, n, err = np.empty(10, np.uint8), C.c_size_t(0), _lib.Err()
    assert L.zpaqhip_preprocess_blocks(ctx._h, a, d.ctypes.data, offs.ctypes.data, 1, out.ctypes.data, 10, C.byref(n), None,
                                       C.byref(err)) == -20
    assert n.value == len(methods.preprocess(d.tobytes(), list(a)))


@pytest.mark.parametrize("m, size", [("x0,3ci1", 10), ("x0,2,0,0,7,16", 10), ("x0,2,65,0,7,16", 10), ("x0,1,4,0,3,16", (1 << 20) + 1)])
def test_refusals_through_the_c_abi(ctx, m, size):
    L = _lib.load()
    args = method.parse_args(m)[1]
    a = (C.c_int32 * 9)(*args)
    model, _ = method.model_of(m)
    d = np.zeros(size, np.uint8)
    offs = np.array([0, size], np.uint64)
    out, n, err = np.empty(1 << 16, np.uint8), C.c_size_t(0), _lib.Err()
    hdr = np.frombuffer(model.header, np.uint8)
    assert L.zpaqhip_preprocess_blocks(ctx._h, a, d.ctypes.data, offs.ctypes.data, 1, out.ctypes.data, out.size, C.byref(n), None,
                                       C.byref(err)) == -25
    assert L.zpaqhip_compress_method_blocks(ctx._h, a, hdr.ctypes.data, hdr.size, None, 0, d.ctypes.data, offs.ctypes.data, 1, None,
                                            out.ctypes.data, out.size, C.byref(n), None, None, C.byref(err)) == -25


class _ShortReader(decompresser.Reader):
    def __init__(self, data, step):
        self.b, self.step = io.BytesIO(data), step

    def read(self, n):
        return self.b.read(min(n, self.step))


class _Sink(decompresser.Writer):
    def __init__(self):
        self.parts = []

    def write(self, b):
        self.parts.append(bytes(b))


@pytest.mark.parametrize("m", ["x0,1,4,0,3,16", "x0,6,5,0,3,16c0,0,511"])
def test_compressor_with_a_method_round_trips_short_reads(ctx, m):
    data = util.text(150_000, seed=4)
    w = _Sink()
    compressor.compress(_ShortReader(data, 777), w, block_size=1 << 16, context=ctx, batch_blocks=2, method=m)
    s = b"".join(w.parts)
    blocks = [data[i:i + (1 << 16)] for i in range(0, len(data), 1 << 16)]
    assert s == ctx.compress_method(m, blocks)
    assert ctx.decompress(s, verify_sha1=True).tobytes() == data


def test_seeded_random_sweep_matches_the_cpu_writer(ctx):
    rng = np.random.default_rng(2026)
    for trial in range(100):
        level, e8 = int(rng.integers(0, 3)), bool(rng.integers(0, 2))
        a0 = int(rng.integers(0, 7))
        a2 = int(rng.integers(1, 65)) if level == 2 else int(rng.integers(0, 20))
        tail = ["", "", "c0,0,511", "ci1"][int(rng.integers(0, 4))]
        m = f"x{a0},{level + 4 * e8},{a2},0,{int(rng.integers(0, 8))},16{tail}"
        n = int(rng.choice([0, 1, 7, 64, 300, 2000, 9000, 30000] if tail else [0, 1, 7, 64, 300, 9000, 70000]))
        kind = "TXR"[int(rng.integers(0, 3))]
        blocks = [_data(kind, n, trial), _data("T", int(rng.integers(0, 3000)), trial + 1000)]
        want = b"".join(methods.compress_block(m, b) for b in blocks)
        assert ctx.compress_method(m, blocks) == want, (trial, m, n, kind)
