"""Level 3 (BWT) compression on the GPU: Context.bwt_blocks / zpaqhip_bwt_blocks equal the reference transform byte for
byte (a suffix array is unique), on small blocks against tools.methods.bwt_level3, on large text blocks against the C++
writer's pre-processor and on degenerate 4 MiB blocks against closed forms; Context.compress_method(bwt=True) writes the
streams of tools.methods.compress_block, which the GPU decoder and the oracle read back; the C ABI's flag bit and capacity
contract; the streaming compressor; a seeded sweep.

The 4 MiB round trips use `x3,3`: a BWT block holds at most 2^(args[0] + 20) - 4096 bytes (LibZPAQ.cs:289; n + 5 must fit
bwtrle's M), so `x2` stops 4096 bytes short of 4 MiB (tests/test_bwt.py pins that refusal)."""
import ctypes as C
import io

import numpy as np
import pytest

import oracle
from tests import util
from tests.test_bwt import one_byte_bwt, period2_bwt
from tools import methods
from zpaqsharp_amd import _lib, compressor, decompresser, method, synth

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 255, 4097, 65536)
MODEL_SIZES = (0, 1, 5, 300, 4097, 20000, 65536)


def _data(kind, n, seed):
    return synth.plain(kind, seed, n).tobytes()


def _special():
    rng = np.random.default_rng(7)
    e8 = bytearray()
    for _ in range(400):                            # runs of E8 / E9 ending in 00 / FF: the E8E9 candidates chain
        e8 += bytes(rng.choice([0xE8, 0xE9], int(rng.integers(1, 9)))) + bytes(rng.choice([0, 0xFF], int(rng.integers(1, 5))))
        e8 += bytes(rng.integers(0, 256, int(rng.integers(0, 4)), dtype=np.uint8))
    return [bytes(300_000), b"ab" * 50_000, bytes(e8), b"\xe8" * 2000 + b"\0" * 10, b"\xe9\xe8\xe8\xe8\xe8\xff\xff\xff\xff"]


@pytest.mark.parametrize("e8", [False, True])
def test_bwt_matches_the_doubling_reference(ctx, e8):
    args = method.parse_args("x0,7" if e8 else "x0,3")[1]
    blocks = [_data(k, n, 11 * n + i) for i, k in enumerate("TXR") for n in SIZES] + _special()
    blocks += [b"ab" * 50_000 + b"a", bytes(range(256)) * 300, bytes(np.random.default_rng(5).integers(0, 3, 40_000, dtype=np.uint8))]
    want = [methods.preprocess(b, args) for b in blocks]
    got = ctx.bwt_blocks(blocks, e8e9=e8)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (e8, i, len(blocks[i]))
    assert ctx.stats().launches > 0 and ctx.stats().blocks == len(blocks)
    assert ctx.bwt_blocks(blocks[:12], e8e9=e8) == want[:12]
    assert ctx.bwt_blocks(blocks[9:11], e8e9=e8) == want[9:11]
    assert ctx.bwt_blocks([], e8e9=e8) == []


@pytest.mark.parametrize("mib", [4, 17])
def test_bwt_of_large_text_blocks(ctx, mib):
    d = _data("T", mib << 20, 40 + mib)
    args = method.parse_args("x5,3")[1]
    assert ctx.bwt_blocks([d]) == [synth.preprocess(args, d)]


def test_bwt_of_degenerate_4mib_blocks(ctx):
    """One byte value and period 2: the common prefixes are as long as the block, the sort still takes its log2(n) rounds.
    Closed forms: tests/test_bwt.py (checked there against bwt_level3 at 4 KiB)."""
    n = 4 << 20
    got = ctx.bwt_blocks([b"z" * n])
    assert got == [one_byte_bwt(122, n)]
    got = ctx.bwt_blocks([b"ab" * (n // 2)])
    assert got == [period2_bwt(97, 98, n // 2)]
    got = ctx.bwt_blocks([b"z" * n, b"ab" * (n // 2), bytes(n)])
    assert got == [one_byte_bwt(122, n), period2_bwt(97, 98, n // 2), one_byte_bwt(0, n)]


@pytest.mark.parametrize("m", ["x0,3ci1", "x0,7ci1", "x4,3ci1", "x0,3", "x0,7"])
def test_compress_method_bwt_matches_the_cpu_writer(ctx, m):
    model, _ = method.model_of(m)
    sizes = MODEL_SIZES if model.n else SIZES
    blocks = [_data(k, n, 3 * n + i) for i, k in enumerate("TR") for n in sizes]
    if not model.n:
        blocks += _special()[:3]
    names = [f"f{i}" for i in range(len(blocks))]
    want = b"".join(methods.compress_block(m, b, names[i].encode()) for i, b in enumerate(blocks))
    got = ctx.compress_method(m, blocks, filenames=names, bwt=True)
    assert got == want, m
    assert ctx.compress_method(m, blocks, filenames=names, batch_blocks=1, bwt=True) == want
    if not model.n:
        assert ctx.stats().kernel_kind == 0
    plain = b"".join(blocks)
    assert oracle.decompress(got, cap=len(plain) + 64) == plain
    assert ctx.decompress(got, verify_sha1=True).tobytes() == plain


def test_level3_stays_refused_without_the_keyword(ctx):
    with pytest.raises(ValueError):
        ctx.compress_method("x0,3", [b"abc"])
    with pytest.raises(ValueError):
        ctx.preprocess_blocks("x0,3", [b"abc"])


@pytest.mark.parametrize("kind", ["T", "R"])
def test_eight_4mib_blocks_round_trip(ctx, kind):
    blocks = [_data(kind, 4 << 20, 100 + i) for i in range(8)]
    s = ctx.compress_method("x3,3", blocks, bwt=True)
    st = ctx.stats()
    assert st.blocks == 8 and st.in_bytes == 8 * (4 << 20) and st.init_ms > 0 and st.kernel_kind == 0
    plain = b"".join(blocks)
    assert ctx.decompress(s, verify_sha1=True).tobytes() == plain
    assert ctx.stats().launches == 1                # zh_store.hip takes plain BWT blocks
    assert oracle.decompress(s, cap=len(plain) + 64) == plain


def test_a_17mib_block_round_trips(ctx):
    d = _data("T", 17 << 20, 7)
    s = ctx.compress_method("x5,3", [d], bwt=True)      # args[0] > 4: bwtrle's list form
    assert ctx.decompress(s, verify_sha1=True).tobytes() == d
    assert ctx.stats().launches == 1


def test_flag_bit_and_capacity_through_the_c_abi(ctx):
    L = _lib.load()
    m = "x0,3ci1"
    args = method.parse_args(m)[1]
    a = (C.c_int32 * 9)(*args)
    model, _ = method.model_of(m)
    blocks = [util.text(5000, seed=i) for i in range(3)]
    d = np.frombuffer(b"".join(blocks), np.uint8)
    offs = np.array([0, 5000, 10000, 15000], np.uint64)
    hdr, pc = np.frombuffer(model.header, np.uint8), np.frombuffer(model.pcomp, np.uint8)
    want = ctx.compress_method(m, blocks, bwt=True)
    assert want == b"".join(methods.compress_block(m, b) for b in blocks)

    def call(flags, cap):
        o = _lib.CompressOpts()
        o.struct_size, o.flags = C.sizeof(_lib.CompressOpts), flags
        out, n, err = np.empty(max(1, cap), np.uint8), C.c_size_t(0), _lib.Err()
        rc = L.zpaqhip_compress_method_blocks(ctx._h, a, hdr.ctypes.data, hdr.size, pc.ctypes.data, pc.size, d.ctypes.data,
                                              offs.ctypes.data, 3, None, out.ctypes.data, cap, C.byref(n), None, C.byref(o), C.byref(err))
        return rc, n.value, out[:min(cap, n.value)].tobytes()

    assert call(3, 1 << 16)[0] == -25
    rc, n, got = call(7, 1 << 16)
    assert rc == 0 and got == want
    rc, n, _ = call(7, 100)
    assert rc == -20 and n == len(want)

    pre = [methods.bwt_level3(b) for b in blocks]
    for cap in (15015, 10):
        out, n, err = np.empty(cap, np.uint8), C.c_size_t(0), _lib.Err()
        oo = np.zeros(4, np.uint64)
        rc = L.zpaqhip_bwt_blocks(ctx._h, 0, d.ctypes.data, offs.ctypes.data, 3, out.ctypes.data, cap, C.byref(n), oo.ctypes.data,
                                  C.byref(err))
        assert n.value == 15015 and list(oo) == [0, 5005, 10010, 15015]
        assert rc == (0 if cap == 15015 else -20)
        if rc == 0:
            assert out.tobytes() == b"".join(pre)
            st = ctx.stats()
            assert st.kernel_ms == st.init_ms > 0 and st.in_bytes == 15000 and st.out_bytes == 15015


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


def test_compressor_with_a_bwt_method_round_trips_short_reads(ctx):
    m = "x0,3ci1"
    data = util.text(150_000, seed=4)
    w = _Sink()
    compressor.compress(_ShortReader(data, 777), w, block_size=60_000, context=ctx, batch_blocks=2, method=m, bwt=True)
    s = b"".join(w.parts)
    blocks = [data[i:i + 60_000] for i in range(0, len(data), 60_000)]
    assert s == ctx.compress_method(m, blocks, bwt=True)
    assert s == b"".join(methods.compress_block(m, b) for b in blocks)
    assert ctx.decompress(s, verify_sha1=True).tobytes() == data


def test_seeded_random_sweep_matches_the_cpu_writer(ctx):
    rng = np.random.default_rng(2027)
    for trial in range(60):
        e8 = bool(rng.integers(0, 2))
        a0 = int(rng.integers(0, 7))
        tail = ["", "ci1"][int(rng.integers(0, 2))]
        m = f"x{a0},{3 + 4 * e8}{tail}"
        n = int(rng.choice([0, 1, 7, 64, 300, 2000, 9000, 30000] if tail else [0, 1, 7, 64, 300, 9000, 70000]))
        kind = "TXR"[int(rng.integers(0, 3))]
        blocks = [_data(kind, n, trial), _data("T", int(rng.integers(0, 3000)), trial + 1000)]
        want = b"".join(methods.compress_block(m, b) for b in blocks)
        assert ctx.compress_method(m, blocks, bwt=True) == want, (trial, m, n, kind)
