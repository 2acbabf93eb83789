"""Numeric levels on the GPU: Context.gap_hist_blocks (zpaqhip_gap_hist_blocks, zh_analyze.hip) against the restatement of
LibZPAQ.cs:242-255, Context.compress_level against compress_method on the literal method strings and through the
decoder, blocks of one call that need different methods, and compressor.compress(level=)."""
import io

import numpy as np
import pytest

from tests import util
from tests.test_levels import LEVEL5_TAIL, MOD7, MOD7_METHOD, TABLE, gap_shapes, ref_gap_hist, ref_periods
from zpaqsharp_amd import compressor, decompresser, method

pytestmark = pytest.mark.gpu

SLICE = 12288                   # ZH_GAP_SLICE (zh_analyze.h): bytes one lane of zh_gap_hist counts


@pytest.fixture(scope="module")
def shapes():
    blocks = gap_shapes(SLICE)
    rng = np.random.default_rng(8)
    blocks.append(rng.integers(0, 256, 64 * SLICE + 5, dtype=np.uint8).tobytes())       # a second workgroup, 5 bytes long
    blocks.append((util.text(50000, seed=4) * 19)[:900001])                            # text, two workgroups
    assert max(map(len, blocks)) <= 1 << 20
    return blocks, np.stack([ref_gap_hist(b) for b in blocks])


def test_gap_hist_equals_the_restatement(ctx, shapes):
    blocks, want = shapes
    assert [len(b) for b in blocks[:10]] == [0, 1, 2, 4095, 4096, 4097, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 1]
    assert want[11, 1] == 69999 and want[12, 4095] > 0 and want[13, 4095] == 0 and want[14, 4095] == 1 and want[15, 4095] == 0
    got = ctx.gap_hist_blocks(blocks)
    assert got.dtype == np.uint32 and got.shape == (len(blocks), 4096)
    assert (got == want).all(), [i for i in range(len(blocks)) if (got[i] != want[i]).any()]
    st = ctx.stats()
    assert st.blocks == len(blocks) and st.in_bytes == sum(map(len, blocks)) and st.launches == 1 and st.kernel_ms > 0
    assert ctx.gap_hist_blocks([]).shape == (0, 4096)
    assert not ctx.gap_hist_blocks([b"", b""]).any()


def test_gap_hist_over_more_blocks_than_a_batch(ctx, shapes):
    blocks, want = shapes                # a batch holds at most 4096 blocks (batch_end)
    ids = [i % 10 for i in range(4100)]
    got = ctx.gap_hist_blocks([blocks[i] for i in ids])
    assert ctx.stats().launches == 2 and ctx.stats().blocks == 4100
    assert (got == want[ids]).all()


def _blocks():
    rng = np.random.default_rng(21)
    return [util.text(16384, seed=3), util.x86ish(5000, seed=4), rng.integers(0, 256, 1024, dtype=np.uint8).tobytes(),
            util.text(3001, seed=5)]


@pytest.mark.parametrize("level", ["0", "1", "2", "3", "4", "1,10,2", "3,4,3", "3,12,1", "4,6,0", "4,128,3"])
def test_compress_level_is_compress_method_of_the_literal_string(ctx, level):
    blocks, literal = _blocks(), TABLE[level]
    got = ctx.compress_level(level, blocks)
    assert ctx.level_methods == [literal] * len(blocks)
    assert got == b"".join(ctx.compress_method(literal, [b], bwt=True, kernel=2) for b in blocks)
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks)


def test_compress_level_5(ctx):
    blocks = [util.text(16384, seed=6), MOD7, util.x86ish(4096, seed=7)]
    plain5 = "x0,0w1i1c256ci1,1,1,1,1,1,2a" + LEVEL5_TAIL
    got = ctx.compress_level("5", blocks, filenames=["a", "b", "c"])
    assert ctx.level_methods == [plain5, MOD7_METHOD, plain5]
    want = [ctx.compress_method(m, [b], bwt=True, kernel=2, filenames=[f]) for m, b, f in zip(ctx.level_methods, blocks, "abc")]
    assert got == b"".join(want)
    hdr = method.model_of(MOD7_METHOD)[0].header
    at = len(want[0]) + 13 + 5                                   # tag, "zPQ", level, 1
    assert got[at:at + len(hdr)] == hdr
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks)


def test_blocks_of_one_call_with_different_methods_keep_their_order(ctx):
    big = (util.text(65536, seed=9) * 16)
    a, b = big[:1044480], big[:1044480] + b"!"
    got = ctx.compress_level("1", [a, b, a[:5000], b])
    assert ctx.level_methods == ["x0,1,5,0,3,20", "x1,1,5,0,3,21", "x0,1,5,0,3,20", "x1,1,5,0,3,21"]
    assert got == (ctx.compress_method("x0,1,5,0,3,20", [a]) + ctx.compress_method("x1,1,5,0,3,21", [b])
                   + ctx.compress_method("x0,1,5,0,3,20", [a[:5000]]) + ctx.compress_method("x1,1,5,0,3,21", [b]))
    assert ctx.decompress(got, verify_sha1=True).tobytes() == a + b + a[:5000] + b
    # level 5: with a period, without, with again
    t = np.random.default_rng(10).integers(0, 256, 6000, dtype=np.uint8).tobytes()
    blocks = [MOD7, t, MOD7[:4099], t[:2000]]
    assert [ref_periods(len(b), ref_gap_hist(b)) for b in blocks] == ["c0,0,1006,255i1c0,7i1", "", "c0,0,1006,255i1c0,7i1", ""]
    got = ctx.compress_level("5", blocks)
    plain5 = "x0,0w1i1c256ci1,1,1,1,1,1,2a" + LEVEL5_TAIL
    assert ctx.level_methods == [MOD7_METHOD, plain5, MOD7_METHOD, plain5]
    assert got == b"".join(ctx.compress_method(m, [b], kernel=2) for m, b in zip(ctx.level_methods, blocks))
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks)


class _Short(decompresser.Reader):
    """A Reader that returns fewer bytes than asked (Reader.cs:14-25 allows it)."""

    def __init__(self, data, step):
        self.f, self.step = io.BytesIO(data), step

    def read(self, n):
        return self.f.read(min(n, self.step))


class _Sink(decompresser.Writer):
    def __init__(self):
        self.parts = []

    def write(self, b):
        self.parts.append(bytes(b))


def test_compress_with_a_level_over_short_reads(ctx):
    data = util.text(50001, seed=12)
    w = _Sink()
    compressor.compress(_Short(data, 777), w, level="1", block_size=20000, context=ctx, batch_blocks=2)
    want = ctx.compress_level("1", [data[i:i + 20000] for i in range(0, len(data), 20000)])
    assert b"".join(w.parts) == want
    assert ctx.decompress(want, verify_sha1=True).tobytes() == data
    assert method.level_block_size("1") == (1 << 24) - 4096     # the cut without block_size=
