"""Context.compress_blocks (zpaqhip_compress_blocks) on the GPU: byte parity with the CPU stream writer (synth /
libzpaqgen) and the oracle's Compressor, round trips through the GPU decoders, the window-parallel CM encoder against the
generic one, batching, the slot overflow path and the output capacity contract."""
import numpy as np
import pytest

import oracle
from tests import util
from zpaqsharp_amd import api, compressor, decompresser, models, synth
from zpaqsharp_amd.zpaql import assemble

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 4097, 65536)
KINDS = ("T", "X", "R")


def _data(kind, n, seed):
    return synth.plain(kind, seed, n).tobytes()


def _cm_model(size_bits, K, limit):
    return assemble(f"comp 0 0 0 0 1\n  0 cm {size_bits} {limit}\nhcomp\n  a<<= {K} *d=a halt\nend\n")


def _want(model, blocks, names=None, sha1=True, tag=True):
    return b"".join(synth.compress_block(model, b, filename=(names[i].encode() if names else b""), sha1=sha1, tag=tag)
                    for i, b in enumerate(blocks))


@pytest.mark.parametrize("model", ["l1", "min", "mid", "max", "max+e8e9"])
def test_compress_blocks_matches_the_cpu_writer(ctx, model):
    sizes = SIZES if not model.startswith("max") else SIZES[:-1]    # max on the one-lane generic encoder: 4097 bytes at most
    blocks = [_data(k, n, 7 * i + j) for i, n in enumerate(sizes) for j, k in enumerate(KINDS)]
    names = [f"f{i}.bin" for i in range(len(blocks))]
    got = ctx.compress_blocks(model, blocks, filenames=names)
    st = ctx.stats()
    assert st.blocks == len(blocks) and st.out_bytes == len(got) and st.in_bytes == sum(map(len, blocks))
    assert st.kernel_kind == (2 if model == "l1" else 1)
    assert got == _want(model, blocks, names)
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks)
    small = [b for b in blocks if len(b) <= 4097]
    got = ctx.compress_blocks(model, small, sha1=False, tag=False)
    assert got == _want(model, small, sha1=False, tag=False)
    assert ctx.decompress(got).tobytes() == b"".join(small)


@pytest.mark.parametrize("model", ["l1", "min", "mid"])
def test_compress_blocks_matches_the_oracle(ctx, model):
    m = models.get(model)
    blocks = [util.text(5000, seed=3), util.x86ish(3000), b"", b"z"]
    got = ctx.compress_blocks(model, blocks, filenames=["a", "b", "", "d"])
    want = b"".join(oracle.compress_block(m.header, b, filename=f) for b, f in zip(blocks, [b"a", b"b", b"", b"d"]))
    assert got == want
    got = ctx.compress_blocks(model, blocks[:1], sha1=False, tag=False)
    assert got == oracle.compress_block(m.header, blocks[0], with_sha1=False, tag=False)


def test_eight_4mib_blocks_of_l1_match_the_stream_writer(ctx):
    bs = 1 << 22
    want, offs = synth.stream("l1", "T", nblocks=8, block_size=bs, threads=16)
    blocks = [synth.plain("T", i, bs) for i in range(8)]
    got = ctx.compress_blocks("l1", blocks)
    assert ctx.stats().kernel_kind == 2
    assert got == want.tobytes()
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(b.tobytes() for b in blocks)


def _fast_cases():
    rng = np.random.default_rng(5)
    return [util.text(70000, seed=9), rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), b"\x41" * 100000,
            bytes(range(256)) * 300, b"\x07", util.text(300, seed=2)]


@pytest.mark.parametrize("model", ["l1"] + [f"cm{s}:{K}:{lim}" for s in (9, 20, 22) for K in (9, 12, 16) for lim in (1, 4, 255)])
def test_window_parallel_cm_encoder_matches_the_generic_one(ctx, model):
    if model == "l1":
        m = models.get("l1")
    else:
        s, K, lim = (int(x) for x in model[2:].split(":"))
        m = _cm_model(s, K, lim)
    blocks = _fast_cases()
    fast = ctx.compress_blocks(m, blocks)
    assert ctx.stats().kernel_kind == 2                 # the window-parallel encoder ran
    slow = ctx.compress_blocks(m, blocks, kernel=1)
    assert ctx.stats().kernel_kind == 1
    assert fast == slow
    assert fast == _want(m, blocks)
    assert ctx.decompress(fast, verify_sha1=True).tobytes() == b"".join(blocks)


@pytest.mark.parametrize("model", ["l1", "mid"])
def test_batches_give_the_same_bytes(ctx, model):
    blocks = [_data(KINDS[i % 3], 1000 + 997 * i, i) for i in range(10)]
    assert ctx.compress_blocks(model, blocks, batch_blocks=3) == ctx.compress_blocks(model, blocks) == _want(model, blocks)


@pytest.mark.parametrize("model", ["l1", "min", "l1+e8e9"])
def test_slot_overflow_gives_the_same_bytes(ctx, model):
    blocks = [_data(k, n, 3) for k in KINDS for n in (1, 255, 5000, 65536)]
    want = ctx.compress_blocks(model, blocks)
    launches = ctx.stats().launches
    assert ctx.compress_blocks(model, blocks, slot_bytes=16) == want == _want(model, blocks)
    assert ctx.stats().launches == launches + 1        # the re-encoding launch of the overflowed blocks ran


def test_short_output_buffer_reports_the_exact_size(ctx):
    m = models.get("l1")
    blocks = [np.frombuffer(util.text(20000, seed=4), np.uint8), np.frombuffer(b"abc", np.uint8)]
    want = _want("l1", [b.tobytes() for b in blocks])
    got, offs, first = ctx._compress(m.header, b"", blocks, None, None, 3, 0, 0, 0, out_cap=100)
    assert first == -20                                  # ZPAQHIP_E_OUTPUT_FULL, then the retry with the size it reported
    assert got == want
    assert list(offs) == [0, len(synth.compress_block("l1", blocks[0])), len(want)]
    with pytest.raises(api.ZpaqError):
        ctx._compress(assemble("comp 0 0 0 0 0\nhcomp\nhalt\nend\n").header, b"", blocks, None, None, 3, 0, 0, 0)


def test_lz77_model_needs_pre_and_codes_it(ctx):
    data = util.text(30000, seed=8)
    with pytest.raises(ValueError):
        ctx.compress_blocks("l1+lz77", [data])
    pre = synth.lz77_encode(data)
    got = ctx.compress_blocks("l1+lz77", [data], pre=[pre])
    assert got == synth.compress_block("l1+lz77", data, pre=pre)
    assert ctx.decompress(got, verify_sha1=True).tobytes() == data


def test_compressor_round_trips_through_reader_and_writer(ctx):
    data = util.text(300000, seed=12)
    w = decompresser.BytesWriter()
    compressor.compress(decompresser.BytesReader(data), w, model="l1", block_size=100000, context=ctx)
    bs = [data[i:i + 100000] for i in range(0, len(data), 100000)]
    assert bytes(w.buf) == _want("l1", bs)
    out = decompresser.BytesWriter()
    decompresser.decompress(decompresser.BytesReader(bytes(w.buf)), out, context=ctx)
    assert bytes(out.buf) == data


class ShortReader(decompresser.Reader):
    """A Reader whose read() returns fewer bytes than asked before its end, like one over a pipe or a socket."""

    def __init__(self, data: bytes, most: int):
        self._d, self._p, self._most = data, 0, most

    def read(self, n: int) -> bytes:
        b = self._d[self._p:self._p + min(n, self._most)]
        self._p += len(b)
        return b


def test_compressor_gathers_short_reads_into_whole_blocks(ctx):
    data = util.text(250000, seed=13)
    w = decompresser.BytesWriter()
    compressor.compress(ShortReader(data, 1000), w, model="l1", block_size=100000, context=ctx)
    bs = [data[i:i + 100000] for i in range(0, len(data), 100000)]
    assert bytes(w.buf) == _want("l1", bs)
    out = decompresser.BytesWriter()
    decompresser.decompress(decompresser.BytesReader(bytes(w.buf)), out, context=ctx)
    assert bytes(out.buf) == data


def test_seeded_random_sweep_matches_the_cpu_writer(ctx):
    rng = np.random.default_rng(2024)
    names = ["l1", "min", "mid", "max", "max+e8e9", "l1+e8e9"]
    draws = {}
    for d in range(200):
        model = names[rng.integers(len(names))]
        n = int(rng.choice([0, 1, 2, 17, 255, 256, 257, 1000, 4096, 9000, 30000]))
        kind = KINDS[rng.integers(3)]
        draws.setdefault(model, []).append(_data(kind, n, d))
    for model, blocks in draws.items():
        got = ctx.compress_blocks(model, blocks)
        assert got == _want(model, blocks), model
