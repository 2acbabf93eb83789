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


E_VERIFY = -28


@pytest.fixture(scope="module")
def five_blocks():
    """Plaintext of 0, 1, 15, 4 097 and 70 000 bytes with x86-like calls, its forward E8E9 transform, and the stream the
    oracle's Compressor writes for l1+e8e9 from the two."""
    m = models.get("l1+e8e9")
    plain = [util.x86ish(n, seed=50 + i) if n > 15 else util.text(n, seed=50 + i) for i, n in enumerate((0, 1, 15, 4097, 70000))]
    pre = [oracle.e8e9(b) for b in plain]
    assert pre[3] != plain[3] and pre[4] != plain[4]
    want = []
    for b, p in zip(plain, pre):
        c = oracle.Compressor(16 * (len(p) + len(m.pcomp) + 8) + len(m.header) + 4096)
        c.write_tag()
        c.start_block(m.header)
        c.start_segment(b"", str(len(b)).encode())
        c.post_process(m.pcomp)
        c.compress(p)
        c.end_segment(oracle.sha1(b))
        c.end_block()
        want.append(c.getvalue())
    return plain, pre, b"".join(want)


def test_host_orig_serves_sha1_and_verify_in_every_batch(ctx, five_blocks):
    """`pre=` puts `orig` on the host: SHA-1 and verify of a batch read one upload of its range of it, and the batches
    behind the first start at non-zero offsets of it."""
    plain, pre, want = five_blocks
    got = ctx.compress_blocks("l1+e8e9", plain, pre=pre, sha1=True, verify=True, batch_blocks=2)
    assert got == want
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(plain)
    bad = list(pre)
    bad[3] = bad[3][:2000] + bytes([bad[3][2000] ^ 0x55]) + bad[3][2001:]
    with pytest.raises(api.ZpaqError) as e:
        ctx.compress_blocks("l1+e8e9", plain, pre=bad, sha1=True, verify=True, batch_blocks=2)
    assert (e.value.code, e.value.block) == (E_VERIFY, 3)


def test_device_orig_at_an_odd_base_gives_the_same_bytes(ctx, five_blocks):
    import torch
    plain, pre, want = five_blocks

    def offs(parts):
        return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)

    def dev(parts, shift):
        buf = np.frombuffer(b"".join(parts), np.uint8).copy()
        t = torch.full((shift + buf.size + 32,), 0x5A, dtype=torch.uint8, device="cuda")
        t[shift:shift + buf.size].copy_(torch.from_numpy(buf))
        return t

    tin, torig = dev(pre, 0), dev(plain, 3)
    tout = torch.zeros(len(want) + 16, dtype=torch.uint8, device="cuda")
    rc, n, off = ctx.compress_blocks_device("l1+e8e9", tin.data_ptr(), offs(pre), tout.data_ptr(), len(want), d_orig=torig.data_ptr() + 3,
                                            orig_off=offs(plain), sha1=True, verify=True, batch_blocks=2)
    assert (rc, n) == (0, len(want))
    assert tout.cpu().numpy()[:n].tobytes() == want
