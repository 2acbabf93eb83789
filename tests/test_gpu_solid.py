"""Solid blocks on the GPU (zpaqhip_compress_solid_blocks[_device]; Context.compress_solid / compress_solid_device;
compressor.compress_files): several segments per block on the lane-per-component and the generic encoder, byte for byte
against the oracle's Compressor driven segment by segment, and back through the GPU decoders with per-segment lengths,
statuses and SHA-1s.  The sizes are small: what can go wrong is at the segment boundaries (empty segments, segments that end
on the edges of the 64-byte input step and of the 256-byte output chunk), not in the bulk."""
import numpy as np
import pytest
import torch

import oracle
from tests import util
from zpaqsharp_amd import api, compressor, decompresser, models, synth

pytestmark = pytest.mark.gpu

OUT_FULL = -20
GUARD = 0xC3


def _want(model, blocks, names=None, pre=None, sha1=True, tag=True):
    """The stream oracle.Compressor writes for the blocks, a list of lists of segments."""
    m = models.get(model) if isinstance(model, str) else model
    out = []
    for bi, segs in enumerate(blocks):
        coded = pre[bi] if pre is not None else segs
        c = oracle.Compressor(16 * (sum(map(len, coded)) + len(m.pcomp or b"") + 8) + len(segs) * 512 + len(m.header) + 4096)
        if tag:
            c.write_tag()
        c.start_block(m.header)
        for si, s in enumerate(segs):
            name = names[bi][si] if names is not None else ""
            c.start_segment(name.encode(), str(len(s)).encode())
            if si == 0:
                c.post_process(m.pcomp or b"")
            c.compress(coded[si])
            c.end_segment(oracle.sha1(s) if sha1 else None)
        c.end_block()
        out.append(c.getvalue())
    return out


def _decodes(ctx, stream, blocks):
    segs = [s for b in blocks for s in b]
    out, res = ctx.decompress_segments(stream, verify_sha1=True)
    assert out.tobytes() == b"".join(segs)
    assert [int(r.out_len) for r in res[:len(segs)]] == [len(s) for s in segs]
    assert all(r.status == 0 for r in res[:len(segs)])


@pytest.fixture(scope="module")
def parts120():
    """120 segments of 0 to 2 500 bytes, every seventh empty, out of 200 KB of text (tests/test_gpu_parity.py's block)."""
    rng = np.random.default_rng(9)
    text = util.text(200000, seed=31)
    parts, pos = [], 0
    for i in range(120):
        n = int(rng.integers(0, 2500)) if i % 7 else 0
        parts.append(text[pos:pos + n])
        pos += n
    return parts


def _shapes(seed):
    x = util.text(700, seed=seed)
    t = util.text(2000, seed=seed + 1)
    return [[b""], [b"", x], [x, b""], [b"a", b"b", b"c", b"d", b"e"], [x],
            [t[0:63], t[63:127], t[127:192]], [t[200:455], t[455:711], t[711:968]]]


def _names(blocks):
    return [[f"b{bi}/f{si}" if (bi + si) % 4 else "" for si in range(len(b))] for bi, b in enumerate(blocks)]


@pytest.mark.parametrize("model,kernel", [("l1", 0), ("l1", 1), ("l1", 2), ("min", 1), ("min", 2), ("mid", 1), ("mid", 2), ("max", 2),
                                          ("max", 1)])
def test_solid_blocks_match_the_oracle(ctx, parts120, model, kernel):
    blocks = _shapes(11)
    if kernel == 2:
        blocks.append(parts120)
    else:                                    # the one-lane encoder: a 20-segment cut of it (max: 4 097 bytes per block at most)
        cut, room = [], 4097 if model == "max" else 1 << 30
        for p in parts120[:20]:
            cut.append(p[:room])
            room -= len(cut[-1])
        blocks.append(cut)
    names = _names(blocks)
    got = ctx.compress_solid(model, blocks, filenames=names, kernel=kernel)
    st = ctx.stats()
    want = _want(model, blocks, names)
    pos = 0
    for bi, w in enumerate(want):            # block by block, for a failure that names the shape
        assert got[pos:pos + len(w)] == w, f"block {bi} ({len(blocks[bi])} segments)"
        pos += len(w)
    assert pos == len(got)
    assert st.blocks == len(blocks) and st.out_bytes == len(got) and st.in_bytes == sum(len(s) for b in blocks for s in b)
    if kernel == 2:                          # the single-CM model's multi-segment blocks too
        assert st.kernel_kind == 3
    _decodes(ctx, got, blocks)
    few = blocks[:6]
    got = ctx.compress_solid(model, few, sha1=False, tag=False, kernel=kernel)
    assert got == b"".join(_want(model, few, sha1=False, tag=False))


@pytest.mark.parametrize("kernel", [1, 2])
def test_solid_blocks_with_a_post_processor(ctx, kernel):
    """A PCOMP and caller-supplied coded bytes: the program goes out in the first segment only, and its state (the LZ77
    history of models.LZ77_PCOMP) spans the segments."""
    rep = util.text(300, seed=4)
    blocks = [[rep * 3, b"", rep[:100] + util.text(500, seed=5) + rep], [b"", rep], [util.text(65, seed=6)]]
    pre = [[bytes(synth.lz77_encode(s)) for s in b] for b in blocks]
    assert sum(len(p) for b in pre for p in b) < sum(len(s) for b in blocks for s in b)
    names = _names(blocks)
    got = ctx.compress_solid("min+lz77", blocks, pre=pre, filenames=names, kernel=kernel)
    assert got == b"".join(_want("min+lz77", blocks, names, pre=pre))
    _decodes(ctx, got, blocks)


@pytest.mark.parametrize("model", ["l1", "min", "mid"])
def test_one_segment_per_block_is_compress_blocks(ctx, model):
    plain = [util.text(5000, seed=3), util.x86ish(3000), b"", b"z", util.text(257, seed=8)]
    names = ["a", "b", "", "d", "e"]
    for kernel in (0, 1, 2):
        want = ctx.compress_blocks(model, plain, filenames=names, kernel=kernel)
        kind = ctx.stats().kernel_kind
        got = ctx.compress_solid(model, [[p] for p in plain], filenames=[[n] for n in names], kernel=kernel)
        assert got == want and ctx.stats().kernel_kind == kind, kernel
        if model == "l1" and kernel == 0:
            assert kind == 2
    assert want == b"".join(oracle.compress_block(models.get(model).header, p, filename=n.encode()) for p, n in zip(plain, names))


@pytest.fixture(scope="module")
def many_blocks():
    text = util.text(300 * 3 * 230, seed=17)
    blocks, pos = [], 0
    for b in range(300):
        segs = []
        for s in range(3):
            n = 170 + (b * 7 + s * 31) % 60
            segs.append(text[pos:pos + n])
            pos += n
        blocks.append(segs)
    return blocks


def test_more_blocks_than_compute_units(ctx, many_blocks):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert len(many_blocks) > cus
    got = ctx.compress_solid("min", many_blocks, kernel=2, enc_waves=0)
    st = ctx.stats()
    assert st.kernel_kind == 3 and st.concurrent > cus
    assert got == b"".join(_want("min", many_blocks))
    one = ctx.compress_solid("min", many_blocks, kernel=2, enc_waves=1)
    assert ctx.stats().concurrent <= cus and one == got
    _decodes(ctx, got, many_blocks)


@pytest.mark.parametrize("model,kernel", [("min", 2), ("min", 1), ("l1", 2)])
def test_slot_overflow_gives_the_same_bytes(ctx, model, kernel):
    rng = np.random.default_rng(12)
    rnd = bytes(rng.integers(0, 256, 900, dtype=np.uint8))
    blocks = [[rnd[:300], rnd[300:301], rnd[301:]], [util.text(40, seed=1), b"", b"q"], [rnd[:257], b"", rnd[257:600]]]
    want = ctx.compress_solid(model, blocks, kernel=kernel)
    got = ctx.compress_solid(model, blocks, kernel=kernel, slot_bytes=64)
    assert ctx.stats().launches > 1          # the retry ran
    assert got == want == b"".join(_want(model, blocks))
    _decodes(ctx, got, blocks)


def _device(ctx, model, blocks, names, out_cap, **kw):
    """compress_solid_device on unaligned buffers (d_in one byte, d_out three bytes into their tensors): (rc, needed, block
    offsets, the out_cap bytes); checks that nothing around them changed."""
    segs = [s for b in blocks for s in b]
    in_off = np.zeros(len(segs) + 1, np.uint64)
    in_off[1:] = np.cumsum([len(s) for s in segs], dtype=np.uint64)
    seg_first = np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint64)
    buf = np.frombuffer(b"".join(segs) + b"\0", np.uint8).copy()
    d_in = torch.full((1 + buf.size + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    d_in[1:1 + buf.size].copy_(torch.from_numpy(buf))
    d_out = torch.full((3 + out_cap + 256,), GUARD, dtype=torch.uint8, device="cuda")
    rc, need, off = ctx.compress_solid_device(model, d_in.data_ptr() + 1, in_off, seg_first, d_out.data_ptr() + 3, out_cap,
                                              filenames=names, **kw)
    got = d_out.cpu().numpy()
    assert (got[:3] == GUARD).all() and (got[3 + out_cap:] == GUARD).all(), "bytes around d_out changed"
    assert (d_in.cpu().numpy()[1:1 + buf.size] == buf).all()
    return rc, need, off, got[3:3 + out_cap]


@pytest.mark.parametrize("case", ["120_segments", "300_blocks"])
def test_device_form_is_the_host_form(ctx, parts120, many_blocks, case):
    blocks = [[b"x"], parts120, [b"", b"y"]] if case == "120_segments" else many_blocks
    names = _names(blocks)
    want = ctx.compress_solid("min", blocks, filenames=names, kernel=2)
    h_st = ctx.stats()
    ends = np.cumsum([len(w) for w in _want("min", blocks, names)])
    assert ends[-1] == len(want)
    rc, need, off, got = _device(ctx, "min", blocks, names, len(want), kernel=2)
    d_st = ctx.stats()
    assert rc == 0 and need == len(want) and got.tobytes() == want
    assert [int(x) for x in off] == [0] + [int(e) for e in ends]
    assert (d_st.blocks, d_st.in_bytes, d_st.out_bytes, d_st.kernel_kind) == (h_st.blocks, h_st.in_bytes, h_st.out_bytes, h_st.kernel_kind)
    # one byte short: the exact size, the earlier blocks intact, nothing of the last one, nothing behind out_cap
    rc, need, off, got = _device(ctx, "min", blocks, names, len(want) - 1, kernel=2)
    assert rc == OUT_FULL and need == len(want)
    last = int(ends[-2])
    assert got[:last].tobytes() == want[:last] and (got[last:] == GUARD).all()
    assert [int(x) for x in off] == [0] + [int(e) for e in ends]


def test_compress_files_packs_small_files_into_solid_blocks(ctx):
    rng = np.random.default_rng(21)
    text = util.text(40 * 3000, seed=23)
    files, pos = [], 0
    for i in range(40):
        n = int(rng.integers(0, 3001)) if i % 9 else 0
        files.append((f"dir/file{i}.txt", text[pos:pos + n]))
        pos += n

    w = decompresser.BytesWriter()
    compressor.compress_files(files, w, model="min", block_size=16384, context=ctx, kernel=2)
    solid = bytes(w.buf)
    groups = compressor.pack_files([len(d) for _, d in files], 16384)
    assert 1 < len(groups) < len(files)
    blocks = [[files[i][1] for i in g] for g in groups]
    assert solid == b"".join(_want("min", blocks, [[files[i][0] for i in g] for g in groups]))
    _decodes(ctx, solid, blocks)
    sc = api.scan(solid)
    s = np.frombuffer(solid, np.uint8)
    got = [bytes(s[int(g.name_off):int(g.name_off) + int(g.name_len)]).decode() for g in sc.segments]
    assert got == [n for n, _ in files] and sc.n_blocks == len(groups)
    apart = ctx.compress_blocks("min", [d for _, d in files], filenames=[n for n, _ in files], kernel=2)
    print(f"solid {len(solid)} bytes, one file per block {len(apart)} bytes, plaintext {pos} bytes")
    assert len(solid) < len(apart)


SEG_TABLE_CASES = [("min", 1), ("min", 2), ("l1", 2)]


@pytest.fixture(scope="module")
def later_batches():
    """Three blocks whose second and third start at non-zero offsets of every per-segment array: an empty one, one of three
    segments (1 byte, none, 4 097 bytes) and one of 300 bytes."""
    t = util.text(4097 + 300 + 1, seed=41)
    return [[b""], [t[:1], b"", t[1:4098]], [t[4098:]]]


@pytest.mark.parametrize("model,kernel", SEG_TABLE_CASES)
def test_a_batch_per_block_frames_the_bytes_of_one_batch(ctx, later_batches, model, kernel):
    """batch_blocks=1: every batch but the first starts at a non-zero segment, coded offset and stream position."""
    want = b"".join(_want(model, later_batches))
    got = ctx.compress_solid(model, later_batches, kernel=kernel, batch_blocks=1)
    assert got == want
    assert got == ctx.compress_solid(model, later_batches, kernel=kernel, batch_blocks=0)
    _decodes(ctx, got, later_batches)


@pytest.mark.parametrize("model,kernel", SEG_TABLE_CASES)
def test_a_batch_per_block_with_a_retry_frames_the_same_bytes(ctx, later_batches, model, kernel):
    """... and with slots of 64 bytes the block of three segments goes again: the retry's segment ends cut the same bytes."""
    got = ctx.compress_solid(model, later_batches, kernel=kernel, batch_blocks=1, slot_bytes=64)
    assert ctx.stats().launches > 3          # a launch per batch, and the retry
    assert got == b"".join(_want(model, later_batches))
    assert got == ctx.compress_solid(model, later_batches, kernel=kernel, batch_blocks=0, slot_bytes=64)
