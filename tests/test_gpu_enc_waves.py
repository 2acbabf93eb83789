"""Several encoder waves per compute unit on the lane-per-component encoder (zh_enc_chain.hip, compress opts.kernel == 2,
opts.enc_waves): a launch with more blocks than the device has compute units puts up to four waves into a workgroup, each
with its own LDS region and arena slot and its own blocks.  Every case compares the stream with the CPU stream writer byte
for byte and decodes it with its SHA-1s checked; stats().concurrent tells how many blocks were in flight."""
import functools

import numpy as np
import pytest

from tests import chain_cases as cc
from tests import util
from zpaqsharp_amd import api, method, models, synth, zpaql

pytestmark = pytest.mark.gpu

BWT = "x0,3ci1"
LENGTHS = (0, 1, 2, 63, 64, 65, 300, 700, 1500, 2048)
# catalogue chains with small tables: the ones whose two nibbles' rows coincide (the encoder's rows_patch), a MATCH buffer
# that wraps, the largest chains (one wave only), the placements of H and M, and two random ones (the long programs of the
# catalogue cost 1700 instructions a byte: they run in the placement test below, on fewer and shorter blocks)
DIRECTED = ["tiny-tables", "tiny-tables-2", "cm4-alone", "cm8-alone", "match-wrap", "match-wrap-2", "n64-h0", "units64",
            "sse-mix2-extremes", "placement-9-12", "placement-9-13", "placement-10-12", "placement-10-13",
            "placement-native-m4-9-12"]
RANDOM = [(0, 0), (3, 5)]
IDENTITY = ["min", "mid", BWT, cc.M4] + DIRECTED + [f"random-{g}-{i}" for g, i in RANDOM]


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _model(name):
    if name in ("min", "mid", "max"):
        return models.get(name)
    if name in (BWT, cc.M4):
        return method.model_of(name)[0]
    if name.startswith("random-"):
        g, i = map(int, name.split("-")[1:])
        return zpaql.assemble(cc.random_group(g, cc.seed())[i])
    return zpaql.assemble(cc.DIRECTED[name].cfg)


@functools.lru_cache(maxsize=None)
def _pool() -> bytes:
    rng = np.random.default_rng(99)
    return util.text(8192, 41) + util.x86ish(4096, 42) + rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()


def _blocks(nb, lengths=LENGTHS, seed=7):
    pool = _pool()
    starts = np.random.default_rng(seed).integers(0, len(pool) - max(lengths), nb)
    return [pool[int(s):int(s) + lengths[i % len(lengths)]] for i, s in enumerate(starts)]


def _encode(ctx, name, blocks, **kw):
    """One kernel=2 call: (stream, stats).  The BWT model codes the transform of each block, as its PCOMP expects."""
    pre = ctx.bwt_blocks(blocks) if name == BWT else None
    got = ctx.compress_blocks(_model(name), blocks, pre=pre, kernel=2, batch_blocks=len(blocks), **kw)
    st = ctx.stats()
    assert st.kernel_kind == 3 and st.blocks == len(blocks) and st.out_bytes == len(got)
    return got, st


def _want(ctx, name, blocks):
    if name != BWT:
        return synth.compress_blocks(_model(name), blocks)
    pre = ctx.bwt_blocks(blocks)
    return [synth.compress_block(_model(name), b, pre=pre[i]) for i, b in enumerate(blocks)]


def _check(ctx, name, blocks, got):
    """The CPU stream writer's bytes, block by block, and the plaintext back from the decoder."""
    want = _want(ctx, name, blocks)
    offs = np.cumsum([0] + [len(w) for w in want])
    assert len(got) == offs[-1], name
    bad = [i for i in range(len(blocks)) if got[offs[i]:offs[i + 1]] != want[i]]
    assert not bad, f"{name}: {len(bad)} of {len(blocks)} blocks differ, first {bad[:8]} (lengths {[len(blocks[i]) for i in bad[:8]]})"
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks), name


@pytest.mark.parametrize("name", IDENTITY)
def test_every_setting_gives_the_same_stream(ctx, name):
    """Three rounds of blocks for every wave the plan allows, and five more: lengths 0 and 1 among them."""
    cus, W = _cus(), api.enc_chain_plan(_model(name))[0]
    assert W >= 1
    blocks = _blocks(3 * cus * W + 5)
    got, st = _encode(ctx, name, blocks)
    assert st.launches == 1
    if name != "mid":                              # (768 arena slots of mid are 100 GB: memory may cap its waves)
        assert st.concurrent == cus * W            # fails before the waves: compression left `concurrent` 0
    for waves in (1, 2, 4):
        other, st = _encode(ctx, name, blocks, enc_waves=waves)
        assert other == got, (name, waves)
        if name != "mid":
            assert st.concurrent == cus * min(W, waves) and st.launches == 1
    _check(ctx, name, blocks, got)


def test_max_runs_two_waves_where_memory_allows(ctx):
    cus = _cus()
    assert api.enc_chain_plan("max")[0] >= 2
    blocks = _blocks(2 * cus + 3, lengths=(1024,))
    got, st = _encode(ctx, "max", blocks)
    assert 1 <= st.concurrent <= 2 * cus
    one, st1 = _encode(ctx, "max", blocks, enc_waves=1)
    assert one == got and 1 <= st1.concurrent <= cus
    _check(ctx, "max", blocks, got)


@pytest.mark.parametrize("name", ["min", BWT, "tiny-tables-2"])
def test_blocks_spread_over_the_compute_units_first(ctx, name):
    """`cus` blocks or fewer run one wave per workgroup, as before the waves; more fill a second, third, fourth wave."""
    cus, W = _cus(), api.enc_chain_plan(_model(name))[0]
    assert W == 4
    for n in (1, 3, cus, cus + 1, cus * W - 1):
        blocks = _blocks(n, seed=n)
        got, st = _encode(ctx, name, blocks)
        assert st.concurrent == n and st.launches == 1, (name, n)
        one, st1 = _encode(ctx, name, blocks, enc_waves=1)
        assert one == got and st1.concurrent == min(n, cus), (name, n)
        _check(ctx, name, blocks, got)


def test_a_long_block_among_short_ones(ctx):
    """One wave of a workgroup codes 256 KiB while the others finish block after block and leave."""
    cus = _cus()
    big = (_pool() * 16)[:256 << 10]
    blocks = _blocks(4 * cus, lengths=(1024,))
    blocks.insert(cus + 1, big)                    # taken by a second wave of some workgroup
    got, st = _encode(ctx, "min", blocks)
    assert st.concurrent == 4 * cus
    _check(ctx, "min", blocks, got)


@pytest.mark.parametrize("name", ["min", "tiny-tables"])
def test_overflowed_blocks_of_a_many_wave_launch_go_again(ctx, name):
    cus = _cus()
    blocks = _blocks(2 * cus + 3)
    got, st = _encode(ctx, name, blocks)
    assert st.launches == 1 and st.concurrent == 2 * cus + 3
    small, st = _encode(ctx, name, blocks, slot_bytes=16)   # most of the blocks code into more than 16 bytes
    assert small == got and st.launches == 2 and st.concurrent == 2 * cus + 3
    _check(ctx, name, blocks, got)


@pytest.mark.parametrize("name", ["placement-9-12", "placement-10-13", "placement-9-13", "placement-10-12", "long-hcomp-2048",
                                  "long-hcomp-2049", "placement-native-min-10-13", "placement-native-m4-9-12", "min", cc.M4])
def test_hcomp_placements_on_more_than_one_wave(ctx, name):
    """H and M in a wave's LDS region or in its arena slot, the program window in LDS or in global memory, interpreted
    programs (the catalogue's) and translated ones (min's, the level 4 model's), three waves to a workgroup."""
    cus, W = _cus(), api.enc_chain_plan(_model(name))[0]
    assert W >= 3
    blocks = _blocks(2 * cus + 3, lengths=LENGTHS[:7] if name.startswith("long-hcomp") else LENGTHS, seed=11)
    got, st = _encode(ctx, name, blocks)
    assert st.concurrent == 2 * cus + 3 and st.launches == 1
    _check(ctx, name, blocks, got)


def test_enc_waves_above_four_is_refused(ctx):
    with pytest.raises(api.ZpaqError):
        ctx.compress_blocks("min", [b"abc"], kernel=2, enc_waves=5)
    assert ctx.compress_blocks("min", [b"abc"], kernel=0, enc_waves=4) == synth.compress_block("min", b"abc")
    assert ctx.stats().kernel_kind == 1 and ctx.stats().concurrent == 0   # no effect without the chain encoder
