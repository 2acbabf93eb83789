"""The lane-per-component encoder (zh_enc_chain.hip, compress opts.kernel == 2) on arbitrary component chains: the seeded
random models and the directed ones of tests/chain_cases.py (tiny tables, a small MATCH buffer, both placements of H, M and
the program, the family's limits and what lies just past them, a model that expands its input), and a launch in which every
wave encodes several blocks.  Byte parity with the CPU stream writer and the one-lane generic encoder; the decoders
(zh_chain.hip, zh_generic.hip) return the plaintext of the same streams.

tests/test_chain_cases.py shows on the CPU that the two CPU writers agree on all of these models."""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests import util
from zpaqsharp_amd import method, models, synth, zpaql

pytestmark = pytest.mark.gpu


def _check(ctx, cfg, blocks, kind=3):
    """One kernel=2 call over `blocks`: the CPU writer's bytes, on the encoder `kind`, and decodable; the two shortest
    blocks also on the one-lane encoder.  Returns (bytes, launches)."""
    m = zpaql.assemble(cfg)
    got = ctx.compress_blocks(m, blocks, kernel=2)
    st = ctx.stats()
    assert st.kernel_kind == kind, cfg
    assert st.blocks == len(blocks) and st.out_bytes == len(got), cfg
    assert got == b"".join(synth.compress_block(m, b) for b in blocks), cfg
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks), cfg
    short = sorted(blocks, key=len)[:2]
    slow = ctx.compress_blocks(m, short, kernel=1)
    assert ctx.stats().kernel_kind == 1, cfg
    assert slow == b"".join(synth.compress_block(m, b) for b in short), cfg
    return got, st.launches


@pytest.mark.parametrize("group", range(cc.GROUPS))
def test_random_chains_on_the_chain_encoder(ctx, group):
    for cfg in cc.random_group(group, cc.seed()):
        _check(ctx, cfg, cc.random_blocks())


@pytest.mark.parametrize("name", list(cc.DIRECTED))
def test_directed_chains(ctx, name):
    case = cc.DIRECTED[name]
    blocks = cc.blocks_of(case)
    got, launches = _check(ctx, case.cfg, blocks, case.kind)
    if case.expands:                               # the automatic slot overflowed: one more launch, and the same bytes as
        worst = 16 * (max(map(len, blocks)) + 1) + 4096   # with a slot that cannot
        assert ctx.compress_blocks(zpaql.assemble(case.cfg), blocks, kernel=2, slot_bytes=worst) == got
        assert ctx.stats().kernel_kind == 3 and ctx.stats().launches == 1 and launches == 2


def _wave_model(name):
    if name == "mid":                              # a translated HCOMP, H and M in LDS
        return models.get("mid")
    if name == "level5":                           # a method model's HCOMP, H in LDS and M (2^16 bytes) in the arena
        return method.model_of(cc.LEVEL5)[0]
    return zpaql.assemble(cc.DIRECTED["placement-10-13"].cfg)   # MATCH + CM + SSE + ICM / ISSE, H and M in the arena


@pytest.mark.parametrize("name", ["mid", "level5", "placement"])
def test_a_wave_encodes_several_blocks(ctx, name):
    """More blocks in one launch than the device has compute units (the grid is at most one wave per unit): every wave
    pulls a second and a third block from the queue, and whatever it kept of the previous one changes the next one's bytes."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = 3 * cus + 5
    lengths = (0, 1, 2, 63, 64, 65, 300)
    rng = np.random.default_rng(99)
    pool = util.text(4096, 41) + util.x86ish(4096, 42) + rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()
    starts = rng.integers(0, len(pool) - 300, nb)
    blocks = [pool[int(s):int(s) + lengths[i % 7]] for i, s in enumerate(starts)]
    m = _wave_model(name)
    got = ctx.compress_blocks(m, blocks, kernel=2, batch_blocks=nb)
    st = ctx.stats()
    # one batch of chain blocks only costs one launch (Call::encode counts the encoders' launches, not the SHA-1's), and none
    # of these blocks outgrows its slot
    assert st.kernel_kind == 3 and st.launches == 1 and st.blocks == nb
    want = synth.compress_blocks(m, blocks)
    offs = np.cumsum([0] + [len(w) for w in want])
    assert len(got) == offs[-1]
    bad = [i for i in range(nb) if got[offs[i]:offs[i + 1]] != want[i]]
    assert not bad, f"{len(bad)} of {nb} blocks differ, first {bad[:8]} (lengths {[len(blocks[i]) for i in bad[:8]]})"
