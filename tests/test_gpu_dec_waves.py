"""Several decoder waves per compute unit on the lane-per-component decoder (zh_chain.hip's zh_decode_chain_mw, decode
opts.dec_waves): a launch with more blocks than the device has compute units puts up to four waves into a workgroup, each
with its own LDS region and arena slot and its own blocks.  The streams come from the CPU stream writer; every case compares
the plaintext (SHA-1s checked) and the per-segment results with those of dec_waves=0, the one-wave kernel;
stats().concurrent tells how many blocks were in flight."""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import zpaqsharp_amd as z
from tests import chain_cases as cc
from tests import util
from zpaqsharp_amd import _lib, api, method, models, synth, zpaql

pytestmark = pytest.mark.gpu

BWT = "x0,3ci1"
LENGTHS = (0, 1, 2, 63, 64, 65, 300, 700, 1500, 2048)
# the catalogue chains of tests/test_gpu_enc_waves.py: small tables, the largest chains (one wave only: the one-wave kernel
# whatever the setting), the placements of H and M, and two random ones
DIRECTED = ["tiny-tables", "tiny-tables-2", "cm4-alone", "cm8-alone", "match-wrap", "match-wrap-2", "n64-h0", "units64",
            "sse-mix2-extremes", "placement-9-12", "placement-9-13", "placement-10-12", "placement-10-13",
            "placement-native-m4-9-12"]
RANDOM = [(0, 0), (3, 5), (3, 6)]                  # (the last one has 16 units: two waves)
SAME = ["min", "mid", BWT, cc.M4] + DIRECTED + [f"random-{g}-{i}" for g, i in RANDOM]


@functools.lru_cache(maxsize=None)
def _cus() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _model(name):
    if name in ("min", "mid", "max"):
        return models.get(name)
    if name in (BWT, cc.M4, cc.LEVEL5):
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


def _write(name, blocks):
    """The CPU stream writer's block for each plaintext.  The BWT model codes the transform of each block, as its PCOMP expects."""
    m = _model(name)
    if name != BWT:
        return synth.compress_blocks(m, blocks)
    args = method.model_of(name)[1]
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda b: synth.compress_block(m, b, pre=synth.preprocess(args, b)), blocks))


def _decode(ctx, stream, nb, damaged=False, **kw):
    """One zpaqhip_decompress_segments call on a stream of `nb` one-segment blocks of at most 2 KiB, all in one batch:
    (plaintext, [(status, pp_state, out_off, out_len, in_used)], stats)."""
    a = np.frombuffer(stream, np.uint8)
    o = api.make_opts(batch_blocks=nb, **kw)
    err, n, nr = _lib.Err(), C.c_size_t(0), C.c_size_t(0)
    res = (_lib.SegResult * nb)()
    # (a damaged block is decoded on to the end of the stream, through the blocks behind it: one in seven is damaged)
    cap = nb * 2048 + ((nb // 7 + 1) * len(stream) * 3 if damaged else 0)
    out = np.empty(max(1, cap), np.uint8)
    rc = ctx._L.zpaqhip_decompress_segments(ctx._h, a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n), res, nb, C.byref(nr),
                                            C.byref(o), C.byref(err))
    st = ctx.stats()
    assert nr.value == nb and n.value <= cap and (damaged or rc == 0), (rc, err.msg)
    return out[:n.value].tobytes(), [(r.status, r.pp_state, r.out_off, r.out_len, r.in_used) for r in res], st


def _shape(st):
    return st.launches, st.concurrent, st.kernel_kind


@pytest.mark.parametrize("name", SAME)
def test_every_setting_gives_the_same_plaintext(ctx, name):
    """Three rounds of blocks for every wave the plan allows, and five more: lengths 0 and 1 among them."""
    cus, W = _cus(), api.dec_chain_plan(_model(name))[0]
    assert W >= 1
    blocks = _blocks(3 * cus * W + 5)
    nb, plain = len(blocks), b"".join(blocks)
    stream = b"".join(_write(name, blocks))
    base, res0, st0 = _decode(ctx, stream, nb, kernel=4, verify_sha1=True)
    assert base == plain and all(r[0] == 0 for r in res0), name
    assert _shape(st0) == (1, min(nb, 256), 3)                 # one block per workgroup, 256 of them: as before the option
    one, res1, st1 = _decode(ctx, stream, nb, kernel=4, verify_sha1=True, dec_waves=1)
    assert (one, res1, _shape(st1)) == (base, res0, _shape(st0)), name
    for waves in (2, 3, 4):
        got, res, st = _decode(ctx, stream, nb, kernel=4, verify_sha1=True, dec_waves=waves)
        assert got == plain, (name, waves)
        assert res == res0, (name, waves)
        if W == 1:
            assert _shape(st) == _shape(st0), (name, waves)
        else:
            print(f"{name}: dec_waves={waves} plan {W}: in flight {st.concurrent}, kernel {st.kernel_ms:.1f} ms "
                  f"(one wave: {st0.kernel_ms:.1f} ms)")
            assert _shape(st) == (1, min(cus, 256) * min(W, waves), 3), (name, waves)   # fails before the waves


@pytest.mark.parametrize("m", ["x0,1,4,0,3,16ci1", "x0,2,12,0,7,16,1c0,0,511i2", "x0,3ci1", "x0,7ci1", "x0,4ci1,1,1,1,2am"])
def test_post_processors_behind_the_new_kernel(ctx, m):
    """lzpre (levels 1 and 2), bwtrle without and with E8E9, and E8E9 alone: the translated post-processors behind a call
    (zh_decode_chain_mw_pc) and the inlined E8E9, each wave with its own PCOMP memories and sink."""
    cus = _cus()
    model, args = method.model_of(m)
    nb, size = 2 * cus + 3, 1500
    stream, offs = synth.method_stream(model, args, "X" if args[1] & 4 else "T", nb, size)
    stream = stream.tobytes()
    base, res0, st0 = _decode(ctx, stream, nb, kernel=4, verify_sha1=True)
    assert len(base) == nb * size and all(r[0] == 0 for r in res0) and {r[1] for r in res0} == {5}
    got, res, st = _decode(ctx, stream, nb, kernel=4, verify_sha1=True, dec_waves=4)
    W = api.dec_chain_plan(model)[0]
    assert W >= 3
    assert got == base and res == res0
    assert _shape(st) == (1, nb, 3) and _shape(st0) == (1, min(nb, 256), 3)


def test_a_wave_s_failure_is_its_own(ctx):
    """Every seventh block damaged (cut short, or a byte of its coded data flipped): the block's wave reports what the
    one-wave kernel reports and goes on to its next block; every other block is whole."""
    cus, W = _cus(), api.dec_chain_plan("min")[0]
    assert W == 4
    blocks = _blocks(cus * W + 9, lengths=(65, 130, 300))        # (short: what follows a damaged block is decoded as its own)
    nb = len(blocks)
    parts = _write("min", blocks)
    for i in range(0, nb, 7):
        g = z.scan(parts[i]).segments[0]
        p = bytearray(parts[i])
        if (i // 7) % 2:                               # a flipped byte in the coded data
            p[g.data_off + 4 + (i % max(1, g.data_len - 8))] ^= 0x55
        else:                                          # the second half of the coded data gone; the end of the segment kept
            p[g.data_off + g.data_len // 2:g.data_off + g.data_len] = b"\0\0\0\0"
        parts[i] = bytes(p)
    stream = b"".join(parts)
    assert z.scan(stream).n_blocks == nb
    base, res0, st0 = _decode(ctx, stream, nb, damaged=True, kernel=4)
    got, res, st = _decode(ctx, stream, nb, damaged=True, kernel=4, dec_waves=4)
    assert [(r[0], r[3]) for r in res] == [(r[0], r[3]) for r in res0]
    assert res == res0 and got == base
    assert st.concurrent == cus * W and st.kernel_kind == 3 and st.launches == st0.launches
    assert sum(r[0] != 0 for r in res) >= nb // 7 // 2          # the damage is seen ...
    for i, r in enumerate(res):                                  # ... and stays where it is
        if i % 7:
            assert r[0] == 0 and got[r[2]:r[2] + r[3]] == blocks[i], i


@pytest.mark.parametrize("name", ["min", BWT])
def test_fewer_blocks_than_compute_units_run_the_one_wave_kernel(ctx, name):
    cus = _cus()
    for n in (1, 3, min(cus, 256)):
        blocks = _blocks(n, seed=n)
        stream = b"".join(_write(name, blocks))
        base, res0, st0 = _decode(ctx, stream, n, kernel=4, verify_sha1=True)
        got, res, st = _decode(ctx, stream, n, kernel=4, verify_sha1=True, dec_waves=4)
        assert got == base == b"".join(blocks) and res == res0
        assert _shape(st) == _shape(st0) == (1, n, 3)


def test_blocks_spread_over_the_compute_units_first(ctx):
    """One block more than workgroups brings the second wave; the blocks in flight are the waves with a block."""
    cus = _cus()
    for n in (cus + 1, 2 * cus + 1, 4 * cus - 1):
        blocks = _blocks(n, seed=n)
        stream = b"".join(_write("min", blocks))
        got, res, st = _decode(ctx, stream, n, kernel=4, verify_sha1=True, dec_waves=4)
        assert got == b"".join(blocks)
        assert _shape(st) == (1, n, 3), n
        got, res, st = _decode(ctx, stream, n, kernel=4, verify_sha1=True, dec_waves=2)
        assert got == b"".join(blocks)
        assert _shape(st) == (1, min(n, 2 * cus), 3), n


def test_default_routing_reaches_the_new_kernel(ctx):
    """kernel=0 sends a chain without a kernel of its own to zh_chain's level walk: dec_waves applies there; min, which
    kernel=0 sends to zh_nibble, is not touched."""
    cus = _cus()
    name = "tiny-tables-2"
    assert api.dec_chain_plan(_model(name))[0] >= 3
    blocks = _blocks(2 * cus + 3)
    nb, plain = len(blocks), b"".join(blocks)
    stream = b"".join(_write(name, blocks))
    base, res0, st0 = _decode(ctx, stream, nb, verify_sha1=True)
    got, res, st = _decode(ctx, stream, nb, verify_sha1=True, dec_waves=4)
    assert got == base == plain and res == res0
    assert _shape(st0) == (1, min(nb, 256), 3) and _shape(st) == (1, nb, 3)
    stream = b"".join(_write("min", blocks))
    base, res0, st0 = _decode(ctx, stream, nb, verify_sha1=True)
    got, res, st = _decode(ctx, stream, nb, verify_sha1=True, dec_waves=4)
    assert got == base == plain and res == res0 and _shape(st) == _shape(st0)
    # ... nor a single CM on zh_chain (kernel=3), nor min on zh_chain's own form of it (kernel=5)
    for kernel, model in ((3, "l1"), (5, "min")):
        stream = b"".join(synth.compress_blocks(model, blocks))
        base, res0, st0 = _decode(ctx, stream, nb, verify_sha1=True, kernel=kernel)
        got, res, st = _decode(ctx, stream, nb, verify_sha1=True, kernel=kernel, dec_waves=4)
        assert got == base == plain and res == res0 and _shape(st) == _shape(st0) == (1, min(nb, 256), 3)


def test_models_of_one_launch_share_the_smallest_plan(ctx):
    """min (4 waves) and mid's shape at level 4 (3 waves) in one kernel=4 launch: three waves, pools sized for the larger."""
    cus = _cus()
    blocks = _blocks(3 * cus + 4)
    nb, plain = len(blocks), b"".join(blocks)
    a, b = _write("min", blocks[0::2]), _write(cc.M4, blocks[1::2])
    parts = [None] * nb
    parts[0::2], parts[1::2] = a, b
    stream = b"".join(parts)
    base, res0, st0 = _decode(ctx, stream, nb, kernel=4, verify_sha1=True)
    got, res, st = _decode(ctx, stream, nb, kernel=4, verify_sha1=True, dec_waves=4)
    assert got == base == plain and res == res0
    assert _shape(st) == (1, 3 * cus, 3)


@pytest.mark.parametrize("name", ["max", cc.LEVEL5])
def test_the_large_models_at_their_plan(ctx, name):
    """2 x W + 1 blocks of 1 KiB: max has two waves (with so few blocks the one-wave kernel still runs: the blocks spread
    over the compute units first), the level 5 recipe one."""
    W = api.dec_chain_plan(_model(name))[0]
    assert W == (2 if name == "max" else 1)
    blocks = _blocks(2 * W + 1, lengths=(1024,))
    nb = len(blocks)
    stream = b"".join(_write(name, blocks))
    kernel = 4 if name == "max" else 0
    base, res0, st0 = _decode(ctx, stream, nb, kernel=kernel, verify_sha1=True)
    got, res, st = _decode(ctx, stream, nb, kernel=kernel, verify_sha1=True, dec_waves=W)
    assert got == base == b"".join(blocks) and res == res0
    assert _shape(st) == _shape(st0) == (1, nb, 3)
