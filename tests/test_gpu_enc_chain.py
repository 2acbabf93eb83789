"""The lane-per-component encoder (zh_enc_chain.hip, compress opts.kernel == 2) on the GPU: byte parity with the CPU stream
writer and the one-lane generic encoder for min / mid / max and the method models, eight 4 MiB blocks of mid, the method
path end to end, routing, the overflow re-encode, batching, a seeded sweep and the streaming compressor.

Not covered: a runaway HCOMP.  The compress ABI has no ZPAQL budget (the encoders run with 2^32 instructions per run()),
and the one-lane encoder of the comparison would need minutes to exhaust it."""
import numpy as np
import pytest

import oracle
from tests import util
from tests.chain_cases import LEVEL5
from tools import methods
from zpaqsharp_amd import compressor, decompresser, method, models, synth
from zpaqsharp_amd.zpaql import assemble

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 4097, 65536)
KINDS = ("T", "X", "R")
NAMED = ["min", "mid", "max", "max+e8e9"]
METHOD_MODELS = ["x0,3ci1", "x0,2,12,0,7,16,1c0,0,511i2", "x0,0ci1,1,1,1,2am", "x0,0ci1,1,1,1,2awm", "x0,6,5,0,3,16c0,0,511", LEVEL5]
MODELS = NAMED + METHOD_MODELS


def _data(kind, n, seed):
    return synth.plain(kind, seed, n).tobytes()


def _model(name):
    """(model, method arguments or None): a named model, or the model of a method string, whose blocks are coded from the
    method's pre-processed bytes so that its PCOMP inverts them."""
    if name in NAMED:
        return models.get(name), None
    return method.model_of(name)


def _pre(args, blocks):
    return None if args is None else [np.frombuffer(methods.preprocess(b, args), np.uint8) for b in blocks]


def _want(model, blocks, pre=None, names=None):
    return b"".join(synth.compress_block(model, b, filename=(names[i].encode() if names else b""),
                                         pre=None if pre is None else pre[i]) for i, b in enumerate(blocks))


@pytest.mark.parametrize("name", MODELS)
def test_chain_encoder_matches_the_cpu_writer_and_the_generic_encoder(ctx, name):
    model, args = _model(name)
    blocks = [_data(k, n, 7 * i + j) for i, n in enumerate(SIZES) for j, k in enumerate(KINDS)]
    pre = _pre(args, blocks)
    names = [f"f{i}.bin" for i in range(len(blocks))]
    got = ctx.compress_blocks(model, blocks, pre=pre, filenames=names, kernel=2)
    st = ctx.stats()
    assert st.kernel_kind == 3
    assert st.blocks == len(blocks) and st.out_bytes == len(got) and st.in_bytes == sum(map(len, blocks))
    want = _want(model, blocks, pre, names)
    assert got == want
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks)
    small = [i for i, b in enumerate(blocks) if len(b) <= 4097]
    sb, sp = [blocks[i] for i in small], None if pre is None else [pre[i] for i in small]
    slow = ctx.compress_blocks(model, sb, pre=sp, kernel=1)
    assert ctx.stats().kernel_kind == 1
    assert slow == ctx.compress_blocks(model, sb, pre=sp, kernel=2) == _want(model, sb, sp)


def test_eight_4mib_blocks_of_mid_match_the_stream_writer(ctx):
    bs = 1 << 22
    want, offs = synth.stream("mid", "T", nblocks=8, block_size=bs, threads=16)
    blocks = [synth.plain("T", i, bs) for i in range(8)]
    got = ctx.compress_blocks("mid", blocks, kernel=2)
    assert ctx.stats().kernel_kind == 3
    assert got == want.tobytes()
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(b.tobytes() for b in blocks)


# the modelled entries of test_gpu_compress_method.py's list, and the BWT method
MODELLED_METHODS = ["x0,6,5,0,3,16c0,0,511", "x0,4ci1,1,1,1,2am", "x0,2,12,0,7,16,1c0,0,511i2", "x0,0ci1,1,1,1,2awm", "x3,3ci1"]


@pytest.mark.parametrize("m", MODELLED_METHODS)
def test_compress_method_on_the_chain_encoder_matches_the_cpu_writer(ctx, m):
    bwt = method.parse_args(m)[1][1] & 3 == 3
    blocks = [_data(k, n, 3 * n + i) for i, k in enumerate("TR") for n in (0, 1, 5, 300, 4097, 20000)]
    names = [f"f{i}" for i in range(len(blocks))]
    want = b"".join(methods.compress_block(m, b, names[i].encode()) for i, b in enumerate(blocks))
    got = ctx.compress_method(m, blocks, filenames=names, kernel=2, bwt=bwt)
    assert ctx.stats().kernel_kind == 3
    assert got == want, m
    assert ctx.compress_method(m, blocks, filenames=names, kernel=2, bwt=bwt, batch_blocks=1) == want


@pytest.mark.parametrize("m", ["x3,3ci1", "x2,2,12,0,7,23,1c0,0,511i2"])
def test_eight_1mib_blocks_of_a_method_round_trip(ctx, m):
    blocks = [_data("T", 1 << 20, 200 + i) for i in range(8)]
    s = ctx.compress_method(m, blocks, kernel=2, bwt=m.startswith("x3,3"))
    assert ctx.stats().kernel_kind == 3
    plain = b"".join(blocks)
    assert ctx.decompress(s, verify_sha1=True).tobytes() == plain
    assert oracle.decompress(s, cap=len(plain) + 64) == plain


def test_routing(ctx):
    blocks = [util.text(3000, seed=1), b"", b"q" * 70]
    assert ctx.compress_blocks("l1", blocks, kernel=2) == _want("l1", blocks)
    assert ctx.stats().kernel_kind == 2                  # single-CM models stay on the window-parallel encoder
    # five mixers: more than the lane-per-component kernels take, so build_model classes the header as generic
    five = assemble("comp 1 2 0 0 6\n  0 icm 5\n  1 mix 0 0 1 24 0\n  2 mix 0 0 2 24 0\n  3 mix 0 0 3 24 0\n"
                    "  4 mix 0 0 4 24 0\n  5 mix 0 0 5 24 0\nhcomp\n  *d=a halt\nend\n")
    assert ctx.compress_blocks(five, blocks, kernel=2) == _want(five, blocks)
    assert ctx.stats().kernel_kind == 1
    assert ctx.compress_blocks("mid", blocks, kernel=0) == _want("mid", blocks)
    assert ctx.stats().kernel_kind == 1


@pytest.mark.parametrize("model", ["min", "mid"])
def test_slot_overflow_reencodes_on_the_chain_encoder(ctx, model):
    blocks = [_data(k, n, 3) for k in KINDS for n in (1, 255, 5000, 65536)]
    want = ctx.compress_blocks(model, blocks, kernel=2)
    launches = ctx.stats().launches
    assert ctx.compress_blocks(model, blocks, kernel=2, slot_bytes=16) == want == _want(model, blocks)
    assert ctx.stats().launches == launches + 1
    assert ctx.stats().kernel_kind == 3


def test_batches_give_the_same_bytes(ctx):
    blocks = [_data(KINDS[i % 3], 1000 + 997 * i, i) for i in range(10)]
    one = ctx.compress_blocks("mid", blocks, kernel=2)
    assert ctx.compress_blocks("mid", blocks, kernel=2, batch_blocks=3) == one == _want("mid", blocks)


def test_seeded_random_sweep_matches_the_cpu_writer(ctx):
    rng = np.random.default_rng(2027)
    draws = {}
    for d in range(200):
        name = MODELS[rng.integers(len(MODELS))]
        n = int(rng.choice([0, 1, 2, 17, 255, 256, 257, 1000, 4096, 9000, 30000]))
        kind = KINDS[rng.integers(3)]
        draws.setdefault(name, []).append(_data(kind, n, d))
    for name, blocks in draws.items():
        model, args = _model(name)
        pre = _pre(args, blocks)
        got = ctx.compress_blocks(model, blocks, pre=pre, kernel=2)
        assert ctx.stats().kernel_kind == 3
        assert got == _want(model, blocks, pre), name


def test_compressor_with_the_chain_encoder_round_trips(ctx):
    data = util.text(300000, seed=12)
    w = decompresser.BytesWriter()
    compressor.compress(decompresser.BytesReader(data), w, model="mid", block_size=100000, context=ctx, kernel=2)
    assert ctx.stats().kernel_kind == 3
    bs = [data[i:i + 100000] for i in range(0, len(data), 100000)]
    assert bytes(w.buf) == _want("mid", bs)
    out = decompresser.BytesWriter()
    decompresser.decompress(decompresser.BytesReader(bytes(w.buf)), out, context=ctx)
    assert bytes(out.buf) == data
