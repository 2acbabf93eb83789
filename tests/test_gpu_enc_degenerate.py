"""The compression side on degenerate plaintext (tests/degenerate_cases.py): constant, periodic, few-valued and half-constant
blocks through every encoder (zh_enc_cm.hip, zh_enc_chain.hip, zh_enc_generic.hip), every pre-processor (zh_pre_*.hip), the
gap analysis (zh_analyze.hip), the numeric levels, launches in which a wave takes several blocks, and the device-resident
forms.  On these inputs probabilities and counts saturate, the coder emits a few bytes and its final flush dominates, every
byte falls into one context window or one hash row, MATCH sits at 255 and then breaks, and a method's coded sequence is a
handful of codes behind a PCOMP header.

Every assertion is byte equality with the CPU writers (synth.compress_block, tools.methods.compress_block /
preprocess, the restated gap histogram), which tests/test_degenerate_cases.py shows to agree with the oracle on this
catalogue; every stream is decoded again with its SHA-1s checked.  The CPU references are computed once per process
(the catalogue caches them)."""
import functools
import hashlib

import numpy as np
import pytest

import oracle
from tests import degenerate_cases as dc
from tests.chain_cases import LEVEL5
from zpaqsharp_amd import method, models, synth
from zpaqsharp_amd.zpaql import assemble

pytestmark = pytest.mark.gpu

NONE = 2**64 - 1
CM_MODELS = ["l1"] + [f"cm{s}:{K}:{lim}" for s in (9, 22) for K in (9, 16) for lim in (1, 255)]
NAMED = ["min", "mid", "max", "max+e8e9"]
METHOD_MODELS = ["x0,3ci1", "x0,2,12,0,7,16,1c0,0,511i2", "x0,0ci1,1,1,1,2am", "x0,0ci1,1,1,1,2awm", "x0,6,5,0,3,16c0,0,511", LEVEL5]
ONE_LANE_SHORT = ("max", "max+e8e9", LEVEL5)        # on the one-lane encoder these code the short forms only
HALF = len(dc.names())                              # blocks()[HALF:] are the short forms
LABELS = dc.names() + [k + "[:257]" for k in dc.names()]


def _cm_model(size_bits, K, limit):
    return assemble(f"comp 0 0 0 0 1\n  0 cm {size_bits} {limit}\nhcomp\n  a<<= {K} *d=a halt\nend\n")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(model, pre-processed blocks or None, the CPU writer's stream of every block of blocks())."""
    if name in NAMED or name == "l1":
        return models.get(name), None, dc.model_streams(name)
    if name.startswith("cm"):
        m = _cm_model(*(int(x) for x in name[2:].split(":")))
        return m, None, tuple(dc.each(lambda b: synth.compress_block(m, b), dc.blocks()))
    m = method.model_of(name)[0]
    pre = dc.pre_of(name)
    want = tuple(dc.each(lambda bp: synth.compress_block(m, bp[0], pre=np.frombuffer(bp[1], np.uint8)), zip(dc.blocks(), pre)))
    return m, pre, want


TAG = bytes([0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3])


def _same_stream(got: bytes, want, labels, what):
    """`got` is the concatenation of `want`, block by block.  The message names the blocks that differ: after one, the walk
    goes on at the next block's tag, so a block of another length does not take the ones behind it along."""
    pos, bad = 0, []
    for w, label in zip(want, labels):
        if got[pos:pos + len(w)] == w:
            pos += len(w)
        else:
            bad.append(label)
            nxt = got.find(TAG, pos + 1)
            pos = nxt if nxt >= 0 else len(got)
    total = sum(map(len, want))
    assert not bad and len(got) == total, f"{what}: {len(got)} bytes for {total}; blocks that differ: {bad}"


def _encode_and_check(ctx, name, kernel, kind, only_short=False):
    """One compress_blocks call over blocks() (or their short forms): the route, the counts, the CPU writer's bytes, and the
    plaintext back from the decoder."""
    model, pre, want = _reference(name)
    sel = slice(HALF, None) if only_short else slice(None)
    blocks, want = dc.blocks()[sel], want[sel]
    pre = None if pre is None else [np.frombuffer(p, np.uint8) for p in pre[sel]]
    got = ctx.compress_blocks(model, blocks, pre=pre, kernel=kernel)
    st = ctx.stats()
    assert st.kernel_kind == kind, (name, kernel)
    assert st.blocks == len(blocks) and st.out_bytes == len(got) and st.in_bytes == sum(map(len, blocks))
    _same_stream(got, want, LABELS[sel], f"{name} kernel={kernel}")
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks)


# ---- 1. the encoders, by model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,kind", [(0, 2), (1, 1)])
@pytest.mark.parametrize("name", CM_MODELS)
def test_single_cm_encoders(ctx, name, kernel, kind):
    """The window-parallel encoder (every byte of `zeros` in one window, `period256` in all of them alike) and the one-lane
    generic encoder: a count limit of 1 and of 255, a table of 2^9 and of 2^22 entries."""
    _encode_and_check(ctx, name, kernel, kind)


@pytest.mark.parametrize("name", NAMED + METHOD_MODELS)
def test_chain_encoder(ctx, name):
    """The lane-per-component encoder; the method models code tools.methods.preprocess of each block."""
    _encode_and_check(ctx, name, 2, 3)


@pytest.mark.parametrize("name", NAMED + METHOD_MODELS)
def test_one_lane_encoder_on_chain_models(ctx, name):
    """The one-lane generic encoder: max, max+e8e9 and the level 5 recipe on the short forms (the suite keeps this encoder to
    4097 bytes of those models), the others on every block."""
    _encode_and_check(ctx, name, 1, 1, only_short=name in ONE_LANE_SHORT)


# ---- 2. methods end to end -------------------------------------------------------------------------------------------------
def _gpu_pre(ctx, m, parse, blocks):
    if parse == "bwt":
        return ctx.bwt_blocks(blocks, e8e9=method.parse_args(m)[1][1] >= 4)
    return {"": ctx.preprocess_blocks, "ht": ctx.lzht_blocks, "sa": ctx.lzsa_blocks}[parse](m, blocks)


@pytest.mark.parametrize("m,parse", dc.METHODS)
def test_methods_end_to_end(ctx, m, parse):
    blocks, want_pre, want = dc.blocks(), dc.pre_of(m, parse), dc.method_streams(m, parse)
    got_pre = _gpu_pre(ctx, m, parse, blocks)
    bad = [LABELS[i] for i in range(len(blocks)) if got_pre[i] != want_pre[i]]
    assert not bad, f"{m} {parse}: pre-processed bytes differ for {bad}"
    modelled = method.model_of(m)[0].n > 0
    got = ctx.compress_method(m, blocks, kernel=2 if modelled else 0, bwt=parse == "bwt", **dc.parse_kw(parse))
    st = ctx.stats()
    assert st.kernel_kind == (3 if modelled else 0) and st.blocks == len(blocks) and st.out_bytes == len(got)
    _same_stream(got, want, LABELS, f"{m} {parse}")
    plain = b"".join(blocks)
    assert oracle.decompress(got, cap=len(plain) + 64) == plain
    assert ctx.decompress(got, verify_sha1=True).tobytes() == plain


# ---- 3. levels -------------------------------------------------------------------------------------------------------------
def test_gap_hist_of_the_catalogue(ctx):
    got = ctx.gap_hist_blocks(dc.blocks())
    want = dc.gap_hists()
    assert got.shape == want.shape and (got == want).all(), [i for i in range(len(want)) if (got[i] != want[i]).any()]


ALL = tuple(range(2 * HALF))
LEVELS = [(lv, "all") for lv in "1234"] + [(lv, part) for lv in ("5", "5,128,1") for part in dc.LEVEL5_PARTS]


def _level_case(level, part):
    """(blocks, their expanded method strings, their streams, their names) of blocks(), or of one part of it at the levels
    whose every method string costs a second (degenerate_cases.LEVEL5_PARTS)."""
    ids = ALL if part == "all" else dc.LEVEL5_PARTS[part]
    return ([dc.blocks()[i] for i in ids], [dc.level_methods(level)[i] for i in ids], [dc.level_streams(level)[i] for i in ids],
            [LABELS[i] for i in ids])


@pytest.mark.parametrize("level,part", LEVELS)
def test_levels(ctx, level, part):
    blocks, want_methods, want, labels = _level_case(level, part)
    got = ctx.compress_level(level, blocks)
    assert ctx.level_methods == want_methods
    if level[0] == "5":                                # periodic models and the plain one in one call
        assert len(set(ctx.level_methods)) >= 4
    _same_stream(got, want, labels, f"level {level}")
    assert ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks)


# ---- 4. several blocks per wave --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cus() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _tiny_reference(name):
    m = method.model_of(LEVEL5)[0] if name == "level5" else models.get(name)
    blocks = dc.tiny_blocks(3 * _cus() + 5)
    return m, blocks, synth.compress_blocks(m, blocks)


@pytest.mark.parametrize("name,enc_waves", [("min", 1), ("min", 0), ("mid", 1), ("mid", 0), ("level5", 1), ("level5", 0), ("max", 0)])
def test_a_wave_encodes_several_degenerate_blocks(ctx, name, enc_waves):
    """Three rounds of blocks per compute unit and five more in one batch: a wave carries what a saturated block left in its
    tables, its LDS region and its arena slot into the next one, which may be empty, one byte or another constant."""
    m, blocks, want = _tiny_reference(name)
    nb = len(blocks)
    got = ctx.compress_blocks(m, blocks, kernel=2, batch_blocks=nb, enc_waves=enc_waves)
    st = ctx.stats()
    assert st.kernel_kind == 3 and st.launches == 1 and st.blocks == nb and st.out_bytes == len(got)
    _same_stream(got, want, [f"{i} ({len(b)} bytes)" for i, b in enumerate(blocks)], f"{name} enc_waves={enc_waves}")
    plain = b"".join(blocks)
    assert ctx.decompress(got, verify_sha1=True, kernel=4, dec_waves=4).tobytes() == plain
    assert ctx.decompress(got, verify_sha1=True).tobytes() == plain


# ---- 5. device-resident forms ----------------------------------------------------------------------------------------------
DEVICE_METHODS = [("x0,2,5,0,3,20c0,0,511", "ht"), ("x0,2,12,0,7,21,1c0,0,511i2", "sa"), ("x0,3ci1", "bwt")]


def _dev(data: bytes, shift: int):
    """`data` in device memory `shift` bytes into its tensor (torch allocations are 512-byte aligned): (tensor, pointer)."""
    import torch
    t = torch.full((shift + len(data) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + shift


def _offs(blocks):
    return [0] + np.cumsum([len(b) for b in blocks]).tolist()


@pytest.mark.parametrize("m,parse", DEVICE_METHODS)
def test_compress_method_device(ctx, m, parse):
    import torch
    blocks = dc.blocks()
    want = b"".join(dc.method_streams(m, parse))
    tin, pin = _dev(b"".join(blocks), 3)
    cap = len(want) + 4096
    for verify in (False, True):
        tout = torch.full((cap,), 0xC3, dtype=torch.uint8, device="cuda")
        rc, n, boff = ctx.compress_method_device(m, pin, _offs(blocks), tout.data_ptr(), cap, kernel=2, bwt=parse == "bwt",
                                                 verify=verify, **dc.parse_kw(parse))
        assert rc == 0 and n == len(want), (m, verify, rc, n)
        assert tout[:n].cpu().numpy().tobytes() == want, (m, verify)
        assert boff.tolist() == _offs(dc.method_streams(m, parse))
        assert bool((tout[n:] == 0xC3).all())
    del tin
    assert ctx.decompress(want, verify_sha1=True).tobytes() == b"".join(blocks)


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("part", list(dc.LEVEL5_PARTS))
def test_compress_level_device(ctx, part, verify):
    import torch
    blocks, want_methods, want, _ = _level_case("5", part)
    stream = b"".join(want)
    tin, pin = _dev(b"".join(blocks), 5)
    cap = len(stream) + 4096
    tout = torch.full((cap,), 0xC3, dtype=torch.uint8, device="cuda")
    rc, n, boff = ctx.compress_level_device("5", pin, _offs(blocks), tout.data_ptr(), cap, verify=verify)
    assert rc == 0 and n == len(stream), (verify, rc, n)
    assert ctx.level_methods == want_methods and len(set(want_methods)) >= 4
    assert tout[:n].cpu().numpy().tobytes() == stream
    assert boff.tolist() == _offs(want)
    assert bool((tout[n:] == 0xC3).all())
    del tin
    assert ctx.decompress(stream, verify_sha1=True).tobytes() == b"".join(blocks)


@pytest.mark.parametrize("m,parse", DEVICE_METHODS)
def test_verify_blocks(ctx, m, parse):
    """The verify pass on the CPU pre-processor's bytes: a few codes that expand to a whole block."""
    blocks, pre = dc.blocks(), dc.pre_of(m, parse)
    rec = ctx.verify_blocks(m, pre, blocks)
    bare = ctx.verify_blocks(m, pre)
    for i, b in enumerate(blocks):
        want = {"status": 0, "out_len": len(b), "first_diff": NONE, "sha1": hashlib.sha1(b).digest()}
        assert rec[i] == want and bare[i] == want, (m, parse, i)
