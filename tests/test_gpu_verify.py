"""The verify pass on the GPU (Compressor.setVerify; zpaqhip_verify_blocks, bit 5 of zpaqhip_compress_opts.flags): the
pre-processed bytes of a block through the block's own post-processor, sized, hashed and compared with the plaintext.

Blocks have 0, 1, 65 535, 65 537 and 200 001 bytes of synthetic text and x86-like data: around the store layout's 64 KiB chunk
and the LZ77 writers' 4 096-literal flush, and more than the 128 KiB ring of the wave-wide post-processors.  The expected
values come from hashlib, numpy and the oracle's post-processor; nothing here is taken from the code under test.

On the parent commit the library has neither the entry points nor the status, so tests 1 to 4 fail there."""
import hashlib

import numpy as np
import pytest
import torch

import oracle
import zpaqsharp_amd as z
from tests import lzcodes
from tests.verify_cases import SUB1, first_diff
from zpaqsharp_amd import method as mth, synth, zpaql

pytestmark = pytest.mark.gpu

NONE = 2**64 - 1
E_VERIFY, E_ZPAQL = -28, -4
SIZES = [0, 1, 65535, 65537, 200001]

# method -> how its blocks are pre-processed (Context method, extra arguments)
ROUTES = {
    "x0,0ci1": [("preprocess_blocks", None)],
    "x0,4ci1,1,1,1,2am": [("preprocess_blocks", None)],
    "x0,1,4,0,3,20": [("preprocess_blocks", None), ("lzht_blocks", None)],
    "x0,5,4,0,3,20": [("preprocess_blocks", None), ("lzht_blocks", None)],
    "x0,2,12,0,7,21,1": [("preprocess_blocks", None), ("lzsa_blocks", None)],
    "x0,6,12,0,7,21,1": [("preprocess_blocks", None), ("lzsa_blocks", None)],
    "x0,3ci1": [("bwt_blocks", False)],
    "x0,7ci1": [("bwt_blocks", True)],
}
CASES = [(m, how, arg) for m, routes in ROUTES.items() for how, arg in routes]

_plain = {}


def plain_blocks():
    if not _plain:
        _plain["b"] = [synth.plain("TX"[i & 1], 40 + i, n).tobytes() for i, n in enumerate(SIZES)] + \
                      [synth.plain("X", 50, 65537).tobytes(), synth.plain("T", 51, 65535).tobytes()]
    return _plain["b"]


def pre_of(ctx, m, how, arg, blocks):
    if how == "bwt_blocks":
        return ctx.bwt_blocks(blocks, e8e9=arg)
    return getattr(ctx, how)(m, blocks)


def dev(data: bytes, shift: int = 0):
    """`data` in device memory, `shift` bytes into its tensor (an unaligned start): (tensor, pointer)."""
    t = torch.zeros(shift + len(data) + 64, dtype=torch.uint8, device="cuda")
    if data:
        t[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + shift


def offs(blocks):
    return [0] + list(np.cumsum([len(b) for b in blocks]).tolist())


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,how,arg", CASES)
def test_round_trip(ctx, m, how, arg):
    blocks = plain_blocks()
    pre = pre_of(ctx, m, how, arg, blocks)
    rec = ctx.verify_blocks(m, pre, blocks)
    st = ctx.stats()
    bare = ctx.verify_blocks(m, pre)
    # the device form, both buffers off any alignment
    tin, pin = dev(b"".join(pre), 3)
    tor, por = dev(b"".join(blocks), 5)
    drec = ctx.verify_blocks_device(m, pin, offs(pre), d_orig=por, orig_off=offs(blocks))
    dbare = ctx.verify_blocks_device(m, pin, offs(pre))
    del tin, tor
    for i, b in enumerate(blocks):
        want = {"status": 0, "out_len": len(b), "first_diff": NONE, "sha1": hashlib.sha1(b).digest()}
        assert rec[i] == want, (m, how, i, len(b))
        assert bare[i] == want, (m, how, i, len(b))
        assert drec[i] == want, (m, how, i, len(b))
        assert dbare[i] == want, (m, how, i, len(b))
    assert st.blocks == len(blocks) and st.in_bytes == sum(len(p) for p in pre) and st.out_bytes == sum(len(b) for b in blocks)
    assert st.launches >= 3 and st.kernel_ms > 0


# ---- 2. crafted codes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", lzcodes.METHODS)
def test_crafted_codes(ctx, method):
    """Every feed of the edge catalogue (zero distance, distance >= |M|, longest and shortest lengths, a code cut off at the
    end) as the pre-processed bytes of a block of its own: size and SHA-1 of the oracle's post-processor on the same bytes.
    (The E8E9 form with a 16 MiB M has one feed that writes more than |M|: like the decoder, the pass runs it on one lane,
    which takes most of this case's ten seconds.)"""
    info = lzcodes.Info(method)
    feeds, names = [], []
    for name, segs in lzcodes.catalogue(method):
        for k, toks in enumerate(segs):
            feeds.append(lzcodes.feed_of(info, toks))
            names.append((name, k))
    hdr = info.model.header
    want = [oracle.run_pcomp(info.model.pcomp, f, hdr[4], hdr[5], cap=len(lzcodes.expand(info, [f])) + 4096) for f in feeds]
    rec = ctx.verify_blocks(info.model, feeds)
    assert len(rec) == len(feeds)
    for r, w, nm in zip(rec, want, names):
        assert r == {"status": 0, "out_len": len(w), "first_diff": NONE, "sha1": hashlib.sha1(w).digest()}, (method, nm)


# ---- 3. detection ----------------------------------------------------------------------------------------------------------
LZ = "x0,2,12,0,7,21,1c0,0,511"


def _lzpre_positions(feed: bytes):
    """(index of a literal byte, index of the last offset byte of a match) in lzpre codes."""
    i, lit, off = 0, None, None
    while i < len(feed) and (lit is None or off is None):
        c = feed[i]
        if c < 64:
            if lit is None:
                lit = i + 1
            i += 2 + c
        else:
            if off is None and i > 200:
                off = i + 1 + (c >> 6)
            i += 2 + (c >> 6)                                   # the code byte and (c >> 6) + 1 offset bytes
    assert lit is not None and off is not None
    return lit, off


@pytest.mark.parametrize("what", ["literal", "offset"])
def test_detection(ctx, what):
    model, _ = mth.model_of(LZ)
    blocks = [synth.plain("T", 60 + i, 6000 + 17 * i).tobytes() for i in range(3)]
    pre = ctx.preprocess_blocks(LZ, blocks)
    assert all(r["status"] == 0 for r in ctx.verify_blocks(model, pre, blocks))
    lit, off = _lzpre_positions(pre[1])
    at = lit if what == "literal" else off
    bad = bytearray(pre[1])
    bad[at] ^= 1
    tampered = [pre[0], bytes(bad), pre[2]]
    got = oracle.run_pcomp(model.pcomp, tampered[1], model.header[4], model.header[5], cap=4 * len(blocks[1]) + 4096)
    want_diff = first_diff(got, blocks[1])
    assert want_diff != NONE
    rec = ctx.verify_blocks(model, tampered, blocks)
    assert [r["status"] for r in rec] == [0, E_VERIFY, 0]
    assert rec[1]["first_diff"] == want_diff and rec[0]["first_diff"] == rec[2]["first_diff"] == NONE
    assert rec[1]["out_len"] == len(got) and rec[1]["sha1"] == hashlib.sha1(got).digest()
    assert ctx.compress_blocks(model, blocks, pre=tampered, kernel=1)               # (unverified: nothing reports it)
    with pytest.raises(z.ZpaqError) as e:
        ctx.compress_blocks(model, blocks, pre=tampered, kernel=1, verify=True)
    assert (e.value.code, e.value.block) == (E_VERIFY, 1)
    assert "Pre/post-processor test failed" in str(e.value)
    # the device form
    tin, pin = dev(b"".join(tampered), 2)
    tor, por = dev(b"".join(blocks), 9)
    cap = 1 << 16
    tout = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    with pytest.raises(z.ZpaqError) as e:
        ctx.compress_blocks_device(model, pin, offs(tampered), tout.data_ptr(), cap, d_orig=por, orig_off=offs(blocks), kernel=1,
                                   verify=True)
    assert (e.value.code, e.value.block) == (E_VERIFY, 1)
    rc, n, _ = ctx.compress_blocks_device(model, pin, offs(tampered), tout.data_ptr(), cap, d_orig=por, orig_off=offs(blocks),
                                          kernel=1, verify=True, raise_on_error=False)
    assert (rc, n) == (E_VERIFY, 0)
    # ... and with the right bytes the verified call writes what the unverified one writes
    tin2, pin2 = dev(b"".join(pre), 2)
    rc, n, _ = ctx.compress_blocks_device(model, pin2, offs(pre), tout.data_ptr(), cap, d_orig=por, orig_off=offs(blocks), kernel=1,
                                          verify=True)
    assert rc == 0 and tout[:n].cpu().numpy().tobytes() == ctx.compress_blocks(model, blocks, pre=pre, kernel=1)


# ---- 4. the post-processor's own errors, and a caller's own program ---------------------------------------------------------
THIRD = "comp 0 0 0 0 0 hcomp halt pcomp third ; a> 255 if halt endif b=a d++ a=d a== 3 if a++ endif a=b out halt end"


def test_custom_pcomp_verifies_clean_on_the_vm(ctx):
    model = zpaql.assemble(SUB1)
    blocks = [b"", b"\x00", synth.plain("T", 70, 5000).tobytes(), bytes(range(256)) * 3]
    pre = [bytes((c + 1) & 255 for c in b) for b in blocks]
    rec = ctx.verify_blocks(model, pre, blocks)
    for r, b in zip(rec, blocks):
        assert r == {"status": 0, "out_len": len(b), "first_diff": NONE, "sha1": hashlib.sha1(b).digest()}
    wrong = ctx.verify_blocks(model, blocks, blocks)              # not what this PCOMP inverts
    assert [r["status"] for r in wrong] == [0, E_VERIFY, E_VERIFY, E_VERIFY] and wrong[2]["first_diff"] == 0


def test_undefined_opcode_on_the_third_byte(ctx):
    model = zpaql.assemble(THIRD)
    jf1, op, bad_op = bytes([zpaql.JF, 1]), zpaql._MNEMONIC["a++"], 120                # `if a++ endif`: the a++ becomes undefined
    assert model.pcomp.count(jf1 + bytes([op])) == 1 and zpaql.is_error_op(bad_op)
    model = zpaql.Model(model.header, model.pcomp.replace(jf1 + bytes([op]), jf1 + bytes([bad_op])), model.pcomp_cmd)
    data = b"abcdefgh"
    with pytest.raises(oracle.OracleError):
        oracle.run_pcomp(model.pcomp, data, 0, 0)
    rec = ctx.verify_blocks(model, [data[:2], data, b""], [data[:2], data, b""])
    assert [r["status"] for r in rec] == [0, E_ZPAQL, 0]
    assert rec[1]["out_len"] == 2 and rec[1]["sha1"] == hashlib.sha1(b"ab").digest()
    assert rec[0]["out_len"] == 2 and rec[0]["first_diff"] == NONE
    lz, _ = mth.model_of(LZ)
    framed = zpaql.Model(lz.header[:4] + bytes([0, 0]) + lz.header[6:], model.pcomp, model.pcomp_cmd)
    with pytest.raises(z.ZpaqError) as e:
        ctx.compress_blocks(framed, [b"xy", data], pre=[b"xy", data], kernel=1, verify=True)
    assert (e.value.code, e.value.block) == (E_ZPAQL, 1)


# ---- 5. same bytes ---------------------------------------------------------------------------------------------------------
def _three():
    b = plain_blocks()
    return [b[2], b[1], b[5]]


@pytest.mark.parametrize("m", list(ROUTES))
def test_same_bytes_methods(ctx, m):
    blocks = _three()
    kw = dict(bwt=True, kernel=2)
    base = ctx.compress_method(m, blocks, **kw)
    l0 = ctx.stats().launches
    assert ctx.compress_method(m, blocks, verify=True, **kw) == base
    st = ctx.stats()
    assert st.launches > l0
    assert ctx.decompress(base, out_cap=sum(map(len, blocks)) + 64).tobytes() == b"".join(blocks)
    for sa, ht in ((True, False), (False, True)):
        if (sa and mth.uses_sa(mth.parse_args(m)[1])) or (ht and mth.uses_ht(mth.parse_args(m)[1])):
            assert ctx.compress_method(m, blocks, sa=sa, ht=ht, verify=True, **kw) == ctx.compress_method(m, blocks, sa=sa, ht=ht, **kw)
    # device forms: the method call and the mixed call
    tin, pin = dev(b"".join(blocks), 3)
    cap = len(base) + 4096
    tout = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    for verify in (False, True):
        rc, n, _ = ctx.compress_method_device(m, pin, offs(blocks), tout.data_ptr(), cap, verify=verify, **kw)
        assert rc == 0 and tout[:n].cpu().numpy().tobytes() == base, (m, verify)
    other = "x0,0ci1" if m != "x0,0ci1" else "x0,3ci1"
    outs = []
    for verify in (False, True):
        rc, n, _ = ctx.compress_mixed_device([m, other], [0, 1, 0], pin, offs(blocks), tout.data_ptr(), cap, verify=verify, **kw)
        assert rc == 0
        outs.append(tout[:n].cpu().numpy().tobytes())
    assert outs[0] == outs[1]
    assert ctx.decompress(outs[1], out_cap=sum(map(len, blocks)) + 64).tobytes() == b"".join(blocks)


@pytest.mark.parametrize("level", ["3,128,0", "3,128,1", "5,128,2"])
def test_same_bytes_levels(ctx, level):
    b = plain_blocks()
    blocks = [b[2][:30000], b[1], b[5][:20000]]
    base = ctx.compress_level(level, blocks)
    assert ctx.compress_level(level, blocks, verify=True) == base
    assert ctx.decompress(base, out_cap=sum(map(len, blocks)) + 64).tobytes() == b"".join(blocks)
    tin, pin = dev(b"".join(blocks), 1)
    cap = len(base) + 4096
    tout = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    for verify in (False, True):
        rc, n, _ = ctx.compress_level_device(level, pin, offs(blocks), tout.data_ptr(), cap, verify=verify)
        assert rc == 0 and tout[:n].cpu().numpy().tobytes() == base, (level, verify)


def test_null_opts_and_clear_bit_launch_what_they_launched(ctx):
    """With the bit clear the call counts the launches it counted before: the pass adds its own only when asked."""
    blocks = _three()
    m = "x0,2,12,0,7,21,1"
    ctx.compress_method(m, blocks)
    plain_launches = ctx.stats().launches
    ctx.compress_method(m, blocks, verify=True)
    verified = ctx.stats().launches
    ctx.compress_method(m, blocks)
    assert ctx.stats().launches == plain_launches and verified >= plain_launches + 3
