"""zh_store.hip with opts.kernel == KERNEL_STORE_E8: unmodelled `lazy2` / `lzpre` blocks with E8E9 decoded by the parser and
flusher waves, their end-of-segment pass run wave-wide (zh_e8e9_wave.h), against the oracle and the plaintext; with any
other opts.kernel the blocks are handed to zh_generic.hip as before (zpaqhip_stats.launches == 2)."""
import types

import numpy as np
import pytest

import oracle
import zpaqsharp_amd as z
from tests import store_e8_cases as cases
from tests import util
from tools import methods
from zpaqsharp_amd import synth

pytestmark = pytest.mark.gpu

K = z.KERNEL_STORE_E8
LAZY2, LZPRE, LAZY2_RB = "x0,5,4,0,3,16", "x0,6,12,0,7,16", "x5,5,4,0,3,16"
SLICE, ROUND = 64, 4096                                  # zh_e8e9_wave.h (tests/test_store_e8.py reads them from the header)


def _decode(ctx, s: bytes, kernel: int, cap=None, sha: bool = True):
    got = ctx.decompress(s, out_cap=cap, kernel=kernel, verify_sha1=sha).tobytes()
    return got, ctx.stats().launches


@pytest.mark.parametrize("kind", ["X", "T"])
@pytest.mark.parametrize("method", [LAZY2, LZPRE, LAZY2_RB])
def test_e8e9_forms_stay_on_the_store_kernel(ctx, method, kind):
    n = 20000 if method == LAZY2_RB else 65536            # (the rb > 0 form has an M of 32 MiB to clear)
    data = synth.plain(kind, 3, n).tobytes()
    s = methods.compress_block(method, data)
    assert oracle.decompress(s, cap=n + 16) == data
    assert _decode(ctx, s, K) == (data, 1)
    assert _decode(ctx, s, 0) == (data, 2)                 # the default hands the block to the generic kernel, as before


def test_pass_inputs_as_plaintexts_and_as_what_the_codes_write(ctx):
    """The dense, run and chain inputs of the host test: as plaintexts (the pass then undoes the encoder's transform), and
    coded as they are, so that the pass on the GPU runs over exactly the bytes it was built for."""
    inputs = cases.pass_inputs(SLICE, ROUND)
    names = [k for k in inputs if k.startswith(("dense", "run", "chain", "boundary", "tail"))]
    for i, name in enumerate(names):
        x = inputs[name]
        method = (LAZY2, LZPRE)[i & 1]
        args = methods.model_of(method)[1]
        s = methods.compress_block(method, x)
        assert oracle.decompress(s, cap=len(x) + 16) == x, name
        assert _decode(ctx, s, K) == (x, 1), name
        for pre in (methods._write_codes(x, args, methods._matches(x, max(4, args[2]), 1 << 12, 60000)), cases.literals(args, x)):
            want = oracle.decompress(methods.compress_block(method, b"", pre=pre), cap=len(x) + 16)
            assert len(want) == len(x), name
            s = methods.compress_block(method, want, pre=pre)                    # (size comment and SHA-1 of what the program gives)
            assert _decode(ctx, s, K) == (want, 1), name


@pytest.mark.parametrize("method", [LAZY2, LZPRE])
def test_short_plaintexts(ctx, method):
    for n in (0, 1, 4, 5, 6):
        data = bytes([0xE8, 0x10, 0x20, 0x30, 0xFF, 0xE9])[:n]
        s = methods.compress_block(method, data)
        assert oracle.decompress(s, cap=64) == data
        assert _decode(ctx, s, K, cap=64) == (data, 1), n
        assert _decode(ctx, s, 0, cap=64) == (data, 2), n


def _device_block(ctx, stream: bytes, sc, cap: int, kernel: int, in_len=None):
    import torch
    a = np.frombuffer(stream + b"\0" * (-len(stream) % 4 + 4), np.uint8)
    d_in = torch.from_numpy(a.copy()).cuda()
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    rc, res = ctx.decode_blocks_device(d_in.data_ptr(), len(stream) if in_len is None else in_len, sc, d_out.data_ptr(), [0], [cap], ids=[0],
                                       raise_on_error=False, kernel=kernel)
    return rc, res, d_out.cpu().numpy().tobytes(), ctx.stats().launches


@pytest.mark.parametrize("method", [LAZY2, LZPRE])
def test_output_capacity_seven_bytes_short(ctx, method):
    data = synth.plain("X", 5, 9000).tobytes()
    s = methods.compress_block(method, data)
    want = oracle.decompress(s, cap=len(data) + 16)
    sc = z.scan(s)
    cap = len(want) - 7
    rc, res, out, launches = _device_block(ctx, s, sc, cap, K)
    print(rc, res[0].status, res[0].out_len, launches)
    assert res[0].status == -20 and res[0].out_len == len(want) and launches == 1      # ZPAQHIP_E_OUTPUT_FULL, per segment
    assert out[:cap] == want[:cap] and out[cap:] == bytes(64)                    # counted, not written


def _two_segments(first_len: int):
    """x0,6,...: |M| = 1 MiB.  Segment 1 writes first_len bytes with patterns in its last 64; segment 2 begins with a match of
    32 bytes at offset 40 — the tail of M as the pass left it — and goes on with literals that hold a pattern."""
    model, args = methods.model_of(LZPRE)
    assert 1 << model.header[5] == 1 << 20
    x = bytearray(util.text(first_len, seed=17))
    for p in range(first_len - 64, first_len - 5, 6):
        x[p], x[p + 4] = 0xE8, (0x00, 0xFF)[p & 1]
    x[first_len - 5], x[first_len - 1] = 0xE9, 0xFF                               # the last position that can trigger
    seg2 = bytearray()
    methods._put_match2(seg2, 32, 40, args[2])
    seg2 += cases.literals(args, bytes([0xE8, 1, 2, 3, 0]) + util.text(300, seed=18))
    return cases.store_block(model, [cases.literals(args, bytes(x)), bytes(seg2)], sizes=[first_len, 32 + 305]), first_len + 32 + 305


def test_second_segment_reads_what_the_pass_left_in_m(ctx):
    s, n = _two_segments(1 << 20)
    want = oracle.decompress(s, cap=n + 64)
    assert len(want) == n
    assert _decode(ctx, s, K, cap=n, sha=False) == (want, 1)
    assert _decode(ctx, s, 0, cap=n, sha=False) == (want, 2)


def test_a_segment_longer_than_m_is_handed_back(ctx):
    s, n = _two_segments((1 << 20) + 1)
    want = oracle.decompress(s, cap=n + 64)
    assert len(want) == n
    assert _decode(ctx, s, K, cap=n, sha=False) == (want, 2)


@pytest.mark.parametrize("method", [LAZY2, LZPRE])
def test_a_changed_operand_of_the_loop_is_handed_back(ctx, method):
    model, args = methods.model_of(method)
    pc = bytearray(model.pcomp)
    assert pc.count(232) == 1
    pc[pc.index(232)] = 233                                                      # a== 232 -> a== 233: same structure, another program
    data = synth.plain("X", 7, 12000).tobytes()
    other = types.SimpleNamespace(header=model.header, pcomp=bytes(pc))
    s = cases.store_block(other, [methods.preprocess(data, args)], sizes=[len(data)])
    want = oracle.decompress(s, cap=len(data) + 16)
    assert len(want) == len(data) and want != data
    assert _decode(ctx, s, K, cap=len(data), sha=False) == (want, 2)


def test_a_chunk_that_ends_inside_the_stream_is_handed_back(ctx):
    """The stream ends in the middle of a stored chunk (the framing scan refuses such a stream, so the segment table is cut by
    hand): the store kernel hands the block back, and the generic kernel gives what it gives with opts.kernel == 1 and what
    the oracle's Decompresser delivers (Decoder.get returns -1: the program takes it for the end of the segment)."""
    data = synth.plain("X", 8, 30000).tobytes()
    s = methods.compress_block(LAZY2, data)
    sc = z.scan(s)
    cut = int(sc.segments[0].data_off) + int(sc.segments[0].data_len) // 2
    sc.segments[0].data_len = cut - int(sc.segments[0].data_off)
    d = oracle.Decompresser(s[:cut])
    assert d.find_block() is not None and d.find_filename() is not None
    d.read_comment()
    try:
        want, werr = d.decompress(-1, cap=len(data) + 64)[0], None
    except oracle.OracleError as e:
        want, werr = None, str(e)
    rc1, res1, out1, _ = _device_block(ctx, s[:cut], sc, len(data), 1)
    rc, res, out, launches = _device_block(ctx, s[:cut], sc, len(data), K)
    print(rc, res[0].status, res[0].out_len, launches, werr, None if want is None else len(want))
    assert launches == 2
    assert (rc, res[0].status, res[0].out_len, out) == (rc1, res1[0].status, res1[0].out_len, out1)
    if werr is None:
        assert res[0].status == 0 and out[:int(res[0].out_len)] == want
    else:
        assert z.strerror(res[0].status) == werr


def test_bwtrle_with_e8e9_is_still_handed_back(ctx):
    d = util.text(30000, seed=5)
    s = methods.compress_block("x0,7", d)
    assert _decode(ctx, s, K) == (d, 2)


def test_300_blocks_of_plain_and_e8e9_forms_in_one_launch(ctx):
    forms = ["x0,1,4,0,3,16", LAZY2, "x0,2,12,0,7,16", LZPRE]
    parts, plain = [], []
    for i in range(300):
        d = synth.plain("XT"[(i >> 2) & 1], i, 1500 + 37 * i).tobytes()
        parts.append(methods.compress_block(forms[i & 3], d))
        plain.append(d)
    s = b"".join(parts)
    got, launches = _decode(ctx, s, K)
    assert launches == 1
    at = 0
    for i, d in enumerate(plain):
        assert got[at:at + len(d)] == d, i
        at += len(d)
    assert at == len(got)
    assert _decode(ctx, s, 0) == (b"".join(plain), 2)
