"""Streams for the post-processors `lzpre` and `bwtrle` with E8E9 behind a model (levels 3 and 4 on executables), shared by
tests/test_model_e8.py and tests/test_gpu_model_e8.py."""
import types

import oracle
from tests import store_e8_cases as cases
from tests import util
from tools import methods

LZ3 = "x0,6,12,0,7,21,1c0,0,511i2"                        # level 3: lzpre + E8E9 behind ICM + ISSE over the parse state
LZ4 = "x0,6,5,0,7,21,1c0,0,511"                           # level 4's form for barely compressible data: one ICM
BWT = "x0,7ci1"                                           # BWT + E8E9
E8 = (LZ3, LZ4, BWT)
TWIN = {LZ3: "x0,2,12,0,7,21,1c0,0,511i2", LZ4: "x0,2,5,0,7,21,1c0,0,511", BWT: "x0,3ci1"}   # the same methods without E8E9


def pre_of(method: str, x: bytes) -> bytes:
    """Post-processor input after which the end-of-segment loop runs over exactly x."""
    if method == BWT:
        return methods.bwt_level3(x)
    return cases.literals(methods.model_of(method)[1], x)


def modelled_block(model, seg_pres, sizes=None) -> bytes:
    """A block of a modelled method with one segment per entry of seg_pres (the bytes the post-processor's program is fed in
    that segment), written by the oracle's Compressor; the first segment carries the program.  No checksums."""
    c = oracle.Compressor(2 * sum(len(p) for p in seg_pres) + (1 << 16))
    c.write_tag()
    c.start_block(model.header)
    for i, pre in enumerate(seg_pres):
        c.start_segment(b"", str(sizes[i]).encode() if sizes else b"")
        if i == 0:
            c.post_process(model.pcomp)
        c.compress(pre)
        c.end_segment(None)
    c.end_block()
    return c.getvalue()


def changed_loop(method: str):
    """The method's model with `a== 232` of the loop turned into `a== 233`: the same structure, another program."""
    model, args = methods.model_of(method)
    pc = bytearray(model.pcomp)
    assert pc.count(232) == 1
    pc[pc.index(232)] = 233
    return types.SimpleNamespace(header=model.header, pcomp=bytes(pc)), args


def two_segments(first_len: int):
    """The modelled twin of tests/test_gpu_store_e8.py's _two_segments: |M| = 1 MiB; segment 1 writes first_len bytes with
    patterns in its last 64 and one at d - 5, segment 2 opens with a match of 32 bytes at offset 40 — the tail of M as the
    pass left it — and goes on with literals that hold a pattern.  Returns (stream, plaintext length)."""
    model, args = methods.model_of(LZ3)
    assert 1 << model.header[5] == 1 << 20
    x = bytearray(util.text(first_len, seed=17))
    for p in range(first_len - 64, first_len - 5, 6):
        x[p], x[p + 4] = 0xE8, (0x00, 0xFF)[p & 1]
    x[first_len - 5], x[first_len - 1] = 0xE9, 0xFF
    seg2 = bytearray()
    methods._put_match2(seg2, 32, 40, args[2])
    seg2 += cases.literals(args, bytes([0xE8, 1, 2, 3, 0]) + util.text(300, seed=18))
    return modelled_block(model, [cases.literals(args, bytes(x)), bytes(seg2)], sizes=[first_len, 32 + 305]), first_len + 32 + 305
