"""Streams for the framing scan of a device-resident stream (zpaqhip_scan_device): the cases of tests/test_scan_walk.py (the
walk of zh_scan_walk.h on the host, no GPU) and tests/test_gpu_scan_device.py (the kernels).  Every case is a (name, bytes)
pair; what the scan has to say about it is what the host scan says (zh_framing.cpp's scan_stream).  Blocks whose coded data
is written by hand are for the scan alone: they do not decode."""
import functools
import os
import re

from tests import util
from tools import methods
from zpaqsharp_amd import models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAG13 = bytes([0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3])
SHA = bytes(range(1, 21))


def piece() -> int:
    """Bytes per wave of the streaming kernel, as zh_scan_walk.h exports it."""
    src = open(os.path.join(ROOT, "zpaqsharp_amd", "csrc", "zh_scan_walk.h")).read()
    return int(re.search(r"#define\s+ZH_SCAN_PIECE\s+(\d+)u", src).group(1))


def stored(payload: bytes) -> bytes:
    """Encoder.compress without a model: length-prefixed chunks, a zero length at the end."""
    return b"".join(len(payload[i:i + 65536]).to_bytes(4, "big") + payload[i:i + 65536]
                    for i in range(0, len(payload), 65536)) + b"\0\0\0\0"


def raw_block(header: bytes, segs, level: int = 2, tag: bytes = TAG13) -> bytes:
    """A block put together by hand: segs = [(name, comment, coded bytes, sha1 or None)]."""
    out = tag + b"zPQ" + bytes([level, 1]) + header
    for name, comment, data, sha in segs:
        out += b"\x01" + name + b"\0" + comment + b"\0\0" + data + (b"\xfd" + sha if sha else b"\xfe")
    return out + b"\xff"


def _mid():
    return models.get("mid").header


def _store_hdr():
    return methods.model_of("x0,0")[0].header


def modelled(data: bytes, **kw) -> bytes:
    """One hand-written modelled segment: `data` is taken as coded bytes (it must end the way coded data ends)."""
    return raw_block(_mid(), [(kw.get("name", b"n"), kw.get("comment", b"7"), data, kw.get("sha", SHA))], tag=kw.get("tag", TAG13))


def store_block(payload: bytes, **kw) -> bytes:
    """A stored block that decodes to `payload` (selector 0: no post-processing)."""
    import hashlib
    return raw_block(_store_hdr(), [(kw.get("name", b""), kw.get("comment", str(len(payload)).encode()), stored(b"\0" + payload),
                                     hashlib.sha1(payload).digest() if kw.get("sha", True) else None)], tag=kw.get("tag", TAG13))


def golden(name: str) -> bytes:
    return open(os.path.join(GOLDEN, name), "rb").read()


@functools.lru_cache(maxsize=None)
def small_archive() -> bytes:
    return util.block("mid", util.text(300, 9), filename=b"inner")


@functools.lru_cache(maxsize=None)
def framing_cases():
    a, b = util.block("l1", util.text(3000, 1)), util.block("mid", util.text(700, 2))
    s0 = methods.compress_block("x0,0", util.text(900, 3), filename=b"st")
    arch = small_archive()
    cases = [
        ("mixed", b"garbage" + a + s0 + golden("max_text_8k.zpaq") + b"\0\0\0" + golden("mid_empty.zpaq") + store_block(b"") + b + b"tail"),
        ("goldens", b"".join(golden(f) for f in sorted(os.listdir(GOLDEN)) if f.endswith(".zpaq"))),
        ("segments", raw_block(_mid(), [(b"a", b"12", b"\x21\x43\0\0\0\0", SHA), (b"", b"", b"\x05\0\0\0\0\0", None),
                                        (b"third", b"x", b"\x99\x98\0\0\0\0\0\0\0", SHA)])
         + raw_block(_store_hdr(), [(b"s1", b"3", stored(b"\0abc"), None), (b"s2", b"", stored(b"defg"), SHA)]) + b),
        ("empty", b""),
        ("tagless", b"no zpaq here" * 100),
        ("short", b"zP"),
        ("bare_start", store_block(b"first", tag=b"") + a),
        ("bare_only", modelled(b"\x21\x43\0\0\0\0", tag=b"")),
        ("bare_behind_255", a + store_block(b"second", tag=b"") + store_block(b"third", tag=b"") + b),
        ("payload_archive", store_block(arch + arch) + b),
        ("name_archive", modelled(b"\x21\0\0\0\0", name=bytes(x for x in arch if x)) + b),
        ("comment_archive", modelled(b"\x21\0\0\0\0", comment=bytes(x for x in arch if x)) + b),
        ("coded_tag", modelled(b"\x21" + TAG13 + b"zPQ\x02\x01" + b"\x33\0\0\0\0") + b),
        ("tiny_blocks", b"".join(store_block(bytes([65 + i % 26, 48 + i % 10]), name=b"%d" % i) for i in range(1600))),
    ]
    for k in range(1, 16):
        cases.append(("gap_%d" % k, a + b"\x11" * k + b + bytes(range(1, k + 1)) + s0))
    for j in range(1, 13):                              # a tag that lacks its first j bytes: its window straddles the end in front
        cases.append(("straddle_%d" % j, a + store_block(b"x%d" % j, tag=TAG13[j:]) + b))
        cases.append(("straddle_gap_%d" % j, a + b"\x37" + store_block(b"y%d" % j, tag=TAG13[j:]) + b))
    return cases


@functools.lru_cache(maxsize=None)
def zero_run_cases():
    b = util.block("mid", util.text(700, 2))
    cases = []
    for k in range(1, 6):
        cases.append(("lead_%d" % k, modelled(b"\0" * k + b"\x21\x43\x65\0\0\0\0") + b))
    cases += [
        ("lead_long", modelled(b"\0" * 9000 + b"\x21\x43\0\0\0\0\0") + b),
        ("lead_only", modelled(b"\0" * 50)),
        ("run_3", modelled(b"\x21\0\0\0\x43\x65\0\0\0\0") + b),
        ("run_3_3", modelled(b"\x21\0\0\0\x43\0\0\0\x65\0\0\0\0") + b),
        ("run_4", modelled(b"\x21\x43\0\0\0\0") + b),
        ("run_7", modelled(b"\x21\x43" + b"\0" * 7) + b),
        ("run_4_then_zero_marker", modelled(b"\x21\x43\0\0\0\0")[:-22] + b"\0" + b),
        ("stored_zeros", store_block(b"ab\0\0\0\0cd\0\0\0\0\0\0") + b),
        ("run_to_end", modelled(b"\x21\x43\0\0\0\0")[:-22]),
        ("run_to_end_long", b + modelled(b"\x21\x43" + b"\0" * 5000)[:-22]),
        ("no_run", b + modelled(b"\x21\x43\x65\0\0\0\x01")[:-22]),
        ("chunk_past_end", b + store_block(b"0123456789" * 20)[:-60]),
        ("chunk_length_cut", b + raw_block(_store_hdr(), [(b"", b"", b"\0\0", None)])[:-2]),
    ]
    return cases


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """A tag, a run of four zeros and a long run of zeros pushed through every residue 0 .. 19 around one piece boundary."""
    P = piece()
    b = util.block("mid", util.text(300, 4))
    cases = []
    for r in range(20):
        at = 2 * P - 10 + r                             # where the feature starts
        blk = modelled(b"\x21\x43\x65\0\0\0\0")
        cases.append(("tag_%d" % r, b"\x11" * at + blk + b))
        zeros = len(blk) - 22 - 4                       # the four zeros that end the coded data
        cases.append(("run4_%d" % r, b"\x11" * (at - zeros) + blk + b))
        blk = modelled(b"\x21" + b"\0" * (P + 37))
        cases.append(("long_%d" % r, b"\x11" * (at - (len(blk) - 22 - (P + 37))) + blk + b))
        cases.append(("long_end_%d" % r, b"\x11" * r + blk[:-22]))
    return cases


MUTATIONS = [                                           # tests/test_abi_and_framing.py, test_scan_errors_match_the_oracle
    ("level", lambda s: s[:13] + b"zPQ\x03" + s[17:], -11, "unsupported ZPAQ level"),
    ("type", lambda s: s[:13] + b"zPQ\x01\x02" + s[18:], -11, "unsupported ZPAQL type"),
    ("cut", lambda s: s[:40], -2, "unexpected end of file"),
    ("marker", lambda s: s[:-22] + b"\x07" + s[-21:], -15, "missing end of segment marker"),
    ("end", lambda s: s[:-1] + b"\x09", -12, "missing segment or end of block"),
]


@functools.lru_cache(maxsize=None)
def error_cases():
    """(name, stream, code, message, blocks kept, block of the error)"""
    base = util.block("mid", util.text(500))
    good1, good2 = util.block("l1", util.text(3000, 1)), util.block("mid", util.text(500, 3))
    cases = []
    for name, mutate, code, msg in MUTATIONS:
        cases.append(("mut_" + name, mutate(base), code, msg, 0, 0))
        cases.append(("mut_behind_" + name, good1 + good2 + mutate(base), code, msg, 2, 2))
    # test_scan_hands_back_the_blocks_before_framing_damage
    bad = bytearray(util.block("l1", util.text(2000, 2)))
    data_off = len(TAG13) + 5 + len(models.get("l1").header) + 1 + 1 + len(b"2000") + 1 + 1
    bad[data_off - 1] = 7                               # the reserved byte after the comment (Decompresser.cs:107)
    cases.append(("reserved", good1 + bytes(bad) + good2, -14, "missing reserved byte", 1, 1))
    cases.append(("half", good1 + good2[:len(good2) // 2], None, None, 1, 1))
    cases.append(("whole", good1 + good2, 0, None, 2, -1))
    cases.append(("bad_component", raw_block(b"\x0a\x00\x00\x00\x00\x00\x01\x0b\x00\x00\x00\x00", []), -5, "Invalid component type", 0, 0))
    cases.append(("level1_store", raw_block(_store_hdr(), [], level=1), -11, "ZPAQ level 1 requires at least 1 component", 0, 0))
    cases.append(("name_cut", (good1 + modelled(b"\x21\0\0\0\0", name=b"abcdefgh"))[:len(good1) + 16 + 2 + len(_mid()) + 4], -13, "unexpected EOF", 1, 1))
    return cases


def all_scan_cases():
    out = []
    for fam, fn in (("framing", framing_cases), ("zeros", zero_run_cases), ("boundary", boundary_cases)):
        out += [(fam + "/" + n, s) for n, s in fn()]
    out += [("errors/" + c[0], c[1]) for c in error_cases()]
    return out
