"""The catalogue of tests/test_lzht.py and tests/test_gpu_lzht.py: the smallest inputs at which LZBuffer's hash-table search
(tools.methods.lz77_ht) can go wrong.  args[0] = 0 unless a case needs check bits that mask the check byte."""
import functools

import numpy as np

from tests import lzsa_cases
from tools import methods
from zpaqsharp_amd import method

L1 = "x0,1,5,0,3,20"                               # level 1's default
METHODS = (L1, "x0,1,4,0,1,15", "x0,1,6,0,3,20", "x0,2,4,0,3,20", "x0,5,4,0,2,16", "x0,2,12,0,2,8")
# The 2 * (lit > 0) term decides alone where 8 l - lg(offset) - 11 is 1 or 2.  Level 2, minMatch 3: l = 3 at an offset in
# 1024..4095; in[i + 3] is the check byte, so a repeat of exactly 3 bytes passes only where the check bits mask the
# difference: args[0] = 5, 7 check bits, fourth bytes 0x80 apart.  Level 1: l = 4 at an offset in 2^18..2^20.
M_MARGINAL2, M_MARGINAL1 = "x5,2,3,0,3,20", "x0,1,4,0,3,20"

_rnd, text, x86, phrases = lzsa_cases._rnd, lzsa_cases.text, lzsa_cases.x86, lzsa_cases.phrases


def small(m):
    """Lengths 0, 1, m - 1, m, m + 1, m + 4 and m + 5 (nothing is stored up to minMatchBoth = m + 4), of one value and of text."""
    ns = (0, 1, m - 1, m, m + 1, m + 4, m + 5)
    return [bytes([97]) * n for n in ns] + [text(m + 5, 5)[:n] for n in ns[2:]]


def invisible(c):
    """An 8-byte phrase at position 0 whose in[3] is c, again at position 8.  h1 is 0 at position 0, whatever the bytes, so
    only a table small enough to be searched whole (M_INVISIBLE: 8 slots, 8 searched) finds that entry, and no later position
    overwrites slot 0 before position 8 in these bytes.  With c = 0 the word stored for position 0 is 0, an empty slot to the
    reference: the match of 8 at offset 8 is not found; with c = 1 it is."""
    r = bytes(np.random.default_rng(1).integers(2, 256, 30, dtype=np.uint8))
    p = r[:3] + bytes([c]) + r[4:8]
    return p + p + r[8:]


M_INVISIBLE = "x0,1,4,0,3,3"


def tails():
    """A block ending in a repeat of an earlier 16-byte phrase, cut at each of its last 8 lengths: h1 is frozen over the last
    minMatchBoth positions and in[i + 3] must lie inside the block."""
    d = _rnd(50, 29) + b"the same phrase!" + _rnd(30, 31) + b"the same phrase!"
    return [d[:len(d) - t] for t in range(8)]


def marginal2():
    """(block, site behind a match, site behind a literal, offsets) for M_MARGINAL2."""
    r = bytearray(x & 0x7F for x in _rnd(3400, 37))
    r[100:104], r[200:204] = b"\x01\x02\x03\x10", b"\x04\x05\x06\x20"
    r[1600:1616] = r[1500:1516]                    # a match of 16 at offset 100 ends at 1616 ...
    r[1616:1620] = b"\x01\x02\x03\x90"             # ... where 3 bytes repeat at offset 1516 (lg = 11): taken, lit == 0
    r[3000:3004] = b"\x04\x05\x06\xa0"             # 3 bytes at offset 2800 (lg = 12) behind literals: not taken
    return bytes(r), 1616, 3000, (1516, 2800)


def marginal1():
    """(block, site behind a match, site behind a literal, offsets) for M_MARGINAL1: about 260 KB, most of it one value."""
    head, z = bytearray(_rnd(600, 41)), 1 << 18
    head[100:105], head[200:205] = b"WXYZ1", b"PQRS1"
    t = bytearray(_rnd(200, 43))
    t[40:56] = head[300:316]                       # a match of 16 ends at 56 ...
    t[56:61] = b"WXYZ2"                            # ... where 4 bytes repeat at an offset of 2^18 and more: taken
    t[150:155] = b"PQRS2"                          # behind literals: not taken
    a, b = 600 + z + 56, 600 + z + 150
    return bytes(head) + bytes(z) + bytes(t), a, b, (a - 100, b - 200)


def blocks_for(m: str):
    """The blocks a method is checked on."""
    args = method.parse_args(m)[1]
    r = _rnd(5000, 3)
    out = small(args[2]) + [bytes(70000), b"ab" * 2048 + b"a", b"abc" * 1365 + b"ab", r + r[:100], phrases(), text(), x86(),
                            invisible(0), invisible(1)] + tails()
    if args[1] == 2:
        out.append(lzsa_cases.offsets(args[2]))
    if args[1] == 2 and args[2] == 4:
        out.append(lzsa_cases.offsets(12))         # (for minMatch 4 a later position overwrites the slot of one of the copies)
    if m == M_MARGINAL2:
        out.append(marginal2()[0])
    if m == M_MARGINAL1:
        out.append(marginal1()[0])
    return out + [b"", b"q", text(777, 7), text(4097, 8), text(20000, 9)]


def knob_methods():
    """args[4] in {0, 1, 2, 3}, args[5] in {1, 8, 15, 20}, minMatch 4..6 at level 1 and 2, 3, 12, 64, 65 (no search) at level
    2, and 7 check bits."""
    out = [f"x0,{lv},{mm},0,{b},20" for lv, mm in ((1, 4), (2, 5)) for b in (0, 1, 2, 3)]
    out += [f"x0,{lv},{mm},0,{min(3, h)},{h}" for lv, mm in ((1, 4), (2, 5)) for h in (1, 8, 15)]
    out += [f"x0,1,{mm},0,3,20" for mm in (5, 6)] + [f"x0,2,{mm},0,3,20" for mm in (2, 3, 12, 64, 65)]
    return out + ["x5,1,4,0,3,20", M_MARGINAL2, M_INVISIBLE]


@functools.lru_cache(maxsize=None)
def want(m: str):
    """tools.methods.preprocess(..., ht=True) of blocks_for(m): computed once per process."""
    args = method.parse_args(m)[1]
    return tuple(methods.preprocess(b, args, ht=True) for b in blocks_for(m))
