"""The catalogue of tests/test_lzsa.py and tests/test_gpu_lzsa.py: the smallest inputs at which LZBuffer's suffix-array
search (tools.methods.lz77_sa) can go wrong.  args[0] = 0 throughout, so the reference's inverse array covers windows of
2^17 positions."""
import functools

import numpy as np

from tools import methods
from zpaqsharp_amd import method, synth

L1, L2 = "x0,1,4,0,7,21,1", "x0,2,12,0,7,21,1c0,0,511i2"
L2E, L1E = "x0,6,5,0,7,211c0,0,511", "x0,5,4,0,3,21,2"
METHODS = (L1, L2, L2E, L1E)


def _rnd(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def text(n=8192, seed=1):
    return synth.plain("T", seed, n).tobytes()


def x86(n=8192, seed=2):
    return synth.plain("X", seed, n).tobytes()


def phrases():
    """A 16-byte phrase 400 times between distinct random fillers: around an early occurrence most neighbours in suffix
    order are later positions, so the bucket runs out on skipped candidates."""
    rng = np.random.default_rng(11)
    out = bytearray()
    for _ in range(400):
        out += b"the same phrase!" + bytes(rng.integers(0, 256, int(rng.integers(5, 20)), dtype=np.uint8))
    return bytes(out)


def offsets(m):
    """Copies of m and m + 1 random bytes at offsets 65 535, 65 536 and 65 537 (level 2 asks one byte more from 2^16 on)."""
    d = bytearray(_rnd(65537 + 700, 13))
    for j, (off, ln) in enumerate((o, l) for o in (65535, 65536, 65537) for l in (m, m + 1)):
        a = 20 + 100 * j
        d[a + off:a + off + ln] = d[a:a + ln]
    return bytes(d)


def window():
    """131 072 + 5 000 bytes with repeats around position 131 071: look-ahead from the last positions of the first window
    reaches into the second, whose inverse array the reference has not built yet."""
    d = bytearray(_rnd(131072 + 5000, 17))
    d[131060:131100] = d[500:540]
    d[131071 - 3:131071 + 30] = d[9000:9033]
    d[131300:131400] = d[131000:131100]
    # "Xabc" at 130 000 and "Yabcdefghijkl" at 130 100; "Xabcdefghijkl" at 131 071, the last position of the first window, where
    # look-ahead 1 would find the 12 bytes behind the 'Y' but is dropped; the same in other letters at 120 000, where it is not
    d[130000:130004], d[130100:130113], d[131071:131084] = b"Xabc", b"Yabcdefghijkl", b"Xabcdefghijkl"
    d[119000:119004], d[119100:119113], d[120000:120013] = b"Wmno", b"Vmnopqrstuvwx", b"Wmnopqrstuvwx"
    return bytes(d)


def small(m):
    """Lengths 0, 1, m - 1, m, m + 1, of one byte value and of text."""
    return [bytes([97]) * n for n in (0, 1, m - 1, m, m + 1)] + [text(m + 1, 5)[:n] for n in (m - 1, m, m + 1)]


def blocks_for(m: str):
    """The blocks a method is checked on."""
    args = method.parse_args(m)[1]
    r = _rnd(5000, 3)
    out = small(args[2]) + [bytes(70000), b"ab" * 2048 + b"a", b"abc" * 1365 + b"ab", r + r[:100], phrases(), text(), x86()]
    if not 4 <= args[1] <= 7:                       # E8E9 changes the bytes, not the search
        out += [offsets(args[2]), window()]
    return out + [b"", b"q", text(777, 7), text(4097, 8), text(20000, 9)]


def knob_methods():
    """args[4] in {0, 1, 3, 7} and args[6] in {0, 1, 2}, levels 1 and 2, for 8 KiB of text."""
    return [f"x0,{lv},{mm},0,{b},21,{la}" for lv, mm in ((1, 4), (2, 5)) for b in (0, 1, 3, 7) for la in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def want(m: str):
    """tools.methods.preprocess(..., sa=True) of blocks_for(m): computed once per process."""
    args = method.parse_args(m)[1]
    return tuple(methods.preprocess(b, args, sa=True) for b in blocks_for(m))
