"""The catalogue of tests/test_degenerate_cases.py and tests/test_gpu_enc_degenerate.py: degenerate plaintext for the
compression side.  Constant, periodic, few-valued and half-constant blocks: the inputs on which probabilities and counts
saturate, the arithmetic coder emits a handful of bytes, every byte falls into one context window or one hash row, MATCH
sits at its longest length, a method's coded sequence is a few codes long and the gap analysis of levels 5..9 finds periods.

N = 12288 bytes: one ZH_GAP_SLICE (zh_analyze.h), three flushes of the LZ77 writers' 4096 literals, and longer than every
MATCH buffer of tests/chain_cases.py.  Everything is drawn from one generator with seed 77, in the order of cases()."""
import functools
from collections import OrderedDict

import numpy as np

N = 12288
SHORT = 257
SEED = 77
TINY_LENGTHS = (0, 1, 2, 63, 64, 65, 300)

# (method string, parse): the methods both test files run end to end.  parse "" is the greedy search of tools.methods, "ht" /
# "sa" the reference's hash-table / suffix-array search, "bwt" the transform of level 3.
METHODS = [("x0,1,4,0,3,20", ""), ("x0,1,4,0,3,20", "ht"), ("x0,5,4,0,3,20", ""), ("x0,5,4,0,3,20", "ht"),
           ("x0,1,4,0,7,21,1", ""), ("x0,1,4,0,7,21,1", "sa"),
           ("x0,2,5,0,3,20c0,0,511", ""), ("x0,2,5,0,3,20c0,0,511", "ht"),
           ("x0,2,12,0,7,21,1c0,0,511i2", ""), ("x0,2,12,0,7,21,1c0,0,511i2", "sa"),
           ("x0,6,5,0,3,16c0,0,511", ""), ("x0,6,5,0,3,16c0,0,511", "ht"),
           ("x0,3ci1", "bwt"), ("x0,7ci1", "bwt"), ("x0,4ci1,1,1,1,2am", ""), ("x0,0ci1,1,1,1,2awm", "")]


def parse_kw(parse: str) -> dict:
    """The sa= / ht= keywords of tools.methods.preprocess / compress_block and Context.compress_method for a parse."""
    return {"sa": parse == "sa", "ht": parse == "ht"}


@functools.lru_cache(maxsize=None)
def _cases(n: int):
    rng = np.random.default_rng(SEED)
    u8 = np.uint8

    def tile(unit, m=n):
        return np.tile(np.asarray(unit, u8), m // len(unit) + 1)[:m]

    d = OrderedDict()
    d["zeros"] = np.zeros(n, u8)
    d["ff"] = np.full(n, 255, u8)
    d["period2"] = tile([0x41, 0x42])
    d["period3"] = tile([1, 2, 3])
    d["period7"] = tile(rng.integers(0, 256, 7, dtype=u8))
    d["period256"] = tile(np.arange(256, dtype=u8))
    d["runs64"] = np.repeat(rng.integers(0, 256, n // 64 + 1, dtype=u8), 64)[:n]
    d["two_symbols"] = (rng.integers(0, 2, n, dtype=u8) * 0x0f + 0x10).astype(u8)
    d["low_nibbles"] = rng.integers(0, 16, n, dtype=u8)
    d["high_nibbles"] = (rng.integers(0, 16, n, dtype=u8) << 4).astype(u8)
    rep = rng.integers(0, 256, 700, dtype=u8)
    d["long_repeats"] = np.concatenate([np.concatenate([rep, rng.integers(0, 256, 300, dtype=u8)])
                                        for _ in range(n // 1000 + 1)])[:n]
    d["e8_runs"] = tile([0xE8] * 7 + [0])             # every E8 with a 00 four bytes on: the E8E9 candidates chain
    half = rng.integers(0, 256, n - n // 2, dtype=u8)
    d["zeros_then_random"] = np.concatenate([np.zeros(n // 2, u8), half])
    d["random_then_zeros"] = np.concatenate([half, np.zeros(n // 2, u8)])
    out = OrderedDict((k, v.tobytes()) for k, v in d.items())
    assert all(len(v) == n for v in out.values())
    return out


def cases(n: int = N) -> "OrderedDict[str, bytes]":
    """name -> plaintext of `n` bytes, in a fixed order."""
    return OrderedDict(_cases(n))


def short(name: str) -> bytes:
    """The first 257 bytes of a case: a block that ends while the model is still saturating."""
    return _cases(N)[name][:SHORT]


def names():
    return list(_cases(N))


def blocks():
    """Every case at N, then every case's short form."""
    return list(_cases(N).values()) + [short(k) for k in _cases(N)]


def short_blocks():
    """The second half of blocks()."""
    return [short(k) for k in _cases(N)]


# blocks() in two parts for the calls of levels 5..9: there every distinct method string is a launch of its own on a model of
# two dozen components, a second per 12 KiB block whatever the number of blocks, and blocks() has six strings.  Each part has
# four (tests/test_degenerate_cases.py pins that): "a" the first seven cases and every short form, "b" the other seven cases.
LEVEL5_PARTS = {"a": tuple(range(0, 7)) + tuple(range(14, 28)), "b": tuple(range(7, 14))}


def tiny_blocks(nb: int):
    """`nb` blocks for a launch with more blocks than compute units: block i is the prefix of length TINY_LENGTHS[i % 7] of
    case i % 14 (7 and 14 share a factor, so the case moves on by one every 14 blocks: every case gets every length)."""
    c = list(_cases(N).values())
    return [c[(i + i // len(c)) % len(c)][:TINY_LENGTHS[i % len(TINY_LENGTHS)]] for i in range(nb)]


# ---- CPU references: computed once per process, shared by the tests that need them, never changed ------------------------
def each(fn, items):
    """[fn(x) for x in items] on a few host threads (the CPU stream writer runs outside the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(fn, items))


@functools.lru_cache(maxsize=None)
def _pre_of(method: str, sa: bool, ht: bool):
    from tools import methods
    args = methods.parse_args(method)[1]
    return tuple(methods.preprocess(b, args, sa, ht) for b in blocks())


def pre_of(method: str, parse: str = ""):
    """tools.methods.preprocess of every block of blocks() for a method and a parse."""
    return _pre_of(method, parse == "sa", parse == "ht")


@functools.lru_cache(maxsize=None)
def _method_streams(method: str, sa: bool, ht: bool):
    from tools import methods
    return tuple(each(lambda bp: methods.compress_block(method, bp[0], pre=bp[1]), zip(blocks(), _pre_of(method, sa, ht))))


def method_streams(method: str, parse: str = ""):
    """tools.methods.compress_block of every block of blocks() (no file names) for a method and a parse."""
    return _method_streams(method, parse == "sa", parse == "ht")


@functools.lru_cache(maxsize=None)
def model_streams(name: str):
    """synth.compress_block of every block of blocks() for a built-in model (`max+e8e9` codes the E8E9 transform)."""
    from zpaqsharp_amd import synth
    return tuple(each(lambda b: synth.compress_block(name, b), blocks()))


@functools.lru_cache(maxsize=None)
def gap_hists():
    """tests.test_levels.ref_gap_hist of every block of blocks(): shape (28, 4096)."""
    from tests.test_levels import ref_gap_hist
    return np.stack([ref_gap_hist(b) for b in blocks()])


@functools.lru_cache(maxsize=None)
def level_methods(level: str):
    """What method.expand_level gives each block of blocks(), from the restated histogram at levels 5..9."""
    from zpaqsharp_amd import method
    h = gap_hists() if level[0] >= "5" else None
    return tuple(method.expand_level(level, len(b), None if h is None else h[i]) for i, b in enumerate(blocks()))


@functools.lru_cache(maxsize=None)
def level_streams(level: str):
    """tools.methods.compress_block(m_i, b_i) over level_methods(level)."""
    from tools import methods
    return tuple(each(lambda mb: methods.compress_block(mb[0], mb[1]), zip(level_methods(level), blocks())))

