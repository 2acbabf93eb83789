"""The catalogue of tests/test_chain_cases.py and tests/test_gpu_enc_chains.py: component chains for the lane-per-component
encoder (zh_enc_chain.hip), random ones inside the family build_model classes as ZH_FAM_CHAIN (at most 64 components, 4 MIX,
ICM + 2 ISSE <= 64 LDS units, every CM >= 4 size bits) and directed ones at and just past its limits.  Configs are text;
every header is assembled from it (the built-in and method models' too: their text with another `comp` line)."""
import functools
import os
from typing import NamedTuple, Tuple

import numpy as np

from tests import util
from zpaqsharp_amd import method, models, zpaql

LEVEL5 = "x0,0w1i1c256ci1,1,1,1,1,1,2ac0,2,0,255i1c0,3,0,0,255i1c0,4,0,0,0,255i1mm16ts19t0"
M4 = "x0,0ci1,1,1,1,2am"


def hcomp(top: int = 0, pad: int = 0) -> str:
    """An HCOMP that uses H, M and R: H[0..2] orders 1-3 from the rotating buffer M, H[3..4] the byte itself, H[5] a hash
    carried from byte to byte in R0, H[6] a byte counter in R1, H[7] the byte 200 back in M (another one where M is smaller),
    H[8] a hash that accumulates in H; with `top`, H[9..top-1] likewise in a loop (the entries coincide where H is smaller);
    `pad` no-ops before halt."""
    s = ("c++ *c=a b=c a=0 d= 0 hash *d=a b-- d++ hash *d=a b-- d++ hash *d=a d++ a=*c a<<= 8 *d=a d++ a=*c a*= 200 *d=a "
         "d++ a=r 0 a+=*c a*= 40 r=a 0 *d=a d++ a=r 1 a++ r=a 1 a>>= 2 *d=a d++ a=c a-= 200 b=a a=*b hash *d=a d++ a=*c hashd ")
    if top > 9:
        s += f"d= 9 do a=d a*= 37 a+=*c hashd d++ a=d a== {top} until "
    return s + "a=a " * pad + "halt"


def config(hh: int, hm: int, comps, prog: str) -> str:
    return f"comp {hh} {hm} 0 0 {len(comps)}\n" + "\n".join(f"  {i} {c}" for i, c in enumerate(comps)) + f"\nhcomp {prog}\nend"


def resized(cfg: str, hh: int, hm: int) -> str:
    """A config text with other H and M sizes (everything else, its HCOMP included, as it was)."""
    head, _, rest = cfg.strip().partition("\n")
    h = head.split()
    assert h[0] == "comp" and len(h) == 6
    h[1], h[2] = str(hh), str(hm)
    return " ".join(h) + "\n" + rest


def hcomp_len(cfg: str) -> int:
    """ZhModel::hcomp_len of a config: the program and its END byte."""
    return len(zpaql.parse_header(zpaql.assemble(cfg).header)[5])


def _rnd(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def mixed(n: int = 2500, seed: int = 21) -> bytes:
    """Text, x86-like and random bytes: long enough that a MATCH buffer of 2^8..2^10 bytes wraps in each part."""
    a = 9 * n // 20
    b = 6 * n // 20
    return util.text(a, seed) + util.x86ish(b, seed + 1) + _rnd(n - a - b, seed + 2)


# ---- random chains

def random_chain(rng) -> str:
    """One model inside the family: 1..24 components of every type with arbitrary input wiring, H of 2^{0,2,3,9,10} words and
    M of 2^{0,3,12,13} bytes (in LDS or in the arena, each), tables from their smallest size.  A fifth MIX becomes a MIX2."""
    n = int(rng.integers(1, 25))
    hh, hm = int(rng.choice([0, 2, 3, 9, 10])), int(rng.choice([0, 3, 12, 13]))
    comps, nmix = [], 0
    for i in range(n):
        choices = ["cm", "icm", "match", "const"] if i == 0 else ["cm", "icm", "isse", "match", "avg", "mix2", "mix", "sse", "const"]
        t = str(rng.choice(choices))
        j, k = (int(rng.integers(0, i)), int(rng.integers(0, i))) if i else (0, 0)
        if t == "mix" and nmix == 4:
            t = "mix2"
        if t == "cm":
            comps.append(f"cm {int(rng.integers(4, 14))} {int(rng.integers(1, 256))}")
        elif t == "icm":
            comps.append(f"icm {int(rng.integers(0, 12))}")
        elif t == "isse":
            comps.append(f"isse {int(rng.integers(0, 12))} {j}")
        elif t == "match":
            comps.append(f"match {int(rng.integers(2, 12))} {int(rng.integers(8, 13))}")
        elif t == "avg":
            comps.append(f"avg {j} {k} {int(rng.integers(0, 256))}")
        elif t == "mix2":
            comps.append(f"mix2 {int(rng.integers(0, 10))} {j} {k} {int(rng.integers(1, 64))} {int(rng.choice([0, 255, 15]))}")
        elif t == "mix":
            m = int(rng.integers(1, i - j + 1))
            comps.append(f"mix {int(rng.integers(0, 10))} {j} {m} {int(rng.integers(1, 64))} {int(rng.choice([0, 255, 240]))}")
            nmix += 1
        elif t == "sse":
            lim = int(rng.integers(1, 256))
            comps.append(f"sse {int(rng.integers(0, 10))} {j} {int(rng.integers(0, min(255, lim * 4) + 1))} {lim}")
        else:
            comps.append(f"const {int(rng.integers(0, 256))}")
    return config(hh, hm, comps, hcomp(24))


GROUPS, PER_GROUP = 8, 12                          # 96 models; a group is one test id


def seed() -> int:
    return int(os.environ.get("ZPAQ_FUZZ_SEED", "12345"))


@functools.lru_cache(maxsize=None)
def random_group(group: int, base_seed: int) -> Tuple[str, ...]:
    rng = np.random.default_rng([base_seed, group])
    return tuple(random_chain(rng) for _ in range(PER_GROUP))


def random_blocks():
    """The blocks every random model codes in one call: the mixed plaintext, random bytes only, and lengths 0, 1 and 17."""
    return [mixed(), _rnd(1500, 77), b"", b"\xe8", mixed()[1100:1117]]


# ---- directed cases

class Case(NamedTuple):
    cfg: str
    blocks: tuple                                  # plaintexts; the tests add lengths 0, 1 and 17 of the first
    kind: int = 3                                  # stats().kernel_kind with kernel=2: 3 lane-per-component, 1 one-lane generic
    expands: bool = False                          # the coded block overflows its automatic slot


def _n64(hh: int, hm: int, n_avg: int = 28, n_mix: int = 4) -> str:
    """icm 3, 31 isse each on its predecessor (63 LDS units), avgs of neighbouring pairs of the chain (so most levels hold an
    ISSE and an AVG), then mixers: two on one level (30), one over lanes 28.. (two of them also feed the first) with both
    of those among its inputs, and a last one over the mixers alone.  Select masks 255 / 0 / 15 / 255."""
    c = ["icm 3"] + [f"isse {3 + i % 3} {i - 1}" for i in range(1, 32)]
    c += [f"avg {i - 32} {i - 31} {(37 * i) & 255}" for i in range(32, 32 + n_avg)]
    a = len(c)                                     # first mixer
    c += ["mix 8 0 30 24 255", f"mix 0 32 {n_avg} 16 0", f"mix 4 28 {a + 2 - 28} 20 15"]
    c += [f"mix 6 {a} {k + 3} 12 255" for k in range(n_mix - 3)]
    return config(hh, hm, c, hcomp(64))


def _units(n_icm: int, n_isse: int = 30) -> str:
    """n_icm ICMs and 30 ISSEs (n_icm + 60 LDS units), ISSE i on component i - n_icm: several ISSEs on every level; then a
    MIX2, an SSE and an AVG sharing a level, and a mixer."""
    c = [f"icm {i % 3}" for i in range(n_icm)] + [f"isse {i % 4} {i - n_icm}" for i in range(n_icm, n_icm + n_isse)]
    a = len(c)
    c += [f"mix2 3 {a - 1} {a - 2} 30 255", f"sse 2 {a - 1} 8 200", f"avg {a - 1} {a - 3} 100", f"mix 5 0 {a + 3} 24 255"]
    return config(3, 3, c, hcomp(40))


_TINY = ["cm 4 255", "icm 0", "isse 0 1", "mix 0 0 3 24 255"]
_TINY2 = ["cm 5 3", "icm 1", "icm 2", "isse 1 2", "isse 2 3", "cm 4 1", "mix 2 0 6 30 255"]
_MATCH = ["icm 0", "isse 0 0", "match 6 8", "mix 4 0 3 24 255"]
_EXTREMES = ["const 0", "const 255", "icm 2", "sse 0 2 255 255", "sse 3 2 0 1", "mix2 0 0 1 63 255", "mix2 0 3 4 63 255",
             "sse 0 5 0 255", "mix2 2 5 1 1 0", "avg 0 1 0", "avg 1 0 255", "mix 3 0 11 24 255"]
_PLACED = ["match 10 12", "cm 10 255", "icm 4", "isse 6 2", "isse 7 3", "sse 5 4 32 255", "mix 8 0 6 24 255"]


def _directed():
    text, x = util.text(1500, 31), mixed()
    tr = util.text(1200, 32) + _rnd(1300, 33)      # text + random bytes
    d = {}
    d["tiny-tables"] = Case(config(3, 3, _TINY, hcomp()), (tr,))
    d["tiny-tables-2"] = Case(config(3, 3, _TINY2, hcomp()), (tr,))
    for b, lim in ((4, 255), (8, 3)):              # n = 1 with < 9 size bits is the chain family, not the single-CM one
        d[f"cm{b}-alone"] = Case(config(0, 0, [f"cm {b} {lim}"], "a<<= 4 *d=a halt"), (tr,))
    p256, p37 = _rnd(256, 34), _rnd(37, 35)
    wraps = (p256 * 12, p37 * 80, text)            # offset = 0 mod the buffer: no match; length saturates at 255; text
    d["match-wrap"] = Case(config(3, 3, _MATCH, hcomp()), wraps)
    d["match-wrap-2"] = Case(config(3, 3, [c.replace("match 6 8", "match 2 8") for c in _MATCH], hcomp()), wraps)
    d["n64-h0"] = Case(_n64(0, 3), (x,))           # H(i) is H[0] for every lane
    d["n64-h10"] = Case(_n64(10, 13), (x,))
    d["units64"] = Case(_units(4), (x,))
    d["outside-5mix"] = Case(_n64(10, 13, 27, 5), (x[:1500],), kind=1)
    d["outside-65units"] = Case(_units(5), (x[:1500],), kind=1)
    d["outside-n65"] = Case(_n64(10, 13, 29, 4), (x[:1500],), kind=1)
    d["outside-cm3"] = Case(config(3, 3, ["cm 3 255"] + _TINY[1:], hcomp()), (tr[:1500],), kind=1)
    d["sse-mix2-extremes"] = Case(config(3, 3, _EXTREMES, hcomp()), (x,))
    # a last component that gives a 1 the probability 3 / 8192 whatever the others say: a 1 costs 11 bits, so bytes of mostly
    # ones code into ten times their length and the mixed plaintext into five times, past the automatic slot
    # (n + n / 8 + 4096) of the encoders and the usual room of the CPU writers
    ones = bytes(np.bitwise_or.reduce(np.frombuffer(_rnd(12000, 36), np.uint8).reshape(4, 3000)))
    d["const0-last"] = Case(config(3, 3, _EXTREMES + ["const 0"], hcomp()), (ones, x), expands=True)
    for hh in (9, 10):                             # H in LDS iff 2^hh <= 512, M iff 2^hm <= 4096
        for hm in (12, 13):
            d[f"placement-{hh}-{hm}"] = Case(config(hh, hm, _PLACED, hcomp(12)), (x,))
    # a translated HCOMP on the switch that does not know its id: the built-in programs with H and M in the arena, the
    # level-4 method model's with both in LDS; and mid's with larger memories that are still in LDS
    for name, cfg in (("min", models.MIN_CFG), ("mid", models.MID_CFG), ("max", models.MAX_CFG)):
        d[f"placement-native-{name}-10-13"] = Case(resized(cfg, 10, 13), (x,))
    d["placement-native-mid-9-12"] = Case(resized(models.MID_CFG, 9, 12), (x,))
    d["placement-native-m4-9-12"] = Case(resized(method.make_config(M4)[0], 9, 12), (x,))
    # the program window fits the kernel's 2048-byte LDS copy exactly (ZH_CODE_PAD = 160 on either side), and is one over
    base = hcomp_len(config(3, 3, _PLACED, hcomp(12)))
    for name, over in (("long-hcomp-2048", 0), ("long-hcomp-2049", 1)):
        d[name] = Case(config(3, 3, _PLACED, hcomp(12, 2048 - 320 - base + over)), (x[800:1400],))
    return d


DIRECTED = _directed()


def blocks_of(case: Case):
    """The blocks a directed case codes in one call: its plaintexts, then lengths 0, 1 and 17 of the first."""
    first = case.blocks[0]
    return list(case.blocks) + [b"", first[:1], first[40:57]]
