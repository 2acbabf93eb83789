"""The catalogue of the verify pass's edge cases, shared by tests/test_verify_cases.py (CPU: the catalogue is what it says) and
tests/test_gpu_verify_edges.py (GPU: zpaqhip_verify_blocks[_device] and bit 5 of zpaqhip_compress_opts.flags return it).

Every case is a triple (pre, post, orig): the pre-processed bytes of a block, what the block's post-processor makes of them,
and the plaintext the pass compares that with.  `pre` comes from the CPU reference (tools.methods.preprocess; for the caller's
own program SUB1, the +1 map), `post` from the oracle's post-processor on those very bytes (oracle.run_pcomp; for a block
without a program, the oracle's decoder on a stored block that holds them), and nothing from the code under test.  All streams
are valid: the cases change the plaintext side (a flipped, shortened or lengthened `orig`), or a literal byte of valid codes.

    positions         store form, blocks of POS_N bytes on a chosen 16-byte phase of the plaintext: one flipped byte at the
                      first and last position and on both sides of a 16-byte group and of a 4 KiB round of the compare
                      kernel; two flips in one block
    clean neighbours  blocks of every length 0 .. 33 back to back: every phase, every group shared with a neighbour
    lengths           every form, `orig` cut short (the post-processor writes more than its room: the second round) or extended
    long output       an lzpre and a lazy2 feed that write more than 4 * len + 4096 bytes (the room without a plaintext)
    tampering         the first / last literal byte of lazy2 and lzpre codes, any byte of a stored block
    batches           seven small lzpre blocks, the last two tampered

Long output: tests/lzcodes.py's catalogue already holds such feeds for both formats (lazy2: `len-65536-dist-*`, 309 bytes that
write 65 837, and the fillers of `ring-dist-*`, `far-dist-*`, `straddle-M`; lzpre: `ring-dist-*`, `far-dist-*`, `straddle-M`,
5 548 bytes that write 132 243), so tests/test_gpu_verify.py::test_crafted_codes has run the second round without a plaintext
before; tests/test_verify_cases.py::test_lzcodes_catalogue_holds_long_output_feeds pins that.  The two feeds here are the
plainest ones: a literal and longest-length matches at distance 1."""
from __future__ import annotations

import hashlib
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import oracle
from tests import lzcodes
from tools import methods
from zpaqsharp_amd import synth, zpaql

NONE = 2**64 - 1
E_VERIFY = -28


def first_diff(a: bytes, b: bytes) -> int:
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return int(d[0]) if d.size else (NONE if len(a) == len(b) else n)


def expected(post: bytes, orig: Optional[bytes]) -> dict:
    """The record verify returns for a block whose post-processor wrote `post`, compared with `orig` (None: not compared)."""
    differs = orig is not None and post != orig
    return {"status": E_VERIFY if differs else 0, "out_len": len(post), "first_diff": first_diff(post, orig) if differs else NONE,
            "sha1": hashlib.sha1(post).digest()}


class Case(NamedTuple):
    name: str
    pre: bytes
    post: bytes
    orig: Optional[bytes]

    @property
    def want(self) -> dict:
        return expected(self.post, self.orig)


# ---------------------------------------------------------------------------------------------------------------------
# post-processor forms
# ---------------------------------------------------------------------------------------------------------------------
SUB1 = "comp 0 0 0 0 0 hcomp halt pcomp sub1 ; a> 255 if halt endif a-- out halt end"
BIG_WAVE, BIG_LANE = 140000, 20000          # more than the 128 KiB ring / what one lane still does in a second


class Form:
    """A post-processor: `method` (None for SUB1), the model verify takes, whether zh_verify_lz.hip takes it wave-wide."""

    def __init__(self, name: str, method: Optional[str], wave: bool, kind: str):
        self.name, self.method, self.wave, self.kind = name, method, wave, kind
        if method is None:
            self.model, self.args = zpaql.assemble(SUB1), None
        else:
            self.model, self.args = methods.model_of(method)
        self.sizes = [0, 1, 300, 5000, BIG_WAVE if wave else BIG_LANE]
        self._plain: Dict[int, Tuple[bytes, bytes, bytes]] = {}

    def pre(self, plain: bytes) -> bytes:
        if self.method is None:
            return ((np.frombuffer(plain, np.uint8).astype(np.uint16) + 1) & 255).astype(np.uint8).tobytes()
        return methods.preprocess(plain, self.args)

    def post(self, pre: bytes, cap: Optional[int] = None) -> bytes:
        cap = cap if cap is not None else 4 * len(pre) + 8192
        if not self.model.pcomp:            # no program: the oracle's decoder on a stored block without a program that holds `pre`
            return oracle.decompress(methods.compress_block("x0,0", pre, pre=pre), cap=cap)
        h = self.model.header
        return oracle.run_pcomp(self.model.pcomp, pre, h[4], h[5], cap=cap)

    def block(self, n: int, seed: int = 0) -> Tuple[bytes, bytes, bytes]:
        """(plain, pre, post) of this form's block of n bytes: computed once, shared, never changed."""
        key = (n, seed)
        if key not in self._plain:
            plain = synth.plain(self.kind, 900 + 16 * seed + len(self.name), n).tobytes()
            pre = self.pre(plain)
            self._plain[key] = (plain, pre, self.post(pre, cap=n + 4096))
        return self._plain[key]


# the method strings are the keys of tests/test_gpu_verify.py's ROUTES
FORMS: Dict[str, Form] = {f.name: f for f in [
    Form("store", "x0,0ci1", True, "T"),
    Form("e8e9", "x0,4ci1,1,1,1,2am", False, "X"),
    Form("lazy2", "x0,1,4,0,3,20", True, "T"),
    Form("lazy2+e8e9", "x0,5,4,0,3,20", True, "X"),
    Form("lzpre", "x0,2,12,0,7,21,1", True, "T"),
    Form("lzpre+e8e9", "x0,6,12,0,7,21,1", True, "X"),
    Form("bwtrle", "x0,3ci1", True, "T"),
    Form("bwtrle+e8e9", "x0,7ci1", False, "X"),
    Form("sub1", None, False, "T"),
]}


def _flip(data: bytes, *at: int) -> bytes:
    b = bytearray(data)
    for p in at:
        b[p] ^= 0x41
    return bytes(b)


def _pattern(n: int, seed: int) -> bytes:
    """n bytes, none of them zero (device memory the pass did not write is not likely to hold them)."""
    return ((np.arange(n, dtype=np.int64) * (2 * seed + 7) + seed) % 255 + 1).astype(np.uint8).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# positions (store form)
# ---------------------------------------------------------------------------------------------------------------------
POS_N = 3 * 4096 + 37
POS_PAD = -POS_N % 16                        # a filler block of this length keeps the next block on the same phase
DEVICE_POSITIONS = ("first", "round", "last")


def flip_positions(ph: int) -> List[int]:
    """Where one byte of a POS_N-byte block on plaintext phase `ph` is flipped: the ends, and both sides of the first 16-byte
    group's and the first two 4 KiB rounds' boundaries (group g holds the positions 16 g - ph .. 16 g + 15 - ph)."""
    n = POS_N
    out = []
    for p in (0, 1, 15 - ph, 16 - ph, 4095 - ph, 4096 - ph, 4097 - ph, 8192 - ph, n - 2, n - 1):
        if p >= 0 and p not in out:
            out.append(p)
    return out


def flip_pairs(ph: int) -> List[Tuple[int, int]]:
    """Two flips in one block, the earlier first: in one 16-byte group; in a late lane of round 0 and an early lane of round 1;
    the first byte and the last."""
    return [(35 - ph, 41 - ph), (4095 - ph, 4098 - ph), (0, POS_N - 1)]


def device_positions(ph: int) -> List[int]:
    return [0, 4096 - ph, POS_N - 1]


def _store_case(name: str, plain: bytes, orig: bytes) -> Case:
    f = FORMS["store"]
    pre = f.pre(plain)
    return Case(name, pre, f.post(pre, cap=len(pre) + 64), orig)


def position_cases(ph: int, lead: bool = True, flips=None) -> List[Case]:
    """Blocks for one call, back to back: with `lead` a filler of `ph` bytes (it sets the phase where the plaintext starts on a
    16-byte boundary), then one block per flip case and a clean one, a filler of POS_PAD bytes behind each, so that every
    POS_N-byte block lies on phase `ph`.  `flips`: tuples of positions (default: flip_positions and flip_pairs)."""
    if flips is None:
        flips = [(p,) for p in flip_positions(ph)] + flip_pairs(ph)
    cases = []
    if lead and ph:
        fill = _pattern(ph, 90)
        cases.append(_store_case(f"lead-{ph}", fill, fill))
    for k, at in enumerate(list(flips) + [()]):
        plain = synth.plain("T", 700 + k, POS_N).tobytes()
        cases.append(_store_case("flip-" + "-".join(map(str, at)) if at else "clean", plain, _flip(plain, *at)))
        if POS_PAD:
            fill = _pattern(POS_PAD, k)
            cases.append(_store_case(f"pad-{k}", fill, fill))
    return cases


def phase_of(cases: List[Case], i: int, start: int = 0) -> int:
    """The 16-byte phase of block i's plaintext when the cases' plaintexts lie back to back from an address with phase `start`."""
    return (start + sum(len(c.orig) for c in cases[:i])) & 15


# ---------------------------------------------------------------------------------------------------------------------
# clean neighbours (store form)
# ---------------------------------------------------------------------------------------------------------------------
def neighbour_cases(flipped: bool) -> List[Case]:
    """Blocks of 0 .. 33 bytes; `flipped`: the last byte of every odd-numbered block differs."""
    out = []
    for n in range(34):
        plain = _pattern(n, n)
        out.append(_store_case(f"len-{n}", plain, _flip(plain, n - 1) if flipped and n & 1 else plain))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# lengths (every form)
# ---------------------------------------------------------------------------------------------------------------------
def length_cases(form: Form) -> Tuple[List[Case], List[Case]]:
    """(cut, extended): for each of the form's sizes n, `orig` cut to 0, 1, n // 2 and n - 1 bytes, and extended by 1 and by
    5 000 bytes.  Size 0 extended by 1 is the pre-processed empty block against a 1-byte plaintext; size 0 itself, empty against
    empty, is the one clean case (among the extended ones)."""
    cut, ext = [], []
    for n in form.sizes:
        plain, pre, post = form.block(n)
        for k in sorted({k for k in (0, 1, n // 2, n - 1) if 0 <= k < n}):
            cut.append(Case(f"{form.name}-{n}-cut-{k}", pre, post, plain[:k]))
        if n == 0:
            ext.append(Case(f"{form.name}-0-clean", pre, post, plain))
        for k in (1, 5000):
            ext.append(Case(f"{form.name}-{n}-plus-{k}", pre, post, plain + _pattern(k, 3)))
    return cut, ext


def true_cases(cases: List[Case]) -> List[Case]:
    """The same blocks with the plaintext their pre-processed bytes stand for."""
    return [Case(c.name + "-true", c.pre, c.post, c.post) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# long output without a plaintext
# ---------------------------------------------------------------------------------------------------------------------
def long_output_cases() -> List[Case]:
    """A literal and longest-length matches at distance 1: lzpre 200 codes of 75 bytes (602 bytes in, 15 001 out), lazy2 two
    codes of 65 536 (more than the ring)."""
    out = []
    for name, count in (("lzpre", 200), ("lazy2", 2)):
        form = FORMS[name]
        info = lzcodes.Info(form.method)
        feed = lzcodes.feed_of(info, [("lit", b"q")] + [("match", info.max_len, 1)] * count)
        out.append(Case(f"{name}-long", feed, form.post(feed, cap=1 + count * info.max_len + 4096), None))
    return out


def room_without_plaintext(form: Form, pre: bytes) -> int:
    """What verify_pass gives a block without a plaintext: four times its input, the selector and the program included, plus
    4 KiB (not less than the issue's 4 * len + 4096)."""
    pc = form.model.pcomp or b""
    return 4 * (len(pre) + (3 + len(pc) if pc else 1)) + 4096


# ---------------------------------------------------------------------------------------------------------------------
# tampering with literal bytes
# ---------------------------------------------------------------------------------------------------------------------
def lzpre_literals(feed: bytes) -> List[int]:
    """Byte index of every literal byte in lzpre codes."""
    out, i = [], 0
    while i < len(feed):
        c = feed[i]
        if c < 64:
            out += range(i + 1, i + 2 + c)
            i += 2 + c
        else:
            i += 2 + (c >> 6)
    return out


def lazy2_literals(feed: bytes, rb: int) -> List[int]:
    """Bit position of every literal byte in lazy2 codes (least significant bit first; a literal need not start on a byte)."""
    total, pos, out = 8 * len(feed), 0, []
    v = int.from_bytes(feed, "little")

    def take(k):
        nonlocal pos
        if pos + k > total:
            raise EOFError
        x = (v >> pos) & ((1 << k) - 1)
        pos += k
        return x

    try:
        while (pos + 7) // 8 < len(feed):
            t, ln = take(2), 1
            if t == 0:
                while take(1):
                    ln = ln * 2 + take(1)
                out += range(pos, pos + 8 * ln, 8)
                take(8 * ln)
            else:
                m = 8 * (t - 1) + take(3)
                while take(1):
                    ln = ln * 2 + take(1)
                take(2 + rb + m)
    except EOFError:
        pass
    return out


def _flip_bit(data: bytes, bit: int) -> bytes:
    b = bytearray(data)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


TAMPER_N = 6000


def tamper_cases() -> List[Case]:
    """The lowest bit of the first and of the last literal byte of a 6 000-byte block's codes flipped (the codes stay valid: the
    same literals and matches, one other value), for lazy2 and lzpre with and without E8E9; one byte of a stored block."""
    out = []
    for name in ("lazy2", "lazy2+e8e9", "lzpre", "lzpre+e8e9"):
        form = FORMS[name]
        plain, pre, _ = form.block(TAMPER_N, seed=1)
        if name.startswith("lazy2"):
            bits = lazy2_literals(pre, lzcodes.Info(form.method).rb)
        else:
            bits = [8 * i for i in lzpre_literals(pre)]
        for which, bit in (("first", bits[0]), ("last", bits[-1])):
            bad = _flip_bit(pre, bit)
            out.append(Case(f"{name}-{which}-literal", bad, form.post(bad, cap=4 * TAMPER_N + 4096), plain))
    form = FORMS["store"]
    plain, pre, _ = form.block(TAMPER_N, seed=1)
    bad = _flip_bit(pre, 8 * (TAMPER_N // 3))
    out.append(Case("store-byte", bad, form.post(bad, cap=TAMPER_N + 64), plain))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------
BATCH_METHOD = "x0,2,12,0,7,21,1c0,0,511"
BATCH_BAD = (5, 6)


def batch_case() -> Tuple[List[bytes], List[bytes], List[bytes]]:
    """(blocks, pre, tampered): seven small blocks for the modelled lzpre method; `tampered` is `pre` with the first literal of
    blocks 5 and 6 changed."""
    args = methods.model_of(BATCH_METHOD)[1]
    blocks = [synth.plain("T", 800 + i, 700 + 17 * i).tobytes() for i in range(7)]
    pre = [methods.preprocess(b, args) for b in blocks]
    tampered = [_flip_bit(p, 8 * lzpre_literals(p)[0]) if i in BATCH_BAD else p for i, p in enumerate(pre)]
    return blocks, pre, tampered
