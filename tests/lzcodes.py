"""LZ77 code streams written token by token, an independent model of what they expand to, and the catalogue of
distance / length edges that tests/test_lz_edges.py (CPU) and tests/test_gpu_lz_edges.py (GPU) share.

The writers take a list of ("lit", bytes) and ("match", length, distance[, width]) tokens and write the distance
field VERBATIM: values no encoder produces (a distance of 0, of |M| and beyond, from before the segment) are the point.

    lzpre  (LZBuffer.cs:109-112, 406-418, 449-485) byte-aligned:
           00llllll                  l + 1 literals follow
           01llllll oo oo            match of l + minlen, offset (= distance - 1) big-endian in 2 bytes
           10llllll oo oo oo         ... in 3 bytes
           11llllll oo oo oo oo      ... in 4 bytes (no encoder writes it; the post-processor reads it)
    lazy2  (LZBuffer.cs:96-107, 387-446) bit-packed, least significant bit first:
           00 <n: interleaved Elias gamma, 1b 1b .. 0> n literal bytes
           mm mmm <n: 1b 1b .. 0 bb> [rb low offset bits] <m offset bits below the implied top one>,  m = 8 (mm - 1) + mmm

The expander is written from that description, not from the post-processor programs: M is an array of 2^pm cells
addressed modulo its size, a match copies one cell at a time (cell ptr + i takes cell ptr + i - distance), every
segment starts again at ptr = 0 with M as the last one left it, and the E8E9 forms write nothing until the segment
ends and then undo the E8E9 transform over the ptr cells in M."""
from __future__ import annotations

import os
import re
from typing import List, Sequence, Tuple

import numpy as np

from tools import methods

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# unmodelled blocks: zh_store.hip; a model in front: zh_nibble.hip's drain; E8E9 forms: translated code / the generic kernel
STORE_METHODS = ["x0,1,4,0,3,16", "x6,1,4,0,3,24", "x0,2,12,0,7,16", "x0,2,3,0,7,16"]
DRAIN_METHODS = ["x0,2,12,0,7,21,1c0,0,511i2", "x0,2,5,0,7,21,1c0,0,511"]
E8_METHODS = ["x0,5,4,0,3,16", "x0,6,5,0,3,16c0,0,511", "x4,6,12,0,7,25,1c0,0,511i2"]
METHODS = STORE_METHODS + DRAIN_METHODS + E8_METHODS
SWEEP_SEED = 20261017
SWEEP_STREAMS = 200
SWEEP_MAX_OUT = 20000


def store_kernel_constants() -> Tuple[int, int]:
    """(kPiece, kRing) as zh_store.hip states them."""
    with open(os.path.join(ROOT, "zpaqsharp_amd", "csrc", "zh_store.hip")) as f:
        src = f.read()
    ring = re.search(r"constexpr uint32_t kRing = (\d+)u << (\d+)", src)
    piece = re.search(r"constexpr uint32_t kPiece = (\d+)u;", src)
    return int(piece.group(1)), int(ring.group(1)) << int(ring.group(2))


class Info:
    """What a method string says about its LZ77 format."""

    def __init__(self, method: str):
        model, args = methods.model_of(method)
        self.method, self.model, self.args = method, model, args
        self.lazy = (args[1] & 3) == 1
        self.e8 = 4 <= args[1] <= 7
        self.rb = args[0] - 4 if args[0] > 4 else 0
        self.minlen = 4 if self.lazy else args[2]
        self.pm = args[0] + 20
        self.msize = 1 << self.pm
        self.modelled = model.n > 0
        # the largest distance / length one code holds
        self.max_dist = (1 << (24 + self.rb)) - (1 << self.rb) if self.lazy else 1 << 32      # lazy2: 23 offset bits under the top one
        self.max_len = (1 << 16) if self.lazy else self.minlen + 63          # lazy2: what LZBuffer writes at most


# ---------------------------------------------------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------------------------------------------------
def lzpre_feed(tokens: Sequence[tuple], minlen: int) -> bytes:
    """lzpre codes.  A match token may name the width of its offset field (2, 3 or 4 bytes) as fourth element; without one
    it gets the narrowest that holds the offset, as the encoder chooses.  Distance 0 is the offset FF FF FF FF."""
    out = bytearray()
    for t in tokens:
        if t[0] == "lit":
            d = t[1]
            for a in range(0, len(d), 64):
                out.append(len(d[a:a + 64]) - 1)
                out += d[a:a + 64]
        else:
            ln, off = t[1], (t[2] - 1) & 0xFFFFFFFF
            width = t[3] if len(t) > 3 else 2 if off < 1 << 16 else 3 if off < 1 << 24 else 4
            assert off < 1 << (8 * width)
            while ln > 0:                                                  # LZBuffer.cs:449-485: lengths over minlen + 63 in several codes
                len1 = minlen + 63 if ln > minlen * 2 + 63 else ln - minlen if ln > minlen + 63 else ln
                assert minlen <= len1 < minlen + 64, (ln, minlen)
                out.append(((width - 1) << 6) + len1 - minlen)
                out += off.to_bytes(width, "big")
                ln -= len1
    return bytes(out)


class _Bits:
    def __init__(self):
        self.out, self.v, self.k, self.n = bytearray(), 0, 0, 0           # whole bytes, the bits behind them, how many; bits in all

    def put(self, x: int, k: int):
        self.v |= (x & ((1 << k) - 1)) << self.k
        self.k += k
        self.n += k
        if self.k >= 8:
            self.out += (self.v & ((1 << (self.k & ~7)) - 1)).to_bytes(self.k >> 3, "little")
            self.v >>= self.k & ~7
            self.k &= 7

    def bytes(self) -> bytes:
        return bytes(self.out) + (bytes([self.v]) if self.k else b"")


def _gamma_pairs(w: _Bits, x: int, below: int):
    """The bits of x under its top one down to (not including) the lowest `below`, each behind a 1."""
    for k in range(x.bit_length() - 2, below - 1, -1):
        w.put(1, 1)
        w.put((x >> k) & 1, 1)


def lazy2_feed(tokens: Sequence[tuple], rb: int, spans: list = None) -> bytes:
    """lazy2 codes.  `spans` collects (token index, length field's first bit, offset field's first bit, end) of the matches."""
    w = _Bits()
    for i, t in enumerate(tokens):
        if t[0] == "lit":
            d = t[1]
            assert len(d) >= 1
            w.put(0, 2)
            _gamma_pairs(w, len(d), 0)
            w.put(0, 1)
            w.put(int.from_bytes(d, "little"), 8 * len(d))
        else:
            ln, dist = t[1], t[2]
            assert ln >= 4 and dist >= 1
            off = dist + (1 << rb) - 1
            m = off.bit_length() - 1 - rb
            assert 0 <= m <= 23, dist
            w.put((m + 8) >> 3, 2)
            w.put(m & 7, 3)
            p_len = w.n
            _gamma_pairs(w, ln, 2)
            w.put(0, 1)
            w.put(ln & 3, 2)
            p_off = w.n
            w.put(off, rb)
            w.put(off >> rb, m)
            if spans is not None:
                spans.append((i, p_len, p_off, w.n))
    return w.bytes()


def feed_of(info: Info, tokens: Sequence[tuple]) -> bytes:
    return lazy2_feed(tokens, info.rb) if info.lazy else lzpre_feed(tokens, info.minlen)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
class Expander:
    """What a post-processor makes of the feeds of a block's segments, one after the other."""

    def __init__(self, info: Info):
        self.i = info
        self.M = bytearray(info.msize)
        self.mask = info.msize - 1

    def _copy(self, out: bytearray, ptr: int, n: int, dist: int) -> int:
        M, mask = self.M, self.mask
        src, dst, d = (ptr - dist) & mask, ptr & mask, dist & mask
        if n <= d <= self.i.msize - n and src + n <= self.i.msize and dst + n <= self.i.msize:
            M[dst:dst + n] = M[src:src + n]          # no cell is read and written: the same as the loop below, all at once
        else:
            for k in range(n):
                M[(dst + k) & mask] = M[(src + k) & mask]
        if not self.i.e8:
            if dst + n <= self.i.msize:
                out += M[dst:dst + n]
            else:
                out += M[dst:] + M[:(dst + n) & mask]
        return (ptr + n) & 0xFFFFFFFF

    def _lits(self, out: bytearray, ptr: int, d: bytes) -> int:
        for c in d:
            self.M[ptr & self.mask] = c
            ptr = (ptr + 1) & 0xFFFFFFFF
        if not self.i.e8:
            out += d
        return ptr

    def segment(self, feed: bytes) -> bytes:
        out = bytearray()
        ptr = self._lazy2(out, feed) if self.i.lazy else self._lzpre(out, feed)
        if self.i.e8:
            self._e8e9_out(out, ptr)
        return bytes(out)

    def _lzpre(self, out: bytearray, feed: bytes) -> int:
        ptr, p, n = 0, 0, len(feed)
        while p < n:
            x = feed[p]
            p += 1
            if x < 64:
                ptr = self._lits(out, ptr, feed[p:p + x + 1])          # (a run the feed cuts short: what there is of it)
                p += x + 1
            else:
                width = (x >> 6) + 1
                if p + width > n:
                    break
                off = int.from_bytes(feed[p:p + width], "big")
                p += width
                ptr = self._copy(out, ptr, (x & 63) + self.i.minlen, (off + 1) & 0xFFFFFFFF)
        return ptr

    def _lazy2(self, out: bytearray, feed: bytes) -> int:
        total, rb = 8 * len(feed), self.i.rb
        ptr, pos = 0, 0

        def take(k):                                            # k <= 24 bits, least significant first
            nonlocal pos
            if pos + k > total:
                raise EOFError
            x = (int.from_bytes(feed[pos >> 3:(pos >> 3) + 5], "little") >> (pos & 7)) & ((1 << k) - 1)
            pos += k
            return x

        def take_bytes(n):                                      # as many of n whole bytes as the feed still holds
            nonlocal pos
            n = min(n, (total - pos) >> 3)
            x = int.from_bytes(feed[pos >> 3:(pos >> 3) + n + 1], "little") >> (pos & 7)
            pos += 8 * n
            return (x & ((1 << (8 * n)) - 1)).to_bytes(n, "little")

        try:
            while (pos + 7) // 8 < len(feed):                  # a code starts with the arrival of a byte
                t = take(2)
                ln = 1
                if t == 0:
                    while take(1):
                        ln = ln * 2 + take(1)
                    got = take_bytes(ln)
                    ptr = self._lits(out, ptr, got)
                    if len(got) < ln:
                        raise EOFError
                else:
                    m = 8 * (t - 1) + take(3)
                    while take(1):
                        ln = ln * 2 + take(1)
                    ln = ln * 4 + take(2)
                    low = take(rb)
                    dist = (1 << m) + take(m)
                    if rb:
                        dist = ((dist << rb) + low - ((1 << rb) - 1)) & 0xFFFFFFFF
                    ptr = self._copy(out, ptr, ln, dist)
        except EOFError:
            pass
        return ptr

    def _e8e9_out(self, out: bytearray, d: int):
        """The E8E9 transform undone over cells 0 .. d-1 of M, front to back, in place; every cell written out as it is passed."""
        M, mask, size = self.M, self.mask, self.i.msize
        pat = re.compile(rb"[\xe8\xe9]")
        b = 0
        while b < d:
            if b < size:                                        # nothing happens before the next E8 / E9: skip to it
                lim = min(d, size)
                hit = pat.search(M, b, lim)
                j = hit.start() if hit else lim
                out += M[b:j]
                b = j
                if b >= d or (b >= size):
                    continue
            if b + 4 < d and (M[b & mask] & 254) == 232 and ((M[(b + 4) & mask] + 1) & 254) == 0:
                a = M[(b + 1) & mask] | M[(b + 2) & mask] << 8 | M[(b + 3) & mask] << 16
                a = (a - b) & 0xFFFFFF
                M[(b + 1) & mask], M[(b + 2) & mask], M[(b + 3) & mask] = a & 255, (a >> 8) & 255, a >> 16
            out.append(M[b & mask])
            b += 1


def expand(info: Info, feeds: Sequence[bytes]) -> bytes:
    e = Expander(info)
    return b"".join(e.segment(f) for f in feeds)


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------
DISTANCES = [1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def _bytes(n: int, seed: int = 1, e8: bool = True) -> bytes:
    """n varied bytes; e8 = False: none of them E8 / E9 (the long fillers: nothing for the E8E9 forms to do)."""
    a = (np.arange(n, dtype=np.int64) * (37 + 2 * seed) + (np.arange(n, dtype=np.int64) >> 8) * 11 + seed) % (251 if e8 else 199)
    return a.astype(np.uint8).tobytes()


def _filler(info: Info, n: int) -> Tuple[List[tuple], int]:
    """Tokens that produce exactly n bytes of output from a small feed: 256 literals, then matches as long as the format allows
    whose source never overlaps their output (distance >= length)."""
    assert n >= 256
    toks, have = [("lit", _bytes(256, 3, e8=False))], 256
    while have < n:
        ln = min(n - have, info.max_len, have if info.lazy else 256)
        if ln < info.minlen:                                    # (the last few bytes)
            toks.append(("lit", _bytes(ln, 5, e8=False)))
        else:
            toks.append(("match", ln, max(ln, 256) if info.lazy else 256))
        have += ln
    return toks, have


def chunk_header_cases(info: Info) -> List[Tuple[str, List[tuple]]]:
    """lazy2 on an unmodelled block: the decoded stream (selector, program, feed) lies in stored chunks of 65 536 bytes.  The
    literals in front are sized so that the second chunk's header falls inside a match's offset bits / length bits."""
    hdr = 3 + len(info.model.pcomp)
    edge = 8 * (65536 - hdr)                                   # feed bit position of the chunk boundary
    out = []
    for what in ("offset", "length"):
        found = None
        for nlit in range(65536 - hdr - 12, 65536 - hdr + 1):
            toks = [("lit", _bytes(nlit, 9)), ("match", 300, 50000), ("lit", b"tail")]
            spans = []
            lazy2_feed(toks, info.rb, spans)
            _, p_len, p_off, end = spans[0]
            lo, hi = (p_off, end) if what == "offset" else (p_len, p_off)
            if lo < edge < hi:
                found = toks
                break
        assert found is not None, what
        out.append((f"chunk-header-in-{what}-bits", found))
    return out


def catalogue(method: str) -> List[Tuple[str, List[List[tuple]]]]:
    """(name, token lists of the block's segments) for every edge case of the method."""
    info = Info(method)
    kpiece, kring = store_kernel_constants()
    mn, mx, M = info.minlen, info.max_len, info.msize
    cases: List[Tuple[str, List[List[tuple]]]] = []

    def add(name, toks):
        cases.append((name, [toks]))

    pre = _bytes(300, 1)
    for d in DISTANCES:
        add(f"dist-{d}", [("lit", pre), ("match", 100, d), ("lit", b"XY"), ("match", mn, d)])
    lengths = [mn, mn + 1, 63, 64, 65, 127, 128, 129, mx]
    if info.lazy:
        lengths += [kpiece - 1, kpiece, kpiece + 1, 3 * kpiece + 17]
    for ln in lengths:
        for d in (1, 2, 63, 64, 65, 200):
            add(f"len-{ln}-dist-{d}", [("lit", pre), ("match", ln, d), ("lit", b"Z")])
    # relative to the bytes written so far
    for ptr, d in ((40, 39), (40, 40), (40, 41), (10, 50), (10, 5000)):
        for ln in sorted({mn, 70, min(d, 5000), min(d + 1, 5001)}):
            if ln >= mn:
                add(f"ptr-{ptr}-dist-{d}-len-{ln}", [("lit", _bytes(ptr, 2)), ("match", ln, d), ("lit", b"after"), ("match", mn + 3, 9)])
    # around the ring of zh_store.hip: output of more than the ring first
    fill, have = _filler(info, kring + 1000)
    for d in (kring - 65, kring - 64, kring - 63, kring):
        add(f"ring-dist-{d}", fill + [("match", 100, d), ("lit", b"r"), ("match", 70, d)])
    for d in (kring + 100,):
        for ln in (d, d + 1):
            add(f"far-dist-{d}-len-{ln}", fill + [("match", ln, d), ("lit", b"f")])
    # modulo |M|
    for d in (M, M + 1, M + 3, M + 63, M + 64, M + 65, 2 * M + 5):
        if d <= info.max_dist:
            for ln in (mn, 100):
                add(f"mod-dist-M{d - M:+d}-len-{ln}", [("lit", pre), ("match", ln, d), ("lit", b"m"), ("match", mn, 3)])
    if not info.lazy:
        for ln in (mn, mn + 63):
            add(f"field-FFFFFFFF-len-{ln}", [("lit", pre), ("match", ln, 0, 4), ("lit", b"go on"), ("match", mn, 2)])
            add(f"field-00000000-len-{ln}", [("lit", pre), ("match", ln, 1, 4), ("lit", b"go on"), ("match", mn, 2)])
        add("field-FFFFFFFF-first-code", [("match", mn + 63, 0, 4), ("lit", b"first"), ("match", mn, 0, 4)])
    # a match that straddles pb = |M|
    fill, have = _filler(info, M - 30)
    add("straddle-M", fill + [("match", 100, 7), ("lit", b"wrapped"), ("match", 90, 40), ("match", mn, M - 3 if M - 3 <= info.max_dist else 5)])
    if info.lazy and not info.modelled:
        for name, toks in chunk_header_cases(info):
            add(name, toks)
    # two segments: the second begins with a match into the first one's bytes (it starts again at ptr = 0, M stays)
    for back in (40, 300):
        cases.append((f"two-segments-back-{back}", [[("lit", _bytes(300, 4))], [("match", 20, M - back), ("lit", b"2nd"), ("match", mn, 5)]]))
    return cases


def sweep(method: str) -> List[List[tuple]]:
    """SWEEP_STREAMS seeded token streams of at most SWEEP_MAX_OUT output bytes: distances and lengths half from the edge sets,
    half at random."""
    info = Info(method)
    M = info.msize
    rng = np.random.default_rng([SWEEP_SEED, METHODS.index(method)])
    edge_d = [d for d in DISTANCES + [M, M + 1, M + 3, M + 63, M + 64, M + 65, 2 * M + 5] if d <= info.max_dist]
    if not info.lazy:
        edge_d.append(0)
    edge_l = [info.minlen, info.minlen + 1, 63, 64, 65, 127, 128, 129, min(info.max_len, 4000)]
    streams = []
    for _ in range(SWEEP_STREAMS):
        limit = int(rng.integers(200, SWEEP_MAX_OUT + 1))
        toks, have = [], 0
        while have < limit:
            if not toks or rng.random() < 0.35:
                n = min(int(rng.integers(1, 120)), limit - have)
                toks.append(("lit", rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
            else:
                d = int(rng.choice(edge_d)) if rng.random() < 0.5 else int(2 ** rng.uniform(0, 15))
                ln = int(rng.choice(edge_l)) if rng.random() < 0.5 else int(rng.integers(info.minlen, 2000))
                ln = min(ln, limit - have)
                if ln < info.minlen:
                    toks.append(("lit", bytes(ln)))
                    n = ln
                elif d == 0:
                    toks.append(("match", ln, 0, 4))
                    n = ln
                else:
                    toks.append(("match", ln, d))
                    n = ln
            have += n
        streams.append(toks)
    return streams


# ---------------------------------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------------------------------
def block_of(info: Info, feeds: Sequence[bytes], plain: bytes = b"x" * 16) -> bytes:
    """The framed block: one segment through tools.methods.compress_block, several through the oracle's Compressor.  `plain`: what
    the size comment and the SHA-1 of a one-segment block describe — the expansion, where the host driver is to place the block by
    its size hint (a hint that is too small costs a second, exact pass: zpaqhip_stats.launches would count it)."""
    import oracle
    if len(feeds) == 1:
        return methods.compress_block(info.method, plain, pre=feeds[0])
    if not info.modelled:
        # the store layout by hand (the Compressor mirror writes modelled blocks only): every segment's bytes in length-prefixed
        # chunks, the first one's behind the selector and the program (Encoder.cs:39-73 with n == 0); no SHA-1 (FE)
        pc = info.model.pcomp
        s = bytes([0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3]) + b"zPQ" + bytes([2, 1]) + info.model.header
        for i, f in enumerate(feeds):
            dec = (bytes([1, len(pc) & 255, len(pc) >> 8]) + pc if i == 0 else b"") + f
            s += b"\x01seg%d\0\0\0" % i + b"".join(len(dec[a:a + 65536]).to_bytes(4, "big") + dec[a:a + 65536] for a in range(0, len(dec), 65536))
            s += b"\0\0\0\0\xfe"
        return s + b"\xff"
    c = oracle.Compressor(sum(map(len, feeds)) * 2 + 70000)
    c.write_tag()
    c.start_block(info.model.header)
    for i, f in enumerate(feeds):
        c.start_segment(b"seg%d" % i, b"")
        if i == 0:
            c.post_process(info.model.pcomp)
        c.compress(f)
        c.end_segment(None)
    c.end_block()
    s = c.getvalue()
    c.close()
    return s
