"""The reference's method strings: block configs with its LZ77 / BWT / E8E9 post-processors, and the matching
pre-processors (host tooling for fixtures; the decode side is the GPU's job).

`make_config(method)` is the equivalent of `LibZPAQ.makeConfig` (LibZPAQ.cs:388-1044): it turns an expanded method
string into ZPAQL config text.  It, `parse_args`, `model_of` and the PCOMP generators live in the product module
zpaqsharp_amd/method.py (Context.compress_method builds its blocks from them) and are re-exported here unchanged.

`preprocess(data, args)` is the equivalent of `LZBuffer` (LZBuffer.cs:96-115 formats, :225-486): it produces the byte
stream those PCOMP programs invert.  Match finding here is a plain greedy hash search — only the CODE FORMAT has to
agree with the reference, not its parse.  With `sa=True`, a level 1 / 2 method with args[5] - args[0] >= 21 gets the
reference's own parse instead: `lz77_sa`, a literal port of LZBuffer's suffix-array search (LZBuffer.cs:246-283, :332-383).
With `ht=True`, a level 1 / 2 method with args[5] - args[0] < 21 gets `lz77_ht`, the port of its hash-table search
(LZBuffer.cs:285-327, :349-368).
"""
from __future__ import annotations

from typing import List

import numpy as np

from zpaqsharp_amd.method import (_E8E9_TAIL, _lg, _nbits, _pcomp_bwtrle, _pcomp_lazy2, _pcomp_lzpre,  # noqa: F401
                                  make_config, model_of, parse_args, uses_ht, uses_sa)


# ---------------------------------------------------------------------------------------------------------------------
# pre-processors (LZBuffer equivalents)
# ---------------------------------------------------------------------------------------------------------------------
def e8e9_forward(data: bytes) -> bytes:
    """LibZPAQ.cs:372-384."""
    b = bytearray(data)
    for i in range(len(b) - 5, -1, -1):
        if (b[i] & 254) == 0xE8 and ((b[i + 4] + 1) & 254) == 0:
            a = ((b[i + 1] | b[i + 2] << 8 | b[i + 3] << 16) + i) & 0xFFFFFF
            b[i + 1], b[i + 2], b[i + 3] = a & 255, (a >> 8) & 255, (a >> 16) & 255
    return bytes(b)


class _BitWriter:
    def __init__(self):
        self.out, self.bits, self.n = bytearray(), 0, 0

    def putb(self, x: int, k: int):                        # LSB first (LZBuffer.cs:50-63)
        x &= (1 << k) - 1
        self.bits |= x << self.n
        self.n += k
        while self.n > 7:
            self.out.append(self.bits & 255)
            self.bits >>= 8
            self.n -= 8

    def flush(self):
        if self.n > 0:
            self.out.append(self.bits & 255)
        self.bits = self.n = 0


def _matches(d: bytes, min_match: int, max_match: int, max_off: int):
    """Greedy parse: yields ('lit', start, end) / ('match', length, offset)."""
    n, i, lit0 = len(d), 0, 0
    last = {}
    while i < n:
        best = 0
        if i + min_match <= n:
            key = d[i:i + min_match]
            j = last.get(key, -1)
            if j >= 0 and 0 < i - j <= max_off:
                m = min_match
                while m < max_match and i + m < n and d[j + m] == d[i + m]:
                    m += 1
                best, off = m, i - j
            last[key] = i
        if best:
            if i > lit0:
                yield ("lit", lit0, i)
            yield ("match", best, off)
            for k in range(i + 1, min(i + best, n - min_match + 1)):
                last[d[k:k + min_match]] = k
            i += best
            lit0 = i
        else:
            i += 1
    if n > lit0:
        yield ("lit", lit0, n)


def _put_literal1(w: _BitWriter, data: bytes, a: int, b: int):
    """write_literal, level 1 (LZBuffer.cs:392-406): data[a:b], b > a."""
    lit = b - a
    ll = _lg(lit)
    w.putb(0, 2)
    ll -= 1
    while ll > 0:
        ll -= 1
        w.putb(1, 1)
        w.putb((lit >> ll) & 1, 1)
    w.putb(0, 1)
    for c in data[a:b]:
        w.putb(c, 8)


def _put_match1(w: _BitWriter, ln: int, off: int, rb: int):
    """write_match, level 1 (LZBuffer.cs:426-448)."""
    ll = _lg(ln) - 1
    off += (1 << rb) - 1
    lo = _lg(off) - 1 - rb
    assert 0 <= lo <= 23 and ll >= 2
    w.putb((lo + 8) >> 3, 2)
    w.putb(lo & 7, 3)
    while ll > 2:
        ll -= 1
        w.putb(1, 1)
        w.putb((ln >> ll) & 1, 1)
    w.putb(0, 1)
    w.putb(ln & 3, 2)
    w.putb(off, rb)
    w.putb(off >> rb, lo)


def _put_literal2(out: bytearray, data: bytes, a: int, b: int):
    """write_literal, level 2 (LZBuffer.cs:407-418)."""
    while a < b:
        k = min(64, b - a)
        out.append(k - 1)
        out += data[a:a + k]
        a += k


def _put_match2(out: bytearray, ln: int, off: int, m: int):
    """write_match, level 2 (LZBuffer.cs:451-485)."""
    off -= 1
    while ln > 0:
        len1 = m + 63 if ln > m * 2 + 63 else ln - m if ln > m + 63 else ln
        assert m <= len1 < m + 64
        if off < (1 << 16):
            out += bytes([64 + len1 - m, off >> 8, off & 255])
        elif off < (1 << 24):
            out += bytes([128 + len1 - m, off >> 16, (off >> 8) & 255, off & 255])
        else:
            out += bytes([192 + len1 - m, off >> 24, (off >> 16) & 255, (off >> 8) & 255, off & 255])
        ln -= len1


def lz77_level1(data: bytes, args: List[int]) -> bytes:
    """Bit-packed codes of LZBuffer level 1 (LZBuffer.cs:96-107, write_literal :387-405, write_match :422-446)."""
    rb = args[0] - 4 if args[0] > 4 else 0
    min_match = max(4, args[2])
    w = _BitWriter()
    for item in _matches(data, min_match, 1 << 16, (1 << 23) - 1):
        if item[0] == "lit":
            _put_literal1(w, data, item[1], item[2])
        else:
            _put_match1(w, item[1], item[2], rb)
    w.flush()
    return bytes(w.out)


def lz77_level2(data: bytes, args: List[int]) -> bytes:
    """Byte-aligned codes of LZBuffer level 2 (LZBuffer.cs:109-112, write_literal :406-418, write_match :449-485)."""
    m = args[2]
    assert 1 <= m <= 64
    out = bytearray()
    for item in _matches(data, max(m, 3), m + 63 + 4 * 64, (1 << 24) - 1):
        if item[0] == "lit":
            _put_literal2(out, data, item[1], item[2])
        else:
            _put_match2(out, item[1], item[2], m)
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's suffix-array match search (LZBuffer's `isa` path: args[5] - args[0] >= 21, levels 1 and 2)
# ---------------------------------------------------------------------------------------------------------------------
MAX_MATCH = 49152                                          # maxMatch = BUFSIZE * 3 (LZBuffer.cs:45, :172)
MAX_LITERAL = 4096                                         # maxLiteral = BUFSIZE / 4 (LZBuffer.cs:174)


def suffix_array(data: bytes) -> np.ndarray:
    """The suffix array divsufsort gives (the end of the block sorts below every byte), by prefix doubling: there is no
    suffix-sorting library here and fixtures are small."""
    n = len(data)
    if n == 0:
        return np.zeros(0, np.int64)
    a = np.frombuffer(data, np.uint8)
    rank = a.astype(np.int64)
    sa = np.argsort(rank, kind="stable")
    k = 1
    while True:
        r2 = np.full(n, -1, np.int64)
        r2[:n - k] = rank[k:]
        order = np.lexsort((r2, rank))
        key = rank[order] * (max(n, 256) + 2) + (r2[order] + 1)      # (ranks start as byte values: the radix must exceed 256 for blocks shorter than that)
        nr = np.zeros(n, np.int64)
        nr[order] = np.concatenate([[0], np.cumsum(key[1:] != key[:-1])])
        rank, sa = nr, order
        if nr.max() == n - 1:
            break
        k *= 2
    return sa


def _match_len(d: bytes, p: int, i: int, l: int, n: int) -> int:
    """for (; i+l<n && l<maxMatch && in[p+l]==in[i+l]; ++l) (LZBuffer.cs:272), comparing slices."""
    lim = min(n - i, MAX_MATCH)
    step = 8
    while l < lim:
        e = min(l + step, lim)
        if d[p + l:p + e] == d[i + l:i + e]:
            l, step = e, step * 2
        elif step > 8:
            step = 8
        else:
            while d[p + l] == d[i + l]:
                l += 1
            return l
    return l


def sa_window_ok(i: int, h: int, n: int, a0: int) -> bool:
    """The closed form of `sa[isa[(h + i) & mask]] == h + i` (LZBuffer.cs:256-264): the inverse array covers the window of
    2^(17 + args[0]) positions that holds i, so look-ahead h is searched iff h + i is inside the block and that window."""
    return h + i < n and (h + i) >> (17 + a0) == i >> (17 + a0)


def lz77_sa_parse(d: bytes, args: List[int], windowed: bool = False):
    """LZBuffer.fill on its `isa` path (LZBuffer.cs:244-283, :329-383) as the calls it makes: ('lit', a, b) for
    write_literal of d[a:b] (b > a) and ('match', length, offset) for write_match.  `windowed` keeps the inverse array the
    way the reference does, one window of 2^(17 + args[0]) slots rebuilt on demand (:256-264), instead of sa_window_ok."""
    level, min_match, bucket, lookahead, a0 = args[1] & 3, args[2], (1 << args[4]) - 1, args[6], args[0]
    if (min_match < 4 and level == 1) or (min_match < 1 and level == 2):
        raise ValueError("match length $3 too small")                # LZBuffer.cs:198-199
    n = len(d)
    sa = [int(x) for x in suffix_array(d)]
    mask = (1 << (17 + a0)) - 1
    if windowed:
        isa = [0] * (mask + 1)                                       # libzpaq::Array starts zeroed
    else:
        full = [0] * n
        for j, s in enumerate(sa):
            full[s] = j
    i = lit = 0
    while i < n:
        blen, bp, blit, bscore = min_match - 1, 0, 0, 0
        if windowed and sa[isa[i & mask]] != i:
            for j in range(n):
                if (sa[j] & ~mask) == (i & ~mask):
                    isa[sa[j] & mask] = j
        for h in range(lookahead + 1):
            if windowed:
                q = isa[(h + i) & mask]
                if sa[q] != h + i:
                    continue
            else:
                if not sa_window_ok(i, h, n, a0):
                    continue
                q = full[h + i]
            for j in (-1, 1):
                for k in range(1, bucket + 1):
                    if not 0 <= q + j * k < n:
                        continue
                    p = sa[q + j * k] - h
                    if not 0 <= p < i:
                        continue
                    l = _match_len(d, p, i, h, n)
                    l1 = h
                    while l1 > 0 and d[p + l1 - 1] == d[i + l1 - 1]:
                        l1 -= 1
                    score = (l - l1) * 8 - _lg(i - p) - 4 * (lit == 0 and l1 > 0) - 11
                    for _ in range(h):
                        score = score * 5 // 8 if score >= 0 else -(-score * 5 // 8)     # C division truncates
                    if score > bscore:
                        blen, bp, blit, bscore = l, p, l1, score
                    if l < blen or l < min_match or l > 255:
                        break
            if bscore <= 0 or blen < min_match:
                break
        off = i - bp
        if off > 0 and bscore > 0 and blen - blit >= min_match + (level == 2) * ((off >= 1 << 16) + (off >= 1 << 24)):
            lit += blit
            if lit:
                yield ("lit", i + blit - lit, i + blit)
            lit = 0
            yield ("match", blen - blit, off)
        else:
            blen = 1
            lit += 1
        i += blen
        if lit >= MAX_LITERAL:
            yield ("lit", i - lit, i)
            lit = 0
    if lit:
        yield ("lit", n - lit, n)


def _write_codes(data: bytes, args: List[int], items) -> bytes:
    """The parse `items` of `data` in the codes of the method's level (1: bits, 2: bytes)."""
    if args[1] & 3 == 1:
        rb = args[0] - 4 if args[0] > 4 else 0
        w = _BitWriter()
        for item in items:
            if item[0] == "lit":
                _put_literal1(w, data, item[1], item[2])
            else:
                _put_match1(w, item[1], item[2], rb)
        w.flush()
        return bytes(w.out)
    out = bytearray()
    for item in items:
        if item[0] == "lit":
            _put_literal2(out, data, item[1], item[2])
        else:
            _put_match2(out, item[1], item[2], args[2])
    return bytes(out)


def lz77_sa(data: bytes, args: List[int], windowed: bool = False) -> bytes:
    """What LZBuffer writes for a level 1 / 2 method with args[5] - args[0] >= 21 (`data` after E8E9 where the method
    asks for it): the suffix-array parse in the codes of the level."""
    assert uses_sa(args)
    return _write_codes(data, args, lz77_sa_parse(data, args, windowed))


# ---------------------------------------------------------------------------------------------------------------------
# the reference's hash-table match search (LZBuffer without `isa`: args[5] - args[0] < 21, levels 1 and 2)
# ---------------------------------------------------------------------------------------------------------------------
def ht_shift1(args: List[int]) -> int:
    """shift1(minMatch>0 ? (args[5]-1)/minMatch+1 : 1) (LZBuffer.cs:182) in C's division, which truncates: args[5] = 0
    gives 1 where Python's // gives 0."""
    return int((args[5] - 1) / args[2]) + 1 if args[2] > 0 else 1


def ht_h1(d: bytes, args: List[int]) -> np.ndarray:
    """h1 before the step at each position 0 .. F, F = max(0, n - minMatchBoth), straight from the bytes.  The update
    h1 = ((h1 * 5) << shift1) + (in[j + minMatch] + 1) * 123456791 (LZBuffer.cs:364) multiplies a term by 5 * 2^shift1 per
    later step and shift1 * minMatch >= args[5], so after minMatch steps a term has left the masked value: h1 before the
    step at e is a sum over in[max(e, minMatch) .. e + minMatch - 1].  From F on no step is made (:353) and h1 stays h1[F]."""
    n, mm = len(d), args[2]
    F = max(0, n - (mm + 4))
    term = ((np.frombuffer(d, np.uint8).astype(np.uint64) + np.uint64(1)) * np.uint64(123456791)) & np.uint64(0xFFFFFFFF)
    W, w = (5 << ht_shift1(args)) & 0xFFFFFFFF, 1
    h = np.zeros(F + 1, np.uint64)
    for t in range(1, min(mm, F) + 1):                               # the term of the step t before: in[e - t + minMatch]
        h[t:] = (h[t:] + np.uint64(w) * term[mm:mm + F + 1 - t]) & np.uint64(0xFFFFFFFF)
        w = (w * W) & 0xFFFFFFFF
    return h & np.uint64((1 << args[5]) - 1)


def lz77_ht_parse(d: bytes, args: List[int], table: bool = False):
    """LZBuffer.fill without `isa` and with minMatch2 = lookahead = 0 (LZBuffer.cs:244-252, :285-383) as the calls it
    makes, in the items of lz77_sa_parse.  `table` keeps h1 and the array ht[] the way the reference does, one store per
    position the walk passes (:352-367; a dict stands for the zeroed array).  Without it h1 comes from the bytes (ht_h1)
    and ht[s] when i is searched is the largest j < i with j + minMatchBoth < n whose slot h1(j) ^ ih(j) is s, whatever the
    parse skipped: what zh_pre_lzht.hip computes."""
    level, mm, a0 = args[1] & 3, args[2], args[0]
    if (mm < 4 and level == 1) or (mm < 1 and level == 2):
        raise ValueError("match length $3 too small")                # LZBuffer.cs:198-199
    if args[3] or args[6] or (level == 2 and mm < 2) or a0 > 11 or args[4] > args[5]:
        raise ValueError("the hash-table search is ported for args[3] = args[6] = 0, level 2 from args[2] = 2, args[0] <= 11 "
                         "and args[4] <= args[5]")
    n = len(d)
    checkbits = 12 - a0
    mask, bucket, htsize, shift1, mmb = (1 << checkbits) - 1, (1 << args[4]) - 1, 1 << args[5], ht_shift1(args), mm + 4
    search = level == 1 or mm <= 64                                  # LZBuffer.cs:288
    if table:
        ht, h1 = {}, 0
    elif search:
        F = max(0, n - mmb)
        H = [int(x) for x in ht_h1(d, args)]
        last, ins = {}, 0
    i = lit = 0
    while i < n:
        blen, bp, bscore = mm - 1, 0, 0
        if search:
            if not table:
                while ins < i:                                       # every earlier position has been stored
                    if ins + mmb < n:
                        last[H[ins] ^ (((ins * 1234547 & 0xFFFFFFFF) >> 19) & bucket)] = ins
                    ins += 1
                h1 = H[min(i, F)]
            for k in range(bucket + 1):
                if table:
                    p = ht.get(h1 ^ k, 0)
                else:
                    j = last.get(h1 ^ k)
                    p = 0 if j is None else (j << checkbits) | (d[j + 3] & mask)
                if p and i + 3 < n and (p & mask) == (d[i + 3] & mask):
                    p >>= checkbits
                    if p < i and i + blen <= n and d[p + blen - 1] == d[i + blen - 1]:
                        l = _match_len(d, p, i, 0, n)
                        score = l * 8 - _lg(i - p) - 2 * (lit > 0) - 11
                        if score > bscore:
                            blen, bp, bscore = l, p, score
                if blen >= 128:
                    break
        off = i - bp
        if off > 0 and bscore > 0 and blen >= mm + (level == 2) * ((off >= 1 << 16) + (off >= 1 << 24)):
            if lit:
                yield ("lit", i - lit, i)
            lit = 0
            yield ("match", blen, off)
        else:
            blen = 1
            lit += 1
        if table:
            for _ in range(blen):
                if i + mmb < n:
                    ih = ((i * 1234547 & 0xFFFFFFFF) >> 19) & bucket
                    ht[h1 ^ ih] = ((i << checkbits) | (d[i + 3] & mask)) & 0xFFFFFFFF
                    h1 = ((((h1 * 5) << shift1) & 0xFFFFFFFF) + (d[i + mm] + 1) * 123456791) & (htsize - 1)
                i += 1
        else:
            i += blen
        if lit >= MAX_LITERAL:
            yield ("lit", i - lit, i)
            lit = 0
    if lit:
        yield ("lit", n - lit, n)


def lz77_ht(data: bytes, args: List[int], table: bool = False) -> bytes:
    """What LZBuffer writes for a level 1 / 2 method with args[5] - args[0] < 21 (`data` after E8E9 where the method asks
    for it): the hash-table parse in the codes of the level."""
    assert uses_ht(args)
    return _write_codes(data, args, lz77_ht_parse(data, args, table))


def bwt_level3(data: bytes) -> bytes:
    """LZBuffer.cs:228-240: BWT with the end-of-string byte coded as 255 and its position in the last 4 bytes."""
    n = len(data)
    if n == 0:
        return bytes([255, 0, 0, 0, 0])
    sa = suffix_array(data)
    out = bytearray([data[n - 1]])
    idx = 0
    for i in range(1, n + 1):
        s = int(sa[i - 1])
        if s == 0:
            idx = i
            out.append(255)
        else:
            out.append(data[s - 1])
    out += idx.to_bytes(4, "little")
    return bytes(out)


def preprocess(data: bytes, args: List[int], sa: bool = False, ht: bool = False) -> bytes:
    """What compressBlock feeds the coder (LibZPAQ.cs:296-311): LZBuffer output for levels 1-3, E8E9 for 4-7.  `sa`: the
    reference's suffix-array parse where the method selects it (uses_sa); `ht`: its hash-table parse where the method
    selects that (uses_ht).  Neither has an effect on any other method."""
    level, doe8 = args[1] & 3, 4 <= args[1] <= 7
    d = e8e9_forward(data) if doe8 else data
    if sa and uses_sa(args):
        return lz77_sa(d, args)
    if ht and uses_ht(args):
        return lz77_ht(d, args)
    if level == 1:
        return lz77_level1(d, args)
    if level == 2:
        return lz77_level2(d, args)
    if level == 3:
        return bwt_level3(d)
    return d


def compress_block(method: str, data: bytes, filename: bytes = b"", pre: bytes = None, sa: bool = False, ht: bool = False) -> bytes:
    """One block the way LibZPAQ.compressBlock frames it (tag, header, segment with the size as comment, SHA-1), coded by
    this repo's CPU stream writer; n = 0 models (methods like "x0,1,4,0,3,24") use the unmodelled store layout.
    `pre`: bytes to feed the post-processor instead of preprocess(data) (tests of the PCOMP programs on input no
    encoder writes; the size comment and SHA-1 still describe `data`).  `sa`, `ht`: as for preprocess."""
    import hashlib

    from zpaqsharp_amd import synth
    model, args = model_of(method)
    if pre is None:
        pre = preprocess(data, args, sa, ht)
    if model.n:
        return synth.compress_block(model, np.frombuffer(data, np.uint8) if data else np.zeros(0, np.uint8), filename=filename,
                                    pre=np.frombuffer(pre, np.uint8) if pre else np.zeros(0, np.uint8))
    # store path (Encoder.cs:39-73 with n == 0): the decoded stream is selector [+ PCOMP] + data in length-prefixed chunks
    dec = (bytes([1, len(model.pcomp) & 255, len(model.pcomp) >> 8]) + model.pcomp if model.pcomp else b"\0") + pre
    body = b"".join(len(dec[i:i + 65536]).to_bytes(4, "big") + dec[i:i + 65536] for i in range(0, len(dec), 65536)) + b"\0\0\0\0"
    tag = bytes([0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3])
    return (tag + b"zPQ" + bytes([2, 1]) + model.header + b"\x01" + filename + b"\0" + str(len(data)).encode() + b"\0\0"
            + body + b"\xfd" + hashlib.sha1(data).digest() + b"\xff")
