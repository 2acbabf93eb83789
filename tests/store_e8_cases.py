"""Inputs for the end-of-segment E8E9 pass of the reference's LZ77 post-processors (`lazy2` / `lzpre` with E8E9,
LibZPAQ.cs:441-462, :581-601): byte strings that the pass is run over (what the LZ77 codes of a segment wrote into M), and
the framing of blocks with several segments.  Shared by tests/test_store_e8.py (the schedule of zh_e8e9_wave.h on the host)
and tests/test_gpu_store_e8.py (zh_store.hip)."""
import hashlib

import numpy as np

from tools import methods

TAG = bytes([0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3])


def pass_model(data: bytes):
    """The program's loop in Python (only to check that a constructed input has the property it was built for; the
    reference in every comparison is the oracle's run of the program).  Returns (final bytes, positions that triggered)."""
    m, d, hits = bytearray(data), len(data), []
    for b in range(d):
        if b + 4 < d and (m[b] & 254) == 232 and ((m[b + 4] + 1) & 254) == 0:
            a = ((m[b + 1] | m[b + 2] << 8 | m[b + 3] << 16) - b) & 0xFFFFFF
            m[b + 1], m[b + 2], m[b + 3] = a & 255, (a >> 8) & 255, a >> 16
            hits.append(b)
    return bytes(m), hits


def plain_filler(n: int, seed: int) -> bytearray:
    """Random bytes without E8 / E9, 00 and FF: nothing in them triggers or completes a pattern."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 255, n, dtype=np.uint8)
    a[(a & 254) == 232] = 0x41
    return bytearray(a.tobytes())


def dense(n: int, seed: int) -> bytes:
    """E8 / E9 every few bytes with 00 / FF (sometimes 01 / FE) four bytes on, over random bytes."""
    rng = np.random.default_rng(seed)
    a = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    i = 0
    while i + 5 <= n:
        a[i] = 0xE8 + int(rng.integers(0, 2))
        a[i + 4] = int(rng.choice([0, 255, 0, 255, 1, 254]))
        i += int(rng.integers(1, 8))
    return bytes(a)


def runs(byte: int, e8_inside: bool, e8_after: bool) -> bytes:
    """4 KiB of 00 or FF between random bytes: every position of the run completes a pattern."""
    a = plain_filler(700, 5) + bytearray([byte]) * 4096 + plain_filler(900, 6)
    if e8_inside:
        for p in (700 + 3, 700 + 1000, 700 + 1001, 700 + 2047, 700 + 4090):
            a[p] = 0xE8
    if e8_after:
        a[700 + 4096] = 0xE9
        a[700 + 4096 + 4] = byte
    return bytes(a)


def chain(start: int, links: int, tail: int = 300, seed: int = 9) -> bytes:
    """A chain in which every trigger writes the next pattern: positions start, start + 3, start + 6, ... (start > 0).  Only
    the first holds an E8 before the pass runs.  The address at p is a = EA << 16 | low with low < p and a low byte of 00 or
    FF (it is the byte four after the link before): a - p borrows, and its top byte, written to p + 3, is E9 where EA stood
    before.  The two lower bytes that the trigger leaves behind are kept clear of E8 / E9."""
    rng = np.random.default_rng(seed)
    a = plain_filler(start + 3 * links + 8 + tail, seed)
    a[start] = 0xE8
    for k in range(links):
        p = start + 3 * k
        cands = [r << 8 | lo for r in range(256) for lo in (0x00, 0xFF) if (r << 8 | lo) < p]
        cands = [c for c in cands if ((c - p) & 254) != 232 and (((c - p) >> 8) & 254) != 232] or cands    # (p = 17 hex modulo 256 leaves none)
        low = cands[int(rng.integers(0, len(cands)))]
        a[p + 1], a[p + 2], a[p + 3] = low & 255, low >> 8, 0xEA
    a[start + 3 * links + 1] = 0xFF                          # the last written E9 triggers too
    return bytes(a)


def boundary(offset: int, slice_: int, round_: int, seed: int = 3) -> bytes:
    """A pattern that starts `offset` bytes from every slice boundary of two rounds (the round boundary among them)."""
    n = 2 * round_ + 2 * slice_ + 9
    a = plain_filler(n, seed + offset + 4)
    rng = np.random.default_rng(seed)
    for b in range(slice_, n, slice_):
        p = b + offset
        if p >= 0 and p + 5 <= n:
            a[p] = 0xE8 + int(rng.integers(0, 2))
            a[p + 4] = int(rng.choice([0, 255]))
    return bytes(a)


def tail_cases():
    """E8 at d - 5 (the last position that can trigger) and at d - 4 (cannot: b + 4 < d fails)."""
    a = plain_filler(200, 12)
    a[195], a[199] = 0xE8, 0x00
    b = plain_filler(200, 13)
    b[196] = 0xE8
    b[199] = 0xFF
    return {"tail_d-5": bytes(a), "tail_d-4": bytes(b)}


def pass_inputs(slice_: int, round_: int) -> dict:
    rng = np.random.default_rng(21)
    cases = {f"len{n}": bytes([0xE8, 1, 2, 3, 0xFF, 0xE9, 7, 8, 0])[:n] for n in range(10)}
    cases["random"] = rng.integers(0, 256, 2 * round_ + 777, dtype=np.uint8).tobytes()
    cases["dense"] = dense(2 * round_ + 333, 31)
    for byte in (0x00, 0xFF):
        for inside in (False, True):
            for after in (False, True):
                cases[f"run{byte:02x}_{int(inside)}{int(after)}"] = runs(byte, inside, after)
    cases["chain"] = chain(5 * slice_ - 10, slice_ + 20)                         # from one slice over three more
    cases["chain_round"] = chain(round_ - 2 * slice_ - 5, slice_ + 10)           # over the round boundary
    for off in range(-4, 4):
        cases[f"boundary{off:+d}"] = boundary(off, slice_, round_)
    cases.update(tail_cases())
    return cases


def store_block(model, seg_pres, seg_plains=None, sizes=None) -> bytes:
    """A block of an unmodelled method (n = 0) with one segment per entry of seg_pres: the bytes the post-processor's
    program is fed in that segment.  The first segment carries the program; seg_plains[i] (optional) gives the SHA-1,
    sizes[i] (optional) the size comment."""
    def body(dec):
        return b"".join(len(dec[i:i + 65536]).to_bytes(4, "big") + dec[i:i + 65536] for i in range(0, len(dec), 65536)) + b"\0\0\0\0"
    s = TAG + b"zPQ" + bytes([2, 1]) + model.header
    for i, pre in enumerate(seg_pres):
        dec = (bytes([1, len(model.pcomp) & 255, len(model.pcomp) >> 8]) + model.pcomp if i == 0 else b"") + pre
        s += b"\x01\0" + (str(sizes[i]).encode() if sizes else b"") + b"\0\0" + body(dec)
        plain = seg_plains[i] if seg_plains else None
        s += b"\xfd" + hashlib.sha1(plain).digest() if plain is not None else b"\xfe"
    return s + b"\xff"


def literals(args, data: bytes) -> bytes:
    """`data` as literal codes of the method's LZ77 level: the program writes exactly these bytes into M."""
    if not data:
        return b""
    items = [("lit", i, min(i + 4000, len(data))) for i in range(0, len(data), 4000)]
    return methods._write_codes(data, args, items)


def self_copy(args, n: int, m_bytes: int) -> bytes:
    """lzpre codes that copy M[0 .. n) onto itself (offset |M| - 1: distance 0 modulo |M|): a later segment that writes
    out what the segment before left in M."""
    out = bytearray()
    if n:
        assert n >= args[2]
        methods._put_match2(out, n, m_bytes, args[2])
    return bytes(out)
