"""zpaqhip_scan_device and zpaqhip_decompress_device (Context.scan_device / decompress_device) against the host forms on the same
bytes: the same block and segment tables, field for field, the same error (code, block, segment, message) and kept prefix;
the same plaintext, with guard bytes around the output.  The streams are tests/scan_cases.py's (a few KiB to a few hundred
KiB): framing, zero runs, every residue around a piece boundary of the streaming kernel, framing damage.  Tables are integers
and plaintext is bytes: equality is the test, and no case skips."""
import numpy as np
import pytest
import torch

import zpaqsharp_amd as z
from tests import scan_cases as sc
from tests import util
from zpaqsharp_amd import _lib, models

import oracle

pytestmark = pytest.mark.gpu

OUT_FULL = -20
GUARD = 0xC3
BLOCK_FIELDS = [f for f, _ in _lib.Block._fields_]
SEG_FIELDS = [f for f, _ in _lib.Segment._fields_ if f != "sha1"]


def to_device(s: bytes, shift: int = 0):
    """The stream `shift` bytes (a multiple of 4) into a tensor, the bytes behind it not zero: (tensor, pointer)."""
    t = torch.full((shift + len(s) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    if s:
        t[shift:shift + len(s)].copy_(torch.from_numpy(np.frombuffer(s, np.uint8).copy()))
    return t, t.data_ptr() + shift


def tables(res):
    return ([tuple(getattr(b, f) for f in BLOCK_FIELDS) for b in res.blocks],
            [tuple(getattr(g, f) for f in SEG_FIELDS) + (bytes(g.sha1),) for g in res.segments])


def same_scan(ctx, s: bytes, shift: int = 0, stream=None):
    """scan_device and scan on the same bytes; returns what differs ('' when nothing does) and the host's result."""
    want, werr = z.scan(s, partial=True)
    t, p = to_device(s, shift)
    got, gerr = ctx.scan_device(p, len(s), stream, partial=True)
    torch.cuda.synchronize()
    why = []
    if tables(got) != tables(want):
        why.append("tables: %d/%d blocks, %d/%d segments" % (got.n_blocks, want.n_blocks, got.n_segments, want.n_segments))
    if (gerr is None) != (werr is None):
        why.append("error %r, host %r" % (gerr, werr))
    elif gerr is not None and (gerr.code, gerr.block, gerr.segment, str(gerr)) != (werr.code, werr.block, werr.segment, str(werr)):
        why.append("error %r (%d %d %d), host %r (%d %d %d)" % (gerr, gerr.code, gerr.block, gerr.segment, werr, werr.code, werr.block, werr.segment))
    return "; ".join(why), (want, werr)


@pytest.mark.parametrize("family", ["framing", "zeros", "boundary"])
def test_scan_device_gives_the_host_scan_tables(ctx, family):
    cases = {"framing": sc.framing_cases, "zeros": sc.zero_run_cases, "boundary": sc.boundary_cases}[family]()
    bad = []
    for name, s in cases:
        why, _ = same_scan(ctx, s)
        if why:
            bad.append(name + ": " + why)
    assert not bad, "\n".join(bad)


def test_scan_device_on_a_stream_that_is_only_4_byte_aligned(ctx):
    for name, s in sc.framing_cases()[:3] + sc.boundary_cases()[:8]:
        for shift in (4, 8, 12):
            why, _ = same_scan(ctx, s, shift)
            assert not why, (name, shift, why)


def test_scan_device_errors_and_kept_prefix(ctx):
    """Every mutation of test_scan_errors_match_the_oracle and test_scan_hands_back_the_blocks_before_framing_damage."""
    for name, s, code, msg, kept, blk in sc.error_cases():
        why, (want, werr) = same_scan(ctx, s)
        assert not why, (name, why)
        assert want.n_blocks == kept
        if code == 0:
            assert werr is None
            continue
        assert werr is not None and werr.block == blk
        if code is not None:
            assert werr.code == code and msg in str(werr)
            t, p = to_device(s)
            with pytest.raises(z.ZpaqError, match=msg) as e:
                ctx.scan_device(p, len(s))
            assert e.value.code == code


def test_scan_device_counts_and_small_tables(ctx):
    import ctypes as C
    L = _lib.load()
    s = dict(sc.framing_cases())["mixed"]
    t, p = to_device(s)
    nb, ns, err = C.c_size_t(0), C.c_size_t(0), _lib.Err()
    assert L.zpaqhip_scan_device(ctx._h, p, len(s), None, 0, C.byref(nb), None, 0, C.byref(ns), None, C.byref(err)) == 0
    assert (nb.value, ns.value) == (6, 6)
    blocks, segs = (_lib.Block * 6)(), (_lib.Segment * 6)()
    rc = L.zpaqhip_scan_device(ctx._h, p, len(s), blocks, 5, C.byref(nb), segs, 6, C.byref(ns), None, C.byref(err))
    assert rc == -25 and (nb.value, ns.value) == (6, 6) and b"too small" in err.msg
    assert L.zpaqhip_scan_device(ctx._h, p + 1, len(s) - 1, None, 0, C.byref(nb), None, 0, C.byref(ns), None, C.byref(err)) == -25
    st = ctx.stats()
    ctx.scan_device(p, len(s))
    st = ctx.stats()
    assert st.h2d_ms == 0 and st.d2h_ms == 0 and st.launches >= 5 and st.init_ms == st.kernel_ms > 0 and st.blocks == 6


def test_scan_device_on_a_callers_stream(ctx):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for name, s in sc.framing_cases()[:2]:
            why, _ = same_scan(ctx, s, 0, side.cuda_stream)
            assert not why, (name, why)
    side.synchronize()


# ---- decompress_device

def plain_block(model, data, comment=None, sha1=True):
    m = models.get(model)
    return oracle.compress_block(m.header, data, filename=b"f", comment=comment, with_sha1=sha1)


def device_decompress(ctx, s: bytes, out_cap: int, stream=None, raise_on_error=True, **opt):
    """(rc, out_len, the out_cap bytes at d_out) with the guards around them checked."""
    t, p = to_device(s)
    out = torch.full((64 + out_cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
    r = ctx.decompress_device(p, len(s), out.data_ptr() + 64, out_cap, stream=stream, raise_on_error=raise_on_error, **opt)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:64] == GUARD).all() and (h[64 + out_cap:] == GUARD).all(), "written outside d_out[0, out_cap)"
    return r + (h[64:64 + out_cap],)


@pytest.fixture(scope="module")
def texts():
    return [util.text(n, seed) for seed, n in enumerate([3000, 1, 70000, 0, 4097, 900, 12345])]


def check_whole(ctx, s, tail_clean=True, **opt):
    """decompress_device against decompress; tail_clean: d_out[out_len, out_cap) is untouched too (it need not be where a
    size comment promised more than its block holds: blocks behind it are decoded further out and moved)."""
    want = ctx.decompress(s, **opt).tobytes()
    rc, n, got = device_decompress(ctx, s, len(want) + 5, **opt)
    assert rc == 0 and n == len(want) and got[:n].tobytes() == want
    assert not tail_clean or (got[n:] == GUARD).all()
    return want


def test_decompress_device_all_sizes_plausible(ctx, texts):
    s = b"".join(plain_block(m, d) for m, d in zip(["l1", "mid", "l1", "mid", "min", "max", "l1"], texts))
    s += sc.store_block(b"stored bytes" * 50) + b"tail"
    want = check_whole(ctx, s)
    assert want == b"".join(texts) + b"stored bytes" * 50
    st = ctx.stats()
    assert st.h2d_ms == 0 and st.d2h_ms == 0 and 0 < st.init_ms < st.kernel_ms and st.blocks == 8 and st.out_bytes == len(want)
    check_whole(ctx, s, verify_sha1=True)
    check_whole(ctx, s, kernel=1)                       # the generic kernel as a cross-check


def test_decompress_device_without_size_comments(ctx, texts):
    s = b"".join(plain_block(m, d, comment=b"") for m, d in zip(["l1", "mid", "l1", "mid", "min"], texts))
    assert check_whole(ctx, s, verify_sha1=True) == b"".join(texts[:5])
    # sizes at first, then none
    s = plain_block("l1", texts[0]) + plain_block("mid", texts[4]) + plain_block("l1", texts[2], comment=b"jpg") + plain_block("min", texts[5])
    assert check_whole(ctx, s, verify_sha1=True) == texts[0] + texts[4] + texts[2] + texts[5]


def test_decompress_device_wrong_size_comments(ctx, texts):
    d = texts
    for small, large in ((b"100", b"99999"), (b"0", b"4098")):
        s = (plain_block("l1", d[0]) + plain_block("mid", d[4], comment=small) + plain_block("l1", d[5]) + plain_block("l1", d[2], comment=b"")
             + plain_block("mid", d[6]))
        assert check_whole(ctx, s, verify_sha1=True) == d[0] + d[4] + d[5] + d[2] + d[6]
        s = plain_block("l1", d[0]) + plain_block("mid", d[4], comment=large) + plain_block("l1", d[5]) + plain_block("min", d[6])
        assert check_whole(ctx, s, tail_clean=False, verify_sha1=True) == d[0] + d[4] + d[5] + d[6]
        s = (plain_block("l1", d[0]) + plain_block("mid", d[4], comment=small) + plain_block("l1", d[5]) + plain_block("mid", d[6], comment=large)
             + plain_block("l1", d[1]) + plain_block("l1", d[2]))
        assert check_whole(ctx, s, tail_clean=False) == d[0] + d[4] + d[5] + d[6] + d[1] + d[2]


def test_decompress_device_wrong_size_comments_and_output_too_small(ctx, texts):
    """Moves and second decodes under clipping: the wrong-size streams above with out_cap one byte short of the total, one
    byte into the block behind the wrong one, and 0.  The total is counted, nothing is written outside d_out[0, out_cap)
    (device_decompress checks the guards)."""
    d = texts
    small, large = b"100", b"99999"
    streams = [
        (plain_block("l1", d[0]) + plain_block("mid", d[4], comment=small) + plain_block("l1", d[5]) + plain_block("l1", d[2], comment=b"")
         + plain_block("mid", d[6]), [d[0], d[4], d[5], d[2], d[6]]),
        (plain_block("l1", d[0]) + plain_block("mid", d[4], comment=large) + plain_block("l1", d[5]) + plain_block("min", d[6]),
         [d[0], d[4], d[5], d[6]]),
        (plain_block("l1", d[0]) + plain_block("mid", d[4], comment=small) + plain_block("l1", d[5]) + plain_block("mid", d[6], comment=large)
         + plain_block("l1", d[1]) + plain_block("l1", d[2]), [d[0], d[4], d[5], d[6], d[1], d[2]]),
    ]
    for s, parts in streams:
        total = sum(len(x) for x in parts)
        for cap in (total - 1, len(parts[0]) + len(parts[1]) + 1, 0):
            rc, n, got = device_decompress(ctx, s, cap)
            assert rc == OUT_FULL and n == total, (len(parts), cap)


def test_decompress_device_output_too_small(ctx, texts):
    for comment in (None, b""):
        s = b"".join(plain_block(m, d, comment=comment) for m, d in zip(["l1", "mid", "l1", "mid"], texts))
        want = b"".join(texts[:4])
        for cap in (len(want) - 1, len(texts[0]) + 1, 0):
            rc, n, got = device_decompress(ctx, s, cap)
            assert rc == OUT_FULL and n == len(want)
        rc, n, got = device_decompress(ctx, s, len(want))
        assert rc == 0 and got.tobytes() == want


def test_decompress_device_damaged_block(ctx, texts):
    blocks = [plain_block("l1", texts[0]), plain_block("mid", texts[4]), bytearray(plain_block("l1", texts[2])), plain_block("l1", texts[5])]
    g = z.scan(bytes(blocks[2])).segments[0]
    blocks[2][g.data_off + g.data_len // 2] ^= 0x10
    s = b"".join(bytes(b) for b in blocks)
    front = texts[0] + texts[4]
    with pytest.raises(z.ZpaqError) as host:
        ctx.decompress(s, verify_sha1=True)
    rc, n, got = device_decompress(ctx, s, len(front) + len(texts[2]) + 5000, raise_on_error=False, verify_sha1=True)
    assert rc == host.value.code and rc != 0 and ctx.last_error.block == 2 == host.value.block
    assert n == len(front) and got[:n].tobytes() == front
    t, p = to_device(s)
    out = torch.empty(200000, dtype=torch.uint8, device="cuda")
    with pytest.raises(z.ZpaqError):
        ctx.decompress_device(p, len(s), out.data_ptr(), out.numel(), verify_sha1=True)
    # framing damage behind good blocks: they are delivered, then the scan's error
    cut = b"".join(bytes(b) for b in blocks[:2]) + plain_block("mid", texts[5])[:40]
    rc, n, got = device_decompress(ctx, cut, len(front) + 10, raise_on_error=False)
    assert rc == -2 and n == len(front) and got[:n].tobytes() == front and ctx.last_error.block == 2


def test_decompress_device_results_and_callers_stream(ctx, texts):
    s = plain_block("l1", texts[0]) + plain_block("mid", texts[4], comment=b"") + plain_block("l1", texts[5])
    want = texts[0] + texts[4] + texts[5]
    t, p = to_device(s)
    out = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rc, n, res = ctx.decompress_device(p, len(s), out.data_ptr(), len(want), results=True, stream=side.cuda_stream, verify_sha1=True)
    side.synchronize()
    assert rc == 0 and n == len(want) and out.cpu().numpy()[:n].tobytes() == want and (out.cpu().numpy()[n:] == GUARD).all()
    assert [(r.status, r.out_off, r.out_len) for r in res] == [(0, 0, len(texts[0])), (0, len(texts[0]), len(texts[4])),
                                                               (0, len(texts[0]) + len(texts[4]), len(texts[5]))]


def test_device_round_trip_without_a_host_copy(ctx):
    """compress_method_device -> scan_device -> decompress_device: the stream never leaves the device."""
    data = [util.text(n, 20 + i) for i, n in enumerate([20000, 1, 65536, 70001, 0, 333])]
    plain = np.frombuffer(b"".join(data) + b"\0", np.uint8).copy()
    offs = np.zeros(len(data) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in data], dtype=np.uint64)
    d_plain = torch.from_numpy(plain).cuda()
    for m in ("x0,1,4,0,3,24", "x0,0ci1,1,1,1,2am"):
        d_stream = torch.full((len(plain) * 2 + 65536,), 0x5A, dtype=torch.uint8, device="cuda")
        rc, n, boffs = ctx.compress_method_device(m, d_plain.data_ptr(), offs, d_stream.data_ptr(), d_stream.numel())
        assert rc == 0
        got = ctx.scan_device(d_stream.data_ptr(), n)
        assert got.n_blocks == len(data) and [int(b.tag_off) for b in got.blocks] == [int(x) for x in boffs[:-1]]
        assert [int(b.usize_hint) for b in got.blocks] == [len(d) for d in data]
        d_back = torch.full((len(plain) + 63,), GUARD, dtype=torch.uint8, device="cuda")
        rc, k = ctx.decompress_device(d_stream.data_ptr(), n, d_back.data_ptr(), len(plain) - 1, verify_sha1=True)
        assert rc == 0 and k == len(plain) - 1
        assert torch.equal(d_back[:k], d_plain[:k]) and bool((d_back[k:] == GUARD).all())
