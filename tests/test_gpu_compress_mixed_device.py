"""zpaqhip_compress_mixed_blocks_device, zpaqhip_gap_hist_blocks_device and Context.compress_level_device against the host
forms on the same arguments (zpaqhip_compress_method_blocks per group, zpaqhip_gap_hist_blocks, Context.compress_level):
the same bytes, offsets and lengths, nothing written outside the blocks that fit, and a round trip through
zpaqhip_decompress_device that is compared on the device.  The shapes are the smallest at which the gather and the group
runs can go wrong: every method family in one call with the groups interleaved, blocks of 0 and 1 bytes and around the
packing kernel's 64 KiB piece, unaligned input and output, several batches, bodies from the retry slots, an output that
is too small."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util
from zpaqsharp_amd import _lib, method, synth

pytestmark = pytest.mark.gpu

OUT_FULL = -20
GUARD = 0xC3
FRONT = 64                     # guard bytes in front of d_out
GAP_SLICE = 12288              # ZH_GAP_SLICE (zh_analyze.h)


def _cat(blocks):
    offs = np.zeros(len(blocks) + 1, np.uint64)
    offs[1:] = np.cumsum([len(b) for b in blocks], dtype=np.uint64)
    return np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy(), offs


def host_reference(ctx, strings, method_of, blocks, names, *, kernel, flags=7):
    """What the contract names: per method, zpaqhip_compress_method_blocks (host form) on the blocks that take it; every
    block's bytes by block_off, in input order."""
    L = _lib.load()
    parts = [None] * len(blocks)
    for g, m in enumerate(strings):
        ids = [i for i, w in enumerate(method_of) if w == g]
        if not ids:
            continue
        mod = method.model_of(m)[0]
        hdr = np.frombuffer(mod.header, np.uint8)
        pc = np.frombuffer(mod.pcomp, np.uint8) if mod.pcomp else None
        buf, offs = _cat([blocks[i] for i in ids])
        cn = (C.c_char_p * len(ids))(*[names[i].encode() for i in ids])
        cap = 2 * int(offs[-1]) + len(ids) * 8192 + 4096
        out = np.zeros(cap, np.uint8)
        boffs = np.zeros(len(ids) + 1, np.uint64)
        o = _lib.CompressOpts()
        o.struct_size, o.flags, o.kernel = C.sizeof(_lib.CompressOpts), flags, kernel
        err, got = _lib.Err(), C.c_size_t(0)
        rc = L.zpaqhip_compress_method_blocks(ctx._h, (C.c_int32 * 9)(*method.parse_args(m)[1]), hdr.ctypes.data, hdr.size,
                                              pc.ctypes.data if pc is not None else None, pc.size if pc is not None else 0,
                                              buf.ctypes.data, offs.ctypes.data, len(ids), cn, out.ctypes.data, cap, C.byref(got),
                                              boffs.ctypes.data, C.byref(o), C.byref(err))
        assert rc == 0, (m, rc, err.msg)
        for j, i in enumerate(ids):
            parts[i] = out[int(boffs[j]):int(boffs[j + 1])].tobytes()
    return parts


def to_device(blocks, shift, tail=32):
    """The blocks back to back `shift` bytes into a tensor (torch allocations are 512-byte aligned): (tensor, offsets)."""
    buf, offs = _cat(blocks)
    n = int(offs[-1])
    t = torch.full((shift + n + tail,), 0x5A, dtype=torch.uint8, device="cuda")
    t[shift:shift + n].copy_(torch.from_numpy(buf[:n]))
    return t, offs


def run_mixed(ctx, strings, method_of, blocks, names, *, out_cap, in_shift=1, out_shift=0, side=None, kernel=2, **kw):
    d_in, in_off = to_device(blocks, in_shift)
    d_out = torch.full((FRONT + out_shift + out_cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
    if side is not None:
        side.wait_stream(torch.cuda.current_stream())              # the buffers were filled there
    rc, need, off = ctx.compress_mixed_device(strings, method_of, d_in.data_ptr() + in_shift, in_off,
                                              d_out.data_ptr() + FRONT + out_shift, out_cap, filenames=names, kernel=kernel, bwt=True,
                                              hip_stream=side.cuda_stream if side is not None else 0, **kw)
    st = ctx.stats()
    torch.cuda.synchronize()
    return rc, need, off, d_out, FRONT + out_shift, st, (d_in, in_shift)


def round_trip_on_device(ctx, d_out, at, n, d_in, in_shift, total):
    back = torch.full((total + 64,), 0x11, dtype=torch.uint8, device="cuda")
    stream = d_out[at:at + n].clone()                              # (decompress_device asks for 4-byte alignment)
    rc, got = ctx.decompress_device(stream.data_ptr(), n, back.data_ptr(), total, verify_sha1=True)
    assert (rc, got) == (0, total)
    assert bool(torch.equal(back[:total], d_in[in_shift:in_shift + total]))      # one scalar comes to the host


# ---- mixed methods -------------------------------------------------------------------------------------------------------
STRINGS = ["x0,0", "x0,1,4,0,3,16", "x0,2,12,0,7,16", "x0,3ci1", "x0,0ci1,1,1,1,2am", "x0,5,4,0,3,16"]     # [2] is used by no block
SIZES = (0, 1, 255, 4097, 65536, 65537)
WHICH = [0, 1, 3, 4, 5, 1, 0, 4, 3, 5, 0, 3]           # interleaved: every used method has blocks apart from each other
BLOCK_SIZES = [65537, 4097, 65536, 255, 65537, 0, 1, 4097, 0, 255, 65536, 1]


@pytest.fixture(scope="module")
def mixed_case(ctx):
    blocks = [synth.plain("X" if WHICH[i] == 5 else "TR"[i % 2], i, n).tobytes() for i, n in enumerate(BLOCK_SIZES)]
    names = ["abcdefg"[:i % 8] for i in range(len(blocks))]
    assert set(BLOCK_SIZES) == set(SIZES) and 2 not in WHICH
    want = host_reference(ctx, STRINGS, WHICH, blocks, names, kernel=2)
    return blocks, names, want


@pytest.mark.parametrize("in_shift, out_shift, side", [(1, 0, False), (13, 3, True), (1, 3, True), (13, 0, False)])
def test_mixed_methods_against_the_host_form(ctx, mixed_case, in_shift, out_shift, side):
    blocks, names, want = mixed_case
    stream, total = b"".join(want), sum(len(b) for b in blocks)
    s = torch.cuda.Stream() if side else None
    rc, need, off, d_out, at, st, (d_in, _) = run_mixed(ctx, STRINGS, WHICH, blocks, names, out_cap=len(stream) + 100,
                                                        in_shift=in_shift, out_shift=out_shift, side=s)
    got = d_out.cpu().numpy()
    print(f"rc {rc} needed {need} / {len(stream)} launches {st.launches} kernel_ms {st.kernel_ms:.3f} gather_us {st.e8_wave_segs} "
          f"scratch {st.model_bytes}")
    assert rc == 0 and need == len(stream)
    assert off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    assert got[at:at + need].tobytes() == stream
    assert (got[:at] == GUARD).all() and (got[at + need:] == GUARD).all(), "written outside d_out[0, *out_len)"
    assert st.blocks == len(blocks) and st.in_bytes == total and st.out_bytes == need and st.kernel_kind == 3
    assert st.model_bytes >= need and st.launches > 5 and st.h2d_ms == 0 and st.d2h_ms == 0
    round_trip_on_device(ctx, d_out, at, need, d_in, in_shift, total)


def test_one_method_is_the_method_form(ctx):
    m = "x0,1,4,0,3,16,1c0,0,511i2"
    blocks = [util.text(n, seed=n) for n in (3000, 0, 1, 70000)]
    names = ["a", "", "ccc", "dd"]
    total = sum(len(b) for b in blocks)
    d_in, in_off = to_device(blocks, 3)
    cap = 2 * total + 40000
    d_a = torch.full((cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
    ra = ctx.compress_method_device(m, d_in.data_ptr() + 3, in_off, d_a.data_ptr(), cap, filenames=names, kernel=2)
    rb = run_mixed(ctx, [m], [0] * 4, blocks, names, out_cap=cap, in_shift=3)
    assert ra[0] == 0 and rb[0] == 0 and ra[1] == rb[1] and np.array_equal(ra[2], rb[2])
    assert bool(torch.equal(d_a, rb[3][FRONT:]))


# ---- short output --------------------------------------------------------------------------------------------------------
def test_output_too_small(ctx, mixed_case):
    blocks, names, want = mixed_case
    stream = b"".join(want)
    off = np.cumsum([0] + [len(w) for w in want]).tolist()
    assert off[7] - off[6] > 2
    for cap in (0, (off[6] + off[7]) // 2, len(stream) - 1):       # nothing; ends inside block 6; one byte short
        rc, need, o, d_out, at, st, _ = run_mixed(ctx, STRINGS, WHICH, blocks, names, out_cap=cap, out_shift=3)
        got = d_out.cpu().numpy()
        fit = sum(1 for i in range(len(blocks)) if off[i + 1] <= cap)              # the blocks that fit in whole: the first ones
        print(f"cap {cap}: rc {rc} needed {need} blocks that fit {fit}")
        assert rc == OUT_FULL and need == len(stream) and o.tolist() == off
        assert got[at:at + off[fit]].tobytes() == stream[:off[fit]]
        # everything at or past out_cap, and every byte of a block that was left out, is still the fill
        assert (got[at + off[fit]:] == GUARD).all() and (got[:at] == GUARD).all()


# ---- several batches, the retry slots ------------------------------------------------------------------------------------
def test_batches_and_retry_slots_give_the_same_bytes(ctx):
    rng = np.random.default_rng(9)
    strings = ["x0,3ci1", "x0,0ci1,1,1,1,2am", "x0,1,4,0,3,16"]
    blocks = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (3000, 2999, 257, 3001, 1, 3000, 0, 2000)]
    which = [0, 1, 2, 1, 0, 0, 1, 2]
    names = ["n%d" % i for i in range(len(blocks))]
    cap = 2 * sum(len(b) for b in blocks) + 80000
    runs = [run_mixed(ctx, strings, which, blocks, names, out_cap=cap, **kw) for kw in ({}, {"batch_blocks": 2}, {"slot_bytes": 64})]
    want = b"".join(host_reference(ctx, strings, which, blocks, names, kernel=2))
    for rc, need, off, d_out, at, st, _ in runs:
        assert rc == 0 and need == len(want) and np.array_equal(off, runs[0][2])
        assert bool(torch.equal(d_out, runs[0][3]))
    assert runs[0][3].cpu().numpy()[FRONT:FRONT + len(want)].tobytes() == want
    assert runs[1][5].launches > runs[0][5].launches and runs[2][5].launches > runs[0][5].launches


# ---- the gap histogram ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gap_case(ctx):
    sizes = (0, 1, 4095, 4096, 4097, GAP_SLICE - 1, GAP_SLICE + 1, 64 * GAP_SLICE + 1)
    rng = np.random.default_rng(5)
    blocks = []
    for kind in range(3):
        for n in sizes:
            i = np.arange(n)
            a = (i % 7 if kind == 0 else (i % 300) & 255 if kind == 1 else rng.integers(0, 256, n)).astype(np.uint8)
            blocks.append(a.tobytes())
    return blocks, ctx.gap_hist_blocks(blocks)


@pytest.mark.parametrize("shift", [0, 1, 8, 15])
def test_gap_histogram_of_device_blocks(ctx, gap_case, shift):
    blocks, want = gap_case
    d_in, in_off = to_device(blocks, shift, tail=0)                # the last block ends at the very end of its tensor
    assert d_in.numel() == shift + int(in_off[-1])
    got = ctx.gap_hist_blocks_device(d_in.data_ptr() + shift, in_off)
    st = ctx.stats()
    assert got.shape == want.shape and np.array_equal(got, want)
    assert st.h2d_ms == 0 and st.blocks == len(blocks) and st.in_bytes == int(in_off[-1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert np.array_equal(ctx.gap_hist_blocks_device(d_in.data_ptr() + shift, in_off, hip_stream=side.cuda_stream), want)


# ---- levels --------------------------------------------------------------------------------------------------------------
def _repetitive(n, seed):
    line = util.text(200, seed=seed)
    return (line * (n // len(line) + 1))[:n]


def _level_blocks(level):
    if level == "5":
        i = np.arange(16384)
        noise = np.random.default_rng(6).integers(0, 256, 16384, dtype=np.uint8)
        return [(i % 7 * 31).astype(np.uint8).tobytes(), (i % 12 * 17).astype(np.uint8).tobytes(), noise.tobytes()]
    # 1 MiB - 4095 bytes take x1, 1 MiB - 4096 take x0: two method strings, two groups
    return [_repetitive((1 << 20) - 4095, 1), _repetitive(3000, 2), _repetitive((1 << 20) - 4096, 3)]


@pytest.mark.parametrize("level", ["1", "2,128,0", "3,200,1", "4,128,2", "5"])
def test_levels_against_compress_level(ctx, level):
    blocks = _level_blocks(level)
    names = ["f%d" % i for i in range(len(blocks))]
    want = ctx.compress_level(level, blocks, filenames=names)
    want_methods = list(ctx.level_methods)
    assert len(set(want_methods)) >= 2, want_methods               # more than one group, or the case shows nothing
    total = sum(len(b) for b in blocks)
    d_in, in_off = to_device(blocks, 5)
    cap = len(want) + 1000
    d_out = torch.full((FRONT + cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
    rc, need, off = ctx.compress_level_device(level, d_in.data_ptr() + 5, in_off, d_out.data_ptr() + FRONT, cap, filenames=names)
    st = ctx.stats()
    print(f"level {level}: {want_methods} needed {need} / {len(want)} kernel_ms {st.kernel_ms:.2f} gather_us {st.e8_wave_segs}")
    assert rc == 0 and need == len(want) and ctx.level_methods == want_methods
    assert set(ctx.level_ms) == {"analysis", "encode"}
    got = d_out.cpu().numpy()
    assert got[FRONT:FRONT + need].tobytes() == want
    assert (got[:FRONT] == GUARD).all() and (got[FRONT + need:] == GUARD).all()
    round_trip_on_device(ctx, d_out, FRONT, need, d_in, 5, total)
