"""The device forms of the compressing entry points (zpaqhip_compress_blocks_device, zpaqhip_compress_method_blocks_device;
Context.compress_blocks_device / compress_method_device) against the host forms on the same arguments: the same return
code, bytes needed, block offsets and bytes, with nothing written outside the blocks that fit, and a round trip through the
GPU decoders.  The shapes are the smallest at which the packing kernel (zh_frame.hip) can go wrong: every residue of the
head's length against the 256-aligned slots, an unaligned output and input, the store layout's chunk edges, bodies from
the retry slots, several batches, an output that is too small.  Everything here needs a few MiB of device memory; no case
skips."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util
from zpaqsharp_amd import _lib, e8e9, method, models, synth

pytestmark = pytest.mark.gpu

OUT_FULL = -20
GUARD = 0xC3
CHUNK = 65536                  # write_store_body's chunk (zh_frame_table.cpp)


def _cat(blocks):
    offs = np.zeros(len(blocks) + 1, np.uint64)
    offs[1:] = np.cumsum([len(b) for b in blocks], dtype=np.uint64)
    return np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy(), offs


def _opts(flags, kernel, batch_blocks, slot_bytes):
    o = _lib.CompressOpts()
    o.struct_size = C.sizeof(_lib.CompressOpts)
    o.flags, o.kernel, o.batch_blocks, o.slot_bytes = flags, kernel, batch_blocks, slot_bytes
    return o


def _host(ctx, header, pcomp, args, blocks, orig, names, o, out_cap):
    """The host form through the C ABI, into a buffer of out_cap bytes and a guard, all pre-filled: (rc, needed, offsets,
    buffer)."""
    L = _lib.load()
    cbuf, coffs = _cat(blocks)
    obuf, ooffs = _cat(orig) if orig is not None else (None, None)
    hdr, pc = np.frombuffer(header, np.uint8), np.frombuffer(pcomp, np.uint8) if pcomp else None
    cn = (C.c_char_p * max(1, len(blocks)))(*[f.encode() for f in names]) if names is not None else None
    out = np.full(out_cap + 64, GUARD, np.uint8)
    boffs = np.zeros(len(blocks) + 1, np.uint64)
    err, got = _lib.Err(), C.c_size_t(0)
    pcp, pcn = (pc.ctypes.data, pc.size) if pc is not None else (None, 0)
    if args is not None:
        rc = L.zpaqhip_compress_method_blocks(ctx._h, (C.c_int32 * 9)(*args), hdr.ctypes.data, hdr.size, pcp, pcn, cbuf.ctypes.data,
                                              coffs.ctypes.data, len(blocks), cn, out.ctypes.data, out_cap, C.byref(got),
                                              boffs.ctypes.data, C.byref(o), C.byref(err))
    else:
        rc = L.zpaqhip_compress_blocks(ctx._h, hdr.ctypes.data, hdr.size, pcp, pcn, cbuf.ctypes.data, coffs.ctypes.data, len(blocks),
                                       obuf.ctypes.data if obuf is not None else None, ooffs.ctypes.data if ooffs is not None else None,
                                       cn, out.ctypes.data, out_cap, C.byref(got), boffs.ctypes.data, C.byref(o), C.byref(err))
    return rc, got.value, boffs, out


def _to_device(blocks, shift):
    """The blocks back to back `shift` bytes into a tensor (torch allocations are 512-byte aligned): (tensor, offsets)."""
    buf, offs = _cat(blocks)
    t = torch.full((shift + buf.size + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    t[shift:shift + buf.size].copy_(torch.from_numpy(buf))
    return t, offs


def pair(ctx, blocks, *, model=None, m=None, orig=None, names=None, sha1=True, tag=True, kernel=0, batch_blocks=0, slot_bytes=0,
         bwt=False, sa=False, ht=False, out_cap=None, shift=0, stream=None, round_trip=True):
    """Runs the host form and the device form on the same arguments and checks the device form against the host form;
    returns (rc, needed, offsets, stream bytes that were written, the two forms' statistics)."""
    if m is not None:
        args = method.parse_args(m)[1]
        mod = method.model_of(m)[0]
    else:
        args, mod = None, models.get(model) if isinstance(model, str) else model
    header, pcomp = mod.header, mod.pcomp or b""
    flags = (1 if sha1 else 0) | (2 if tag else 0) | (4 if bwt else 0) | (8 if sa else 0) | (16 if ht else 0)
    total = sum(len(b) for b in blocks)
    if out_cap is None:
        out_cap = 2 * total + len(blocks) * (len(header) + 2 * len(pcomp) + 4096) + 4096
    o = _opts(flags, kernel, batch_blocks, slot_bytes)
    h_rc, h_need, h_off, h_out = _host(ctx, header, pcomp, args, blocks, orig, names, o, out_cap)
    h_st = ctx.stats()
    assert h_rc in (0, OUT_FULL)

    d_in, in_off = _to_device(blocks, shift)
    d_orig, orig_off = _to_device(orig, shift + 1) if orig is not None else (None, None)
    d_out = torch.full((shift + out_cap + 64,), GUARD, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())            # the buffers were filled there
    hs = stream.cuda_stream if stream is not None else 0
    if m is not None:
        rc, need, off = ctx.compress_method_device(m, d_in.data_ptr() + shift, in_off, d_out.data_ptr() + shift, out_cap,
                                                   filenames=names, sha1=sha1, tag=tag, kernel=kernel, batch_blocks=batch_blocks,
                                                   slot_bytes=slot_bytes, bwt=bwt, sa=sa, ht=ht, hip_stream=hs)
    else:
        rc, need, off = ctx.compress_blocks_device(mod, d_in.data_ptr() + shift, in_off, d_out.data_ptr() + shift, out_cap,
                                                   d_orig=d_orig.data_ptr() + shift + 1 if d_orig is not None else 0,
                                                   orig_off=orig_off, filenames=names, sha1=sha1, tag=tag, kernel=kernel,
                                                   batch_blocks=batch_blocks, slot_bytes=slot_bytes, hip_stream=hs)
    d_st = ctx.stats()
    got = d_out.cpu().numpy()
    print(f"rc {rc} / {h_rc}  needed {need} / {h_need}  launches {d_st.launches} / {h_st.launches}")
    assert (rc, need) == (h_rc, h_need) and np.array_equal(off, h_off)
    assert (got[:shift] == GUARD).all(), "bytes in front of d_out changed"
    # the host form's buffer holds the blocks that fit and the fill everywhere else: the device form's is the same, guard included
    assert np.array_equal(got[shift:], h_out), "the device form's output differs from the host form's"
    fit = int(sum(1 for i in range(len(blocks)) if off[i + 1] <= out_cap))
    end = int(off[fit])
    assert (got[shift + end:] == GUARD).all(), "bytes behind the last block that fits changed"
    assert (rc == 0) == (need <= out_cap) and (rc != 0 or end == need)
    for f in ("blocks", "in_bytes", "out_bytes", "kernel_kind", "concurrent"):
        assert getattr(d_st, f) == getattr(h_st, f), f
    assert d_st.launches >= h_st.launches
    stream_bytes = got[shift:shift + end].tobytes()
    if round_trip and rc == 0:
        plain = b"".join(orig if orig is not None else blocks)
        assert ctx.decompress(stream_bytes, verify_sha1=sha1).tobytes() == plain
    return rc, need, off, stream_bytes, (h_st, d_st)


SWEEP_SIZES = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 19999, 20000, 20001, 20480)


def _sweep_blocks():
    return [synth.plain("TXR"[i % 3], i, n).tobytes() for i, n in enumerate(SWEEP_SIZES)]


@pytest.mark.parametrize("shift", [0, 1, 3, 13])
@pytest.mark.parametrize("sha1, tag", [(True, True), (False, True), (True, False), (False, False)])
def test_modelled_blocks_alignment_sweep(ctx, shift, sha1, tag):
    blocks = _sweep_blocks()
    names = ["abcdefg"[:i % 8] for i in range(len(blocks))]       # head lengths: every residue mod 16 against the 256-aligned slots
    st = pair(ctx, blocks, model="min", names=names, sha1=sha1, tag=tag, kernel=2, shift=shift)[4][1]
    assert st.kernel_kind == 3


@pytest.mark.parametrize("model, kernel, kind", [("l1", 0, 2), ("min", 1, 1)])
def test_the_same_packing_behind_every_encoder(ctx, model, kernel, kind):
    blocks = [b"", b"q", util.text(3001, seed=2), synth.plain("R", 4, 700).tobytes()]
    st = pair(ctx, blocks, model=model, kernel=kernel, names=["", "n", "nn", "nnn"], shift=3)[4][1]
    assert st.kernel_kind == kind


@pytest.mark.parametrize("m", ["x0,1,4,0,3,16", "x0,5,4,0,3,16", "x0,2,12,0,7,16", "x0,6,5,0,3,16"])
def test_store_layout_chunk_edges(ctx, m):
    assert method.model_of(m)[0].header[6] == 0           # no model: the store layout
    data = synth.plain("X", 5, 2 * CHUNK + 5).tobytes()
    noise = np.random.default_rng(11).integers(0, 256, 2 * CHUNK + 5, dtype=np.uint8).tobytes()    # its codes fill three chunks
    blocks = [data[:n] for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1)] + [noise]
    for tag in (True, False):
        pair(ctx, blocks, m=m, names=["s" * i for i in range(len(blocks))], tag=tag, shift=1 if tag else 0)


def test_store_layout_at_exact_chunk_edges_with_level_0(ctx):
    # level 0 without a model stores the plaintext itself (selector 0 in front): the decoded stream is 1 + n bytes, so the
    # chunk's edges are hit exactly: one chunk minus 1, one chunk, one chunk plus 1, two chunks plus 5
    data = synth.plain("T", 3, 2 * CHUNK + 8).tobytes()
    blocks = [data[:n] for n in (0, 1, CHUNK - 2, CHUNK - 1, CHUNK, 2 * CHUNK + 4)]
    for m in ("x0,0", "x0,4"):
        assert method.model_of(m)[0].header[6] == 0
        for shift in (0, 13):
            pair(ctx, blocks, m=m, names=["abcdefg"[:i] for i in range(len(blocks))], shift=shift)


@pytest.mark.parametrize("m, kw", [("x0,2,12,0,7,16,1c0,0,511i2", {}), ("x0,3ci1", {"bwt": True}),
                                   ("x0,1,4,0,7,21,1ci1", {"sa": True}), ("x0,1,4,0,3,20ci1", {"ht": True})])
def test_modelled_methods_take_device_input(ctx, m, kw):
    blocks = [util.text(8192, seed=21), util.x86ish(8192)]
    pair(ctx, blocks, m=m, names=["a", "bb"], kernel=2, shift=3, **kw)


def test_bodies_from_the_retry_slots_and_the_first_slots_in_one_batch(ctx):
    rng = np.random.default_rng(3)
    blocks = [b"", b"a", util.text(5000, seed=3), rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), b"zz",
              util.text(1000, seed=4), rng.integers(0, 256, 257, dtype=np.uint8).tobytes()]
    names = ["abcdefg"[:i] for i in range(len(blocks))]
    for model, kernel in (("min", 2), ("l1", 0)):
        plain_run = pair(ctx, blocks, model=model, kernel=kernel, names=names, shift=1)
        retried = pair(ctx, blocks, model=model, kernel=kernel, names=names, shift=1, slot_bytes=16)
        assert retried[3] == plain_run[3]
        # the re-encoding launch of the overflowed blocks ran, in both forms; the empty block's slot was large enough
        assert retried[4][0].launches == plain_run[4][0].launches + 1
        assert retried[4][1].launches == plain_run[4][1].launches + 1


def test_block_offsets_continue_across_batches(ctx):
    blocks = [synth.plain("TXR"[i % 3], i, 500 + 333 * i).tobytes() for i in range(12)]
    one = pair(ctx, blocks, model="min", kernel=2, shift=3)
    cut = pair(ctx, blocks, model="min", kernel=2, shift=3, batch_blocks=5)
    assert cut[3] == one[3] and np.array_equal(cut[2], one[2])
    assert cut[4][1].launches > one[4][1].launches        # three batches: three launches of the encoder and of the packing kernel
    st = pair(ctx, blocks, m="x0,1,4,0,3,16", batch_blocks=5, shift=1)
    assert st[3] == pair(ctx, blocks, m="x0,1,4,0,3,16", shift=1)[3]


@pytest.mark.parametrize("store", [False, True])
def test_output_too_small(ctx, store):
    blocks = [synth.plain("TXR"[i % 3], i, 900 + 411 * i).tobytes() for i in range(7)]
    kw = dict(m="x0,1,4,0,3,16") if store else dict(model="min", kernel=2)
    rc, need, off, full, _ = pair(ctx, blocks, shift=3, **kw)
    assert rc == 0 and need == len(full)
    for cap, fit in ((need - 1, 6), (int(off[3]), 3), (int(off[3]) - 1, 2), (0, 0)):
        rc, n, o, part, _ = pair(ctx, blocks, shift=3, out_cap=cap, batch_blocks=4, **kw)
        assert rc == OUT_FULL and n == need and np.array_equal(o, off)
        assert part == full[:int(off[fit])]


def test_d_orig_gives_the_size_comment_and_the_digest(ctx):
    plain = [util.x86ish(6000), util.text(3000, seed=8), b"", util.x86ish(257)]
    coded = [e8e9.forward(np.frombuffer(b, np.uint8)).tobytes() for b in plain]
    assert coded[0] != plain[0]
    rc, _, _, got, _ = pair(ctx, coded, model="l1+e8e9", orig=plain, names=["a", "", "ccc", "dd"], shift=5)
    assert rc == 0 and got == ctx.compress_blocks("l1+e8e9", plain, filenames=["a", "", "ccc", "dd"])


def test_a_callers_stream(ctx):
    s = torch.cuda.Stream()
    blocks = [util.text(7000, seed=1), b"x", synth.plain("R", 2, 1234).tobytes()]
    a = pair(ctx, blocks, model="min", kernel=2, shift=3, stream=s)
    b = pair(ctx, blocks, m="x0,2,12,0,7,16", shift=3, stream=s)
    torch.cuda.synchronize()
    assert a[3] == pair(ctx, blocks, model="min", kernel=2)[3] and b[3] == pair(ctx, blocks, m="x0,2,12,0,7,16")[3]
