"""zpaqhip_compress_solid_blocks[_device] without a GPU: the declarations and their ctypes mirrors, the argument errors that
come back before the device is touched (reached with a context handle that is not NULL and never read, as in
tests/test_compress_mixed.py), the Python wrappers' refusals, and compress_files' packing rule."""
import ctypes as C
import os

import numpy as np
import pytest

from zpaqsharp_amd import _lib, api, compressor, method, models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -25
NAMES = ("zpaqhip_compress_solid_blocks", "zpaqhip_compress_solid_blocks_device")
SOME = 0x10000                     # stands for a device address: never dereferenced on these paths


def test_exports_and_declarations():
    L = _lib.load()
    text = open(os.path.join(ROOT, "include", "zpaqhip.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
        decl = text[text.index("int " + name + "("):]
        decl = decl[:decl.index(";")]
        args = [a.strip() for a in decl[decl.index("(") + 1:].rstrip(")").split(",")]
        assert len(args) == len(getattr(L, name).argtypes)
        assert args[7] == "const uint64_t *seg_first" and args[8] == "size_t n_blocks"
    host, dev = L.zpaqhip_compress_solid_blocks.argtypes, L.zpaqhip_compress_solid_blocks_device.argtypes
    assert len(host) == len(L.zpaqhip_compress_blocks.argtypes) + 1 and len(dev) == len(host) + 1
    assert dev[-2] is C.c_void_p and dev[-1] is host[-1]


class _Fake:
    """A context handle that is not NULL: the argument checks return before anything reads it."""

    def __init__(self):
        self.buf = (C.c_uint8 * 4096)()
        self.h = C.addressof(self.buf)


def _solid(h, seg_first, in_off, *, model="min", orig_off=None, flags=3, enc_waves=0, device=False, out=SOME, out_cap=16, inp=SOME):
    L = _lib.load()
    m = models.get(model) if isinstance(model, str) else model
    hdr = np.frombuffer(m if isinstance(m, bytes) else m.header, np.uint8)
    sf, off = np.asarray(seg_first, np.uint64), np.asarray(in_off, np.uint64)
    oo = np.asarray(orig_off, np.uint64) if orig_off is not None else None
    o = _lib.CompressOpts()
    o.struct_size, o.flags, o.enc_waves = C.sizeof(_lib.CompressOpts), flags, enc_waves
    err, got = _lib.Err(), C.c_size_t(77)
    err.block = err.segment = -7
    args = [h, hdr.ctypes.data, hdr.size, None, 0, inp, off.ctypes.data, sf.ctypes.data, sf.size - 1, SOME if oo is not None else None,
            oo.ctypes.data if oo is not None else None, None, out, out_cap, C.byref(got), None, C.byref(o)]
    if device:
        rc = L.zpaqhip_compress_solid_blocks_device(*args, None, C.byref(err))
    else:
        rc = L.zpaqhip_compress_solid_blocks(*args, C.byref(err))
    return rc, err


@pytest.mark.parametrize("device", [False, True])
def test_argument_errors_come_back_before_the_device_is_touched(device):
    f = _Fake()
    kw = {"device": device}
    assert _solid(None, [0, 1], [0, 4], **kw)[0] == E_ARG                          # no context
    assert _solid(f.h, [0, 1], [0, 4], out=None, **kw)[0] == E_ARG                 # no output buffer with a capacity
    # a block without a segment: the second of three
    rc, err = _solid(f.h, [0, 2, 2, 3], [0, 4, 8, 12], **kw)
    assert rc == E_ARG and err.block == 1 and b"at least one segment" in err.msg
    # seg_first that decreases, and one that does not start at 0
    rc, err = _solid(f.h, [0, 2, 1, 3], [0, 4, 8, 12], **kw)
    assert rc == E_ARG and err.block == 1 and b"decrease" in err.msg
    rc, err = _solid(f.h, [1, 2], [0, 4, 8], **kw)
    assert rc == E_ARG and err.block == 0
    # offsets that decrease: the block and the segment within it
    rc, err = _solid(f.h, [0, 1, 4], [0, 4, 8, 6, 12], **kw)
    assert rc == E_ARG and err.block == 1 and err.segment == 1 and b"decrease" in err.msg
    rc, err = _solid(f.h, [0, 1, 4], [0, 4, 8, 10, 12], orig_off=[0, 9, 9, 8, 20], **kw)
    assert rc == E_ARG and err.block == 1 and err.segment == 1
    # n == 0 headers: modelled blocks only, as zpaqhip_compress_blocks
    rc, err = _solid(f.h, [0, 1], [0, 4], model=method.model_of("x0,0")[0].header, **kw)
    assert rc == E_ARG and b"modelled" in err.msg
    # flags: verify (bit 5) and the method opt-ins (bits 2 to 4)
    for bit in (4, 8, 16, 32):
        rc, err = _solid(f.h, [0, 1], [0, 4], flags=3 | bit, **kw)
        assert rc == E_ARG and b"flags" in err.msg, bit
    assert _solid(f.h, [0, 1], [0, 4], enc_waves=5, **kw)[0] == E_ARG              # as zpaqhip_compress_blocks
    assert _solid(f.h, [0, 1], [0, 4], inp=None, **kw)[0] == E_ARG                 # bytes to code, but no input


def test_python_wrappers_refuse_before_the_device_is_touched():
    class NoDevice(api.Context):
        def __init__(self):                                # no zpaqhip_ctx_create
            self._L, self._h = _lib.load(), None

    ctx = NoDevice()
    with pytest.raises(ValueError):
        ctx.compress_solid("min", [[b"a"], []])                                    # a block without a segment
    with pytest.raises(ValueError):
        ctx.compress_solid("min", [b"ab", b"cd"])                                  # blocks are lists of segments
    with pytest.raises(ValueError):
        ctx.compress_solid("min", [[b"a", b"b"]], filenames=[["x"]])
    with pytest.raises(ValueError):
        ctx.compress_solid("min", [[b"a", b"b"]], pre=[[b"a"], [b"b"]])            # pre has the shape of blocks
    with pytest.raises(ValueError):
        ctx.compress_solid("min+lz77", [[b"a", b"b"]])                             # a post-processor needs pre=
    with pytest.raises(ValueError):
        ctx.compress_solid_device("min", SOME, [0, 1, 2], [0, 3], SOME, 100)       # in_off: one per segment and one more
    with pytest.raises(ValueError):
        ctx.compress_solid_device("min", SOME, [0, 1, 2], [0, 2], SOME, 100, filenames=["a"])
    # what passes the wrappers reaches the library, whose own NULL-context error comes back
    with pytest.raises(api.ZpaqError) as e:
        ctx.compress_solid("min", [[b"a", b""], [b"b"]], filenames=[["x", "y"], ["z"]])
    assert e.value.code == E_ARG
    with pytest.raises(api.ZpaqError) as e:
        ctx.compress_solid_device("min", SOME, [0, 1, 2], [0, 2], SOME, 100, filenames=["a", "b"])
    assert e.value.code == E_ARG


def test_pack_files_rule():
    pack = compressor.pack_files
    assert pack([], 100) == []
    assert pack([0], 100) == [[0]]
    assert pack([0, 0, 0], 1) == [[0, 1, 2]]                                       # empty files cost nothing
    assert pack([40, 60, 1, 99, 100, 101, 5], 100) == [[0, 1], [2, 3], [4], [5], [6]]
    assert pack([101, 0, 100, 0], 100) == [[0], [1, 2, 3]]                         # a file above the size gets a block of its own
    assert pack([50] * 5, 100) == [[0, 1], [2, 3], [4]]
    assert pack([200, 300], 100) == [[0], [1]]
    with pytest.raises(ValueError):
        pack([1], 0)
    # every file once, in order, no empty block, no block above the size unless it is a single file
    rng = np.random.default_rng(3)
    for _ in range(50):
        sizes = [int(x) for x in rng.integers(0, 3001, int(rng.integers(1, 60)))]
        bs = int(rng.integers(1, 5000))
        got = pack(sizes, bs)
        assert [i for g in got for i in g] == list(range(len(sizes))) and all(got)
        for k, g in enumerate(got):
            total = sum(sizes[i] for i in g)
            assert total <= bs or len(g) == 1
            if k + 1 < len(got):                                                   # greedy: the next file would not have fitted
                assert total + sizes[got[k + 1][0]] > bs
