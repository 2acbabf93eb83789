"""Thin Python layer over the C ABI (include/zpaqhip.h): scan, Context, errors.

Everything that decodes goes through libzpaqhip.so and therefore through the
HIP kernels; nothing here implements or falls back to a CPU decoder.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import Block, CompressOpts, Err, Opts, SegResult, Segment, Stats, UINT64_MAX, VerifyResult


class ZpaqError(RuntimeError):
    """Raised for any non-zero zpaqhip_status; `.code`, `.block`, `.segment` say where."""

    def __init__(self, code: int, block: int = -1, segment: int = -1, msg: str = ""):
        self.code, self.block, self.segment = code, block, segment
        super().__init__(msg or _lib.load().zpaqhip_strerror(code).decode())


def _raise(err: Err, rc: int):
    raise ZpaqError(rc, err.block, err.segment, err.msg.decode(errors="replace"))


def _as_u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        a = data.view(np.uint8).reshape(-1)
        return a if a.flags.c_contiguous else np.ascontiguousarray(a)
    return np.frombuffer(bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)


def _cat(parts):
    """Blocks back to back, and their offsets (len(parts) + 1 of them)."""
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64) if parts else []
    buf = np.concatenate(parts) if parts and offs[-1] else np.zeros(1, np.uint8)
    return np.ascontiguousarray(buf), offs


def version() -> int:
    return _lib.load().zpaqhip_version()


def device_count() -> int:
    return _lib.load().zpaqhip_device_count()


def strerror(code: int) -> str:
    return _lib.load().zpaqhip_strerror(code).decode()


@dataclass
class ScanResult:
    blocks: "C.Array[Block]"
    segments: "C.Array[Segment]"

    @property
    def n_blocks(self) -> int:
        return len(self.blocks)

    @property
    def n_segments(self) -> int:
        return len(self.segments)


def scan(stream, partial: bool = False):
    """Host-side framing scan (Decompresser.findBlock/findFilename/readComment/
    readSegmentEnd, Decompresser.cs:29-108,163-194) → block and segment tables.
    partial=True: a framing error does not raise; the blocks parsed before the damage are returned together with
    the error, (ScanResult, ZpaqError | None) — the reference's Decompresser delivers those blocks too."""
    L = _lib.load()
    a = _as_u8(stream)
    nb, ns, err = C.c_size_t(0), C.c_size_t(0), Err()
    rc = L.zpaqhip_scan(a.ctypes.data, a.size, None, 0, C.byref(nb), None, 0, C.byref(ns), C.byref(err))
    if rc and not partial:
        _raise(err, rc)
    blocks = (Block * max(1, nb.value))()
    segs = (Segment * max(1, ns.value))()
    rc = L.zpaqhip_scan(a.ctypes.data, a.size, blocks, nb.value, C.byref(nb), segs, ns.value, C.byref(ns), C.byref(err))
    if rc and not partial:
        _raise(err, rc)
    res = ScanResult((Block * nb.value).from_buffer(blocks) if nb.value else (Block * 0)(),
                     (Segment * ns.value).from_buffer(segs) if ns.value else (Segment * 0)())
    if partial:
        return res, (ZpaqError(rc, err.block, err.segment, err.msg.decode(errors="replace")) if rc else None)
    return res


def block_costs(stream, sc: "ScanResult") -> np.ndarray:
    """zpaqhip_block_costs: estimated decode cost per block (plaintext bytes x cycles per byte of the block's
    kernel), the weight of every multi-GPU plan (multigpu.py, zpaqhip_decompress_multi).  Host-side."""
    L = _lib.load()
    a = _as_u8(stream)
    cost = np.zeros(max(1, sc.n_blocks), np.uint64)
    err = Err()
    rc = L.zpaqhip_block_costs(a.ctypes.data, a.size, sc.blocks, sc.n_blocks, sc.segments, sc.n_segments, cost.ctypes.data, C.byref(err))
    if rc:
        _raise(err, rc)
    return cost[:sc.n_blocks]


def decompress_multi(devices: Sequence[int], stream, out_cap: Optional[int] = None, per_device: Optional[list] = None,
                     partial: bool = False, **opt):
    """zpaqhip_decompress_multi(_stats): LibZPAQ.decompress over several GPUs of one node (one context + host thread
    per entry of `devices`; an entry may repeat), the threads pulling chunks of `queue_blocks` blocks from one
    cost-ordered work queue; plaintext in stream order.  per_device: a list that receives one Stats per device.
    partial=True: a damaged block does not raise; returns (plaintext before it, ZpaqError | None)."""
    L = _lib.load()
    a = _as_u8(stream)
    o = make_opts(**opt)
    err, n = Err(), C.c_size_t(0)
    devs = (C.c_int * len(devices))(*devices)
    if out_cap is None:
        sc = scan(a, partial=True)[0]
        out_cap = 0
        for b in sc.blocks:
            coded = sum(int(sc.segments[b.first_seg + i].data_len) for i in range(b.n_seg))
            out_cap += int(b.usize_hint) if b.usize_hint != UINT64_MAX and b.usize_hint <= 1 << 40 else 8 * coded + (64 << 10)
    st = (Stats * len(devices))()
    for _ in range(2):
        out = np.empty(max(1, out_cap), np.uint8)
        rc = L.zpaqhip_decompress_multi_stats(devs, len(devices), a.ctypes.data, a.size, out.ctypes.data, out_cap, C.byref(n),
                                              C.byref(o), st, C.byref(err))
        if not (rc == -20 and n.value > out_cap):
            break
        out_cap = n.value
    if per_device is not None:
        per_device[:] = [Stats.from_buffer_copy(bytes(x)) for x in st]
    if partial:
        e = ZpaqError(rc, err.block, err.segment, err.msg.decode(errors="replace")) if rc else None
        return out[:min(n.value, out_cap)], e
    if rc:
        _raise(err, rc)
    return out[:n.value]


def _chain_plan(fn, model):
    from . import models
    if isinstance(model, str):
        model = models.get(model)
    hdr = _as_u8(model if isinstance(model, (bytes, bytearray, np.ndarray)) else model.header)
    waves, lds, err = C.c_uint32(0), C.c_uint32(0), Err()
    rc = fn(hdr.ctypes.data, hdr.size, C.byref(waves), C.byref(lds), C.byref(err))
    if rc:
        _raise(err, rc)
    return waves.value, lds.value


def enc_chain_plan(model):
    """zpaqhip_enc_chain_plan: (waves, lds_bytes) of the lane-per-component encoder for a model (a models name, a zpaql.Model
    or header bytes): the most encoder waves one compute unit holds for it (1 to 4; what enc_waves=0 uses at most) and the
    LDS of such a workgroup, or (0, 0) for a model that encoder does not take.  Host-side."""
    return _chain_plan(_lib.load().zpaqhip_enc_chain_plan, model)


def dec_chain_plan(model):
    """zpaqhip_dec_chain_plan: (waves, lds_bytes) of the lane-per-component decoder (zh_chain.hip) for a model (a models
    name, a zpaql.Model or header bytes): the most decoder waves one compute unit holds for it (1 to 4; what dec_waves= uses
    at most) and the LDS of such a workgroup, or (0, 0) for a model that kernel does not take.  Host-side."""
    return _chain_plan(_lib.load().zpaqhip_dec_chain_plan, model)


def multi_trim() -> None:
    """zpaqhip_multi_trim: destroy the contexts decompress_multi keeps between calls."""
    _lib.load().zpaqhip_multi_trim()


# opts.kernel value (include/zpaqhip.h has the table): as 0, and the E8E9 forms of lazy2 / lzpre in unmodelled blocks stay on
# zh_store.hip instead of going to zh_generic.hip in a second launch
KERNEL_STORE_E8 = 10
# ... as 10, and zh_nibble.hip runs lzpre / bwtrle with E8E9 behind a model (levels 3 and 4 on executables) wave-wide, the
# end-of-segment E8E9 loop included; Context.stats().e8_wave_segs counts the segments
KERNEL_MODEL_E8 = 11


def compress_flags(sha1: bool = True, tag: bool = True, bwt: bool = False, sa: bool = False, ht: bool = False,
                   verify: bool = False) -> int:
    """zpaqhip_compress_opts.flags from the keywords of the compressing calls (bit 5, value 32: verify)."""
    return (1 if sha1 else 0) | (2 if tag else 0) | (4 if bwt else 0) | (8 if sa else 0) | (16 if ht else 0) | (32 if verify else 0)


def make_opts(verify_sha1: bool = False, max_concurrent: int = 0, kernel: int = 0, zpaql_budget: int = 0,
              batch_blocks: int = 0, queue_blocks: int = 0, dec_waves: int = 0) -> Opts:
    """zpaqhip_opts from keywords (include/zpaqhip.h describes each): every decode entry point below takes them as **opt.
    `dec_waves`: 2 to 4 puts up to that many decoder waves (blocks in flight) on a compute unit for blocks that zh_chain
    decodes with its run-time level walk (kernel=0's other models, every chain model with kernel=4), as many as the models'
    LDS plan (dec_chain_plan) allows; 0 or 1 one; more than 4 is 4.  The plaintext never depends on it.
    `kernel`: 0 auto; 1 everything on zh_generic; 2 / 6 single-CM blocks one / two per workgroup; 3 single-CM blocks on
    zh_chain; 4 every specialised model and stored blocks on zh_chain; 5 / 9 the older forms of min / mid / max;
    KERNEL_STORE_E8 (10) as 0, and unmodelled lazy2 / lzpre blocks with E8E9 stay on zh_store (one launch instead of two);
    KERNEL_MODEL_E8 (11) as 10, and the modelled lzpre / bwtrle blocks with E8E9 (methods x..,6,..c0,0,511.., x..,7ci1) have
    their post-processor run wave-wide on zh_nibble (stats().e8_wave_segs counts the segments); any other value as 0.  The
    plaintext never depends on it."""
    o = Opts()
    o.struct_size = C.sizeof(Opts)
    o.verify_sha1 = int(verify_sha1)
    o.max_concurrent = max_concurrent
    o.kernel = kernel
    o.zpaql_budget = zpaql_budget
    o.batch_blocks = batch_blocks
    o.queue_blocks = queue_blocks
    o.dec_waves = dec_waves
    return o


class Context:
    """One zpaqhip_ctx: bound to one GPU, not thread-safe (LICENSE:44-46 contract)."""

    def __init__(self, device: int = 0):
        self._L = _lib.load()
        h, err = C.c_void_p(), Err()
        rc = self._L.zpaqhip_ctx_create(device, C.byref(h), C.byref(err))
        if rc:
            _raise(err, rc)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.zpaqhip_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()

    def stats(self) -> Stats:
        s = Stats()
        self._L.zpaqhip_last_stats(self._h, C.byref(s))
        return s

    def device_tables(self):
        """(squash, stretch, dt, dt2k, ns) as read back from device memory."""
        sq, st = np.zeros(4096, np.uint16), np.zeros(32768, np.int16)
        dt, dt2k, ns = np.zeros(1024, np.int32), np.zeros(256, np.int32), np.zeros(1024, np.uint8)
        err = Err()
        rc = self._L.zpaqhip_read_device_tables(self._h, sq.ctypes.data, st.ctypes.data, dt.ctypes.data,
                                                dt2k.ctypes.data, ns.ctypes.data, C.byref(err))
        if rc:
            _raise(err, rc)
        return sq, st, dt, dt2k, ns

    def compress_blocks(self, model, blocks, *, pre=None, filenames=None, sha1: bool = True, tag: bool = True, kernel: int = 0,
                        batch_blocks: int = 0, slot_bytes: int = 0, enc_waves: int = 0, verify: bool = False) -> bytes:
        """Compressor.startBlock .. endBlock for each block (LibZPAQ.cs:296-323 framing, one segment per block), coded on
        the GPU: the same bytes the CPU stream writer (synth.compress_block) produces.  `model` is a models name or a
        zpaql.Model.  A `+e8e9` model codes the forward E8E9 transform of each block; a `+lz77` model needs `pre`, the
        pre-processed bytes of each block (size comment and SHA-1 still describe `blocks`).  `kernel`: 0 single-CM models
        on the window-parallel encoder, the rest on the one-lane generic encoder; 1 everything on the generic encoder;
        2 as 0, but models that fit the lane-per-component kernel (ICM / ISSE / MATCH / MIX chains of at most 64
        components and 4 mixers: min, mid, max, the method models) on the lane-per-component encoder
        (stats().kernel_kind == 3).  `enc_waves`: that encoder's waves (blocks in flight) per compute unit: 0 as many as
        the model's LDS plan (enc_chain_plan), the blocks and device memory allow, up to four; 1 one; 2 to 4 a cap; more is
        an error.  The bytes never depend on it; stats().concurrent tells the blocks in flight of the largest launch.
        `verify` (every compressing call has it): Compressor.setVerify, the coded sequence of each block runs through the
        block's own post-processor on the GPU before it is coded (verify_blocks), and a block that does not come back as
        its plaintext raises ZpaqError(-28, block) or the post-processor's own error; the bytes do not depend on it."""
        from . import e8e9, models
        m = models.get(model) if isinstance(model, str) else model
        plain = [_as_u8(b) for b in blocks]
        coded, orig = plain, None
        if pre is not None:
            if len(pre) != len(plain):
                raise ValueError("pre needs one entry per block")
            coded, orig = [_as_u8(p) for p in pre], plain
        elif m.pcomp_cmd.startswith("e8e9"):
            coded, orig = [e8e9.forward(b) for b in plain], plain
        elif m.pcomp_cmd.startswith("lz77"):
            raise ValueError("a +lz77 model needs the pre-processed blocks (pre=)")
        flags = compress_flags(sha1, tag, verify=verify)
        return self._compress(m.header, m.pcomp or b"", coded, orig, filenames, flags, kernel, batch_blocks, slot_bytes,
                              enc_waves=enc_waves)[0]

    def _pre_blocks(self, fn, first, plain, cap: int, retry: bool = False) -> List[bytes]:
        """A zpaqhip_*_blocks entry point `fn` (`first` is its argument after the context: the method's args or the E8E9 flag) on
        a list of blocks: their pre-processed bytes.  `retry`: once more when `cap` was too small (ZPAQHIP_E_OUTPUT_FULL
        tells the size)."""
        buf, offs = _cat(plain)
        oo = np.zeros(len(plain) + 1, np.uint64)
        for _ in range(2 if retry else 1):
            out = np.empty(max(1, cap), np.uint8)
            err, got = Err(), C.c_size_t(0)
            rc = fn(self._h, first, buf.ctypes.data, offs.ctypes.data, len(plain), out.ctypes.data, cap, C.byref(got), oo.ctypes.data,
                    C.byref(err))
            if retry and rc == -20 and got.value > cap:
                cap = got.value
                continue
            if rc:
                _raise(err, rc)
            return [out[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(len(plain))]
        _raise(err, rc)

    def preprocess_blocks(self, method: str, blocks) -> List[bytes]:
        """What LibZPAQ.compressBlock feeds the coder for `method` (LibZPAQ.cs:296-311: E8E9, LZBuffer levels 1 / 2), computed
        on the GPU for each block: equal to tools.methods.preprocess.  Useful on its own as `pre=` of compress_blocks."""
        from . import method as mth
        args = mth.parse_args(method)[1]
        plain = [_as_u8(b) for b in blocks]
        mth.check_blocks(args, [p.size for p in plain])
        return self._pre_blocks(self._L.zpaqhip_preprocess_blocks, (C.c_int32 * 9)(*args), plain,
                                sum(mth.pre_bound(args, p.size) for p in plain), retry=True)

    def bwt_blocks(self, blocks, e8e9: bool = False) -> List[bytes]:
        """LZBuffer's level 3 (LZBuffer.cs:228-240) of each block on the GPU (zpaqhip_bwt_blocks): the Burrows-Wheeler
        transform from a suffix array in which the end of the block sorts first, n + 5 bytes for n; with `e8e9`, of the
        forward E8E9 transform of the block.  Equal to tools.methods.preprocess for `x0,3` / `x0,7`."""
        plain = [_as_u8(b) for b in blocks]
        for i, p in enumerate(plain):
            if p.size > (1 << 31) - 1:
                raise ValueError(f"block {i} has {p.size} bytes; a BWT block holds at most 2^31 - 1")
        return self._pre_blocks(self._L.zpaqhip_bwt_blocks, int(bool(e8e9)), plain, sum(p.size + 5 for p in plain))

    def lzsa_blocks(self, method: str, blocks) -> List[bytes]:
        """LZBuffer's codes of each block for a level 1 / 2 method with args[5] - args[0] >= 21, from the reference's
        suffix-array search (LZBuffer.cs:246-283, :329-383) on the GPU (zpaqhip_lzsa_blocks), after E8E9 where the method
        asks for it: equal to tools.methods.preprocess(..., sa=True).  ValueError for any other method."""
        from . import method as mth
        args = mth.parse_args(method)[1]
        if not mth.uses_sa(args):
            raise ValueError("not a level 1 / 2 method with args[5] - args[0] >= 21")
        plain = [_as_u8(b) for b in blocks]
        mth.check_blocks(args, [p.size for p in plain], sa=True)
        return self._pre_blocks(self._L.zpaqhip_lzsa_blocks, (C.c_int32 * 9)(*args), plain,
                                sum(mth.pre_bound(args, p.size) for p in plain))

    def lzht_blocks(self, method: str, blocks) -> List[bytes]:
        """LZBuffer's codes of each block for a level 1 / 2 method with args[5] - args[0] < 21, from the reference's
        hash-table search (LZBuffer.cs:285-327, :349-368) on the GPU (zpaqhip_lzht_blocks), after E8E9 where the method asks
        for it: equal to tools.methods.preprocess(..., ht=True).  ValueError for any other method, and for what the route
        does not take (method.check_blocks): args[3] != 0, args[6] != 0, level 1 with args[2] < 4, level 2 with args[2] < 2,
        args[2] > 255, args[0] > 11, args[4] > args[5] or > 6, args[5] > 30, a block longer than 2^24 bytes."""
        from . import method as mth
        args = mth.parse_args(method)[1]
        if not mth.uses_ht(args):
            raise ValueError("not a level 1 / 2 method with args[5] - args[0] < 21")
        plain = [_as_u8(b) for b in blocks]
        mth.check_blocks(args, [p.size for p in plain], ht=True)
        return self._pre_blocks(self._L.zpaqhip_lzht_blocks, (C.c_int32 * 9)(*args), plain,
                                sum(mth.pre_bound(args, p.size) for p in plain))

    def compress_method(self, method: str, blocks, *, filenames=None, sha1: bool = True, tag: bool = True, kernel: int = 0,
                        batch_blocks: int = 0, slot_bytes: int = 0, bwt: bool = False, sa: bool = False, ht: bool = False,
                        enc_waves: int = 0, verify: bool = False) -> bytes:
        """LibZPAQ.compressBlock(method) for each block (LibZPAQ.cs:296-323, one segment per block) on the GPU: the bytes
        tools.methods.compress_block writes.  Levels 0, 1 and 2 with or without E8E9, and with `bwt=True` level 3; the
        model of an n >= 1 method codes the pre-processed bytes on the encoders of compress_blocks (kernel, batch_blocks,
        slot_bytes, enc_waves as there: kernel=2 puts the chain models of levels 3 and 4 on the lane-per-component encoder), an
        n = 0 method stores them.  ValueError, before the device is touched, for level 3 without
        `bwt=True`, a level 2 `m` outside 1..64 and a block longer than 2^(args[0] + 20) bytes at level 1 or 2 (4096
        less at level 3).  `sa=True`: a level 1 / 2 method with args[5] - args[0] >= 21 gets the reference's suffix-array
        parse (lzsa_blocks; the bytes of tools.methods.compress_block(..., sa=True)); no effect on any other method.
        `ht=True`: one with args[5] - args[0] < 21 gets the reference's hash-table parse (lzht_blocks, with its refusals;
        the bytes of tools.methods.compress_block(..., ht=True)); no effect on any other method.  Both may be given."""
        return self._compress_method(method, blocks, filenames, sha1, tag, kernel, batch_blocks, slot_bytes, bwt, sa, ht, enc_waves,
                                     verify)[0]

    def _compress_method(self, method: str, blocks, filenames, sha1: bool, tag: bool, kernel: int, batch_blocks: int,
                         slot_bytes: int, bwt: bool, sa: bool = False, ht: bool = False, enc_waves: int = 0, verify: bool = False):
        """compress_method: (stream bytes, block offsets)."""
        from . import method as mth
        args = mth.parse_args(method)[1]
        plain = [_as_u8(b) for b in blocks]
        mth.check_blocks(args, [p.size for p in plain], bwt=bwt, sa=sa, ht=ht)
        model, _ = mth.model_of(method)
        cap = sum(mth.pre_bound(args, p.size) for p in plain) + len(plain) * (len(model.header) + 2 * len(model.pcomp) + 4096) + 4096
        return self._compress(model.header, model.pcomp or b"", plain, None, filenames,
                              compress_flags(sha1, tag, bwt, sa, ht, verify), kernel, batch_blocks, slot_bytes, out_cap=cap,
                              args=args, enc_waves=enc_waves)[:2]

    def gap_hist_blocks(self, blocks) -> np.ndarray:
        """The repetition-gap histogram LibZPAQ.compressBlock takes of a block at levels 5..9 (LibZPAQ.cs:242-255), of each
        block on the GPU (zpaqhip_gap_hist_blocks): shape (len(blocks), 4096), uint32, [b, k] = positions of block b whose
        byte value last occurred k positions earlier, or, as the reference's table starts at zero, was first seen at
        position k.  Equal to synth.gap_hist; method.expand_level reads the periodic models of a level off a row."""
        plain = [_as_u8(b) for b in blocks]
        for i, p in enumerate(plain):
            if p.size > (1 << 31) - 1:
                raise ValueError(f"block {i} has {p.size} bytes; the analysis takes at most 2^31 - 1")
        hist = np.zeros((len(plain), 4096), np.uint32)
        if not plain:
            return hist
        buf, offs = _cat(plain)
        err = Err()
        rc = self._L.zpaqhip_gap_hist_blocks(self._h, buf.ctypes.data, offs.ctypes.data, len(plain), hist.ctypes.data, C.byref(err))
        if rc:
            _raise(err, rc)
        return hist

    def compress_level(self, level: str, blocks, *, filenames=None, sha1: bool = True, tag: bool = True, kernel: int = 2,
                       batch_blocks: int = 0, slot_bytes: int = 0, sa: bool = False, ht: bool = False, enc_waves: int = 0,
                       verify: bool = False) -> bytes:
        """LibZPAQ.compressBlock with a numeric method "LB,R,t" (LibZPAQ.cs:124-323) for each block: `level` is expanded per
        block by method.expand_level (the block's length gives the x<N> argument; at levels 5..9 its gap histogram, taken by
        gap_hist_blocks, gives the periodic models), the blocks are grouped by the string they got, each group goes through
        compress_method(string, ..., bwt=True, kernel=kernel), and the blocks come back in input order.  `kernel` defaults to
        the lane-per-component encoder for chain models (2): the one-lane encoder needs seconds per 64 KiB of a level 5
        model.  `level_methods` keeps the expanded string of each block of the last call, `level_ms` its wall time in ms
        spent on the analysis and on the encoding.  `sa` is compress_method's: the LZ77 strings of levels 2, 3 and 4 then
        get the reference's suffix-array parse.  `ht` likewise: the LZ77 strings of level 1, and those levels 2 to 4 give
        blocks of low redundancy, then get its hash-table parse.  `enc_waves` is compress_blocks'."""
        import time

        from . import method as mth
        if not level or not level[0].isdigit():
            raise ValueError("a numeric method starts with its level, a digit")
        plain = [_as_u8(b) for b in blocks]
        if filenames is not None and len(filenames) != len(plain):
            raise ValueError("filenames needs one entry per block")
        t0 = time.perf_counter()
        hist = self.gap_hist_blocks(plain) if int(level[0]) >= 5 else None
        t1 = time.perf_counter()
        expanded = [mth.expand_level(level, p.size, None if hist is None else hist[i]) for i, p in enumerate(plain)]
        groups = {}
        for i, m in enumerate(expanded):
            groups.setdefault(m, []).append(i)
        parts = [b""] * len(plain)
        for m, ids in groups.items():
            try:
                out, off = self._compress_method(m, [plain[i] for i in ids], None if filenames is None else [filenames[i] for i in ids],
                                                 sha1, tag, kernel, batch_blocks, slot_bytes, True, sa, ht, enc_waves, verify)
            except ZpaqError as e:                         # (the block's index in the call, not in its group)
                if 0 <= e.block < len(ids):
                    raise ZpaqError(e.code, ids[e.block], e.segment, str(e)) from None
                raise
            for j, i in enumerate(ids):
                parts[i] = out[int(off[j]):int(off[j + 1])]
        self.level_methods = expanded
        self.level_ms = {"analysis": (t1 - t0) * 1e3, "encode": (time.perf_counter() - t1) * 1e3}
        return b"".join(parts)

    # the compressing entry points by (method form, solid form, device form)
    _ENTRY = {(False, False, False): "zpaqhip_compress_blocks", (False, False, True): "zpaqhip_compress_blocks_device",
              (True, False, False): "zpaqhip_compress_method_blocks", (True, False, True): "zpaqhip_compress_method_blocks_device",
              (False, True, False): "zpaqhip_compress_solid_blocks", (False, True, True): "zpaqhip_compress_solid_blocks_device"}

    def _entry(self, header: bytes, pcomp: bytes, *, src, in_off, n: int, opts, args=None, seg_first=None, orig=None, orig_off=None,
               names=None, device: bool = False):
        """What every compressing entry point takes in front of its output: (function, leading arguments, what they point
        into).  `args` selects the method form (which has no `orig`), `seg_first` the solid form, `device` the device forms;
        `src` and `orig` are addresses or uint8 arrays, the offsets uint64 arrays, `names` a flat list with an entry per
        segment or None, `opts` (flags, kernel, batch_blocks, slot_bytes, enc_waves)."""
        if names is not None:
            if seg_first is None and len(names) != n:
                raise ValueError("filenames needs one entry per block")
            names = (C.c_char_p * max(1, len(names)))(*[(f.encode() if isinstance(f, str) else f) for f in names])
        o = CompressOpts()
        o.struct_size = C.sizeof(CompressOpts)
        o.flags, o.kernel, o.batch_blocks, o.slot_bytes, o.enc_waves = opts
        hdr = _as_u8(header)
        pc = _as_u8(pcomp) if pcomp else None
        keep = (o, hdr, pc, src, in_off, seg_first, orig, orig_off, names)

        def ptr(x):
            return x.ctypes.data if isinstance(x, np.ndarray) else x

        front = [self._h]
        if args is not None:
            front.append((C.c_int32 * 9)(*args))
        front += [ptr(hdr), hdr.size, ptr(pc), pc.size if pc is not None else 0, ptr(src), ptr(in_off)]
        if seg_first is not None:
            front.append(ptr(seg_first))
        front.append(n)
        if args is None:
            front += [ptr(orig), ptr(orig_off)]
        front.append(names)
        return getattr(self._L, self._ENTRY[args is not None, seg_first is not None, device]), front, keep

    def _run_host(self, entry, n: int, out_cap: int):
        """A host entry point into a buffer of out_cap bytes, and once more when that was too small (ZPAQHIP_E_OUTPUT_FULL
        tells the exact size): (stream bytes, block offsets, status of the first call)."""
        fn, front, keep = entry
        boffs = np.zeros(n + 1, np.uint64)
        first = None
        for _ in range(2):
            out = np.empty(max(1, out_cap), np.uint8)
            err, got = Err(), C.c_size_t(0)
            rc = fn(*front, out.ctypes.data, out_cap, C.byref(got), boffs.ctypes.data, C.byref(keep[0]), C.byref(err))
            first = rc if first is None else first
            if rc == -20 and got.value > out_cap:
                out_cap = got.value
                continue
            if rc:
                _raise(err, rc)
            return out[:got.value].tobytes(), boffs, first
        _raise(err, rc)

    def _run_device(self, entry, n: int, d_out: int, out_cap: int, hip_stream: int, raise_on_error: bool):
        """A device entry point: (status, bytes needed, block offsets)."""
        fn, front, keep = entry
        boffs = np.zeros(n + 1, np.uint64)
        err, got = Err(), C.c_size_t(0)
        rc = fn(*front, d_out or None, out_cap, C.byref(got), boffs.ctypes.data, C.byref(keep[0]), hip_stream or None, C.byref(err))
        if rc and rc != -20 and raise_on_error:
            _raise(err, rc)
        return rc, got.value, boffs

    def _compress(self, header: bytes, pcomp: bytes, coded, orig, filenames, flags: int, kernel: int, batch_blocks: int,
                  slot_bytes: int, out_cap: Optional[int] = None, args: Optional[List[int]] = None, enc_waves: int = 0):
        """zpaqhip_compress_blocks (zpaqhip_compress_method_blocks with `args`: `coded` is then the plaintext) on lists of
        blocks: (stream bytes, block offsets, status of the first call)."""
        n = len(coded)
        cbuf, coffs = _cat(coded)
        obuf, ooffs = _cat(orig) if orig is not None else (None, None)
        entry = self._entry(header, pcomp, args=args, src=cbuf, in_off=coffs, orig=obuf, orig_off=ooffs, names=filenames, n=n,
                            opts=(flags, kernel, batch_blocks, slot_bytes, enc_waves))
        if out_cap is None:
            out_cap = int(coffs[-1]) + int(coffs[-1]) // 8 + n * (len(header) + 128 + 4096) + 4096
        return self._run_host(entry, n, out_cap)

    def compress_blocks_device(self, model, d_in: int, in_off: Sequence[int], d_out: int, out_cap: int, *, d_orig: int = 0,
                               orig_off: Optional[Sequence[int]] = None, filenames=None, sha1: bool = True, tag: bool = True,
                               kernel: int = 0, batch_blocks: int = 0, slot_bytes: int = 0, enc_waves: int = 0,
                               hip_stream: int = 0, raise_on_error: bool = True, verify: bool = False):
        """zpaqhip_compress_blocks_device: compress_blocks on device buffers (pointers as ints; the caller holds the memory,
        e.g. torch tensors' .data_ptr()).  Block i codes the bytes d_in + in_off[i] .. d_in + in_off[i + 1] as they are (no
        E8E9 here: a `+e8e9` or `+lz77` model takes its pre-processed bytes in d_in and, for the size comment and SHA-1, the
        plaintext in d_orig / orig_off); the stream goes to d_out, at most out_cap bytes.  `model`, the options and the
        bytes are compress_blocks'.  Returns (rc, out_len, block_off): rc 0, or -20 (ZPAQHIP_E_OUTPUT_FULL) with out_len the
        bytes needed and the blocks that fit in whole written; any other status raises unless raise_on_error is False."""
        from . import models
        m = models.get(model) if isinstance(model, str) else model
        flags = compress_flags(sha1, tag, verify=verify)
        return self._compress_device(m.header, m.pcomp or b"", None, d_in, in_off, d_orig, orig_off, filenames, flags, kernel,
                                     batch_blocks, slot_bytes, enc_waves, d_out, out_cap, hip_stream, raise_on_error)

    def compress_method_device(self, method: str, d_in: int, in_off: Sequence[int], d_out: int, out_cap: int, *, filenames=None,
                               sha1: bool = True, tag: bool = True, kernel: int = 0, batch_blocks: int = 0, slot_bytes: int = 0,
                               bwt: bool = False, sa: bool = False, ht: bool = False, enc_waves: int = 0, hip_stream: int = 0,
                               raise_on_error: bool = True, verify: bool = False):
        """zpaqhip_compress_method_blocks_device: compress_method on device buffers, in the style of compress_blocks_device:
        the plaintext of block i at d_in + in_off[i], the stream to d_out, (rc, out_len, block_off) back.  The method's
        refusals (ValueError before the device is touched) and the options are compress_method's."""
        from . import method as mth
        args = mth.parse_args(method)[1]
        off = [int(x) for x in in_off]
        mth.check_blocks(args, [b - a for a, b in zip(off, off[1:])], bwt=bwt, sa=sa, ht=ht)
        model, _ = mth.model_of(method)
        flags = compress_flags(sha1, tag, bwt, sa, ht, verify)
        return self._compress_device(model.header, model.pcomp or b"", args, d_in, off, 0, None, filenames, flags, kernel,
                                     batch_blocks, slot_bytes, enc_waves, d_out, out_cap, hip_stream, raise_on_error)

    def _compress_device(self, header: bytes, pcomp: bytes, args, d_in: int, in_off, d_orig: int, orig_off, filenames, flags: int,
                         kernel: int, batch_blocks: int, slot_bytes: int, enc_waves: int, d_out: int, out_cap: int,
                         hip_stream: int, raise_on_error: bool):
        """The two device forms (`args`: the method form): (status, bytes needed, block offsets)."""
        coffs = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = max(0, coffs.size - 1)
        ooffs = np.ascontiguousarray(orig_off, dtype=np.uint64) if orig_off is not None else None
        if ooffs is not None and ooffs.size != coffs.size:
            raise ValueError("orig_off needs one entry per entry of in_off")
        entry = self._entry(header, pcomp, args=args, src=d_in or None, in_off=coffs, orig=d_orig or None, orig_off=ooffs,
                            names=filenames, n=n, opts=(flags, kernel, batch_blocks, slot_bytes, enc_waves), device=True)
        return self._run_device(entry, n, d_out, out_cap, hip_stream, raise_on_error)

    def compress_solid(self, model, blocks, *, pre=None, filenames=None, sha1: bool = True, tag: bool = True, kernel: int = 0,
                       enc_waves: int = 0, batch_blocks: int = 0, slot_bytes: int = 0) -> bytes:
        """zpaqhip_compress_solid_blocks: compress_blocks with several segments per block (Compressor.startSegment ..
        endSegment, repeated; the post-processor is sent in a block's first segment only).  `blocks` is a list of lists of
        byte strings, a block's segments; a block needs at least one, and a segment may be empty.  `pre` (the coded bytes
        of each segment when they are not the segment itself; size comment and SHA-1 then still describe `blocks`) and
        `filenames` have the same shape.  Model, coder interval and post-processor state carry over from a segment to the
        next: many small files share one block's statistics.  Nothing is pre-processed here: a model with a
        post-processor needs `pre`, and the caller sees to it that the segments' coded bytes, one after the other, are what
        the post-processor turns into `blocks`.  The options are compress_blocks' (no verify); a block of one segment is
        coded where compress_blocks codes it, to the same bytes; a block of several segments of a single-CM model goes to
        the lane-per-component encoder with kernel=2 and to the generic one otherwise."""
        from . import models
        m = models.get(model) if isinstance(model, str) else model
        if pre is None and m.pcomp:
            raise ValueError("a model with a post-processor needs the pre-processed segments (pre=)")
        flat, seg_first = self._solid_lists(blocks, "blocks")
        plain = [_as_u8(b) for b in flat]
        coded, orig = plain, None
        if pre is not None:
            flat, pf = self._solid_lists(pre, "pre")
            if pf != seg_first:
                raise ValueError("pre needs the shape of blocks")
            coded, orig = [_as_u8(p) for p in flat], plain
        n, ns = len(seg_first) - 1, len(coded)
        cbuf, coffs = _cat(coded)
        obuf, ooffs = _cat(orig) if orig is not None else (None, None)
        entry = self._entry(m.header, m.pcomp or b"", src=cbuf, in_off=coffs, seg_first=np.asarray(seg_first, np.uint64), orig=obuf,
                            orig_off=ooffs, names=self._solid_names(filenames, seg_first), n=n,
                            opts=(compress_flags(sha1, tag), kernel, batch_blocks, slot_bytes, enc_waves))
        out_cap = int(coffs[-1]) + int(coffs[-1]) // 8 + n * (len(m.header) + 4096) + ns * 128 + 4096
        return self._run_host(entry, n, out_cap)[0]

    @staticmethod
    def _solid_lists(blocks, what: str):
        """A list of lists flattened: (the segments in order, seg_first)."""
        flat, seg_first = [], [0]
        for b in blocks:
            if isinstance(b, (bytes, bytearray, memoryview, str, np.ndarray)) or len(b) == 0:
                raise ValueError(f"{what}: every block is a list of at least one segment")
            flat.extend(b)
            seg_first.append(len(flat))
        return flat, seg_first

    @staticmethod
    def _solid_names(filenames, seg_first):
        """The per-segment names of a solid call as a flat list (None: no names)."""
        if filenames is None:
            return None
        flat, ff = Context._solid_lists(filenames, "filenames") if len(filenames) and not isinstance(filenames[0], (bytes, str)) \
            else (list(filenames), None)
        if (ff is not None and ff != list(seg_first)) or len(flat) != seg_first[-1]:
            raise ValueError("filenames needs one entry per segment")
        return flat

    def compress_solid_device(self, model, d_in: int, in_off: Sequence[int], seg_first: Sequence[int], d_out: int, out_cap: int, *,
                              d_orig: int = 0, orig_off: Optional[Sequence[int]] = None, filenames=None, sha1: bool = True,
                              tag: bool = True, kernel: int = 0, enc_waves: int = 0, batch_blocks: int = 0, slot_bytes: int = 0,
                              hip_stream: int = 0, raise_on_error: bool = True):
        """zpaqhip_compress_solid_blocks_device: compress_solid on device buffers, in the style of compress_blocks_device.
        Segment s codes the bytes d_in + in_off[s] .. d_in + in_off[s + 1]; block i holds the segments seg_first[i] ..
        seg_first[i + 1]; `filenames` is a flat list, one per segment, or a list of lists in the blocks' shape.  Returns
        (rc, out_len, block_off) as compress_blocks_device does."""
        from . import models
        m = models.get(model) if isinstance(model, str) else model
        coffs = np.ascontiguousarray(in_off, dtype=np.uint64)
        sf = np.ascontiguousarray(seg_first, dtype=np.uint64)
        n = max(0, sf.size - 1)
        if sf.size == 0 or coffs.size != int(sf[-1]) + 1:
            raise ValueError("in_off needs one entry per segment and one more")
        ooffs = np.ascontiguousarray(orig_off, dtype=np.uint64) if orig_off is not None else None
        if ooffs is not None and ooffs.size != coffs.size:
            raise ValueError("orig_off needs one entry per entry of in_off")
        entry = self._entry(m.header, m.pcomp or b"", src=d_in or None, in_off=coffs, seg_first=sf, orig=d_orig or None,
                            orig_off=ooffs, names=self._solid_names(filenames, [int(x) for x in sf]), n=n,
                            opts=(compress_flags(sha1, tag), kernel, batch_blocks, slot_bytes, enc_waves), device=True)
        return self._run_device(entry, n, d_out, out_cap, hip_stream, raise_on_error)

    @staticmethod
    def _verify_model(model_or_method):
        """(header, pcomp) of a models name, a zpaql.Model or a method string (`x...` / a numeric level is not one)."""
        from . import method as mth, models
        if isinstance(model_or_method, str):
            if model_or_method[:1] == "x":
                m = mth.model_of(model_or_method)[0]
            else:
                m = models.get(model_or_method)
        else:
            m = model_or_method
        return m.header, m.pcomp or b""

    @staticmethod
    def _verify_records(rec, n):
        return [{"status": int(rec[i].status), "out_len": int(rec[i].out_len), "first_diff": int(rec[i].first_diff),
                 "sha1": bytes(rec[i].sha1)} for i in range(n)]

    def verify_blocks(self, model_or_method, pre, orig=None) -> List[dict]:
        """zpaqhip_verify_blocks: Compressor.endSegmentChecksum for a set of blocks.  `pre[i]` are the pre-processed bytes of
        block i (what preprocess_blocks / bwt_blocks / lzsa_blocks / lzht_blocks give, or a caller's own); they run through
        the post-processor of `model_or_method` (a models name, a zpaql.Model or a method string) on the GPU as they would
        after the decoder.  One dict per block: `status` (0, -28 when `orig` is given and differs, or the post-processor's
        own error), `out_len` and `sha1` of what it wrote, `first_diff` (the first offset at which that differs from
        orig[i]; 2**64 - 1 when equal or without `orig`)."""
        header, pcomp = self._verify_model(model_or_method)
        coded = [_as_u8(p) for p in pre]
        n = len(coded)
        if orig is not None and len(orig) != n:
            raise ValueError("orig needs one entry per block")
        cbuf, coffs = _cat(coded)
        obuf, ooffs = _cat([_as_u8(b) for b in orig]) if orig is not None else (None, None)
        hdr = _as_u8(header)
        pc = _as_u8(pcomp) if pcomp else None
        rec = (VerifyResult * max(1, n))()
        err = Err()
        rc = self._L.zpaqhip_verify_blocks(self._h, hdr.ctypes.data, hdr.size, pc.ctypes.data if pc is not None else None,
                                           pc.size if pc is not None else 0, cbuf.ctypes.data, coffs.ctypes.data, n,
                                           obuf.ctypes.data if obuf is not None else None,
                                           ooffs.ctypes.data if ooffs is not None else None, rec, C.byref(err))
        if rc:
            _raise(err, rc)
        return self._verify_records(rec, n)

    def verify_blocks_device(self, model_or_method, d_in: int, in_off: Sequence[int], *, d_orig: int = 0,
                             orig_off: Optional[Sequence[int]] = None, hip_stream: int = 0) -> List[dict]:
        """zpaqhip_verify_blocks_device: verify_blocks on device buffers (pointers as ints): the pre-processed bytes of block i
        at d_in + in_off[i], its plaintext (optional) at d_orig + orig_off[i]; only the records come back."""
        header, pcomp = self._verify_model(model_or_method)
        coffs = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = max(0, coffs.size - 1)
        ooffs = np.ascontiguousarray(orig_off, dtype=np.uint64) if orig_off is not None else None
        if ooffs is not None and ooffs.size != coffs.size:
            raise ValueError("orig_off needs one entry per entry of in_off")
        if (ooffs is None) != (not d_orig):
            raise ValueError("d_orig and orig_off go together")
        hdr = _as_u8(header)
        pc = _as_u8(pcomp) if pcomp else None
        rec = (VerifyResult * max(1, n))()
        err = Err()
        rc = self._L.zpaqhip_verify_blocks_device(self._h, hdr.ctypes.data, hdr.size, pc.ctypes.data if pc is not None else None,
                                                  pc.size if pc is not None else 0, d_in or None, coffs.ctypes.data, n,
                                                  d_orig or None, ooffs.ctypes.data if ooffs is not None else None, rec,
                                                  hip_stream or None, C.byref(err))
        if rc:
            _raise(err, rc)
        return self._verify_records(rec, n)

    def gap_hist_blocks_device(self, d_in: int, in_off: Sequence[int], hip_stream: int = 0) -> np.ndarray:
        """zpaqhip_gap_hist_blocks_device: gap_hist_blocks of blocks in device memory (block i at d_in + in_off[i], read where
        it is, any alignment): the same array, and all that crosses the bus."""
        offs = np.ascontiguousarray(in_off, dtype=np.uint64)
        n = max(0, offs.size - 1)
        for i in range(n):
            if int(offs[i + 1]) - int(offs[i]) > (1 << 31) - 1:
                raise ValueError(f"block {i} has {int(offs[i + 1]) - int(offs[i])} bytes; the analysis takes at most 2^31 - 1")
        hist = np.zeros((n, 4096), np.uint32)
        if not n:
            return hist
        err = Err()
        rc = self._L.zpaqhip_gap_hist_blocks_device(self._h, d_in or None, offs.ctypes.data, n, hist.ctypes.data, hip_stream or None,
                                                    C.byref(err))
        if rc:
            _raise(err, rc)
        return hist

    def compress_mixed_device(self, methods: List[str], method_of: Sequence[int], d_in: int, in_off: Sequence[int], d_out: int,
                              out_cap: int, *, filenames=None, sha1: bool = True, tag: bool = True, kernel: int = 0,
                              batch_blocks: int = 0, slot_bytes: int = 0, bwt: bool = False, sa: bool = False, ht: bool = False,
                              enc_waves: int = 0, hip_stream: int = 0, raise_on_error: bool = True, verify: bool = False):
        """zpaqhip_compress_mixed_blocks_device: compress_method_device with a method per block: block i takes
        methods[method_of[i]], and the stream in d_out has the blocks in input order, each the bytes compress_method writes
        for it.  (rc, out_len, block_off) as compress_method_device.  Every method that a block takes is checked against
        its own blocks (compress_method's refusals: ValueError before the device is touched); one that no block takes is
        not."""
        from . import method as mth
        off = [int(x) for x in in_off]
        n = max(0, len(off) - 1)
        which = np.ascontiguousarray(method_of, dtype=np.int64).reshape(-1)
        if which.size != n:
            raise ValueError("method_of needs one entry per block")
        if n and (which.min() < 0 or which.max() >= len(methods)):
            raise ValueError("method_of names no entry of methods")
        if filenames is not None and len(filenames) != n:
            raise ValueError("filenames needs one entry per block")
        lens = [b - a for a, b in zip(off, off[1:])]
        table = (_lib.Method * max(1, len(methods)))()
        keep = []                                          # the headers and programs the table points into
        for g, m in enumerate(methods):
            args = mth.parse_args(m)[1]
            used = [lens[i] for i in range(n) if which[i] == g]
            if used:
                mth.check_blocks(args, used, bwt=bwt, sa=sa, ht=ht)
            model, _ = mth.model_of(m)
            hdr, pc = _as_u8(model.header), _as_u8(model.pcomp) if model.pcomp else None
            keep += [hdr, pc]
            table[g].args = (C.c_int32 * 9)(*args)
            table[g].hdr, table[g].hdr_len = hdr.ctypes.data, hdr.size
            table[g].pcomp, table[g].pcomp_len = (pc.ctypes.data, pc.size) if pc is not None else (None, 0)
        which = np.ascontiguousarray(which, dtype=np.uint32)
        coffs = np.ascontiguousarray(off, dtype=np.uint64)
        names = None
        if filenames is not None:
            names = (C.c_char_p * max(1, n))(*[(f.encode() if isinstance(f, str) else f) for f in filenames])
        o = CompressOpts()
        o.struct_size = C.sizeof(CompressOpts)
        o.flags = compress_flags(sha1, tag, bwt, sa, ht, verify)
        o.kernel, o.batch_blocks, o.slot_bytes, o.enc_waves = kernel, batch_blocks, slot_bytes, enc_waves
        boffs = np.zeros(n + 1, np.uint64)
        err, got = Err(), C.c_size_t(0)
        rc = self._L.zpaqhip_compress_mixed_blocks_device(
            self._h, table, len(methods), which.ctypes.data, d_in or None, coffs.ctypes.data, n, names, d_out or None, out_cap,
            C.byref(got), boffs.ctypes.data, C.byref(o), hip_stream or None, C.byref(err))
        if rc and rc != -20 and raise_on_error:
            _raise(err, rc)
        return rc, got.value, boffs

    def compress_level_device(self, level: str, d_in: int, in_off: Sequence[int], d_out: int, out_cap: int, *, filenames=None,
                              sha1: bool = True, tag: bool = True, kernel: int = 2, batch_blocks: int = 0, slot_bytes: int = 0,
                              sa: bool = False, ht: bool = False, enc_waves: int = 0, hip_stream: int = 0,
                              raise_on_error: bool = True, verify: bool = False):
        """compress_level on device buffers, in the style of compress_method_device: the plaintext of block i at d_in +
        in_off[i], the stream of compress_level(level, ...) to d_out, (rc, out_len, block_off) back.  At levels 5..9 the
        histogram is taken where the blocks are (gap_hist_blocks_device); method.expand_level runs per block on the host,
        from lengths and histograms alone; one compress_mixed_device call (bwt=True) then codes every block with the string
        it got.  `level_methods` and `level_ms` as compress_level sets them."""
        import time

        from . import method as mth
        if not level or not level[0].isdigit():
            raise ValueError("a numeric method starts with its level, a digit")
        off = [int(x) for x in in_off]
        n = max(0, len(off) - 1)
        if filenames is not None and len(filenames) != n:
            raise ValueError("filenames needs one entry per block")
        t0 = time.perf_counter()
        hist = self.gap_hist_blocks_device(d_in, off, hip_stream) if int(level[0]) >= 5 else None
        t1 = time.perf_counter()
        expanded = [mth.expand_level(level, off[i + 1] - off[i], None if hist is None else hist[i]) for i in range(n)]
        index = {}
        which = [index.setdefault(m, len(index)) for m in expanded]
        r = self.compress_mixed_device(list(index), which, d_in, off, d_out, out_cap, filenames=filenames, sha1=sha1, tag=tag,
                                       kernel=kernel, batch_blocks=batch_blocks, slot_bytes=slot_bytes, bwt=True, sa=sa, ht=ht,
                                       enc_waves=enc_waves, hip_stream=hip_stream, raise_on_error=raise_on_error, verify=verify)
        self.level_methods = expanded
        self.level_ms = {"analysis": (t1 - t0) * 1e3, "encode": (time.perf_counter() - t1) * 1e3}
        return r

    def decompress(self, stream, out_cap: Optional[int] = None, **opt) -> np.ndarray:
        """LibZPAQ.decompress(Reader, Writer) (LibZPAQ.cs:65-79) on host buffers."""
        a = _as_u8(stream)
        o = make_opts(**opt)
        err, n = Err(), C.c_size_t(0)
        if out_cap is None:
            sc = scan(a)
            hints = [b.usize_hint for b in sc.blocks]
            out_cap = sum(h for h in hints if h != UINT64_MAX) if hints and all(h != UINT64_MAX for h in hints) else 0
        out = np.empty(max(1, out_cap), np.uint8)
        rc = self._L.zpaqhip_decompress(self._h, a.ctypes.data, a.size, out.ctypes.data, out_cap, C.byref(n), C.byref(o), C.byref(err))
        if rc == -20 and n.value > out_cap:             # ZPAQHIP_E_OUTPUT_FULL: now we know the size
            out_cap = n.value
            out = np.empty(max(1, out_cap), np.uint8)
            rc = self._L.zpaqhip_decompress(self._h, a.ctypes.data, a.size, out.ctypes.data, out_cap, C.byref(n), C.byref(o), C.byref(err))
        if rc:
            _raise(err, rc)
        return out[:n.value]

    def decompress_into(self, stream: np.ndarray, out: np.ndarray, **opt) -> int:
        """zpaqhip_decompress on caller-owned host buffers (e.g. pinned memory): returns the plaintext length."""
        o = make_opts(**opt)
        err, n = Err(), C.c_size_t(0)
        rc = self._L.zpaqhip_decompress(self._h, stream.ctypes.data, stream.size, out.ctypes.data, out.size, C.byref(n), C.byref(o), C.byref(err))
        if rc:
            _raise(err, rc)
        return n.value

    def block_pcomp(self, stream, block: int) -> bytes:
        """Decompresser.pcomp() (Decompresser.cs:155-158): b"" if block `block` has no PCOMP, else
        length-lo, length-hi, program bytes (ZPAQL.write(out, true), ZPAQL.cs:171-177)."""
        a = _as_u8(stream)
        err, n = Err(), C.c_size_t(0)
        out = np.empty(65536 + 2, np.uint8)
        rc = self._L.zpaqhip_block_pcomp(self._h, a.ctypes.data, a.size, block, out.ctypes.data, out.size, C.byref(n), C.byref(err))
        if rc:
            _raise(err, rc)
        return out[:n.value].tobytes()

    def decompress_segments(self, stream, **opt):
        """Whole stream, but per-segment outcomes are returned instead of raised:
        (plaintext ndarray, SegResult array indexed like scan(stream).segments)."""
        a = _as_u8(stream)
        o = make_opts(**opt)
        err, n, nr = Err(), C.c_size_t(0), C.c_size_t(0)
        res = (SegResult * 1)()
        out = np.empty(1, np.uint8)
        cap, rcap = 0, 0
        for _ in range(3):
            rc = self._L.zpaqhip_decompress_segments(self._h, a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n),
                                                     res, rcap, C.byref(nr), C.byref(o), C.byref(err))
            if rc in (-20, -25) and (n.value > cap or nr.value > rcap):   # learn sizes, then retry
                cap, rcap = max(cap, n.value), max(rcap, nr.value)
                out = np.empty(max(1, cap), np.uint8)
                res = (SegResult * max(1, rcap))()
                continue
            break
        # a framing error behind the last good block: the results of the blocks before it are valid; the caller finds
        # the error in `framing_error` and raises it on reaching that point (as the reference would)
        self.framing_error = None
        if rc in (-2, -5, -11, -12, -13, -14, -15) and nr.value <= rcap and n.value <= cap:
            self.framing_error = ZpaqError(rc, err.block, err.segment, err.msg.decode(errors="replace"))
            rc = 0
        if rc:
            _raise(err, rc)
        return out[:n.value], res

    def decompress_cb(self, read_fn, write_fn, **opt) -> None:
        """Streaming form: read_fn(n)->bytes ('' at EOF), write_fn(bytes)."""
        o = make_opts(**opt)
        err = Err()
        exc: List[BaseException] = []

        def _r(_u, buf, n):
            try:
                b = read_fn(n)
                C.memmove(buf, b, len(b))
                return len(b)
            except BaseException as e:                  # noqa: BLE001 - must not unwind through C
                exc.append(e)
                return -1

        def _w(_u, buf, n):
            try:
                write_fn(C.string_at(buf, n))
                return 0
            except BaseException as e:                  # noqa: BLE001
                exc.append(e)
                return -1

        rc = self._L.zpaqhip_decompress_cb(self._h, _lib.READ_FN(_r), _lib.WRITE_FN(_w), None, C.byref(o), C.byref(err))
        if exc:
            raise exc[0]
        if rc:
            _raise(err, rc)

    def scan_device(self, d_in: int, in_len: int, stream=None, partial: bool = False):
        """zpaqhip_scan_device: scan() of a stream that lies in device memory (d_in: pointer as int, 4-byte aligned, readable
        up to in_len rounded up to a multiple of 4; `stream`: a hipStream_t as int, None = the context's own).  Returns what
        scan() returns for the same bytes, and raises what it raises; partial=True as for scan()."""
        nb, ns, err = C.c_size_t(0), C.c_size_t(0), Err()
        hs = int(stream) if stream else None
        rc = self._L.zpaqhip_scan_device(self._h, d_in or None, in_len, None, 0, C.byref(nb), None, 0, C.byref(ns), hs, C.byref(err))
        if rc and not partial:
            _raise(err, rc)
        blocks = (Block * max(1, nb.value))()
        segs = (Segment * max(1, ns.value))()
        if nb.value:
            rc = self._L.zpaqhip_scan_device(self._h, d_in or None, in_len, blocks, nb.value, C.byref(nb), segs, ns.value,
                                             C.byref(ns), hs, C.byref(err))
            if rc and not partial:
                _raise(err, rc)
        res = ScanResult((Block * nb.value).from_buffer(blocks) if nb.value else (Block * 0)(),
                         (Segment * ns.value).from_buffer(segs) if ns.value else (Segment * 0)())
        if partial:
            return res, (ZpaqError(rc, err.block, err.segment, err.msg.decode(errors="replace")) if rc else None)
        return res

    def decompress_device(self, d_in: int, in_len: int, d_out: int, out_cap: int, *, results: bool = False, stream=None,
                          raise_on_error: bool = True, **opt):
        """zpaqhip_decompress_device: decompress() with the stream at d_in and the plaintext to d_out, both in device memory
        (pointers as ints; `stream`: a hipStream_t as int, None = the context's own).  Returns (rc, out_len), with
        results=True (rc, out_len, SegResult array): rc 0, or -20 (ZPAQHIP_E_OUTPUT_FULL) with out_len the bytes needed and
        nothing written at or past d_out + out_cap.  Any other status raises unless raise_on_error is False; then rc is the
        status, out_len the bytes of the whole blocks in front of the damaged one, which are at d_out, and self.last_error
        the error.  **opt as for decompress()."""
        o = make_opts(**opt)
        err, n, nr = Err(), C.c_size_t(0), C.c_size_t(0)
        hs = int(stream) if stream else None
        res, rcap = None, 0
        if results:
            rcap = max(1, self.scan_device(d_in, in_len, stream, partial=True)[0].n_segments)
            res = (SegResult * rcap)()
        rc = self._L.zpaqhip_decompress_device(self._h, d_in or None, in_len, d_out or None, out_cap, C.byref(n), res, rcap,
                                               C.byref(nr), C.byref(o), hs, C.byref(err))
        self.last_error = ZpaqError(rc, err.block, err.segment, err.msg.decode(errors="replace")) if rc else None
        if rc and rc != -20 and raise_on_error:
            _raise(err, rc)
        if results:
            return rc, n.value, (SegResult * nr.value).from_buffer(res) if nr.value else (SegResult * 0)()
        return rc, n.value

    def decode_blocks_device(self, d_in: int, in_len: int, sc: ScanResult, d_out: int,
                             out_off: Sequence[int], out_cap: Sequence[int], ids: Optional[Sequence[int]] = None,
                             h_in=None, hip_stream: int = 0, raise_on_error: bool = True, **opt):
        """Explicit block-table form on device buffers (pointers as ints)."""
        o = make_opts(**opt)
        err = Err()
        nsel = len(ids) if ids is not None else sc.n_blocks
        ids_a = (C.c_uint32 * max(1, nsel))(*ids) if ids is not None else None
        off_a = (C.c_uint64 * max(1, nsel))(*out_off)
        cap_a = (C.c_uint64 * max(1, nsel))(*out_cap)
        res = (SegResult * max(1, sc.n_segments))()
        h = _as_u8(h_in) if h_in is not None else None
        rc = self._L.zpaqhip_decode_blocks_device(
            self._h, d_in, h.ctypes.data if h is not None else None, in_len, sc.blocks, sc.n_blocks, sc.segments,
            sc.n_segments, ids_a, nsel if ids is not None else 0, d_out, off_a, cap_a, res, C.byref(o),
            hip_stream or None, C.byref(err))
        if rc and raise_on_error:
            _raise(err, rc)
        return rc, res
