"""LibZPAQ.compress(Reader, Writer, ...) (LibZPAQ.cs:84-108, 296-323) on the GPU, with a model or an expanded method string.

The input is cut into blocks of `block_size` bytes; each becomes one block with one segment (size comment, SHA-1), coded by
Context.compress_blocks (a model; a model that needs a pre-processor other than E8E9 is refused there) or, with `method`,
by Context.compress_method (LibZPAQ.compressBlock's pre-processing levels 0, 1 and 2, with or without E8E9, and with
`bwt=True` level 3, the Burrows-Wheeler transform; without the keyword a level 3 method is refused).  `kernel` is the
encoder choice of both (2: ICM / ISSE / MIX chain models on the lane-per-component encoder) and `enc_waves` that encoder's
waves per compute unit (0 automatic, 1 to 4; Context.compress_blocks).  `sa=True` gives the LZ77
methods with args[5] - args[0] >= 21 the reference's suffix-array parse (Context.compress_method), with `method` and `level`;
`ht=True` gives those with args[5] - args[0] < 21 its hash-table parse (args[3] = args[6] = 0 and the other limits of
Context.lzht_blocks).  `verify=True` is Compressor.setVerify: every block's coded sequence goes through its own
post-processor on the GPU before it is coded, and a block that does not come back as its plaintext raises ZpaqError(-28)
(Context.compress_blocks).

With `level`, a numeric method "LB,R,t" (level, block size digits, redundancy, type), this is LibZPAQ.compress as the
reference's callers use it (LibZPAQ.cs:84-108): the block size is (2^20 << B) - 4096 unless `block_size` is given, and
Context.compress_level picks each block's method (LibZPAQ.cs:124-283), on the lane-per-component encoder unless `kernel`
says otherwise.

compress_files packs many (name, bytes) pairs into solid blocks instead: several segments per block, one per file, coded by
Context.compress_solid.
"""
from __future__ import annotations

from typing import Optional

from . import api
from .decompresser import Reader, Writer


def compress(reader: Reader, writer: Writer, model="l1", block_size: Optional[int] = None, context: Optional[api.Context] = None,
             batch_blocks: int = 64, method: Optional[str] = None, bwt: bool = False, kernel: Optional[int] = None,
             level: Optional[str] = None, sa: bool = False, ht: bool = False, enc_waves: int = 0, verify: bool = False) -> None:
    if level is not None:
        from . import method as mth
        if method is not None:
            raise ValueError("give a numeric level or an expanded method, not both")
        if not level or not level[0].isdigit():
            raise ValueError("a numeric method starts with its level, a digit")
        if block_size is None:
            block_size = mth.level_block_size(level)
    elif block_size is None:
        block_size = 1 << 22
    if block_size < 1:
        raise ValueError("block_size must be positive")
    if method is not None:
        from . import method as mth
        mth.check_blocks(mth.parse_args(method)[1], [block_size], bwt=bwt, sa=sa, ht=ht)
    ctx = context or api.Context(0)
    try:
        blocks = []

        def flush():
            if blocks:
                if level is not None:
                    writer.write(ctx.compress_level(level, blocks, kernel=2 if kernel is None else kernel, sa=sa, ht=ht,
                                                      enc_waves=enc_waves, verify=verify))
                else:
                    writer.write(ctx.compress_blocks(model, blocks, kernel=kernel or 0, enc_waves=enc_waves, verify=verify) if method is None
                                 else ctx.compress_method(method, blocks, bwt=bwt, kernel=kernel or 0, sa=sa, ht=ht,
                                                          enc_waves=enc_waves, verify=verify))
                blocks.clear()

        # A Reader may return fewer bytes than asked before its end (Reader.cs:14-25): only an empty read ends the input,
        # as in LibZPAQ.compress (LibZPAQ.cs:84-108).  Short reads are gathered into whole blocks.
        cur = bytearray()
        while True:
            b = reader.read(block_size - len(cur))
            if not b:
                break
            cur += b
            if len(cur) == block_size:
                blocks.append(bytes(cur))
                cur.clear()
                if len(blocks) >= batch_blocks:
                    flush()
        if cur:
            blocks.append(bytes(cur))
        flush()
    finally:
        if context is None:
            ctx.close()


def pack_files(sizes, block_size: int):
    """compress_files' packing rule on a list of file sizes: consecutive files go into one block while their plaintext stays
    within `block_size` bytes; a file larger than that gets a block of its own.  Returns the blocks as lists of file
    indices, in order; every file is in exactly one block and no block is empty."""
    if block_size < 1:
        raise ValueError("block_size must be positive")
    blocks, cur, used = [], [], 0
    for i, n in enumerate(sizes):
        if cur and used + n > block_size:
            blocks.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += n
    if cur:
        blocks.append(cur)
    return blocks


def compress_files(files, writer: Writer, model="min", block_size: int = 1 << 22, context: Optional[api.Context] = None,
                   kernel: int = 2, enc_waves: int = 0, batch_blocks: int = 0) -> None:
    """Many files into solid blocks: `files` is a list of (name, bytes) pairs; pack_files puts them, in order, into blocks of
    at most `block_size` plaintext bytes, every file a segment with its name, its size comment and its SHA-1, and
    Context.compress_solid codes the blocks.  A block's model is warm from its second file on and its header is paid once,
    which is what small files need.  `model` is a models name or a zpaql.Model without a post-processor."""
    files = [(n, bytes(d)) for n, d in files]
    groups = pack_files([len(d) for _, d in files], block_size)
    if not groups:
        return
    ctx = context or api.Context(0)
    try:
        writer.write(ctx.compress_solid(model, [[files[i][1] for i in g] for g in groups],
                                        filenames=[[files[i][0] for i in g] for g in groups], kernel=kernel, enc_waves=enc_waves,
                                        batch_blocks=batch_blocks))
    finally:
        if context is None:
            ctx.close()
