"""GPU parity, part 2 (round 2): the cases VERDICT r01 listed as untested — EOF inside the coder's priming
bytes, the three PostProcessor header errors, random ZPAQL programs on the device VM, and full 4 MiB blocks of
the min / mid / max(+E8E9) models.  Everything goes through the C ABI; the oracle is the checker."""
import os

import numpy as np
import pytest

import oracle
import zpaqsharp_amd as z
from tests import util
from zpaqsharp_amd import models, synth, zpaql

pytestmark = pytest.mark.gpu

TAG = bytes([0x37, 0x6b, 0x53, 0x74, 0xa0, 0x31, 0x83, 0xd3, 0x8c, 0xb2, 0x28, 0xb0, 0xd3])


def _oracle_segment(stream: bytes):
    """First segment through the oracle's step-wise Decompresser, one byte per call, so that the bytes delivered
    before an error() are known: (bytes, message or None)."""
    d = oracle.Decompresser(stream)
    assert d.find_block() is not None and d.find_filename() is not None
    d.read_comment()
    out = bytearray()
    try:
        more = True
        while more:
            b, more = d.decompress(1, cap=16)
            out += b
    except oracle.OracleError as e:
        return bytes(out), str(e)
    return bytes(out), None


def _gpu_segment(ctx, stream: bytes, sc, kernel: int, cap: int = 1 << 16):
    """The same segment through zpaqhip_decode_blocks_device with the given (possibly hand-made) tables."""
    import torch
    a = np.frombuffer(stream + b"\0" * (-len(stream) % 4 + 4), np.uint8)      # readable up to the 4-byte rounded end
    d_in = torch.from_numpy(a.copy()).cuda()
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    rc, res = ctx.decode_blocks_device(d_in.data_ptr(), len(stream), sc, d_out.data_ptr(), [0], [cap], ids=[0],
                                       raise_on_error=False, kernel=kernel)
    r = res[sc.blocks[0].first_seg]
    return bytes(d_out[:int(r.out_len)].cpu().numpy().tobytes()), int(r.status)


@pytest.mark.parametrize("model,kernels", [("l1", (0, 1, 3)), ("min", (0, 1, 4)), ("mid", (0, 1)), ("max", (0, 1))])
@pytest.mark.parametrize("keep", [0, 1, 2, 3])
def test_eof_inside_the_priming_bytes(ctx, model, kernels, keep):
    """Decoder.cs:36-40: `curr = curr << 8 | get()` with get() == -1 sets all 32 bits of curr.  A stream that ends
    after `keep` < 4 coded bytes is refused by the framing scan, so the segment table is cut by hand and handed to the
    block-table entry point; every kernel must then deliver what the oracle delivers and stop with its message."""
    good = util.block(model, util.text(3000, seed=keep + 1))
    sc = z.scan(good)
    g = sc.segments[0]
    cut = good[:g.data_off + keep]
    want_out, want_err = _oracle_segment(cut)
    assert want_err is not None
    sc.segments[0].data_len = keep
    for kernel in kernels:
        got_out, status = _gpu_segment(ctx, cut, sc, kernel)
        assert z.strerror(status) == want_err, (kernel, status)
        assert got_out == want_out, kernel


def test_eof_inside_the_priming_bytes_of_a_store_block(ctx):
    """Unmodelled (n = 0) path, Decoder.cs:58-67: priming with get() == -1 gives curr = 0xFFFFFFFF, `--curr; return get()`
    then returns -1, which the caller takes for the end of the segment."""
    hdr = zpaql.assemble("comp 0 0 0 0 0 hcomp halt end").header
    payload = b"\0" + bytes(range(50))
    body = len(payload).to_bytes(4, "big") + payload + b"\0\0\0\0"
    good = TAG + b"zPQ" + bytes([2, 1]) + hdr + b"\x01name\0comment\0\0" + body + bytes([254, 255])
    sc = z.scan(good)
    g = sc.segments[0]
    for keep in (0, 1, 2, 3):
        cut = good[:g.data_off + keep]
        want_out, want_err = _oracle_segment(cut)
        sc.segments[0].data_len = keep
        got_out, status = _gpu_segment(ctx, cut, sc, 0)
        # the oracle's decompress() ends the segment without a message (EOS came out of get()); the library
        # reports the same bytes and flags that the coded data did not end where the table said it would
        assert got_out == want_out
        if want_err is None:
            assert status in (0, -15), status
        else:
            assert z.strerror(status) == want_err


def _raw_block(model: str, decoded: bytes) -> bytes:
    """A block whose decoded byte stream (what PostProcessor.write is fed) is exactly `decoded`."""
    m = models.get(model)
    c = oracle.Compressor(len(decoded) * 2 + 4096)
    c.write_tag(); c.start_block(m.header)
    c.start_segment(b"x", b"")
    c.begin_raw()
    c.compress(decoded)
    c.end_segment(None)
    c.end_block()
    s = c.getvalue()
    c.close()
    return s


def _store_block(decoded: bytes) -> bytes:
    """An unmodelled (n = 0) block whose stored bytes are exactly `decoded` (as test_eof_inside_the_priming_bytes_of_a_store_block)."""
    hdr = zpaql.assemble("comp 0 0 0 0 0 hcomp halt end").header
    body = (len(decoded).to_bytes(4, "big") + decoded if decoded else b"") + b"\0\0\0\0"
    return TAG + b"zPQ" + bytes([2, 1]) + hdr + b"\x01name\0comment\0\0" + body + bytes([254, 255])


@pytest.mark.parametrize("decoded,msg", [
    (b"", "Unexpected EOS"),                         # state 0: EOS where the PASS/PROG selector should be   (PostProcessor.cs:43)
    (b"\x02abc", "unknown post processing type"),    # selector > 1                                          (:45)
    (b"\x07", "unknown post processing type"),
    (b"\x01", "Unexpected EOS"),                     # state 2: EOS instead of the PCOMP length, low byte    (:52)
    (b"\x01\x05", "Unexpected EOS"),                 # state 3: ... high byte                                (:57)
    (b"\x01\x00\x00", "Empty PCOMP"),                # length 0                                              (:59)
    (b"\x01\x05\x00\x38\x38", "Unexpected EOS"),     # state 4: EOS inside the program bytes                 (:68)
])
def test_postprocessor_header_errors(ctx, decoded, msg):
    # every kernel's copy of the header states (zh_generic.hip's and zh_store.hip's is zh_core.h's pp_head_step): zh_cm / zh_chain / zh_nibble /
    # zh_generic as routed for l1 and mid, zh_chain2's three instances (max at its default, mid and min at kernel=9), min at its
    # default, and zh_store for an unmodelled block (default and kernel=10)
    routes = [(model, _raw_block(model, decoded), kernels) for model, kernels in
              (("l1", (0, 1, 3)), ("mid", (0, 1, 4, 9)), ("max", (0,)), ("min", (0, 9)))]
    routes.append(("store", _store_block(decoded), (0, 10)))
    for model, s, kernels in routes:
        with pytest.raises(oracle.OracleError, match=msg):
            oracle.decompress(s)
        for kernel in kernels:
            with pytest.raises(z.ZpaqError) as e:
                ctx.decompress(s, kernel=kernel)
            assert msg in str(e.value), (model, kernel, str(e.value))


# ---------------------------------------------------------------------------------------
# random ZPAQL programs
# ---------------------------------------------------------------------------------------
_CONTROL = {zpaql.JT, zpaql.JF, zpaql.JMP, zpaql.LJ, 56}
_PLAIN_OPS = [op for op in range(256) if not zpaql.is_error_op(op) and op not in _CONTROL and op != 57]


def random_program(rng, n_ins: int, with_out: bool) -> bytes:
    """Straight-line code over EVERY defined opcode (all unary forms on a b c d *b *c *d, every assignment, every
    ALU form incl. / % ^= |= on register, memory and immediate operands, hash, hashd, a=r / r=a, *b<>a ...) with forward
    jt / jf / jmp / lj sprinkled in, so it always halts.  Returns the bytes incl. the trailing END 0."""
    ins = []                                         # (opcode, operand or None) ; jumps as ("j", opcode, target index)
    for i in range(n_ins):
        r = rng.random()
        if r < 0.12 and i + 2 < n_ins:
            op = int(rng.choice([zpaql.JT, zpaql.JF, zpaql.JMP, zpaql.LJ]))
            ins.append(("j", op, int(rng.integers(i + 1, min(n_ins, i + 12) + 1))))
        elif with_out and r < 0.22:
            ins.append((57, None))
        else:
            op = int(rng.choice(_PLAIN_OPS))
            ins.append((op, int(rng.integers(0, 256)) if op & 7 == 7 else None))
    ins.append((56, None))                           # halt
    size = [3 if (x[0] == "j" and x[1] == zpaql.LJ) else 2 if (x[0] == "j" or x[1] is not None) else 1 for x in ins]
    pos = np.concatenate([[0], np.cumsum(size)])
    code = bytearray()
    for i, x in enumerate(ins):
        if x[0] == "j":
            _, op, tgt = x
            if op == zpaql.LJ:
                code += bytes([op, int(pos[tgt]) & 255, int(pos[tgt]) >> 8])
            else:
                off = int(pos[tgt]) - int(pos[i + 1])
                if off > 127:                        # too far for a short jump: fall through instead
                    code += bytes([op, 0])
                else:
                    code += bytes([op, off])
        else:
            code.append(x[0])
            if x[1] is not None:
                code.append(x[1])
    return bytes(code) + b"\0"


def _model_with(hh, hm, ph, pm, comp: bytes, n: int, hcomp: bytes, pcomp: bytes = b"") -> zpaql.Model:
    body = bytes([hh, hm, ph, pm, n]) + comp + b"\0" + hcomp
    return zpaql.Model(bytes([len(body) & 255, len(body) >> 8]) + body, pcomp, "fuzz")


def test_random_zpaql_programs_as_hcomp(ctx):
    """The device VM (zh_core.h vm_run) against the oracle's independent interpreter: a random HCOMP computes the
    contexts of a two-component chain, so any divergence in any opcode changes the decoded bytes."""
    rng = np.random.default_rng(int(os.environ.get("ZPAQ_FUZZ_SEED", "4242")))
    data = util.text(1500, seed=3) + bytes(rng.integers(0, 256, 500, dtype=np.uint8))
    comp = bytes([3, 6, 8, 9, 0])                      # icm 6 ; isse 9 0
    seen = set()
    for trial in range(int(os.environ.get("ZPAQ_FUZZ_TRIALS", "24"))):
        hh, hm = int(rng.integers(1, 5)), int(rng.integers(0, 6))
        hcomp = random_program(rng, int(rng.integers(20, 120)), with_out=trial % 4 == 0)
        seen.update(x.split()[0] for x in zpaql.disassemble_code(hcomp[:-1]))
        m = _model_with(hh, hm, 0, 0, comp, 2, hcomp)
        s = synth.compress_block(m, data)
        assert oracle.decompress(s) == data, (trial, zpaql.disassemble_code(hcomp[:-1]))
        for kernel in (0, 1):
            got = ctx.decompress(s, verify_sha1=True, kernel=kernel).tobytes()
            assert got == data, (trial, kernel, zpaql.disassemble_code(hcomp[:-1]))
    assert len(seen) > 150                             # distinct mnemonics: nearly all of the defined opcodes took part


def test_random_zpaql_programs_as_pcomp(ctx):
    """The same VM as the post-processor: OUT bytes of a random program, fed the decoded bytes and then EOF
    (a = 0xFFFFFFFF, PostProcessor.cs:80-83), must equal the oracle's."""
    rng = np.random.default_rng(int(os.environ.get("ZPAQ_FUZZ_SEED", "4242")) + 1)
    data = util.text(1200, seed=5) + bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    l1 = models.get("l1")
    hh, hm, _, _, comps, hcomp = zpaql.parse_header(l1.header)
    comp = b"".join(bytes(c) for c in comps)
    for trial in range(int(os.environ.get("ZPAQ_FUZZ_TRIALS", "24"))):
        ph, pm = int(rng.integers(0, 5)), int(rng.integers(0, 12))
        pcomp = random_program(rng, int(rng.integers(10, 150)), with_out=True)
        m = _model_with(hh, hm, ph, pm, comp, 1, hcomp, pcomp)
        s = synth.compress_block(m, data, sha1=False)
        want = oracle.decompress(s)
        assert want == oracle.run_pcomp(pcomp, data, ph, pm, cap=1 << 20), trial
        for kernel in (0, 1, 3):
            got = ctx.decompress(s, kernel=kernel).tobytes()
            assert got == want, (trial, kernel, zpaql.disassemble_code(pcomp[:-1]))


# ---------------------------------------------------------------------------------------
# full block size (BASELINE configs[2], [4] shapes at reduced block count)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,kind", [("min", "T"), ("mid", "T"), ("max+e8e9", "X")])
def test_full_size_blocks_of_the_chain_models(ctx, model, kind):
    """8 x 4 MiB: table saturation, the 16 MiB MATCH ring, hash-row eviction at scale.  Checked against the
    generator's plaintext and the in-stream SHA-1 (the oracle would need minutes per block at this size)."""
    nb, bs = 8, 4 << 20
    s, _ = synth.stream(model, kind, nblocks=nb, block_size=bs, first_block=1000)
    got = ctx.decompress(s, verify_sha1=True)
    assert ctx.stats().kernel_kind == 3
    assert got.size == nb * bs
    for b in range(nb):
        assert np.array_equal(got[b * bs:(b + 1) * bs], synth.plain(kind, 1000 + b, bs)), b


def _repetitive_plaintexts(n=48 << 10):
    """Inputs whose consecutive contexts share hash rows, mixer rows and MATCH candidates: the cases in which a row the
    decoder wave has just written back (or still holds) is also among the rows requested for the next nibble / byte —
    by the decoder wave itself or, ahead of it, by the helper wave of zh_chain2.hip."""
    rng = np.random.default_rng(77)
    yield "zeros", np.zeros(n, np.uint8)
    yield "ff", np.full(n, 255, np.uint8)
    yield "period2", np.tile(np.array([0x41, 0x42], np.uint8), n // 2)
    yield "period3", np.tile(np.array([1, 2, 3], np.uint8), n // 3 + 1)[:n]
    yield "period256", np.tile(np.arange(256, dtype=np.uint8), n // 256)
    yield "runs", np.repeat(rng.integers(0, 256, n // 64, dtype=np.uint8), 64)
    yield "two_symbols", rng.integers(0, 2, n, dtype=np.uint8) * 0x0f + 0x10
    yield "low_nibbles", rng.integers(0, 16, n, dtype=np.uint8)
    yield "high_nibbles", (rng.integers(0, 16, n, dtype=np.uint8) << 4).astype(np.uint8)
    rep = rng.integers(0, 256, 700, dtype=np.uint8)
    yield "long_repeats", np.concatenate([rep, rng.integers(0, 256, 300, dtype=np.uint8)] * (n // 1000))


@pytest.mark.parametrize("model", ["min", "mid", "max", "max+e8e9"])
def test_chain_models_on_repetitive_plaintext(ctx, model):
    """One stream of ten blocks per model; GPU output against the oracle's and the plaintext."""
    names, plains, blocks = [], [], []
    for name, d in _repetitive_plaintexts():
        names.append(name)
        plains.append(d.tobytes())
        blocks.append(synth.compress_block(model, d))
    s = b"".join(blocks)
    want = b"".join(plains)
    assert oracle.decompress(s, cap=len(want) + 16) == want
    got = ctx.decompress(s, verify_sha1=True).tobytes()
    assert ctx.stats().kernel_kind == 3
    off = 0
    for name, p_ in zip(names, plains):
        assert got[off:off + len(p_)] == p_, (model, name)
        off += len(p_)
    assert len(got) == len(want)


@pytest.mark.parametrize("schedule", ["lpt", "queue"])
def test_two_ranks_on_one_gpu_run_the_sharded_hip_decode(tmp_path, schedule):
    """bench.py's N > 1 path — shared stream, broadcast table, plan over the estimated block costs (or, `queue`, chunks
    pulled from the counter on the job's store), zpaqhip_decode_blocks_device(ids), all_gather of the results — rehearsed
    with two gloo ranks that share this box's one GPU."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29577" if schedule == "lpt" else "29579", WORLD_SIZE="2")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--share-gpu", "--model", "mid",
           "--blocks", "5", "--block-bytes", "40000", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--gen-threads", "2",
           "--schedule", schedule, "--queue-blocks", "2"]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
             for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1].decode()[-2000:] for o in outs]
    line = json.loads(outs[0][0].decode().strip().splitlines()[-1])
    assert line["bit_exact"] is True and line["n_gpus"] == 2 and line["value"] > 0
    assert sum(line["config"]["shard_blocks"]) == 10 and line["config"]["kernel_kind"] == 3
    if schedule == "lpt":
        assert sorted(line["config"]["shard_blocks"]) == [5, 5]
    assert len(line["config"]["rank_kernel_ms"]) == 2 and max(line["config"]["rank_kernel_ms"]) > 0


def _stored_block(d):
    """An unmodelled (n = 0) store block, Decoder.cs:58-67: [len32 BE, bytes]*, 0, in two chunks."""
    store_hdr = zpaql.assemble("comp 0 0 0 0 0 hcomp halt end").header
    pay = b"\0" + d                                            # leading 0 = PASS
    cut = len(pay) // 3
    body = b"".join(len(c).to_bytes(4, "big") + c for c in (pay[:cut], pay[cut:])) + b"\0\0\0\0"
    return (TAG + b"zPQ" + bytes([2, 1]) + store_hdr + b"\x01\0" + str(len(d)).encode() + b"\0\0" + body
            + bytes([253]) + oracle.sha1(d) + bytes([255]))


def _mixed_stream(n_blocks=23, seed=5):
    rng = np.random.default_rng(seed)
    parts, plain = [], []
    for i in range(n_blocks):
        if i % 5 == 3:
            # Chunks longer than one ragged read of the Reader test, so that a read ends inside a chunk (the scan has to ask
            # for more input, not give up)
            d = util.text(int(rng.integers(6000, 20000)), seed=100 + i)
            parts.append(_stored_block(d))
            plain.append(d)
            continue
        model = ("l1", "min", "mid")[i % 3]
        d = util.text(int(rng.integers(0, 9000)), seed=100 + i)
        kw = {}
        if i % 4 == 1:
            kw["comment"] = b"jDC\x01"                      # journaling-style comment: no size
        if i % 4 == 2:
            kw["comment"] = b"123456789012 not a size"      # digits that are not the size (a date, say)
        parts.append(util.block(model, d, **kw))
        plain.append(d)
    return b"".join(parts), b"".join(plain)


def test_pipeline_batches_and_unknown_sizes_cost_one_decode(ctx):
    """Several batches through the H2D / kernel / D2H pipeline; blocks without (or with a wrong) size hint are decoded
    once into provisional slots (zpaqhip_stats.launches counts the kernel launches of the call)."""
    s, want = _mixed_stream()
    for bb in (0, 4, 7):
        got = ctx.decompress(s, out_cap=len(want), verify_sha1=True, batch_blocks=bb).tobytes()
        assert got == want, bb
        st = ctx.stats()
        nbatch = 1 if bb == 0 else -(-23 // bb)
        assert st.launches <= 4 * nbatch, (bb, st.launches)           # <= one launch per kernel family (cm, min, mid, store) and batch: no second pass
        assert st.out_bytes == len(want)
    # a block far larger than its provisional slot (16 x coded size) is the one case that is decoded twice
    big = b"\0" * 3_000_000
    s2 = util.block("l1", big, comment=b"no size")
    assert len(s2) * 16 < len(big)
    assert ctx.decompress(s2, out_cap=len(big), verify_sha1=True).tobytes() == big
    assert ctx.stats().launches == 2
    # a hostile size hint (12-digit "size") neither allocates terabytes nor fails
    s3 = util.block("l1", b"abc" * 1000, comment=b"999999999999")
    assert ctx.decompress(s3, out_cap=3000, verify_sha1=True).tobytes() == b"abc" * 1000
    # a caller's buffer smaller than the plaintext, over three batches: what fits arrives, nothing behind out_cap is touched,
    # *out_len reports the full size
    import ctypes as C
    parts = [util.text(500 + 190 * i, seed=70 + i) for i in range(8)]
    s4 = np.frombuffer(b"".join(util.block(("l1", "min", "mid")[i % 3], d, **({"comment": b"no size"} if i == 4 else {}))
                                for i, d in enumerate(parts)), np.uint8)
    want4 = b"".join(parts)
    for cap in (len(want4) - 1, len(want4) // 2, 0):
        buf = np.full(len(want4) + 64, 0xA5, np.uint8)
        o, err, n = z.make_opts(batch_blocks=3), z.api.Err(), C.c_size_t(0)
        rc = ctx._L.zpaqhip_decompress(ctx._h, s4.ctypes.data, s4.size, buf.ctypes.data, cap, C.byref(n), C.byref(o), C.byref(err))
        assert rc == -20 and n.value == len(want4), (cap, rc, n.value)       # ZPAQHIP_E_OUTPUT_FULL
        assert buf[:cap].tobytes() == want4[:cap] and (buf[cap:] == 0xA5).all(), cap


def test_reader_writer_streaming_in_batches(ctx):
    """zpaqhip_decompress_cb reads incrementally (short reads), scans batch by batch and writes in stream order."""
    s, want = _mixed_stream(n_blocks=31, seed=9)
    for bb in (0, 5):
        pos, out, reads = [0], bytearray(), [0]

        def rd(n):
            k = min(n, 1 + (reads[0] * 7919) % 5000)         # ragged short reads
            reads[0] += 1
            chunk = s[pos[0]:pos[0] + k]
            pos[0] += len(chunk)
            return chunk

        ctx.decompress_cb(rd, out.extend, verify_sha1=True, batch_blocks=bb)
        assert bytes(out) == want, bb
    # trailing garbage and leading junk are skipped like findBlock does
    pos, out = [0], bytearray()
    s2 = b"junk" * 10 + s + b"tail" * 5

    def rd2(n):
        chunk = s2[pos[0]:pos[0] + min(n, 4096)]
        pos[0] += len(chunk)
        return chunk

    ctx.decompress_cb(rd2, out.extend, batch_blocks=3)
    assert bytes(out) == want


def test_good_blocks_before_damage_are_delivered(ctx):
    """Framing damage or a corrupt segment in block k: blocks 0..k-1 arrive, then the error is raised — for the buffer
    form, the Reader/Writer form and the Decompresser mirror (the reference fails only on reaching the damage)."""
    from zpaqsharp_amd import decompresser as D
    a, b, c = util.text(5000, 1), util.text(3000, 2), util.text(700, 3)
    good1, good3 = util.block("l1", a), util.block("mid", c)
    bad = bytearray(util.block("min", b))
    g = z.scan(bytes(bad)).segments[0]
    framing = bytearray(bad); framing[g.data_off - 1] = 9          # reserved byte
    coded = bytearray(bad); coded[g.data_off + 40] ^= 0x20         # inside the coded data
    for dmg, msg in ((bytes(framing), "missing reserved byte"), (bytes(coded), None)):
        s = good1 + dmg + good3
        out = bytearray()
        pos = [0]

        def rd(n):
            chunk = s[pos[0]:pos[0] + min(n, 3000)]
            pos[0] += len(chunk)
            return chunk

        with pytest.raises(z.ZpaqError) as e:
            ctx.decompress_cb(rd, out.extend, batch_blocks=1 if msg else 0)
        if msg:
            assert msg in str(e.value)
        assert bytes(out[:len(a)]) == a and len(out) < len(a) + len(b) + len(c)
        # the mirror: first block complete, then the error where the reference raises it
        d = D.Decompresser(ctx)
        d.setInput(D.BytesReader(s))
        w = D.BytesWriter(); d.setOutput(w)
        assert d.findBlock() and d.findFilename()
        d.readComment(); assert d.decompress() is False; d.readSegmentEnd()
        assert bytes(w.buf) == a and not d.findFilename()
        with pytest.raises(z.ZpaqError):
            if d.findBlock() and d.findFilename():
                d.readComment()
                d.decompress()


def test_multi_device_entry_point_with_contexts_sharing_this_gpu(ctx):
    """zpaqhip_decompress_multi (the C# host's way to use several GPUs): N contexts on N host threads pulling chunks
    from one cost-ordered queue, output in stream order.  This box has one GPU, so the device list repeats it.  Sizes
    from the comments (direct placement); missing / wrong sizes (that block is held back and put in place, nothing is
    decoded twice); damage behind good blocks (they are delivered, then the damaged block's error)."""
    s, want = _mixed_stream(n_blocks=19, seed=3)                 # some comments carry no or a bogus size
    for devs, qb in (([0], 0), ([0, 0], 4), ([0, 0, 0], 3), ([0, 0], 1)):
        per = []
        assert z.decompress_multi(devs, s, verify_sha1=True, queue_blocks=qb, per_device=per).tobytes() == want, devs
        assert sum(int(p_.blocks) for p_ in per) == 19 and len(per) == len(devs)        # every block decoded once
        assert sum(int(p_.launches) for p_ in per) == (1 if qb == 0 else -(-19 // qb))   # chunks taken
        assert sum(int(p_.out_bytes) for p_ in per) == len(want)
    parts = [util.text(20000 + 3000 * i, seed=50 + i) for i in range(9)]
    s2 = b"".join(util.block(("l1", "mid", "min")[i % 3], d) for i, d in enumerate(parts))   # every block sized: placed path
    assert z.decompress_multi([0, 0], s2, verify_sha1=True, queue_blocks=2).tobytes() == b"".join(parts)
    # wrong sizes, too small and too large, between sized blocks: only those blocks are re-placed
    blocks = [util.block("l1", parts[0]), util.block("l1", parts[1], comment=b"5"), util.block("mid", parts[2]),
              util.block("min", parts[3], comment=b"900000"), util.block("l1", parts[4]), util.block("mid", parts[5], comment=b"x"),
              util.block("l1", parts[6], comment=str(len(parts[6]) + 1).encode()), util.block("l1", parts[7])]
    wrong = b"".join(blocks)
    for qb in (1, 3, 0):
        per = []
        got = z.decompress_multi([0, 0], wrong, verify_sha1=True, queue_blocks=qb, per_device=per).tobytes()
        assert got == b"".join(parts[:8]), qb
        assert sum(int(p_.blocks) for p_ in per) == 8
    assert z.decompress_multi([0, 0], wrong, out_cap=len(b"".join(parts[:8])), queue_blocks=2).tobytes() == b"".join(parts[:8])
    # damage in block 5 of 9: blocks 0-4 arrive, the error is the one a single context reports
    cut = z.scan(s2).blocks
    bad = bytearray(s2)
    bad[z.scan(s2).segments[cut[5].first_seg].data_off + 30] ^= 4
    with pytest.raises(z.ZpaqError) as e1:
        ctx.decompress(bytes(bad))
    for qb in (2, 0):
        got, e2 = z.decompress_multi([0, 0], bytes(bad), queue_blocks=qb, partial=True)
        assert e2 is not None and e2.code == e1.value.code and e2.block == 5
        assert got.tobytes() == b"".join(parts[:5])
    with pytest.raises(z.ZpaqError):
        z.decompress_multi([0, 0], bytes(bad))
    # what the two entry points deliver of the DAMAGED block differs, on purpose (zpaqhip.h): the Reader/Writer form writes as
    # it decodes, like the reference, so the bytes block 5 produced before its error arrive too; the multi-device form
    # places whole blocks and stops in front of it — its plaintext is a prefix of the other's
    single = bytearray()
    with pytest.raises(z.ZpaqError):
        ctx.decompress_cb(lambda n, _p=[0]: (lambda c: (_p.__setitem__(0, _p[0] + len(c)), c)[1])(bytes(bad)[_p[0]:_p[0] + n]), single.extend)
    front = b"".join(parts[:5])
    assert bytes(single[:len(front)]) == front and len(front) <= len(single) < len(front) + len(parts[5])
    assert bytes(single[len(front):]) == parts[5][:len(single) - len(front)]
    z.multi_trim()                                               # the contexts the calls above kept are destroyed; the next call makes new ones
    assert z.decompress_multi([0, 0], s2, verify_sha1=True, queue_blocks=2).tobytes() == b"".join(parts)


def test_multi_device_queue_on_an_archive_that_mixes_models(ctx):
    """An archive of l1 / mid / max blocks of uneven sizes, two contexts on this GPU pulling from the cost-ordered queue:
    bit-exact, every block decoded once, both device threads at work.  (Kernel times of two contexts that share one GPU say
    nothing about balance — their allocations and kernels serialise each other; the plan's balance is measured below.)"""
    rng = np.random.default_rng(12)
    parts, blocks = [], []
    for i in range(120):
        model = ("l1", "mid", "max")[i % 3]
        d = util.text(int(rng.integers(8000, 40000)), seed=300 + i)
        parts.append(d)
        blocks.append(synth.compress_block(model, np.frombuffer(d, np.uint8)))
    s = b"".join(blocks)
    want = b"".join(parts)
    per = []
    got = z.decompress_multi([0, 0], s, verify_sha1=True, queue_blocks=2, per_device=per).tobytes()
    assert got == want
    assert sum(int(p_.blocks) for p_ in per) == 120 and sum(int(p_.launches) for p_ in per) == 60
    assert min(int(p_.launches) for p_ in per) >= 10, [int(p_.launches) for p_ in per]


def test_cost_weighted_plan_balances_kernel_time_on_an_archive_that_mixes_models(ctx):
    """The weights of the multi-GPU plan (zpaqhip_block_costs: plaintext bytes x cycles per byte of the block's
    kernel) against the clock: 1 800 blocks of the l1 / mid / max models in three sizes (more blocks per kernel family and
    shard than the GPU has CUs, so a shard's kernel time is its work, not its longest block), dealt to two ranks
    longest-first; each rank's shard is decoded by zpaqhip_decode_blocks_device(ids = shard) — one after the other on
    this box's one GPU — and their kernel times (HIP events) must agree within 10 %.  The round-2 weights (coded bytes)
    put an l1 block above a max block of the same plaintext although it decodes 18 x faster: their plan is timed beside it."""
    import torch
    from zpaqsharp_amd import multigpu
    streams = []
    for mi, model in enumerate(("l1", "mid", "max")):
        for si, size in enumerate((4096, 8192, 16384)):
            st, _ = synth.stream(model, "T", nblocks=200, block_size=size, first_block=1000 * (3 * mi + si), threads=8)
            streams.append(st)
    stream = np.concatenate(streams)
    dev = torch.device("cuda", 0)
    job = multigpu.ShardedJob.single(ctx, stream, dev)
    sc = job.sc
    assert sc.n_blocks == 1800
    sizes = [int(b.usize_hint) for b in sc.blocks]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_out = torch.zeros(int(off[-1]), dtype=torch.uint8, device=dev)
    costs = [int(x) for x in z.block_costs(stream, sc)]
    coded = [sum(int(sc.segments[b.first_seg + i].data_len) for i in range(b.n_seg)) for b in sc.blocks]

    def run(plan):
        times = []
        for shard in plan:
            job.shard = shard
            for _ in range(2):                                   # (the first pass of a shard allocates)
                t = job.decode(d_out, [int(off[b]) for b in shard], [sizes[b] for b in shard], verify_sha1=True)
            assert all(int(t[b, 0]) == 0 and int(t[b, 1]) == sizes[b] for b in shard)
            times.append(job.kernel_ms)
        return times
    k = run(multigpu.lpt_assign(costs, 2))
    assert abs(k[0] - k[1]) / max(k) < 0.10, k
    k_old = run(multigpu.lpt_assign(coded, 2))
    print("kernel ms per rank: cost-weighted plan", k, "coded-bytes plan", k_old)


def test_kernel_families_side_by_side_and_one_after_the_other_agree(ctx):
    """A batch whose blocks need several kernels (l1, min, mid, max, stored) runs them on forked streams with one arena
    region each; ZPAQHIP_SERIAL_FAMILIES=1 is the round-2 order (one family after the other in one region).  Same
    results either way, every segment's SHA-1 verified."""
    s, want = _mixed_stream(n_blocks=31, seed=21)
    extra = [util.text(30000, seed=400 + i) for i in range(4)]
    s2 = s + b"".join(util.block(m, d) for m, d in zip(("max", "mid", "max", "l1"), extra))
    want2 = want + b"".join(extra)
    got = ctx.decompress(s2, verify_sha1=True).tobytes()
    assert got == want2 and ctx.stats().launches >= 5
    os.environ["ZPAQHIP_SERIAL_FAMILIES"] = "1"
    try:
        assert ctx.decompress(s2, verify_sha1=True).tobytes() == want2
    finally:
        del os.environ["ZPAQHIP_SERIAL_FAMILIES"]


def test_launches_and_blocks_in_flight_are_the_plan_s(ctx):
    """The launch plan (zh_dec_plan.h, tests/test_dec_plan.py on the host) on a real launch: two blocks of 4 KiB of each of
    l1, min, mid, max and stored are five kernel groups, one launch each, side by side or one after the other; a group has
    min(2, slots) blocks in flight, and max_concurrent = 1 leaves every group one slot.  (_mixed_stream has no max block: the
    stream is built here.)"""
    plain = [util.text(4096, seed=700 + i) for i in range(10)]
    s = b"".join(_stored_block(d) if i % 5 == 4 else util.block(("l1", "min", "mid", "max")[i % 5], d) for i, d in enumerate(plain))
    want = b"".join(plain)
    families = 5
    assert ctx.decompress(s, verify_sha1=True).tobytes() == want
    assert (ctx.stats().launches, ctx.stats().concurrent) == (families, 2)
    os.environ["ZPAQHIP_SERIAL_FAMILIES"] = "1"
    try:
        assert ctx.decompress(s, verify_sha1=True).tobytes() == want
        assert (ctx.stats().launches, ctx.stats().concurrent) == (families, 2)
    finally:
        del os.environ["ZPAQHIP_SERIAL_FAMILIES"]
    assert ctx.decompress(s, verify_sha1=True, max_concurrent=1).tobytes() == want
    assert (ctx.stats().launches, ctx.stats().concurrent) == (families, 1)


def test_nibble_kernels_and_their_assembly_loops_match_the_oracle(ctx):
    """zh_nibble.hip (round 5): the built-in min and mid models decoded a nibble at a time, the byte loop in hand-laid assembly
    (zh_nb_fast.h / zh_nb_fast_mid.h) with the C++ form of the same loop for every byte the assembly does not take.  Inputs
    that walk every way out of and back into the assembly loop — blocks shorter than its 40-byte look-ahead, empty and
    one-byte segments, several segments per block, chunk refills on incompressible data, 256-byte output flushes at odd block
    offsets — and the ones that stress its forwarding and patch paths: runs (every level trains the entry the next one
    reads), two-symbol data (hash rows of one bucket written back and probed again at once), long repeats (MATCH verify
    beyond 64 bytes).  Both kernels (opts.kernel 0: nibble, 9: bit at a time) against the oracle and the plaintext."""
    rng = np.random.default_rng(2025)
    cases = {
        "text": util.text(200000, seed=21),
        "tiny": b"xyz",
        "zeros": bytes(70000),
        "runs": np.repeat(rng.integers(0, 256, 3000, dtype=np.uint8), 37).tobytes(),
        "two": rng.integers(0, 2, 90000, dtype=np.uint8).tobytes(),
        "random": rng.integers(0, 256, 120000, dtype=np.uint8).tobytes(),
        "repeat": (util.text(700, seed=5) * 200)[:130000],
        "period3": (b"abc" * 40000)[:100001],
    }
    for model in ("min", "mid"):
        m = models.get(model)
        for name, data in cases.items():
            s = util.block(model, data)
            want = oracle.decompress(s, cap=len(data) + 16) if len(data) <= 130000 else data
            assert want == data
            for kernel in (0, 9):
                got = ctx.decompress(s, verify_sha1=True, kernel=kernel, out_cap=len(data) + 16).tobytes()
                assert got == data, (model, name, kernel)
        # several segments, some empty, in one block; then many blocks at odd output offsets in one launch
        parts = [cases["text"][:33333], b"", b"q", cases["runs"][:20001], cases["random"][:7]]
        c = oracle.Compressor(400000)
        c.write_tag(); c.start_block(m.header)
        for i, part in enumerate(parts):
            c.start_segment(b"f%d" % i, str(len(part)).encode())
            if i == 0:
                c.post_process(m.pcomp)
            c.compress(part)
            c.end_segment(oracle.sha1(part))
        c.end_block()
        ms = c.getvalue(); c.close()
        assert ctx.decompress(ms, verify_sha1=True).tobytes() == b"".join(parts), model
        sizes = [1, 39, 40, 41, 255, 256, 257, 1000, 4097, 30011]
        blocks = [util.text(n, seed=100 + n) for n in sizes] * 3
        st = b"".join(util.block(model, d) for d in blocks)
        assert ctx.decompress(st, verify_sha1=True).tobytes() == b"".join(blocks), model
        # damage: whatever the oracle makes of a flipped bit or a cut stream (garbage that ends in an error, or an error at once),
        # the assembly loop's range tests and its hand-over to the general form report the same
        good = util.block(model, cases["text"][:60000])
        g = z.scan(good).segments[0]
        for trial in range(8):
            dmg = bytearray(good)
            pos = int(g.data_off + rng.integers(4, g.data_len - 8))
            dmg[pos] ^= 1 << int(rng.integers(0, 8))
            if bytes(dmg[pos - 3:pos + 4]).count(0) >= 4:
                continue
            for stream in (bytes(dmg), good[:g.data_off + g.data_len // 2] + b"\0\0\0\0" + bytes([254, 255])):
                try:
                    want = ("ok", oracle.decompress(stream, cap=1 << 20))
                except oracle.OracleError as e:
                    want = ("err", str(e))
                try:
                    got = ("ok", ctx.decompress(stream).tobytes())
                except z.ZpaqError as e:
                    got = ("err", str(e))
                assert got == want, (model, trial, pos)
