"""zh_stream_plan.h — the rules of the whole-stream pipeline (batches, staging slots, the second pass, the first failure, what is
delivered where), of zpaqhip_decompress_multi (queue, slots, outcome, settle_places) and of zpaqhip_decompress_device (direct
and staged placing, moves, the second decode, the gather, the result records) — driven on the host in a stand-alone
C++ program built with -fsanitize=address,undefined (tests/native/stream_plan_main.cpp).  The program copies with memcpy between
heap buffers of exactly the planned sizes, so a rule that would write past a caller's out_cap is an ASan report here, not a heap
overrun in a GPU run.  No GPU, and no Python under a sanitizer."""
import os
import shutil
import subprocess

import pytest

import oracle
from tests import chain_cases as cc
from tests import util
from zpaqsharp_amd import method, multigpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zpaqsharp_amd", "csrc")
NONE = (1 << 64) - 1                                      # no size in the comment
KIB, MIB = 1 << 10, 1 << 20
E_HM_TOO_BIG, E_OUTPUT_FULL, E_CORRUPT, E_SKIPPED, E_SHA1 = -6, -20, -1, -100, -21
BATCH_BLOCKS = (1, 2, 3, 7, 8, 0)
READS = (0, 97, 777)                                      # the memory source, callback sources with short reads


def _tok(v):
    return "-" if v == NONE else str(v)


def plain(g, n):
    """stream_plan_main.cpp's plaintext of block g."""
    return bytes((g * 53 + i * 7 + 1) & 255 for i in range(n))


# ---- the streams of the batch cases: seven blocks of at most 2 KiB of plaintext
def _blocks():
    out = []
    for i in range(7):
        d = util.text(300 + 250 * i, seed=40 + i)
        if i == 5:                                        # level 4's text model: a header of its own
            out.append((oracle.compress_block(method.model_of(cc.M4)[0].header, d), len(d)))
        else:
            kw = {"comment": b"jDC\x01"} if i == 2 else {}
            out.append((util.block(("l1", "min", "mid")[i % 3], d, **kw), NONE if i == 2 else len(d)))
    return out


def _streams():
    blocks = _blocks()
    raw = [b for b, _ in blocks]
    start = [sum(len(b) for b in raw[:k]) for k in range(8)]
    whole = b"".join(raw)
    hdr_off = 16 + 2                                      # tag, level, type; then the header
    bad = bytearray(whole)
    bad[start[3] + hdr_off + 2] = 33                      # hh = 33: the framing scan passes it, the model builder says "H too big"
    return blocks, start, {
        "whole": (whole, 7, None),
        "cut-header": (whole[:start[4] + hdr_off + 5], 4, "damage"),
        "cut-data": (whole[:start[5] - 40], 4, "damage"),
        "cut-end": (whole[:start[5]], 5, None),
        "bad-model": (bytes(bad), 3, "model"),
    }


def _parse_batches(lines):
    out = []
    for ln in lines:
        kind, _, rest = ln.partition(" ")
        f = dict(kv.split("=") for kv in rest.split(" "))
        if kind == "batch":
            out.append({**{k: int(v) for k, v in f.items()}, "rows": []})
        else:
            out[-1]["rows"].append(ln)
    return out


# ---- restatements
def slot_rule(hint, coded, budget):
    if hint != NONE and hint <= 1 << 40 and hint <= budget:
        return hint
    return min(max(16 * coded, 64 * KIB), 256 * MIB)


REAL = [300, 0, 120, 77, 200, 64]                         # the delivery cases' batch: block 3 overflowed its slot and was redone
SLOT = [300, 0, 120, 40, 200, 64]
FIX = [0, 0, 0, 1, 0, 0]
TOTAL = sum(REAL)
PLACED = [(100, 1, 0, 40), (60, 1, 40, 90), (80, 0, 130, 80), (50, 0, 210, 50)]   # real, redone, place, place_cap; cap = 200, blk0 = 2
SETTLE = [(200, 90), (100, 100), (50, 120), (NONE, 70), (0, 0), (60, 60), (10, 40), (80, 80)]   # promised, real


def _deliver_case(name, form, cap, upto, partial, total0=0):
    rows = " ".join("%d %d %d 0 0" % (r, s, f) for r, s, f in zip(REAL, SLOT, FIX))
    return "deliver %s %s %d %d %d %d 0 %d %s" % (name, form, cap, upto, partial, total0, len(REAL), rows)


def _delivered(upto, partial):
    return b"".join(plain(b, REAL[b]) for b in range(min(upto, 6))) + (plain(upto, min(partial, REAL[upto])) if upto < 6 else b"")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stream_plan")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the stand-alone check of the stream rules"
    exe = str(tmp / "stream_plan")
    about = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = "-static-libsan" if "clang" in about else "-static-libasan"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           static, "-I", CSRC, os.path.join(ROOT, "tests", "native", "stream_plan_main.cpp"),
                           os.path.join(CSRC, "zh_framing.cpp"), "-o", exe])

    def go(cases):
        """{case name: its printed lines} of a list of case lines."""
        path = tmp / "cases.txt"
        path.write_text("\n".join(cases) + "\n")
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        got = {}
        for line in r.stdout.split("\n")[:-1]:
            head = line.split(" ")
            if head[0] in ("slots", "batches", "second", "deliver", "queue", "places", "device", "modelcut") and len(head) >= 2 and "=" not in head[1]:
                cur = got.setdefault(head[1], [line])
            elif head[0] == "limit":
                got[" ".join(head[:3])] = [line]
            else:
                cur.append(line)
        return got
    go.tmp = tmp
    return go


def _ints(line):
    v = line.split("=", 1)[1]
    return [int(x) for x in v.split(",")] if v else []


def test_batch_limits(run):
    got = run(["limit 0 0", "limit 0 1", "limit 0 3", "limit 5 0", "limit 5 4"])
    assert got["limit 0 0"] == ["limit 0 0 min_blocks=512 min_blocks_other=256 min_bytes=33554432 max_blocks=4096"]
    assert got["limit 0 1"][0].endswith(got["limit 0 0"][0][9:])
    assert "min_blocks=512 min_blocks_other=768 " in got["limit 0 3"][0]
    for k in ("limit 5 0", "limit 5 4"):
        assert got[k][0].endswith("min_blocks=5 min_blocks_other=0 min_bytes=0 max_blocks=5")


def test_staging_slots(run):
    big = 1 << 42
    edge = [(NONE, c) for c in (4095, 4096, 4097, 16 * MIB - 1, 16 * MIB, 16 * MIB + 1)]
    hints = [(NONE, 100), (1234, 100), (1 << 40, 100), ((1 << 40) + 1, 100), (999999999999, 100), (3 << 30, 5000)]
    cases = {
        "edge": (big, edge), "hints-big": (big, hints), "hints-1g": (1 << 30, hints[:2] + hints[4:]),
        "short-a": (12000, [(1000, 1), (5000, 1), (3000, 1), (NONE, 100), (2000, 1)]),
        "short-b": (5500, [(1000, 1), (5000, 1), (3000, 1), (NONE, 100), (2000, 1)]),
        "ties": (8200, [(4000, 1), (4000, 1), (4000, 1), (100, 1), (4000, 1)]),
        "nothing-fits": (10, [(4000, 1), (NONE, 1)]),
        "empty": (10, []),
    }
    got = run(["slots %s %d %d %s" % (n, bud, len(bl), " ".join(_tok(h) + " " + str(c) for h, c in bl)) for n, (bud, bl) in cases.items()])
    table = {n: (_ints(got[n][1]), _ints(got[n][2]), int(got[n][0].split("total=")[1])) for n in cases}
    assert table["edge"][0] == [65536, 65536, 65552, 268435440, 268435456, 268435456]
    assert table["hints-big"][0] == [65536, 1234, 1 << 40, 65536, 999999999999, 3 << 30]
    assert table["hints-1g"][0] == [65536, 1234, 65536, 80000]           # the 12-digit "size" and the 3 GiB one: above the budget
    assert table["short-a"] == ([1000, 5000, 3000, 0, 2000], [0, 1000, 6000, 9000, 9000], 11000)
    assert table["short-b"] == ([1000, 0, 0, 0, 2000], [0, 1000, 1000, 1000, 1000], 3000)
    assert table["nothing-fits"] == ([0, 0], [0, 0], 0) and table["empty"] == ([], [], 0)
    for n, (budget, bl) in cases.items():
        cap, off, total = table[n]
        full = [slot_rule(h, c, budget) for h, c in bl]
        assert all(c in (0, f) for c, f in zip(cap, full)), n
        assert off == [sum(cap[:k]) for k in range(len(cap))] and total == sum(cap) and total <= budget, n
        dropped = [f for c, f in zip(cap, full) if c == 0 and f]
        assert not dropped or sum(full) > budget, n
        assert not dropped or min(dropped) >= max(cap), n                  # nothing dropped is smaller than something kept
        assert not dropped or total + min(dropped) > budget, n             # ... and no more was dropped than had to be
    assert sorted(table["ties"][0]) == [0, 0, 100, 4000, 4000]


def test_batches_are_the_same_from_memory_and_from_a_reader(run):
    blocks, start, streams = _streams()
    cases, names = [], []
    for sname, (data, _, _) in streams.items():
        path = run.tmp / (sname + ".zpaq")
        path.write_bytes(data)
        for bb in BATCH_BLOCKS:
            for rd in READS:
                names.append((sname, bb, rd))
                cases.append("batches %s-%d-%d %s %d 0 %d" % (sname, bb, rd, path, bb, rd))
    got = run(cases)
    for sname, (data, n_good, trouble) in streams.items():
        for bb in BATCH_BLOCKS:
            mem = got["%s-%d-0" % (sname, bb)][1:]
            for rd in READS[1:]:
                assert got["%s-%d-%d" % (sname, bb, rd)][1:] == mem, (sname, bb, rd)
            bt = _parse_batches(mem)
            # whole blocks in stream order, every batch but the last of batch_blocks blocks
            size = bb or 512
            assert sum(b["blocks"] for b in bt) == n_good, (sname, bb)
            assert [b["blocks"] for b in bt[:-1]] == [size] * (len(bt) - 1) and bt[-1]["blocks"] <= size
            assert [b["last"] for b in bt[:-1]] == [0] * (len(bt) - 1)
            assert bt[-1]["last"] == 1 or (bt[-1]["blocks"] == 0 and trouble is None)
            assert all(b["rc_after"] == 0 for b in bt[:-1])
            k = 0
            for b in bt:
                assert b["blk0"] == k and b["seg0"] == k and b["segs"] == b["blocks"]
                if b["blocks"]:
                    assert b["stream_off"] == start[k] and b["len"] == start[k + b["blocks"]] - start[k]
                for j in range(b["blocks"]):
                    raw, hint = blocks[k + j]
                    if sname == "bad-model" and k + j == 3:
                        raw = data[start[3]:start[4]]
                    row = b["rows"][j]
                    assert row.startswith("block tag=%d hdr=%d+" % (start[k + j] - start[k], start[k + j] - start[k] + 18)), row
                    assert " end=%d segs=%d+1 " % (start[k + j + 1] - start[k], j) in row, row
                    assert row.endswith(" hint=%d sum=%d" % (hint, sum(raw) & 0xffff)), row
                k += b["blocks"]
            end = bt[-1]
            if trouble is None:
                assert end["rc_after"] == 0
            else:
                # the error sits behind the batch's last block; the batch ends at the block before it
                assert end["rc_after"] < 0 and end["err_block"] == end["blocks"] and end["blk0"] + end["blocks"] == n_good
            if trouble == "model":
                assert end["rc_after"] == E_HM_TOO_BIG and end["err_seg"] == -1 and end["err_block"] == 3 - end["blk0"]
                assert end["len"] == start[3] - start[end["blk0"]]
    one = _parse_batches(got["bad-model-0-0"][1:])
    assert len(one) == 1 and one[0]["err_block"] == 3 and one[0]["len"] == start[3]
    assert [len(_parse_batches(got["whole-%d-0" % bb][1:])) for bb in BATCH_BLOCKS] == [8, 4, 3, 2, 1, 1]


def test_second_pass_first_failure_and_segment_records(run):
    got = run(["second a 4  100 2 0 40 0 60  50 1 0 80  0 1 %d 30  10 1 0 0" % E_OUTPUT_FULL,
               "second b 3  100 2 0 40 0 60  64 2 0 10 %d 0  16 1 0 7" % E_SKIPPED])
    a, b = got["a"], got["b"]
    assert a[0] == "second a bytes=110" and a[1:5] == ["real=100,80,30,0", "redo=1,2", "off2=0,80", "cap2=80,30"]
    assert a[5] == "first found=1 ok_blocks=2 partial=0 rc=%d code=%d block=12 seg=23" % (E_OUTPUT_FULL, E_OUTPUT_FULL)
    assert b[0] == "second b bytes=0" and b[1:3] == ["real=100,10,7", "redo="]
    assert b[5] == "first found=1 ok_blocks=1 partial=10 rc=%d code=%d block=11 seg=23" % (E_CORRUPT, E_CORRUPT)
    assert b[6:] == ["rec_off=1000,1040,1100,1110,1110", "rec_block=10,10,11,11,12"]


def test_delivery_to_memory_and_to_a_writer(run):
    shapes = [(6, 0), (2, 5), (0, 0)]
    caps = [TOTAL, TOTAL - 1, REAL[0], 0]
    cases = [_deliver_case("mem-%d-%d-%d" % (cap, u, p), "mem", cap, u, p) for cap in caps for u, p in shapes]
    cases += [_deliver_case("wr-%d-%d" % (u, p), "writer", 0, u, p, total0=777) for u, p in shapes]
    cases += [_deliver_case("mem-second-batch", "mem", 150, 6, 0, total0=100), _deliver_case("mem-past-cap", "mem", 150, 6, 0, total0=150)]
    got = run(cases)

    def parts(name):
        lines = got[name][1:]
        copies = [tuple(int(kv.split("=")[1]) for kv in ln.split(" ")[1:]) for ln in lines if ln.startswith("copy ")]
        return copies, int(lines[-2].split("=")[1]), bytes.fromhex(lines[-1].split("=")[1])

    # block 0 and block 2 lie side by side in the staging buffer (block 1 is empty): one copy; block 3 was redone into the
    # second-pass buffer: a copy of its own; blocks 4 and 5 again one
    assert parts("mem-%d-6-0" % TOTAL)[0] == [(0, 0, 420, 0, -1), (1, 0, 77, 420, -1), (0, 460, 264, 497, -1)]
    assert parts("mem-%d-6-0" % (TOTAL - 1))[0] == [(0, 0, 420, 0, -1), (1, 0, 77, 420, -1), (0, 460, 263, 497, -1)]
    assert parts("mem-300-6-0")[0] == [(0, 0, 300, 0, -1)] and parts("mem-0-6-0")[0] == []
    assert parts("mem-%d-2-5" % TOTAL)[0] == [(0, 0, 305, 0, -1)] and parts("mem-%d-0-0" % TOTAL)[0] == []
    for cap in caps:
        for u, p in shapes:
            want = _delivered(u, p)
            copies, total, out = parts("mem-%d-%d-%d" % (cap, u, p))
            assert total == len(want)                                       # counted past the capacity
            assert out == want[:cap] + b"\xee" * (cap - min(cap, len(want))), (cap, u, p)
            assert sum(c[2] for c in copies) == min(cap, len(want))
    for u, p in shapes:
        copies, total, out = parts("wr-%d-%d" % (u, p))
        assert out == _delivered(u, p) and total == 777 + len(out)
        assert copies == [(f, s, n, 777 + d, sp) for f, s, n, d, sp in parts("mem-%d-%d-%d" % (TOTAL, u, p))[0]]
    copies, total, out = parts("mem-second-batch")
    assert copies == [(0, 0, 50, 100, -1)] and total == 100 + TOTAL and out == b"\xee" * 100 + _delivered(6, 0)[:50]
    assert parts("mem-past-cap") == ([], 150 + TOTAL, b"\xee" * 150)


def test_delivery_to_places(run):
    rows = " ".join("%d %d %d %d %d" % (r, r, f, at, pc) for r, f, at, pc in PLACED)
    got = run(["deliver placed placed 200 4 0 1000 2 4 " + rows, "deliver placed-3 placed 200 3 9 0 2 4 " + rows])
    lines = got["placed"][1:]
    copies = [tuple(int(kv.split("=")[1]) for kv in ln.split(" ")[1:]) for ln in lines if ln.startswith("copy ")]
    # block 2: larger than its slot, spilled whole, nothing in place; block 3: smaller than its slot; block 4: straddles the
    # capacity; block 5: behind it
    assert copies == [(1, 0, 100, 0, 2), (1, 100, 60, 40, -1), (0, 160, 70, 130, -1)]
    want = b"\xee" * 40 + plain(3, 60) + b"\xee" * 30 + plain(4, 70)
    assert lines[len(copies)] == "total=1290"                              # every block's size, delivered or not
    assert bytes.fromhex(lines[len(copies) + 1].split("=")[1]) == want
    assert lines[len(copies) + 2] == "sizes=0,0,100,60,80,50"
    assert lines[len(copies) + 3:] == ["spill 2 bytes=" + plain(2, 100).hex()]
    assert "total=240" in got["placed-3"] and "sizes=0,0,100,60,80,0" in got["placed-3"]    # whole blocks only: no partial one


def _costs(nb):
    return [(i * 7919) % 13 + 1 for i in range(nb)]                         # plenty of ties


def test_multi_device_queue_is_multigpu_s(run):
    """The C statement of the queue rule against the Python one (multigpu.default_queue_blocks, multigpu.queue_chunks)."""
    shapes = [(nb, nd, cm) for nb in (1, 2, 7, 256, 300, 2048) for nd in (1, 2, 8) for cm in (0, 1)]
    got = run(["queue q-%d-%d-%d %d %d %d %s" % (nb, nd, cm, nd, cm, nb, " ".join(map(str, _costs(nb)))) for nb, nd, cm in shapes])
    for nb, nd, cm in shapes:
        lines = got["q-%d-%d-%d" % (nb, nd, cm)]
        chunk = multigpu.default_queue_blocks(nb, nd, bool(cm))
        want = multigpu.queue_chunks(_costs(nb), chunk)
        assert lines[0].endswith(" chunk=%d K=%d" % (chunk, len(want))), lines[0]
        assert [_ints(ln.split(" ")[2]) for ln in lines[1:]] == want, (nb, nd, cm)
        assert [int(ln.split(" ")[1][4:]) for ln in lines[1:]] == [int(c[-1] - c[0] + 1 == len(c)) for c in want]
    assert got["q-2048-8-0"][0].endswith("chunk=64 K=32") and got["q-2048-1-1"][0].endswith("chunk=512 K=4")


def test_settle_places(run):
    out_len = sum(r for _, r in SETTLE)
    rows = " ".join(_tok(h) + " " + str(r) for h, r in SETTLE)
    got = run(["places all %d -1 8 %s" % (out_len, rows), "places damaged-5 %d 5 8 %s" % (out_len, rows),
               "places short %d -1 8 %s" % (out_len - 1, rows), "places exact 160 -1 2 100 100 60 60"])
    whole = b"".join(plain(b, r) for b, (_, r) in enumerate(SETTLE))
    assert got["all"][1:3] == ["slot_off=0,200,300,350,350,350,410,420,500", "slot_cap=200,100,50,0,0,60,10,80"]
    assert got["all"][3] == "rc=0 out_len=%d moved=1" % out_len and bytes.fromhex(got["all"][4][4:]) == whole
    front = sum(r for _, r in SETTLE[:5])
    assert got["damaged-5"][3] == "rc=0 out_len=%d moved=1" % front and bytes.fromhex(got["damaged-5"][4][4:]) == whole[:front]
    assert got["short"][3] == "rc=%d out_len=%d moved=0" % (E_OUTPUT_FULL, out_len)
    assert got["exact"][3] == "rc=0 out_len=160 moved=0" and bytes.fromhex(got["exact"][4][4:]) == plain(0, 100) + plain(1, 60)


# ---- zpaqhip_decompress_device: the whole sequence over heap buffers of exactly out_cap, the planned staging bytes and
# fix_bytes.  A case: blocks as (size hint or NONE, plaintext size, segments), out_cap, the staging budget, an optional
# damaged segment (failing from its block's n-th decode on) and an optional segment whose checksum differs.  What is
# expected is worked out here from the case alone.
PLENTY = 1 << 30
HINTS = {
    "right": [(300, 300, 1), (0, 0, 1), (250, 250, 2), (411, 411, 1), (120, 120, 1)],
    "absent": [(NONE, 300, 1), (NONE, 0, 1), (NONE, 250, 2), (NONE, 411, 1), (NONE, 120, 1)],
    "middle": [(300, 300, 1), (250, 250, 2), (NONE, 411, 1), (120, 120, 1), (77, 77, 1)],          # k = 2
    "implausible": [(300, 300, 1), ((1 << 40) + 1, 250, 1), (120, 120, 1)],
    "small": [(300, 300, 1), (100, 250, 2), (411, 411, 1), (120, 120, 1)],
    "large": [(300, 300, 1), (999, 250, 2), (411, 411, 1), (120, 120, 1)],
    "small-large": [(300, 300, 1), (100, 250, 1), (411, 411, 1), (999, 120, 1), (77, 77, 1), (200, 200, 2)],
    # too large by one byte: blocks 2 and 3 are whole, one byte behind their final places, and overlap them
    "large-by-one": [(300, 300, 1), (251, 250, 1), (411, 411, 2), (120, 120, 1)],
    "zeros": [(0, 0, 1), (0, 200, 1), (300, 300, 1), (0, 0, 1), (50, 50, 1)],
    "staged-wrong": [(300, 300, 1), (NONE, 250, 1), (100, 411, 2), (999, 120, 1)],               # wrong hints behind k: slots only
}


def _plausible(h):
    return h != NONE and h <= 1 << 40


class DevCase:
    def __init__(self, name, blocks, out_cap, budget=PLENTY, no_staging=0, damaged=-1, damaged_at=1, sha_bad=-1, rooms=None):
        self.name, self.blocks, self.out_cap = name, blocks, out_cap
        self.line = "device %s %d %d %d %d %d %d %d %s" % (name, out_cap, budget, no_staging, damaged, damaged_at, sha_bad, len(blocks),
                                                         "  ".join("%s %d %d" % (_tok(h), r, n) for h, r, n in blocks))
        nb = len(blocks)
        self.seg_block = [b for b, (_, _, n) in enumerate(blocks) for _ in range(n)]
        self.seg_len = [r // n if i + 1 < n else r - r // n * (n - 1) for _, r, n in blocks for i in range(n)]
        self.first_seg = [self.seg_block.index(b) for b in range(nb)]
        k = next((b for b, (h, _, _) in enumerate(blocks) if not _plausible(h)), nb)
        place = [sum(h for h, _, _ in blocks[:b]) for b in range(k)]
        room = [max(0, min(blocks[b][0], out_cap - place[b])) for b in range(k)]
        # behind k: the slot rule (the hint when plausible and within the budget, else the provisional 64 KiB of these small
        # blocks); `rooms` where the budget drops slots, nothing where the reservation fails
        room += rooms if rooms is not None else [0 if no_staging else (h if _plausible(h) and h <= budget else 64 * KIB) for h, _, _ in blocks[k:]]
        dblock = self.seg_block[damaged] if damaged >= 0 else nb
        count, limit, self.code, self.bad_seg = [0] * nb, nb, 0, -1

        def fail(b, code, seg):
            nonlocal limit
            if b < limit:
                limit, self.code, self.bad_seg = b, code, seg
        for b in range(k):
            count[b] = 1
        if damaged_at == 1 and dblock < k:
            fail(dblock, E_CORRUPT, damaged)
        if limit > k:                                     # the staged blocks are decoded only when something of them can be delivered
            for b in range(k, nb):
                count[b] = 1
            if damaged_at == 1:
                fail(dblock, E_CORRUPT, damaged)
        for b in range(limit):
            count[b] += blocks[b][1] > room[b]
        if damaged_at == 2 and dblock < limit and count[dblock] == 2:
            fail(dblock, E_CORRUPT, damaged)
        if sha_bad >= 0:
            fail(self.seg_block[sha_bad], E_SHA1, sha_bad)
        self.k, self.count, self.limit = k, count, limit
        self.want = b"".join(plain(b, blocks[b][1]) for b in range(limit))
        self.total = len(self.want)
        self.n_res = self.first_seg[limit] + blocks[limit][2] if limit < nb else len(self.seg_len)
        # a hint that promised more than its block holds (a block that failed, or lies behind one that did, holds nothing):
        # blocks behind it were decoded further out in d_out, and what they left behind the delivered bytes stays
        self.tail_clean = limit == nb and all(h <= r for h, r, _ in blocks[:k])

    def check(self, lines):
        head = dict(kv.split("=") for kv in lines[0].split(" ")[2:])
        out = bytes.fromhex(lines[-1].split("=", 1)[1])
        assert len(out) == self.out_cap
        assert int(head["out_len"]) == self.total, self.name
        assert int(head["k"]) == self.k, self.name
        decodes = _ints(lines[1])
        assert max(decodes) <= 2 and decodes == self.count, (self.name, decodes, self.count)
        if self.code:
            assert (int(head["rc"]), int(head["block"]), int(head["seg"])) == (self.code, self.limit, self.bad_seg), self.name
        else:
            assert int(head["rc"]) == (E_OUTPUT_FULL if self.total > self.out_cap else 0) and head["block"] == "-1", self.name
        assert int(head["n_res"]) == self.n_res, self.name
        # the records of the delivered blocks: stream-order offsets
        n_ok = self.first_seg[self.limit] if self.limit < len(self.blocks) else self.n_res
        assert _ints(lines[3])[:n_ok] == [sum(self.seg_len[:s]) for s in range(n_ok)], self.name
        assert _ints(lines[4])[:n_ok] == self.seg_len[:n_ok] and _ints(lines[2])[:n_ok] == [0] * n_ok, self.name
        if self.total <= self.out_cap:
            assert out[:self.total] == self.want, self.name
            assert not self.tail_clean or out[self.total:] == b"\xee" * (self.out_cap - self.total), self.name
        else:                                             # (more than the header promises; every case here gets the exact prefix)
            assert out == self.want[:self.out_cap], self.name
        return head


def _caps(blocks):
    """total + 5, total, total - 1, 0, and one byte into and one byte short of the end of every block."""
    real = [r for _, r, _ in blocks]
    start = [sum(real[:b]) for b in range(len(real) + 1)]
    return sorted({start[-1] + 5, start[-1], start[-1] - 1, 0} | {start[b] + 1 for b in range(len(real))} | {max(0, start[b + 1] - 1) for b in range(len(real))})


def _run_device(run, cases):
    got = run([c.line for c in cases])
    return {c.name: c.check(got[c.name]) for c in cases}


def test_device_form_hints_and_out_cap(run):
    """Every hint set (all right, none, present then absent, implausible, too small, too large, both, too large by one byte,
    zero-length blocks and a hint of 0 on a non-empty block) at every out_cap position: above, at and below the total, one
    byte into and one byte short of the end of every block (directly placed, moved, staged, redone), and 0."""
    cases = [DevCase("%s-%d" % (n, cap), bl, cap) for n, bl in HINTS.items() for cap in _caps(bl)]
    heads = _run_device(run, cases)
    total = {n: sum(r for _, r, _ in bl) for n, bl in HINTS.items()}
    for n in ("right", "absent", "middle", "implausible"):                  # nothing wrong: nothing moved, nothing decoded twice
        h = heads["%s-%d" % (n, total[n] + 5)]
        assert (h["fix"], h["moves"]) == ("0", "0"), n
    assert [heads["%s-%d" % (n, total[n])]["k"] for n in ("right", "absent", "middle", "implausible")] == ["5", "0", "2", "1"]
    assert heads["small-%d" % total["small"]]["moves"] == "2" and heads["small-%d" % total["small"]]["fix"] == str(250 + 411 + 120)
    by_one = heads["large-by-one-%d" % (total["large-by-one"] + 5)]
    assert by_one["moves"] == "2" and by_one["fix"] == "531"
    by_one = heads["large-by-one-%d" % total["large-by-one"]]               # the last block, one byte further out, is clipped: decoded again
    assert by_one["moves"] == "1" and by_one["fix"] == "531"
    assert heads["small-large-%d" % total["small-large"]]["moves"] == "2"   # blocks 2 and 3; 4 and 5 were placed behind out_cap: decoded again
    assert heads["zeros-%d" % total["zeros"]]["moves"] == "2"               # block 3 is empty: it "moves" without an entry


def test_device_form_staging_budget(run):
    bl = [(NONE, 200, 1), (300, 300, 2), (500, 500, 1)]
    cases = []
    for cap in _caps(bl):
        # 65536 + 300 + 500 is over the budget: the largest slot becomes count-only, its block is decoded a second time
        cases.append(DevCase("short-%d" % cap, bl, cap, budget=66000, rooms=[0, 300, 500]))
        cases.append(DevCase("hint-over-%d" % cap, bl, cap, budget=400, rooms=[0, 300, 0]))   # 500 > budget: a provisional slot, dropped too
    for n in ("absent", "middle", "small", "staged-wrong"):
        cases += [DevCase("none-%s-%d" % (n, cap), HINTS[n], cap, no_staging=1) for cap in _caps(HINTS[n])]
    heads = _run_device(run, cases)
    assert heads["short-1005"]["staging"] == "800" and heads["short-1005"]["fix"] == "200"
    assert heads["hint-over-1005"]["staging"] == "300" and heads["hint-over-1005"]["fix"] == "700"
    assert heads["none-absent-1086"]["staging"] == "0" and heads["none-absent-1086"]["fix"] == "1081"


def test_device_form_damage_and_results(run):
    """Whole blocks in front of the lowest failed block are delivered; out_len is their sum; error block, segment and the number
    of result records as zpaqhip_decompress_device gives them."""
    cases = []
    for cap in (2000, 551, 300, 0):
        cases += [
            DevCase("direct-%d" % cap, HINTS["right"], cap, damaged=3),                     # second segment of block 2
            DevCase("direct-first-%d" % cap, HINTS["right"], cap, damaged=0),
            DevCase("staged-%d" % cap, HINTS["middle"], cap, damaged=3),                    # block 2, the first staged one
            DevCase("staged-last-%d" % cap, HINTS["middle"], cap, damaged=5),
            DevCase("direct-of-middle-%d" % cap, HINTS["middle"], cap, damaged=2),          # in front of k: nothing is staged at all
            DevCase("second-decode-%d" % cap, HINTS["small"], cap, damaged=2, damaged_at=2),      # block 1 outgrew its hint
            DevCase("second-decode-staged-%d" % cap, HINTS["staged-wrong"], cap, damaged=3, damaged_at=2),
            DevCase("never-seen-%d" % cap, HINTS["right"], 2000 + cap, damaged=3, damaged_at=2),  # decoded once: no damage shows
            DevCase("sha-direct-%d" % cap, HINTS["right"], cap, sha_bad=4),
            DevCase("sha-moved-%d" % cap, HINTS["large"], cap, sha_bad=3),                  # block 2, moved out of the way
            DevCase("sha-redone-%d" % cap, HINTS["small"], cap, sha_bad=1),
            DevCase("sha-staged-%d" % cap, HINTS["middle"], cap, sha_bad=4),
            DevCase("sha-behind-damage-%d" % cap, HINTS["small-large"], cap, damaged=4, sha_bad=2),
        ]
    heads = _run_device(run, cases)
    assert (heads["direct-2000"]["rc"], heads["direct-2000"]["out_len"], heads["direct-2000"]["n_res"]) == (str(E_CORRUPT), "300", "4")
    assert (heads["sha-moved-2000"]["rc"], heads["sha-moved-2000"]["block"], heads["sha-moved-2000"]["out_len"]) == (str(E_SHA1), "2", "550")
    assert heads["direct-of-middle-2000"]["staging"] == "0"
    # a two-segment block among moved blocks: every record is the stream-order offset (DevCase.check), here spelled out
    got = run([DevCase("two-seg-moved", HINTS["large-by-one"], 1081).line])["two-seg-moved"]
    assert got[3] == "res_off=0,300,550,755,961" and got[4] == "res_len=300,250,205,206,120"


def test_model_cut_is_the_same_through_an_accessor(run):
    """first_bad_model over a function that hands out one header at a time (the device form copies each from the GPU) against
    cut_at_bad_model over the batch's bytes: the same cut, code, block and message."""
    _, _, streams = _streams()
    for sname in ("bad-model", "whole"):
        (run.tmp / (sname + ".zpaq")).write_bytes(streams[sname][0])
    got = run(["modelcut %s %s" % (n, run.tmp / (n + ".zpaq")) for n in ("bad-model", "whole")])
    batch, acc = got["bad-model"][1], got["bad-model"][2]
    assert batch.startswith("batch nb=3 rc=%d block=3 seg=-1 msg=" % E_HM_TOO_BIG) and len(batch.split("msg=")[1]) > 3
    assert acc.startswith("accessor" + batch[5:]) and acc.endswith(" call=0 fetched=4")
    assert got["whole"][1].startswith("batch nb=7 rc=0 ") and got["whole"][2].startswith("accessor nb=7 rc=0 ")
    assert got["whole"][2].endswith(" call=0 fetched=7")
