"""zh_stream_plan.h — the rules of the whole-stream pipeline (batches, staging slots, the second pass, the first failure, what is
delivered where) and of zpaqhip_decompress_multi (queue, slots, outcome, settle_places) — driven on the host in a stand-alone
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
E_HM_TOO_BIG, E_OUTPUT_FULL, E_CORRUPT, E_SKIPPED = -6, -20, -1, -100
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
            if head[0] in ("slots", "batches", "second", "deliver", "queue", "places") and len(head) >= 2 and "=" not in head[1]:
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
