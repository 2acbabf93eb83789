"""zh_dec_plan.h — the decode driver's launch plan (which kernel decodes a block; slots, waves, workgroups and arena region of
every kernel group) — driven on the host in a stand-alone C++ program built with -fsanitize=address,undefined
(tests/native/dec_plan_main.cpp), against a restatement of the rules written here: include/zpaqhip.h's table for opts.kernel,
max_concurrent and dec_waves, DESIGN.md's arena layout.  No GPU, and no Python under a sanitizer."""
import os
import shutil
import subprocess

import pytest

from tests import chain_cases as cc
from zpaqsharp_amd import method, models, zpaql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zpaqsharp_amd", "csrc")
E_DEVICE_MEM = -23
LDS, TABLES, FIXED, MAX_WAVES = 163840, 79872, 16320, 4   # zh_chain's several-waves kernel (tests/test_dec_waves.py)
BLOCKS = 256                                              # blocks in flight a launch asks for: one per compute unit
STORE_E8, MODEL_E8 = 2, 4                                 # launch flags of kernel 10 / 11
NIBBLE_HAS, CHAIN2_HAS = 0b0110, 0b1110                   # zh_nibble: min, mid; zh_chain2: min, mid, max
# family numbers: a group's work-queue head, arena region and place in the launch order
GENERIC, CM1, CHAIN, MIN, MID, MAX, STORE, MID8, MIN1 = range(9)

# name -> (model, what include/zpaqhip.h calls it)
MODELS = {
    "l1": (models.get("l1"), "cm"),
    "min": (models.get("min"), "min"),
    "mid": (models.get("mid"), "mid"),
    "max": (models.get("max"), "max"),
    "m4": (method.model_of(cc.M4)[0], "level4"),                          # `ci1,1,1,1,2am`: mid's shape, its own HCOMP
    "lz4": (method.model_of("x0,2,5,0,7,21,1c0,0,511")[0], "level4-icm"),  # level 4's one-ICM model
    "level5": (method.model_of(cc.LEVEL5)[0], "chain"),                   # fits the lane-per-component kernel, no specialisation
    "stored": (method.model_of("x0,1,4,0,3,24")[0], "stored"),
    "outside": (zpaql.assemble(cc.DIRECTED["outside-5mix"].cfg), "rest"),  # five mixers: outside every family
}
NAMES = list(MODELS)


def _up256(x):
    return (x + 255) & ~255


def _arena_bytes(m):
    """A block's arena slot: per component its cm / a16 table and its hash table, then H, M of HCOMP and of PCOMP and the
    PCOMP program buffer, every piece on a 256-byte boundary (zh_model.h)."""
    hh, hm, ph, pm, comps, _ = zpaql.parse_header(m.header)
    off = 0
    for c in comps:
        t, a = c[0], c[1:]
        cm = {2: 4 << a[0], 3: 1024, 4: 4 << a[0], 6: 2 << a[0], 8: 2048, 9: 128 << a[0]}.get(t, 0)
        ht = {3: 64 << a[0], 8: 64 << a[0]}.get(t, 0)
        if t == 4:
            ht = 1 << a[1]
        if t == 7:
            cm = (4 << a[0]) * a[2]
        off = _up256(off + ((cm + 15) & ~15))
        off = _up256(off + ((ht + 15) & ~15))
    for piece in (4 << hh, 1 << hm, 4 << ph, 1 << pm, 65536 + 320):
        off = _up256(off + piece)
    return off


def _units(m):
    comps = zpaql.parse_header(m.header)[4]
    return sum(1 if c[0] == 3 else 2 if c[0] == 8 else 0 for c in comps)


def _lds_stride(units):
    return (units * 1024 + FIXED + 15) & ~15


def _fit(name):
    """zpaqhip_dec_chain_plan's waves: none for a model outside the lane-per-component family."""
    if MODELS[name][1] in ("cm", "stored", "rest"):
        return 0
    return min(MAX_WAVES, (LDS - TABLES) // _lds_stride(_units(MODELS[name][0])))


def route(name, K, pp_only):
    """include/zpaqhip.h, opts.kernel: (family, kernel, spec, flags)."""
    what = MODELS[name][1]
    nb = MODEL_E8 if K == 11 else 0
    if K == 1 or what == "rest" or (what == "stored" and pp_only):
        return GENERIC, "generic", 0, 0
    if what == "cm":
        return (CHAIN, "chain", 0, 0) if K == 3 else (CM1, "cm", 0, 0)
    if what == "chain":
        return CHAIN, "chain", 0, 0
    if K == 4:                                           # what auto sends to zh_nibble, zh_chain2 or zh_store: on zh_chain
        return CHAIN, "chain", 0, 0
    if what == "stored":
        return STORE, "store", 0, STORE_E8 if K in (10, 11) else 0
    if what in ("level4", "level4-icm"):
        if K in (5, 9):
            return CHAIN, "chain", 0, 0
        return (MID, "nibble", 2, nb) if what == "level4" else (MIN1, "nibble", 6, nb)
    fam, spec = {"min": (MIN, 1), "mid": (MID, 2), "max": (MAX, 3)}[what]
    if K == 5:
        return fam, "chain", spec, 0
    if what == "max" or K == 9:
        return fam, "chain2", spec, 0
    return fam, "nibble", spec, nb


def plan(case):
    """The lines dec_plan_main prints for a case."""
    K, mc, dw = case["kernel"], case["max_concurrent"], case["dec_waves"]
    prof, budget, cus = case["prof"], case["budget"], case["cus"]
    groups = {}
    for k, (name, _) in enumerate(case["blocks"]):
        r = route(name, K, case["pp_only"])
        g = groups.setdefault(r[0], {"route": r, "blocks": []})
        g["route"] = r
        g["blocks"].append(k)
    groups = [groups[f] for f in sorted(groups)]
    for g in groups:
        ms = [MODELS[case["blocks"][k][0]][0] for k in g["blocks"]]
        g["stride"] = max(_arena_bytes(m) for m in ms)
        g["pcall"] = int(any(m.header[4] or m.header[5] for m in ms))
    out = ["case " + case["name"]]
    out.append("wish %d" % sum(g["stride"] * min(len(g["blocks"]), mc or BLOCKS) for g in groups))
    need = total = 0
    for g in groups:
        n, (fam, kernel, spec, flags) = len(g["blocks"]), g["route"]
        max_slots = budget // g["stride"]
        if max_slots == 0:
            return out + ["error %d %d" % (E_DEVICE_MEM, E_DEVICE_MEM)]
        # single-CM blocks: one per workgroup up to one per compute unit, beyond that two per workgroup
        x2 = kernel == "cm" and not prof and K != 2 and (K == 6 or (not mc and n > BLOCKS))
        slots = min(mc or (2 * BLOCKS if x2 else BLOCKS), max_slots, n)
        if x2:
            slots += slots & 1
            if slots > max_slots:
                slots = max_slots & ~1
                if slots < 2:
                    x2, slots = False, 1
        waves = pool = lds_stride = 0
        grid = slots // 2 if x2 else slots
        if kernel == "chain" and spec == 0 and not prof and dw >= 2:
            names = [case["blocks"][k][0] for k in g["blocks"]]
            units = max(_units(MODELS[nm][0]) if _fit(nm) else 0 for nm in names)
            wgs = min(slots, cus)                        # the blocks spread over the compute units first
            w = min(min(_fit(nm) for nm in names), dw, -(-n // wgs))
            room = min(max_slots, mc or 1 << 32)
            while w > 1 and wgs * w > room:              # memory short of a slot per wave: the waves go before the workgroups
                w -= 1
            if w > 1:
                waves, pool, lds_stride, grid, slots = w, units * 1024, _lds_stride(units), wgs, wgs * w
        g.update(x2=int(x2), slots=slots, grid=grid, waves=waves, pool=pool, lds_stride=lds_stride, off=total)
        need = max(need, slots * g["stride"])
        total += _up256(slots * g["stride"])
    side = len(groups) > 1 and total <= budget and not case["serial"]
    base, order_all, concurrent, kind = 0, [], 0, 0
    for g in groups:
        fam, kernel, spec, flags = g["route"]
        order = sorted(g["blocks"], key=lambda k: -case["blocks"][k][1])     # stable: equal weights keep their order
        out.append("group fam=%d kernel=%s spec=%d flags=%d x2=%d pcall=%d grid=%d slots=%d waves=%d pool=%d lds_stride=%d stride=%d off=%d base=%d order=%s"
                   % (fam, kernel, spec, flags, g["x2"], g["pcall"], g["grid"], g["slots"], g["waves"], g["pool"], g["lds_stride"],
                      g["stride"], g["off"] if side else 0, base, ",".join(map(str, order))))
        base += len(order)
        order_all += order
        concurrent = max(concurrent, min(g["slots"], len(order)) if g["waves"] > 1 else g["slots"])
        kind = max(kind, 1 if kernel in ("generic", "store") else 2 if kernel == "cm" else 3)
    out.append("sorted=" + ",".join(map(str, order_all)))
    out.append("plan side=%d arena=%d launches=%d concurrent=%d kind=%d" % (side, total if side else need, len(groups), concurrent, kind))
    return out


def _case(name, blocks, kernel=0, max_concurrent=0, dec_waves=0, pp_only=0, prof=0, serial=0, cus=256, budget=1 << 40):
    return dict(name=name, blocks=blocks, kernel=kernel, max_concurrent=max_concurrent, dec_waves=dec_waves, pp_only=pp_only,
                prof=prof, serial=serial, cus=cus, budget=budget)


def _weights(name, n):
    return [(name, 1000 + (k * 7919) % 613) for k in range(n)]      # distinct enough to be reordered, with repeats


def _cases():
    out = []
    stride = {n: _arena_bytes(MODELS[n][0]) for n in NAMES}
    # routing: every model under every kernel, one block each
    for K in (0, 1, 2, 3, 4, 5, 6, 9, 10, 11):
        for pp in (0, 1):
            for n in NAMES:
                out.append(_case(f"route-{n}-k{K}-pp{pp}", [(n, 5)], kernel=K, pp_only=pp))
    # slots of single-CM blocks: the two-per-workgroup form above 256 blocks, its rounding to even, its fallback to one slot
    for n in (1, 256, 257, 600):
        for K in (0, 2, 6):
            for mc in (0, 1, 7):
                out.append(_case(f"slots-{n}-k{K}-mc{mc}", _weights("l1", n), kernel=K, max_concurrent=mc))
            for s in (1, 2, 3):
                out.append(_case(f"slots-{n}-k{K}-mem{s}", _weights("l1", n), kernel=K, budget=s * stride["l1"]))
            out.append(_case(f"slots-{n}-k{K}-prof", _weights("l1", n), kernel=K, prof=1))
    # dec_waves on four compute units
    for n in (3, 4, 5, 16, 17):
        for dw in (0, 1, 2, 4):
            out.append(_case(f"waves-min-{n}-dw{dw}", _weights("min", n), kernel=4, dec_waves=dw, cus=4))
    mixed = [(("min", "m4")[k % 2], 100 + k) for k in range(40)]
    out.append(_case("waves-min-and-mid-shape", mixed, kernel=4, dec_waves=4, cus=4))
    big = max(stride["min"], stride["m4"])
    for slots in (4, 7, 8, 11, 12):                      # memory short of a slot per wave: three, two, one wave on four workgroups
        out.append(_case(f"waves-mem{slots}", mixed, kernel=4, dec_waves=4, cus=4, budget=slots * big))
    out.append(_case("waves-mem3", mixed, kernel=4, dec_waves=4, cus=4, budget=3 * big))   # ... and fewer slots than units
    out.append(_case("waves-mc5", _weights("min", 17), kernel=4, dec_waves=4, cus=4, max_concurrent=5))
    out.append(_case("waves-prof", _weights("min", 17), kernel=4, dec_waves=4, cus=4, prof=1))
    out.append(_case("waves-l1-k3", _weights("l1", 17), kernel=3, dec_waves=4, cus=4))      # single CM on zh_chain: no plan, no waves
    out.append(_case("waves-min-k5", _weights("min", 17), kernel=5, dec_waves=4, cus=4))    # the built-in form: no waves
    out.append(_case("waves-min-and-stored", [(("min", "stored")[k % 2], k) for k in range(17)], kernel=4, dec_waves=4, cus=4))
    out.append(_case("waves-level5", _weights("level5", 17), dec_waves=4, cus=4))            # 27 units: one wave fits
    # arena: three families at once
    three = [(("l1", "mid", "stored")[k % 3], 50 + k % 4) for k in range(10)]
    total = sum(_up256(len([b for b in three if b[0] == n]) * stride[n]) for n in ("l1", "mid", "stored"))
    for name, kw in (("fits", dict(budget=total)), ("short", dict(budget=total - 1)), ("serial", dict(budget=total, serial=1)),
                     ("none", dict(budget=stride["mid"] - 1))):
        out.append(_case("arena-" + name, three, **kw))
    # LPT order: equal weights keep input order, otherwise descending
    out.append(_case("lpt-equal", [("mid", 9)] * 6))
    out.append(_case("lpt-mixed", [("mid", w) for w in (3, 9, 3, 1, 9, 0, 7)] + [("l1", w) for w in (2, 2, 8)]))
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dec_plan")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the stand-alone check of the launch plan"
    exe = str(tmp / "dec_plan")
    about = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = "-static-libsan" if "clang" in about else "-static-libasan"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           static, "-I", CSRC, os.path.join(ROOT, "tests", "native", "dec_plan_main.cpp"),
                           os.path.join(CSRC, "zh_framing.cpp"), "-o", exe])
    cases = _cases()
    lines = []
    for c in cases:
        used = sorted({n for n, _ in c["blocks"]}, key=NAMES.index)
        lines.append("case %s has %d %d models %d %s" % (c["name"], NIBBLE_HAS, CHAIN2_HAS, len(used),
                                                         " ".join(MODELS[n][0].header.hex() for n in used)))
        lines.append("opts %d %d %d %d %d %d %d %d" % (c["kernel"], c["max_concurrent"], c["dec_waves"], c["pp_only"], c["prof"],
                                                       c["serial"], c["cus"], c["budget"]))
        lines.append("blocks %d %s" % (len(c["blocks"]), " ".join("%d %d" % (used.index(n), w) for n, w in c["blocks"])))
    path = tmp / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = {}
    for line in r.stdout.split("\n")[:-1]:
        if line.startswith("case "):
            cur = got.setdefault(line[5:], [line])
        else:
            cur.append(line)
    assert list(got) == [c["name"] for c in cases]
    return got, {c["name"]: plan(c) for c in cases}


def _field(line, key):
    return line.split(" " + key + "=")[1].split(" ")[0]


def test_every_case_is_planned_as_the_rules_say(printed):
    got, want = printed
    for name in want:
        assert got[name] == want[name], name


def test_the_routing_table(printed):
    """What the rules above have to give to be include/zpaqhip.h's table, model by model."""
    got, _ = printed
    def r(n, K, pp=0):
        g = got[f"route-{n}-k{K}-pp{pp}"][2]
        return _field(g, "kernel"), int(_field(g, "spec")), int(_field(g, "flags"))
    assert [r(n, 0) for n in NAMES] == [("cm", 0, 0), ("nibble", 1, 0), ("nibble", 2, 0), ("chain2", 3, 0), ("nibble", 2, 0),
                                        ("nibble", 6, 0), ("chain", 0, 0), ("store", 0, 0), ("generic", 0, 0)]
    assert {r(n, 1) for n in NAMES} == {("generic", 0, 0)}
    assert r("l1", 3) == ("chain", 0, 0) and r("min", 3) == ("nibble", 1, 0)
    assert {r(n, 4) for n in NAMES[1:8]} == {("chain", 0, 0)} and r("l1", 4) == ("cm", 0, 0)
    assert [r(n, 5) for n in ("min", "mid", "max", "m4", "lz4")] == [("chain", 1, 0), ("chain", 2, 0), ("chain", 3, 0), ("chain", 0, 0), ("chain", 0, 0)]
    assert [r(n, 9) for n in ("min", "mid", "max", "m4", "lz4")] == [("chain2", 1, 0), ("chain2", 2, 0), ("chain2", 3, 0), ("chain", 0, 0), ("chain", 0, 0)]
    assert r("stored", 10) == ("store", 0, STORE_E8) and r("mid", 10) == ("nibble", 2, 0)
    assert r("stored", 11) == ("store", 0, STORE_E8) and r("mid", 11) == ("nibble", 2, MODEL_E8) and r("lz4", 11) == ("nibble", 6, MODEL_E8)
    assert r("stored", 0, pp=1) == ("generic", 0, 0) and r("mid", 0, pp=1) == ("nibble", 2, 0)
    assert [got[f"route-{n}-k0-pp0"][-1].split("kind=")[1] for n in NAMES] == ["2", "3", "3", "3", "3", "3", "3", "1", "1"]


def test_single_cm_slots(printed):
    got, _ = printed
    def g(name):
        line = got["slots-" + name][2]
        return int(_field(line, "x2")), int(_field(line, "grid")), int(_field(line, "slots"))
    assert g("256-k0-mc0") == (0, 256, 256) and g("257-k0-mc0") == (1, 129, 258) and g("600-k0-mc0") == (1, 256, 512)
    assert g("600-k2-mc0") == (0, 256, 256) and g("1-k6-mc0") == (1, 1, 2) and g("600-k6-mc7") == (1, 4, 8)
    assert g("600-k0-mc7") == (0, 7, 7) and g("600-k6-mc1") == (1, 1, 2)
    assert g("600-k6-mem1") == (0, 1, 1) and g("600-k6-mem2") == (1, 1, 2) and g("600-k6-mem3") == (1, 1, 2)
    assert g("600-k0-prof") == (0, 256, 256) and g("600-k6-prof") == (0, 256, 256)


def test_dec_waves(printed):
    got, _ = printed
    def g(name):
        line = got["waves-" + name][2]
        return int(_field(line, "grid")), int(_field(line, "slots")), int(_field(line, "waves")), int(_field(line, "pool"))
    def concurrent(name):
        return int(got["waves-" + name][-1].split("concurrent=")[1].split(" ")[0])
    assert g("min-4-dw4") == (4, 4, 0, 0) and g("min-5-dw4") == (4, 8, 2, 3072) and g("min-17-dw4") == (4, 16, 4, 3072)
    assert g("min-16-dw2") == (4, 8, 2, 3072) and g("min-17-dw1") == (17, 17, 0, 0) and g("min-3-dw4") == (3, 3, 0, 0)
    assert concurrent("min-5-dw4") == 5 and concurrent("min-17-dw4") == 16
    assert g("min-and-mid-shape") == (4, 12, 3, 11264)   # mid's shape: 11 units, three waves
    assert [g(f"mem{s}")[:3] for s in (12, 11, 8, 7, 4, 3)] == [(4, 12, 3), (4, 8, 2), (4, 8, 2), (7, 7, 0), (4, 4, 0), (3, 3, 0)]
    assert g("mc5") == (5, 5, 0, 0) and g("prof")[2] == 0 and g("l1-k3")[2] == 0 and g("min-k5")[2] == 0
    assert g("min-and-stored")[2] == 0 and g("level5")[2] == 0


def test_the_arena(printed):
    got, _ = printed
    for name, side in (("fits", 1), ("short", 0), ("serial", 0)):
        lines = got["arena-" + name]
        groups = [ln for ln in lines if ln.startswith("group ")]
        assert len(groups) == 3 and lines[-1].startswith("plan side=%d " % side)
        offs = [int(_field(ln, "off")) for ln in groups]
        sizes = [int(_field(ln, "slots")) * int(_field(ln, "stride")) for ln in groups]
        arena = int(_field(lines[-1], "arena"))
        assert all(o % 256 == 0 for o in offs)
        if side:
            assert offs == [0, _up256(sizes[0]), _up256(sizes[0]) + _up256(sizes[1])] and arena == offs[2] + _up256(sizes[2])
        else:
            assert offs == [0, 0, 0] and arena == max(sizes)
    assert got["arena-none"][-1] == "error %d %d" % (E_DEVICE_MEM, E_DEVICE_MEM)


def test_lpt_order(printed):
    got, _ = printed
    assert _field(got["lpt-equal"][2], "order") == "0,1,2,3,4,5"
    assert [_field(ln, "order") for ln in got["lpt-mixed"][2:4]] == ["9,7,8", "1,4,6,0,2,3,5"]
    assert got["lpt-mixed"][4] == "sorted=9,7,8,1,4,6,0,2,3,5"
