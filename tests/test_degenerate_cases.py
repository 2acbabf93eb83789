"""The yardstick of tests/test_gpu_enc_degenerate.py is sound, and its catalogue (tests/degenerate_cases.py) is what it says.

1. On every block of the catalogue the two CPU stream writers (libzpaqgen behind synth.compress_block, and the oracle's
   Compressor mirror) agree byte for byte for min, mid, max and the level 5 recipe, and the oracle's decoder returns the
   plaintext: the bytes the GPU encoders are compared with rest on two independent restatements.
2. Every (method, parse) the GPU tests run end to end inverts on the CPU: the oracle's PCOMP interpreter turns
   tools.methods.preprocess back into the block, and the oracle decodes tools.methods.compress_block to it.
3. Pins that keep the catalogue degenerate: the sizes of the coded sequences, the periods the gap analysis reads off, the
   method strings of level 5.

Pins corrected to what the restatements give (the cases stay):
- the lzpre output of `zeros` is not below 64 bytes: a level 2 match code carries at most m + 63 bytes, so 12288 zeros are
  one literal and 164 three-byte codes, 494 bytes, with the suffix-array parse (560 with the greedy parse, whose matches end
  at m + 63 + 256).  It is the level 1 (lazy2) output that is a handful of bytes: 6.
- tests.test_levels.ref_periods gives no period for `period2`, `period3` and `runs64`: the analysis sets the gaps 1, 2 and
  3 aside and takes periods above 4 only (LibZPAQ.cs:256-281).  `period7` and `period256` have one; so have `two_symbols`
  (two), `long_repeats` (1000) and `e8_runs` (8).  `zeros_then_random` has none."""
import numpy as np
import pytest

import oracle
from tests import degenerate_cases as dc
from tests.chain_cases import LEVEL5
from tests.test_levels import LEVEL5_TAIL, ref_gap_hist, ref_periods
from tools import methods
from zpaqsharp_amd import method, models, synth

NAMES = ["zeros", "ff", "period2", "period3", "period7", "period256", "runs64", "two_symbols", "low_nibbles", "high_nibbles",
         "long_repeats", "e8_runs", "zeros_then_random", "random_then_zeros"]


def test_the_catalogue_is_what_it_says():
    c = dc.cases()
    assert list(c) == NAMES == dc.names() and all(len(v) == dc.N == 12288 for v in c.values())
    assert dc.cases() == c and dc.cases() is not c                    # deterministic, and a copy
    assert c["zeros"] == bytes(dc.N) and c["ff"] == b"\xff" * dc.N and c["period2"] == b"AB" * (dc.N // 2)
    assert c["period3"] == (b"\1\2\3" * dc.N)[:dc.N] and c["period256"] == bytes(range(256)) * (dc.N // 256)
    assert c["period7"] == (c["period7"][:7] * dc.N)[:dc.N] and len(set(c["period7"][:7])) > 1
    r = np.frombuffer(c["runs64"], np.uint8).reshape(-1, 64)
    assert (r == r[:, :1]).all() and len(set(r[:, 0].tolist())) > 100
    assert set(c["two_symbols"]) == {0x10, 0x1f} and set(c["low_nibbles"]) == set(range(16))
    assert set(c["high_nibbles"]) == set(range(0, 256, 16))
    lr = c["long_repeats"]
    assert all(lr[k:k + 700] == lr[:700] for k in range(0, dc.N - 700, 1000)) and lr[700:1000] != lr[1700:2000]
    assert c["e8_runs"] == (b"\xe8" * 7 + b"\0") * (dc.N // 8)
    assert methods.e8e9_forward(c["e8_runs"]) != c["e8_runs"]          # the transform finds candidates
    a, b = c["zeros_then_random"], c["random_then_zeros"]
    assert a[:dc.N // 2] == bytes(dc.N // 2) == b[dc.N // 2:] and a[dc.N // 2:] == b[:dc.N // 2] and len(set(b[:dc.N // 2])) == 256
    bl = dc.blocks()
    assert bl[:14] == list(c.values()) and bl[14:] == [v[:257] for v in c.values()] == dc.short_blocks()
    assert dc.short("period3") == c["period3"][:257]
    t = dc.tiny_blocks(14 * 7)
    assert [len(x) for x in t[:7]] == [0, 1, 2, 63, 64, 65, 300]
    for n in dc.TINY_LENGTHS:                                           # every case at every length
        assert {x for x in t if len(x) == n} == {v[:n] for v in c.values()}, n
    assert dc.tiny_blocks(30) == t[:30]


@pytest.mark.parametrize("name", ["min", "mid", "max", "level5"])
def test_the_cpu_writers_agree_on_the_catalogue(name):
    m = method.model_of(LEVEL5)[0] if name == "level5" else models.get(name)
    assert not m.pcomp
    for i, b in enumerate(dc.blocks()):
        s = synth.compress_block(m, b)
        assert s == oracle.compress_block(m.header, b), (name, i)
        assert oracle.decompress(s, cap=len(b) + 64) == b, (name, i)


@pytest.mark.parametrize("m,parse", dc.METHODS)
def test_every_method_inverts_on_the_cpu(m, parse):
    model, args = method.model_of(m)
    blocks, pre, streams = dc.blocks(), dc.pre_of(m, parse), dc.method_streams(m, parse)
    for i, b in enumerate(blocks):
        if model.pcomp:
            assert oracle.run_pcomp(model.pcomp, pre[i], model.header[4], model.header[5], cap=len(b) + 4096) == b, (m, parse, i)
        else:
            assert pre[i] == b
        assert streams[i] == methods.compress_block(m, b, **dc.parse_kw(parse)), (m, parse, i)
    plain = b"".join(blocks)
    assert oracle.decompress(b"".join(streams), cap=len(plain) + 64) == plain


def _pre(m, parse, name):
    return methods.preprocess(dc.cases()[name], method.parse_args(m)[1], **dc.parse_kw(parse))


def test_the_coded_sequences_are_a_few_codes():
    """(The figures of the module docstring.)"""
    for parse, want in (("", 6), ("ht", 10)):
        assert len(_pre("x0,1,4,0,3,20", parse, "zeros")) == want
    assert len(_pre("x0,1,4,0,7,21,1", "sa", "zeros")) == 6
    assert len(_pre("x0,2,12,0,7,21,1c0,0,511i2", "", "zeros")) == 560
    assert len(_pre("x0,2,12,0,7,21,1c0,0,511i2", "sa", "zeros")) == 494 == 2 + 164 * 3      # one literal, 164 codes of 75
    assert 12288 - 1 == 163 * 75 + 62
    for name in ("ff", "period2", "period3", "period7", "e8_runs"):
        assert len(_pre("x0,1,4,0,3,20", "ht", name)) <= 17, name
        assert len(_pre("x0,2,5,0,3,20c0,0,511", "ht", name)) < 600, name
    for name in ("low_nibbles", "high_nibbles"):                         # nothing to match: literals and their length bytes
        assert len(_pre("x0,2,12,0,7,21,1c0,0,511i2", "sa", name)) == 12288 + 12288 // 64
    # the BWT of a periodic block is a few long runs
    for name, runs in (("zeros", 2), ("period2", 3), ("period3", 4), ("period7", 8), ("period256", 256)):
        a = np.frombuffer(methods.bwt_level3(dc.cases()[name])[:-4], np.uint8)
        assert 1 + int((a[1:] != a[:-1]).sum()) == runs, name


def test_a_whole_block_codes_into_a_few_bytes():
    """Header, framing and SHA-1 included: the coder's own bytes are what is left of these."""
    for name, most in (("min", 100), ("mid", 150), ("max", 280)):
        hdr = len(models.get(name).header)
        for case in ("zeros", "ff", "period2", "period3"):
            s = synth.compress_block(name, dc.cases()[case])
            assert len(s) <= most and len(s) - hdr - 13 - 5 - 21 - 10 < 64, (name, case, len(s))
    half = len(synth.compress_block("mid", dc.cases()["zeros_then_random"]))
    assert dc.N // 2 < half < dc.N // 2 + 300


def test_the_periods_the_analysis_reads_off():
    want = {"zeros": "", "ff": "", "period2": "", "period3": "", "period7": "c0,0,1006,255i1c0,7i1",
            "period256": "c0,0,1255,255i1", "runs64": "", "two_symbols": "c0,0,1004,255i1c0,5i1c0,0,1005,255i1c0,6i1",
            "low_nibbles": "", "high_nibbles": "", "long_repeats": "c0,0,1999,255i1", "e8_runs": "c0,0,1007,255i1c0,8i1",
            "zeros_then_random": "", "random_then_zeros": ""}
    got = {k: ref_periods(len(v), ref_gap_hist(v)) for k, v in dc.cases().items()}
    assert got == want
    h = dc.gap_hists()
    assert h.shape == (28, 4096) and (h[0] == ref_gap_hist(dc.cases()["zeros"])).all() and h[0, 1] == dc.N - 1
    short = {k: ref_periods(257, ref_gap_hist(dc.short(k))) for k in dc.names()}
    assert {k for k, v in short.items() if v} == {"period7", "e8_runs"}
    # level 5 over blocks(): six method strings in one call, the plain one among them
    strings = dc.level_methods("5")
    assert len(set(strings)) == 6 and LEVEL5 in strings and LEVEL5.endswith(LEVEL5_TAIL)
    assert all(s.startswith("x0,0w1i1c256ci1,1,1,1,1,1,2a") and s.endswith(LEVEL5_TAIL) for s in strings)
    assert len(set(dc.level_methods("5,128,1"))) == 6
    # ... and four in each of the two parts the GPU tests call a level 5 with; the parts are all of blocks()
    assert sorted(dc.LEVEL5_PARTS["a"] + dc.LEVEL5_PARTS["b"]) == list(range(28))
    for lv in ("5", "5,128,1"):
        for ids in dc.LEVEL5_PARTS.values():
            assert len({dc.level_methods(lv)[i] for i in ids}) == 4
    for lv in "1234":
        assert len(set(dc.level_methods(lv))) == 1
