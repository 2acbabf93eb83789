"""tools.methods.lz77_ht, the port of LZBuffer's hash-table match search (LZBuffer.cs:285-327, :349-368), which the GPU route
(zh_pre_lzht.hip, tests/test_gpu_lzht.py) is held to: the C++ twin in libzpaqgen, which keeps the reference's table, a
Python version that keeps it too, the cases of tests/lzht_cases.py really occurring, the reference's text, the refusals,
the bound, and the oracle's decoder on every stream of the catalogue."""
import os
import re

import numpy as np
import pytest

import oracle
from tests import lzht_cases as cases
from tests.conftest import REFERENCE
from tools import methods
from zpaqsharp_amd import method, synth

ALL = cases.METHODS + (cases.M_MARGINAL1, cases.M_MARGINAL2)


def _e8(args, b):
    return methods.e8e9_forward(b) if 4 <= args[1] <= 7 else b


@pytest.mark.parametrize("m", ALL)
def test_the_cpp_twin_and_the_table_agree_on_the_catalogue(m):
    args = method.parse_args(m)[1]
    for i, (b, w) in enumerate(zip(cases.blocks_for(m), cases.want(m))):
        assert synth.preprocess(args, _e8(args, b), ht=True) == w, (m, i)
        if len(b) <= 20000:
            assert methods.lz77_ht(_e8(args, b), args, table=True) == w, (m, i)
        assert len(w) <= method.pre_bound(args, len(b)), (m, i)


def test_the_cpp_twin_and_the_table_agree_on_the_knobs():
    d = cases.text()
    for m in cases.knob_methods():
        args = method.parse_args(m)[1]
        for b in (d, d[:3000]):
            assert synth.preprocess(args, b, ht=True) == methods.preprocess(b, args, ht=True) == methods.lz77_ht(b, args, table=True), m


def test_random_blocks_over_few_symbols():
    # small tables and long runs: the break at 128 bytes, and filters that depend on the blen of the moment
    rng = np.random.default_rng(5)
    for _ in range(300):
        d = bytes(rng.integers(0, int(rng.integers(2, 5)), int(rng.integers(0, 2049)), dtype=np.uint8))
        lv = int(rng.integers(1, 3))
        h = int(rng.choice([1, 4, 8]))
        args = [0, lv, int(rng.integers(4, 7)) if lv == 1 else int(rng.integers(2, 6)), 0, int(rng.integers(0, min(h, 3) + 1)), h, 0, 0, 0]
        a = methods.lz77_ht(d, args)
        assert a == synth.preprocess(args, d, ht=True) == methods.lz77_ht(d, args, table=True), (args, d)


def test_the_cases_occur():
    a = method.parse_args("x0,2,12,0,3,20")[1]
    parse = list(methods.lz77_ht_parse(cases.lzsa_cases.offsets(12), a))
    assert ("match", 12, 65535) in parse and ("match", 13, 65536) in parse and ("match", 13, 65537) in parse
    assert ("match", 12, 65536) not in parse and ("match", 12, 65537) not in parse      # one byte more from 2^16 on
    for m, f in ((cases.M_MARGINAL2, cases.marginal2), (cases.M_MARGINAL1, cases.marginal1)):
        d, _, _, offs = f()
        args = method.parse_args(m)[1]
        parse = list(methods.lz77_ht_parse(d, args))
        assert ("match", args[2], offs[0]) in parse and ("match", args[2], offs[1]) not in parse, m
    a = method.parse_args(cases.M_INVISIBLE)[1]
    assert ("match", 8, 8) not in list(methods.lz77_ht_parse(cases.invisible(0), a))
    assert ("match", 8, 8) in list(methods.lz77_ht_parse(cases.invisible(1), a))
    # maxMatch cuts at 49 152; level 2 with minMatch 65 searches nothing
    # (h1 of the first minMatch positions holds fewer terms than any later one: the run is found from position 6 on)
    assert list(methods.lz77_ht_parse(bytes(70000), method.parse_args(cases.L1)[1])) == [("lit", 0, 6), ("match", 49152, 1), ("match", 70000 - 49158, 7)]
    assert list(methods.lz77_ht_parse(bytes(5000), method.parse_args("x0,2,65,0,3,20")[1])) == [("lit", 0, 4096), ("lit", 4096, 5000)]
    r = cases._rnd(5000, 3)
    assert list(methods.lz77_ht_parse(r + r[:100], method.parse_args(cases.L1)[1]))[:3] == [("lit", 0, 4096), ("lit", 4096, 5005), ("match", 95, 5000)]


def test_shift1_divides_as_c_does():
    assert methods.ht_shift1([0, 2, 4, 0, 0, 0, 0, 0, 0]) == 1
    assert methods.ht_shift1([0, 1, 5, 0, 3, 20, 0, 0, 0]) == 4 and methods.ht_shift1([0, 2, 12, 0, 2, 8, 0, 0, 0]) == 1
    d = cases.text(500)
    for m in ("x0,2,4,0,0,0", "x0,1,4,0,0,0"):
        args = method.parse_args(m)[1]
        assert methods.lz77_ht(d, args) == synth.preprocess(args, d, ht=True) == methods.lz77_ht(d, args, table=True)


@pytest.mark.reference
def test_the_port_follows_the_reference_text():
    with open(os.path.join(REFERENCE, "LZBuffer.cs"), encoding="utf-8", errors="replace") as f:
        src = re.sub(r"\s+", "", f.read())
    for piece in ("1234547", "123456791u", ">>19", "-2*(lit>0)-11", "if(blen>=128)break", "i+minMatchBoth<n",
                  "MAX(minMatch,minMatch2+lookahead)+4", "unsignedih=((i*1234547)>>19)&bucket;",
                  "constunsignedp=(i<<checkbits)|(in[i+3]&mask);", "ht[h1^ih]=p;",
                  "h1=(((h1*5)<<shift1)+(in[i+minMatch]+1)*123456791u)&(htsize-1);", "unsignedp=ht[h1^k];",
                  "if(p&&i+3<n&&(p&mask)==(in[i+3]&mask))", "if(p<i&&i+blen<=n&&in[p+blen-1]==in[i+blen-1])",
                  "for(l=0;i+l<n&&l<maxMatch&&in[p+l]==in[i+l];++l);", "intscore=l*8-lg(i-p)-2*(lit>0)-11;",
                  "if(score>bscore)blen=l,bp=p,blit=0,bscore=score;", "elseif(level==1||minMatch<=64)",
                  "shift1(minMatch>0?(args[5]-1)/minMatch+1:1)", "checkbits(args[5]-args[0]<21?12-args[0]:17+args[0])"):
        assert piece in src, piece


def test_the_refusals():
    ok = [0, 1, 4, 0, 3, 20, 0, 0, 0]
    method.check_blocks(ok, [1 << 20], ht=True)
    method.check_blocks([0, 2, 65, 0, 3, 20, 0, 0, 0], [100], ht=True)       # level 2 above 64: no search, all literals
    method.check_blocks([5, 1, 4, 0, 3, 25, 0, 0, 0], [1 << 24], ht=True)
    bad = ([0, 1, 4, 1, 3, 20, 0, 0, 0], [0, 1, 4, 0, 3, 20, 1, 0, 0], [0, 1, 3, 0, 3, 20, 0, 0, 0], [0, 2, 1, 0, 3, 20, 0, 0, 0],
           [0, 2, 256, 0, 3, 20, 0, 0, 0], [12, 1, 4, 0, 3, 20, 0, 0, 0], [0, 1, 4, 0, 4, 3, 0, 0, 0],
           [0, 1, 4, 0, method.HT_MAX_BUCKET_BITS + 1, 20, 0, 0, 0], [11, 1, 4, 0, 3, 31, 0, 0, 0])
    for a in bad:
        with pytest.raises(ValueError):
            method.check_blocks(a, [10], ht=True)
    with pytest.raises(ValueError):
        method.check_blocks([5, 1, 4, 0, 3, 25, 0, 0, 0], [(1 << 24) + 1], ht=True)
    method.check_blocks([5, 1, 4, 0, 3, 25, 0, 0, 0], [(1 << 24) + 1])
    with pytest.raises(ValueError):
        method.check_blocks([0, 2, 65, 0, 3, 20, 0, 0, 0], [100])              # without the keyword: as before
    for a in bad[:2]:                                                          # the port and the twin refuse too
        with pytest.raises(ValueError):
            methods.preprocess(b"abcdabcdabcd", a, ht=True)
        with pytest.raises(ValueError):
            synth.preprocess(a, b"abcdabcdabcd", ht=True)
    assert method.uses_ht(ok) and not method.uses_ht([0, 1, 4, 0, 7, 21, 1, 0, 0]) and not method.uses_ht([0, 3, 0, 0, 0, 0, 0, 0, 0])
    assert method.HT_MAX_BUCKET_BITS >= 6


@pytest.mark.parametrize("m", ALL)
def test_the_oracle_decodes_every_catalogue_stream(m):
    for i, b in enumerate(cases.blocks_for(m)):
        s = methods.compress_block(m, b, ht=True, pre=cases.want(m)[i])
        assert oracle.decompress(s, cap=len(b) + 64) == b, (m, i)
    b = cases.text(3000)
    assert oracle.decompress(methods.compress_block("x0,1,4,0,3,20ci1", b, ht=True), cap=4096) == b


def test_without_the_keyword_nothing_changes():
    d = cases.text()
    for m in cases.METHODS:
        args = method.parse_args(m)[1]
        e = _e8(args, d)
        assert methods.preprocess(d, args) == methods.preprocess(d, args, sa=True) == (methods.lz77_level1(e, args) if args[1] & 3 == 1 else methods.lz77_level2(e, args))
        assert methods.compress_block(m, d) == methods.compress_block(m, d, ht=False) != methods.compress_block(m, d, ht=True)
    for m in ("x0,1,4,0,7,21,1", "x0,3", "x0,4", "x0,0"):                      # the keyword touches no other method
        args = method.parse_args(m)[1]
        assert methods.preprocess(d, args, ht=True) == methods.preprocess(d, args)
    m = "x0,1,4,0,7,21,1"
    assert methods.compress_block(m, d, sa=True, ht=True) == methods.compress_block(m, d, sa=True)


def test_stream_generator_takes_the_keyword():
    m = cases.L1
    model, args = method.model_of(m)
    s, off = synth.method_stream(model, args, "T", 2, 5000, ht=True)
    blocks = [synth.plain("T", i, 5000).tobytes() for i in range(2)]
    assert s.tobytes() == b"".join(methods.compress_block(m, b, ht=True) for b in blocks)
    assert synth.method_stream(model, args, "T", 2, 5000)[0].tobytes() != s.tobytes()
