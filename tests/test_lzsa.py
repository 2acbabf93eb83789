"""tools.methods.lz77_sa, the literal port of LZBuffer's suffix-array match search (LZBuffer.cs:246-283, :329-383), which the
GPU route (zh_pre_lzsa.hip, tests/test_gpu_lzsa.py) is held to: codes worked by hand, the reference's text, the closed
window rule against the reference's windowed inverse array, the C++ twin in libzpaqgen, and the oracle's decoder on every
stream of the catalogue (tests/lzsa_cases.py)."""
import os
import re

import pytest

import oracle
from tests import lzsa_cases as cases
from tests.conftest import REFERENCE
from tools import methods
from zpaqsharp_amd import method, synth

A2 = [0, 2, 4, 0, 3, 21, 1, 0, 0]                  # level 2, minMatch 4, 7 neighbours a side, look-ahead 1
A1 = [0, 1, 4, 0, 3, 21, 1, 0, 0]


def _bits(fields):
    """LSB-first packing of (value, width) fields, zero-padded to a byte: LZBuffer.putb / flush."""
    acc = n = 0
    for v, w in fields:
        acc |= (v & ((1 << w) - 1)) << n
        n += w
    return acc.to_bytes((n + 7) // 8, "little")


def test_a_plain_repeat_by_hand():
    # i = 4: the only earlier suffix next to "abcd" is position 0, l = 4, score = 32 - lg(4) - 11 = 18 > 0: match 4 at offset 4
    d = b"abcdabcd"
    assert list(methods.lz77_sa_parse(d, A2)) == [("lit", 0, 4), ("match", 4, 4)]
    assert methods.lz77_sa(d, A2) == b"\x03abcd" + bytes([64 + 0, 0, 3])
    # level 1: 00, n = 4 as 1,0 1,0 0, the bytes; mm,mmm of lo = lg(4) - 1 = 2 -> 01, 010; length 4: 0, ll = 00; q = 4 in 2 bits
    lit = [(0, 2), (1, 1), (0, 1), (1, 1), (0, 1), (0, 1)] + [(c, 8) for c in b"abcd"]
    assert methods.lz77_sa(d, A1) == _bits(lit + [(1, 2), (2, 3), (0, 1), (0, 2), (4, 2)])


def test_nothing_to_match_by_hand():
    assert methods.lz77_sa(b"", A2) == b"" == methods.lz77_sa(b"", A1)
    assert methods.lz77_sa(b"abc", A2) == b"\x02abc"
    assert methods.lz77_sa(b"aaaa", A2) == b"\x03aaaa"               # l = 3 at i = 1: below minMatch
    # "aaaaa": at i = 1 the neighbour is position 0 with l = 4, score 32 - 1 - 11: a match of 4 at offset 1
    assert methods.lz77_sa(b"aaaaa", A2) == b"\x00a" + bytes([64, 0, 0])


def test_look_ahead_wins_after_literals_by_hand():
    # i = 21 (lit > 0): h = 0 finds "Xabc" at 0, score 32 - lg(21) - 11 = 16; h = 1 finds "abcdefghijkl" at 7 behind a 'Y', so
    # l = 13, l1 = 1, score (96 - lg(15) - 11) * 5 / 8 = 50: 'X' joins the literals, 12 bytes are copied from offset 15
    d = b"Xabc__Yabcdefghijkl--Xabcdefghijkl"
    assert list(methods.lz77_sa_parse(d, A2)) == [("lit", 0, 22), ("match", 12, 15)]
    assert methods.lz77_sa(d, A2) == bytes([21]) + d[:22] + bytes([64 + 8, 0, 14])
    # without look-ahead the 4 bytes at h = 0 are taken
    assert list(methods.lz77_sa_parse(d, A2[:6] + [0, 0, 0]))[:2] == [("lit", 0, 21), ("match", 4, 21)]


def test_look_ahead_wins_right_after_a_match_by_hand():
    # i = 19 copies "__Yab" (5 bytes, offset 15), so i = 24 is reached with lit == 0: h = 0 scores 32 - lg(24) - 11 = 16, h = 1
    # (96 - lg(18) - 4 - 11) * 5 / 8 = 47 with the 4 that a literal run started for the match costs
    d = b"Xabc__Yabcdefghijkl__YabXabcdefghijkl"
    assert list(methods.lz77_sa_parse(d, A2)) == [("lit", 0, 19), ("match", 5, 15), ("lit", 24, 25), ("match", 12, 18)]
    assert methods.lz77_sa(d, A2) == bytes([18]) + d[:19] + bytes([65, 0, 14]) + b"\x00X" + bytes([72, 0, 17])


def test_long_runs_by_hand():
    # one byte value: i = 1 takes maxMatch = 49 152 bytes at offset 1 (the l > 255 stop), then the rest
    d = bytes(70000)
    assert list(methods.lz77_sa_parse(d, A2)) == [("lit", 0, 1), ("match", 49152, 1), ("match", 70000 - 49153, 1)]
    # level 2 splits 49 152 = 722 * 67 + 64 + 714 - ...: every piece has minMatch .. minMatch + 63 bytes
    out = methods.lz77_sa(d, A2)
    assert out[:2] == b"\x00\x00" and len(out) == 2 + 3 * (-(-49152 // 67) + -(-(70000 - 49153) // 67))
    # 5 000 random bytes: a literal run is flushed every maxLiteral = 4 096 bytes
    r = cases._rnd(5000, 3)
    assert list(methods.lz77_sa_parse(r + r[:100], A1)) == [("lit", 0, 4096), ("lit", 4096, 5000), ("match", 100, 5000)]


@pytest.mark.reference
def test_the_port_follows_the_reference_text():
    with open(os.path.join(REFERENCE, "LZBuffer.cs"), encoding="utf-8", errors="replace") as f:
        src = re.sub(r"\s+", "", f.read())
    for piece in ("enum{BUFSIZE=1<<14};", "maxMatch(BUFSIZE*3)", "maxLiteral(BUFSIZE/4)", "bucket((1<<args[4])-1)", "lookahead(args[6])",
                  "checkbits(args[5]-args[0]<21?12-args[0]:17+args[0])", "if(args[5]-args[0]>=21||level==3)",
                  "unsignedblen=minMatch-1;", "if(sa[q]!=h+i)continue;", "if(q+j*k<n&&(p=sa[q+j*k]-h)<i)",
                  "for(l=h;i+l<n&&l<maxMatch&&in[p+l]==in[i+l];++l);", "for(l1=h;l1>0&&in[p+l1-1]==in[i+l1-1];--l1);",
                  "intscore=int(l-l1)*8-lg(i-p)-4*(lit==0&&l1>0)-11;", "for(unsigneda=0;a<h;++a)score=score*5/8;",
                  "if(score>bscore)blen=l,bp=p,blit=l1,bscore=score;", "if(l<blen||l<minMatch||l>255)break;",
                  "if(bscore<=0||blen<minMatch)break;",
                  "if(off>0&&bscore>0&&blen-blit>=minMatch+(level==2)*((off>=(1<<16))+(off>=(1<<24))))",
                  "if(isa)i+=blen;", "if(lit>=maxLiteral)write_literal(i,lit);"):
        assert piece in src, piece
    assert methods.MAX_MATCH == 3 << 14 and methods.MAX_LITERAL == (1 << 14) // 4


def test_the_window_rule_equals_the_windowed_inverse_array():
    d = cases.window()
    for m in (cases.L1, cases.L2, "x0,2,4,0,3,21,3"):
        args = method.parse_args(m)[1]
        assert methods.lz77_sa(d, args) == methods.lz77_sa(d, args, windowed=True), m
    # look-ahead is dropped at the last position of the first window and nowhere else (tests/lzsa_cases.window)
    args = method.parse_args("x0,2,4,0,3,21,3")[1]
    parse = list(methods.lz77_sa_parse(d, args))
    assert ("match", 12, 120001 - 119101) in parse and ("match", 4, 120000 - 119000) not in parse
    assert ("match", 4, 131071 - 130000) in parse and ("match", 12, 131072 - 130101) not in parse
    for b in (cases.phrases(), cases.text(3000), bytes(5000), b"ab" * 700):
        assert methods.lz77_sa(b, args) == methods.lz77_sa(b, args, windowed=True)


@pytest.mark.parametrize("m", cases.METHODS)
def test_the_cpp_twin_agrees_on_the_catalogue(m):
    args = method.parse_args(m)[1]
    for i, (b, w) in enumerate(zip(cases.blocks_for(m), cases.want(m))):
        d = methods.e8e9_forward(b) if 4 <= args[1] <= 7 else b
        assert synth.preprocess(args, d, sa=True) == w, (m, i)


def test_the_cpp_twin_agrees_on_the_knobs():
    d = cases.text()
    for m in cases.knob_methods():
        args = method.parse_args(m)[1]
        assert synth.preprocess(args, d, sa=True) == methods.preprocess(d, args, sa=True), m


@pytest.mark.parametrize("m", cases.METHODS)
def test_the_oracle_decodes_every_catalogue_stream(m):
    for i, b in enumerate(cases.blocks_for(m)):
        s = methods.compress_block(m, b, sa=True, pre=cases.want(m)[i])
        assert oracle.decompress(s, cap=len(b) + 64) == b, (m, i)


def test_without_the_keyword_nothing_changes():
    d = cases.text()
    for m in cases.METHODS:
        args = method.parse_args(m)[1]
        e = methods.e8e9_forward(d) if 4 <= args[1] <= 7 else d
        assert methods.preprocess(d, args) == (methods.lz77_level1(e, args) if args[1] & 3 == 1 else methods.lz77_level2(e, args))
        assert methods.compress_block(m, d) == methods.compress_block(m, d, sa=False) != methods.compress_block(m, d, sa=True)
    for m in ("x0,1,4,0,3,20", "x0,3", "x0,4", "x0,2,12,0,7,20,1"):                  # the keyword touches no other method
        args = method.parse_args(m)[1]
        assert methods.preprocess(d, args, sa=True) == methods.preprocess(d, args)


def test_stream_generator_takes_the_keyword():
    m = cases.L1
    model, args = method.model_of(m)
    s, off = synth.method_stream(model, args, "T", 2, 5000, sa=True)
    blocks = [synth.plain("T", i, 5000).tobytes() for i in range(2)]
    assert s.tobytes() == b"".join(methods.compress_block(m, b, sa=True) for b in blocks)
    assert synth.method_stream(model, args, "T", 2, 5000)[0].tobytes() != s.tobytes()


def test_check_blocks_and_bound():
    args = method.parse_args(cases.L2)[1]
    method.check_blocks(args, [1 << 20], sa=True)
    a = method.parse_args("x5,2,12,0,7,26,1")[1]
    method.check_blocks(a, [1 << 25])
    with pytest.raises(ValueError):
        method.check_blocks(a, [(1 << 24) + 1], sa=True)              # offsets of 2^24 and more are not written
    with pytest.raises(ValueError):
        method.check_blocks(method.parse_args("x0,1,3,0,3,21")[1], [10], sa=True)
    for m in cases.METHODS:
        for b, w in zip(cases.blocks_for(m), cases.want(m)):
            assert len(w) <= method.pre_bound(method.parse_args(m)[1], len(b))
