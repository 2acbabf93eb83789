"""The yardstick of tests/test_gpu_enc_chains.py is sound: on every model of tests/chain_cases.py the two CPU stream writers
(libzpaqgen and the oracle's Compressor mirror) agree byte for byte, and the oracle's decoder returns the plaintext."""
import pytest

import oracle
from tests import chain_cases as cc
from zpaqsharp_amd import synth, zpaql


def _agree(cfg, blocks):
    m = zpaql.assemble(cfg)
    out = []
    for b in blocks:
        s = synth.compress_block(m, b)
        assert s == oracle.compress_block(m.header, b), cfg
        assert oracle.decompress(s, cap=len(b) + 64) == b, cfg
        out.append(s)
    return out


@pytest.mark.parametrize("group", range(cc.GROUPS))
def test_the_cpu_writers_agree_on_the_random_chains(group):
    for cfg in cc.random_group(group, cc.seed()):
        _agree(cfg, cc.random_blocks())


@pytest.mark.parametrize("name", list(cc.DIRECTED))
def test_the_cpu_writers_agree_on_the_directed_chains(name):
    case = cc.DIRECTED[name]
    coded = _agree(case.cfg, cc.blocks_of(case))
    if case.expands:                               # really past the encoders' automatic slot, n + n / 8 + 4096 of the coded n
        n = len(case.blocks[0]) + 1
        assert len(coded[0]) > n + n // 8 + 4096 + 100


def test_the_random_chains_are_inside_the_family_and_varied():
    """What build_model asks of ZH_FAM_CHAIN, on the text (the GPU tests assert the route itself), and that the draws reach
    what they are for: both placements of H and M, H smaller than n, every component type, a fifth mixer."""
    seen, fifth = set(), 0
    for g in range(cc.GROUPS):
        for cfg in cc.random_group(g, 12345):
            hh, hm, _, _, comps, _ = zpaql.parse_header(zpaql.assemble(cfg).header)
            names = [zpaql.COMP_NAMES[c[0]] for c in comps]
            assert 1 <= len(comps) <= 24 and names.count("mix") <= 4
            assert names.count("icm") + 2 * names.count("isse") <= 64
            assert all(c[1] >= 4 for c in comps if zpaql.COMP_NAMES[c[0]] == "cm")
            seen |= set(names) | {("hh", hh), ("hm", hm)} | ({"h-wraps"} if (1 << hh) < len(comps) else set())
            fifth += names.count("mix") == 4 and "mix2" in names
    assert seen >= set(zpaql.COMP_NAMES[1:]) | {("hh", h) for h in (0, 2, 3, 9, 10)} | {("hm", m) for m in (0, 3, 12, 13)} | {"h-wraps"}
    assert fifth


def _shape(cfg):
    comps = zpaql.parse_header(zpaql.assemble(cfg).header)[4]
    names = [zpaql.COMP_NAMES[c[0]] for c in comps]
    cm = min([c[1] for c in comps if zpaql.COMP_NAMES[c[0]] == "cm"], default=32)
    return len(comps), names.count("icm") + 2 * names.count("isse"), names.count("mix"), cm


def test_the_directed_limits_are_what_they_say():
    """(components, LDS units, mixers, smallest CM) of the models at the family's limits and of each one just past them: one
    limit exceeded, the others kept; and every case's expected route is the family rule's."""
    d = cc.DIRECTED
    assert _shape(d["n64-h0"].cfg) == _shape(d["n64-h10"].cfg) == (64, 63, 4, 32)
    assert _shape(d["units64"].cfg)[:3] == (38, 64, 1)
    assert _shape(d["outside-5mix"].cfg) == (64, 63, 5, 32)
    assert _shape(d["outside-65units"].cfg)[:3] == (39, 65, 1)
    assert _shape(d["outside-n65"].cfg) == (65, 63, 4, 32)
    assert _shape(d["outside-cm3"].cfg) == (4, 3, 1, 3)
    for name, case in d.items():
        n, units, nmix, cm = _shape(case.cfg)
        assert (case.kind == 3) == (n <= 64 and units <= 64 and nmix <= 4 and cm >= 4), name


def test_the_long_programs_sit_on_the_window_limit():
    assert cc.hcomp_len(cc.DIRECTED["long-hcomp-2048"].cfg) + 2 * 160 == 2048
    assert cc.hcomp_len(cc.DIRECTED["long-hcomp-2049"].cfg) + 2 * 160 == 2049


REUSED = ["tiny-tables", "match-wrap-2", "n64-h10", "units64", "sse-mix2-extremes", "placement-9-12", "placement-10-13",
          "placement-native-mid-10-13"]


@pytest.mark.parametrize("name", REUSED + [f"random-{g}" for g in range(cc.GROUPS)])
def test_the_many_block_writer_is_the_one_block_writer(name):
    """synth.compress_blocks keeps a writer's memory from block to block and initialises it again for each (the one-block
    writer starts from fresh zero pages): on one thread, so that every block but the first finds what the last one left."""
    cfgs = [cc.DIRECTED[name].cfg] if name in cc.DIRECTED else cc.random_group(int(name[7:]), 12345)[:4]
    pool = cc.mixed()
    blocks = [pool[97 * i:97 * i + n] for i, n in enumerate((700, 0, 1, 2, 63, 64, 65, 300, 0, 17, 1000))]
    for cfg in cfgs:
        m = zpaql.assemble(cfg)
        want = [synth.compress_block(m, b) for b in blocks]
        assert synth.compress_blocks(m, blocks, 1) == want, cfg
        assert synth.compress_blocks(m, blocks, 3) == want, cfg
    assert synth.compress_blocks(zpaql.assemble(cfgs[0]), []) == []
