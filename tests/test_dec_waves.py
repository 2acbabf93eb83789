"""The host side of the lane-per-component decoder's waves per compute unit (zh_chain.hip's zh_decode_chain_mw, decode
opts.dec_waves): the options field, and zpaqhip_dec_chain_plan, the LDS plan of a model: one copy of the tables for the
workgroup and, per wave, the model's ICM / ISSE pool (1 KiB per unit: ICM 1, ISSE 2) and a fixed part of 16 320 bytes (the
nibble cache, H, M, R and the program window of HCOMP and PCOMP, both machines, the sink), in 163 840 bytes.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import chain_cases as cc
from zpaqsharp_amd import _lib, api, method, models, zpaql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 163840
TABLES = 79872                                     # sizeof(ZhTables): squash, stretch, dt, dt2k, ns
FIXED = 16320                                      # what a decoder wave keeps next to its pool
LEVEL5 = method.expand_level("5", 65536, np.zeros(4096, np.uint32))


def _units(model) -> int:
    """ICM + 2 ISSE of a model: its LDS pool in KiB."""
    comps = zpaql.parse_header(model.header)[4]
    return sum(1 if c[0] == 3 else 2 if c[0] == 8 else 0 for c in comps)


def _stride(units: int) -> int:
    return (units * 1024 + FIXED + 15) & ~15


def _model(name):
    return models.get(name) if name in ("min", "mid", "max") else method.model_of(name)[0]


def test_opts_carry_dec_waves_where_reserved0_was(tmp_path):
    assert _lib.Opts.dec_waves.offset == 40 and _lib.Opts.dec_waves.size == 8
    assert _lib.Opts.reserved.offset == 48 and C.sizeof(_lib.Opts) == 56
    o = api.make_opts(dec_waves=3, kernel=4)
    assert (o.struct_size, o.dec_waves, o.kernel, o.reserved[0]) == (56, 3, 4, 0)
    # the header's struct, as a C compiler lays it out
    src = tmp_path / "o.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zpaqhip.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   "sizeof(zpaqhip_opts),offsetof(zpaqhip_opts,queue_blocks),offsetof(zpaqhip_opts,dec_waves),"
                   "offsetof(zpaqhip_opts,reserved));return 0;}\n")
    exe = tmp_path / "o"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [56, 32, 40, 48]


def test_the_plan_is_exported_and_declared():
    assert "zpaqhip_dec_chain_plan" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "zpaqhip_dec_chain_plan")


@pytest.mark.parametrize("name", ["min", "mid", "max", "x0,3ci1", cc.M4, LEVEL5])
def test_built_in_and_method_models_get_their_waves(name):
    assert LEVEL5 == cc.LEVEL5                     # (the recipe compressBlock writes is the catalogue's)
    m = _model(name)
    waves, lds = api.dec_chain_plan(m)
    stride = _stride(_units(m))
    assert 1 <= waves <= 4
    assert lds <= LDS
    assert lds == TABLES + waves * stride
    assert waves == 4 or lds + stride > LDS


def test_the_waves_by_unit_count():
    """4 waves up to 4 units, 3 up to 11, 2 up to 25, then 1: min 3 units, mid 11, max 20; the level 5 recipe has 27 (two
    regions of 43 968 bytes are 3 968 bytes more than the tables leave) and keeps one wave."""
    for units in range(65):
        want = 4 if units <= 4 else 3 if units <= 11 else 2 if units <= 25 else 1
        assert min(4, (LDS - TABLES) // _stride(units)) == want, units
    got = {n: (_units(_model(n)), api.dec_chain_plan(_model(n))[0]) for n in ("min", "mid", "max", "x0,3ci1", cc.M4, LEVEL5)}
    assert got == {"min": (3, 4), "mid": (11, 3), "max": (20, 2), "x0,3ci1": (3, 4), cc.M4: (11, 3), LEVEL5: (27, 1)}


def test_the_largest_chains_keep_one_wave():
    for name in ("n64-h0", "n64-h10", "units64"):  # 63, 63 and 64 units
        m = zpaql.assemble(cc.DIRECTED[name].cfg)
        assert _units(m) in (63, 64)
        assert api.dec_chain_plan(m) == (1, TABLES + _stride(_units(m))), name
    assert {_units(zpaql.assemble(cc.DIRECTED[n].cfg)) for n in ("n64-h0", "units64")} == {63, 64}


def test_models_outside_the_family_get_none():
    for name in ("outside-5mix", "outside-65units", "outside-n65", "outside-cm3"):
        assert cc.DIRECTED[name].kind == 1
        assert api.dec_chain_plan(zpaql.assemble(cc.DIRECTED[name].cfg)) == (0, 0), name
    assert api.dec_chain_plan("l1") == (0, 0)      # a single CM has its own decoder (kernel=3 sends it to the one-wave form)
    assert api.dec_chain_plan(method.model_of("x0,1,4,0,3,24")[0]) == (0, 0)   # stored blocks: n = 0


def test_every_catalogue_plan_fits_the_lds():
    seen = set()
    for name, case in cc.DIRECTED.items():
        m = zpaql.assemble(case.cfg)
        waves, lds = api.dec_chain_plan(m)
        inside = not name.startswith("outside-")
        assert (waves >= 1) == inside, name
        assert (waves, lds) == ((min(4, (LDS - TABLES) // _stride(_units(m))), TABLES + waves * _stride(_units(m))) if inside else (0, 0)), name
        seen.add(waves)
    for g in range(cc.GROUPS):
        for i, cfg in enumerate(cc.random_group(g, cc.seed())):
            m = zpaql.assemble(cfg)
            waves, lds = api.dec_chain_plan(m)
            assert 1 <= waves <= 4 and lds == TABLES + waves * _stride(_units(m)) <= LDS, (g, i)
            seen.add(waves)
    assert seen == {0, 1, 2, 3, 4}


def test_the_plan_rejects_what_is_no_header():
    with pytest.raises(api.ZpaqError):
        api.dec_chain_plan(b"\x05\x00\x01\x02")
