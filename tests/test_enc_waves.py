"""The host side of the lane-per-component encoder's waves per compute unit (zh_enc_chain.hip, compress opts.enc_waves): the
options field, and zpaqhip_enc_chain_plan, the LDS plan of a model: one copy of the tables for the workgroup and, per wave,
the model's ICM / ISSE pool (1 KiB per unit: ICM 1, ISSE 2) and a fixed part, in 163 840 bytes.  No GPU needed."""
import ctypes as C

import pytest

from tests import chain_cases as cc
from zpaqsharp_amd import _lib, api, method, models, zpaql

LDS = 163840
TABLES = 79872                                     # sizeof(ZhTables): squash, stretch, dt, dt2k, ns


def _units(model) -> int:
    """ICM + 2 ISSE of a model: its LDS pool in KiB."""
    comps = zpaql.parse_header(model.header)[4]
    return sum(1 if c[0] == 3 else 2 if c[0] == 8 else 0 for c in comps)


def _catalogue():
    for name, case in cc.DIRECTED.items():
        yield name, zpaql.assemble(case.cfg)
    for g in range(cc.GROUPS):
        for i, cfg in enumerate(cc.random_group(g, cc.seed())):
            yield f"random-{g}-{i}", zpaql.assemble(cfg)


def test_compress_opts_carry_enc_waves_where_reserved0_was():
    assert _lib.CompressOpts.enc_waves.offset == 12 and _lib.CompressOpts.enc_waves.size == 4
    assert _lib.CompressOpts.batch_blocks.offset == 16 and C.sizeof(_lib.CompressOpts) == 48
    assert not hasattr(_lib.CompressOpts, "reserved0")


def test_the_plan_is_exported_and_declared():
    assert "zpaqhip_enc_chain_plan" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "zpaqhip_enc_chain_plan")


@pytest.mark.parametrize("name, floor", [("min", 4), ("mid", 3), ("max", 2), ("x0,3ci1", 4), ("x0,0ci1,1,1,1,2am", 3)])
def test_built_in_and_method_models_get_their_waves(name, floor):
    m = models.get(name) if name in ("min", "mid", "max") else method.model_of(name)[0]
    waves, lds = api.enc_chain_plan(m)
    assert floor <= waves <= 4
    assert TABLES + waves * 1024 * _units(m) < lds <= LDS


def test_the_largest_chains_keep_one_wave():
    for name in ("n64-h0", "n64-h10", "units64"):  # 63, 63 and 64 units: two pools alone are past what the tables leave
        m = zpaql.assemble(cc.DIRECTED[name].cfg)
        assert _units(m) in (63, 64)
        waves, lds = api.enc_chain_plan(m)
        assert waves == 1 and TABLES + 1024 * _units(m) < lds <= LDS, name
    assert {_units(zpaql.assemble(cc.DIRECTED[n].cfg)) for n in ("n64-h0", "units64")} == {63, 64}


def test_models_outside_the_family_get_none():
    for name in ("outside-5mix", "outside-65units", "outside-n65", "outside-cm3"):
        assert cc.DIRECTED[name].kind == 1
        assert api.enc_chain_plan(zpaql.assemble(cc.DIRECTED[name].cfg)) == (0, 0), name
    assert api.enc_chain_plan("l1") == (0, 0)      # a single CM has its own encoder


def test_every_catalogue_plan_fits_the_lds_and_repeats():
    seen = set()
    for name, m in _catalogue():
        waves, lds = api.enc_chain_plan(m)
        assert api.enc_chain_plan(m) == (waves, lds), name
        assert 0 <= waves <= 4 and lds <= LDS, name
        inside = not name.startswith("outside-")
        assert (waves >= 1) == inside and (lds > TABLES) == inside, name
        if waves:
            # the pools of the waves, the tables and something for the rest of each wave; and no further wave would fit
            per_wave = (lds - TABLES) // waves
            assert (lds - TABLES) % waves == 0 and per_wave > 1024 * _units(m), name
            assert waves == 4 or lds + per_wave > LDS, name
        seen.add(waves)
    assert seen >= {0, 1, 4}


def test_the_plan_rejects_what_is_no_header():
    with pytest.raises(api.ZpaqError):
        api.enc_chain_plan(b"\x05\x00\x01\x02")
