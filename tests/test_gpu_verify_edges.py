"""The verify pass where it could miss a difference: the compare kernel's group and round arithmetic on every plaintext phase,
length mismatches and the second round of a post-processor that writes more than its room, and the failing block's index
across batches.  Every expected record comes from tests/verify_cases.py (the CPU reference's pre-processors, the oracle's
post-processor, hashlib, numpy; tests/test_verify_cases.py checks the catalogue itself); all streams are valid.

zh_verify_compare's byte-per-lane branch (two ranges on different alignments) is not run here or anywhere: verify_pass always
places the post-processor's output on the plaintext's phase."""
import pytest
import torch

import zpaqsharp_amd as z
from tests import lzcodes, verify_cases as vc
from tests.test_gpu_verify import ROUTES, dev, offs
from tests.verify_cases import E_VERIFY, FORMS, NONE, POS_N
from zpaqsharp_amd import method as mth

pytestmark = pytest.mark.gpu

STORE = FORMS["store"].method


def check(rec, cases, what=""):
    assert len(rec) == len(cases)
    for i, (r, c) in enumerate(zip(rec, cases)):
        assert r == c.want, (what, i, c.name)


def host(ctx, model, cases):
    return ctx.verify_blocks(model, [c.pre for c in cases], [c.orig for c in cases] if cases[0].orig is not None else None)


def device(ctx, model, cases, shift, in_shift=3):
    """verify_blocks_device with the plaintexts back to back from an address of 16-byte phase `shift`."""
    tin, pin = dev(b"".join(c.pre for c in cases), in_shift)
    tor, por = dev(b"".join(c.orig for c in cases), shift)
    assert (tor.data_ptr() & 15) == 0 and (por & 15) == shift & 15
    rec = ctx.verify_blocks_device(model, pin, offs([c.pre for c in cases]), d_orig=por, orig_off=offs([c.orig for c in cases]))
    del tin, tor
    return rec


def test_forms_are_routes():
    assert {f.method for f in FORMS.values() if f.method} == set(ROUTES)


# ---- 1. positions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ph", (0, 1, 15))
def test_positions_host(ctx, ph):
    """One call: a block per flipped position (and per pair of flips: the earlier one is reported) and a clean block, all on
    plaintext phase `ph` (the upload of `orig` starts on a 16-byte boundary; a leading block of `ph` bytes shifts the rest)."""
    cases = vc.position_cases(ph)
    rec = host(ctx, STORE, cases)
    check(rec, cases, ph)
    big = [r for r, c in zip(rec, cases) if len(c.post) == POS_N]
    assert [r["first_diff"] for r in big] == vc.flip_positions(ph) + [a for a, _ in vc.flip_pairs(ph)] + [NONE]
    assert [r["status"] for r in big] == [E_VERIFY] * (len(big) - 1) + [0]


@pytest.mark.parametrize("shift", range(16))
def test_positions_device(ctx, shift):
    """d_orig on each of the sixteen phases: the first byte, the first byte of the compare's second round, the last byte."""
    cases = vc.position_cases(shift, lead=False, flips=[(p,) for p in vc.device_positions(shift)])
    rec = device(ctx, STORE, cases, shift)
    check(rec, cases, shift)
    assert [r["first_diff"] for r, c in zip(rec, cases) if len(c.post) == POS_N] == vc.device_positions(shift) + [NONE]


# ---- 2. neighbours ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flipped", (False, True))
def test_neighbours(ctx, flipped):
    """Blocks of 0 .. 33 bytes back to back: every aligned group the compare loads also holds a neighbour's bytes (plaintext
    side) or bytes nobody wrote (post-processor side); none of them counts.  With `flipped`, exactly the odd blocks fail, at
    their last byte.  (How hard the clean half checks the masking depends on what the output buffer holds where the pass did
    not write: the catalogue's bytes are never zero, so a zeroed or stale buffer differs from the neighbour's plaintext almost
    everywhere, but nothing here sets those bytes.)"""
    cases = vc.neighbour_cases(flipped)
    want = [(E_VERIFY, n - 1) if flipped and n & 1 else (0, NONE) for n in range(34)]
    for what, rec in (("host", host(ctx, STORE, cases)), ("device", device(ctx, STORE, cases, 0)), ("device+11", device(ctx, STORE, cases, 11, 6))):
        check(rec, cases, what)
        assert [(r["status"], r["first_diff"]) for r in rec] == want, what


# ---- 3. lengths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FORMS))
def test_lengths(ctx, name):
    """`orig` cut short: the room is the plaintext's length, the post-processor counts past it and the block goes through a
    second round with the size it reported; the record is the whole output's.  `orig` extended: the output ends first."""
    form = FORMS[name]
    cut, ext = vc.length_cases(form)
    cases = cut + ext
    true = vc.true_cases(cases)
    check(host(ctx, form.model, true), true, "true")
    first_round_only = ctx.stats().launches
    rec = host(ctx, form.model, cases)
    st = ctx.stats()
    check(rec, cases, "host")
    assert st.launches > first_round_only                                      # the second round ran
    assert st.out_bytes == sum(len(c.post) for c in cases)
    assert [r["first_diff"] for r in rec[:len(cut)]] == [len(c.orig) for c in cut]
    check(device(ctx, form.model, cut, 7), cut, "device")


# ---- 4. long output without a plaintext -------------------------------------------------------------------------------------
def test_long_output_without_plaintext(ctx):
    """More than 4 * len + 4096 bytes from a block without a plaintext: the second round, which a feed of one match does not
    need."""
    for c in vc.long_output_cases():
        form = FORMS[c.name.split("-")[0]]
        short = lzcodes.feed_of(lzcodes.Info(form.method), [("lit", b"q"), ("match", 60, 1)])
        assert ctx.verify_blocks(form.model, [short]) == [vc.expected(form.post(short), None)]
        fits = ctx.stats().launches
        rec = ctx.verify_blocks(form.model, [c.pre])
        assert rec == [c.want], c.name
        assert rec[0]["status"] == 0 and rec[0]["first_diff"] == NONE and ctx.stats().launches > fits


# ---- 5. tampered literals ---------------------------------------------------------------------------------------------------
def test_tampered_literals(ctx):
    cases = vc.tamper_cases()
    for name in sorted({c.name.rsplit("-", 2)[0] for c in cases}):
        mine = [c for c in cases if c.name.rsplit("-", 2)[0] == name]
        rec = host(ctx, FORMS[name].model, mine)
        check(rec, mine, name)
        assert all(r["status"] == E_VERIFY for r in rec)


# ---- 6. batches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", (1, 2))
def test_failing_block_across_batches(ctx, kernel):
    """Seven blocks in batches of two, blocks 5 and 6 tampered: the error names block 5, the first failing block of the third
    batch (Call::verify: B.b0 + j).  The device call reports out_len 0 although the first two batches are in d_out by then:
    compress_impl sets `*out_len = 0` before the batch loop (zh_compress.cpp, `*out_len = 0;` under the argument check) and
    leaves the loop with `return rc` on the failing batch (`(rc = c.verify(B))) return rc;`), never reaching finish_call, the
    only place that writes the stream's length.  What d_out holds inside its capacity after a failing call is not promised and
    not asserted here."""
    blocks, pre, tampered = vc.batch_case()
    model, _ = mth.model_of(vc.BATCH_METHOD)
    kw = dict(kernel=kernel, batch_blocks=2)
    rec = ctx.verify_blocks(model, tampered, blocks)
    assert [r["status"] for r in rec] == [0] * 5 + [E_VERIFY] * 2
    clean = ctx.compress_blocks(model, blocks, pre=pre, verify=True, **kw)
    assert clean == ctx.compress_blocks(model, blocks, pre=pre, **kw)
    with pytest.raises(z.ZpaqError) as e:
        ctx.compress_blocks(model, blocks, pre=tampered, verify=True, **kw)
    assert (e.value.code, e.value.block) == (E_VERIFY, 5)
    # the device form, d_out between two guards
    guard, cap, fill = 4096, 1 << 16, 0xA5
    assert len(clean) < cap
    tin, pin = dev(b"".join(tampered), 2)
    tor, por = dev(b"".join(blocks), 9)
    tout = torch.full((guard + cap + guard,), fill, dtype=torch.uint8, device="cuda")
    args = (model, pin, offs(tampered), tout.data_ptr() + guard, cap)
    dkw = dict(d_orig=por, orig_off=offs(blocks), verify=True, **kw)
    with pytest.raises(z.ZpaqError) as e:
        ctx.compress_blocks_device(*args, **dkw)
    assert (e.value.code, e.value.block) == (E_VERIFY, 5)
    rc, n, _ = ctx.compress_blocks_device(*args, raise_on_error=False, **dkw)
    assert (rc, n) == (E_VERIFY, 0)
    got = tout.cpu().numpy()
    assert (got[:guard] == fill).all() and (got[guard + cap:] == fill).all()
