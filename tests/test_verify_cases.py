"""tests/verify_cases.py is what it says, before any GPU sees it: every form's pre-processed bytes come back as the plaintext
through the oracle's post-processor, every case differs where its name says, and expected() is the record of hand-written
pairs."""
import hashlib

import pytest

import oracle
from tests import lzcodes, verify_cases as vc
from tests.verify_cases import E_VERIFY, FORMS, NONE, POS_N


def _rec(status, out_len, diff, data):
    return {"status": status, "out_len": out_len, "first_diff": diff, "sha1": hashlib.sha1(data).digest()}


def test_first_diff_and_expected_on_hand_written_pairs():
    assert vc.first_diff(b"", b"") == NONE and vc.first_diff(b"abc", b"abc") == NONE
    assert vc.first_diff(b"abc", b"abd") == 2 and vc.first_diff(b"xbc", b"abc") == 0
    assert vc.first_diff(b"abc", b"ab") == 2 and vc.first_diff(b"ab", b"abc") == 2 and vc.first_diff(b"", b"a") == 0
    assert vc.first_diff(b"xbc", b"ab") == 0                                  # a difference before the shorter one's end
    assert vc.expected(b"abc", b"abc") == _rec(0, 3, NONE, b"abc")
    assert vc.expected(b"abc", None) == _rec(0, 3, NONE, b"abc")
    assert vc.expected(b"", b"") == _rec(0, 0, NONE, b"")
    assert vc.expected(b"abc", b"abd") == _rec(E_VERIFY, 3, 2, b"abc")        # size and digest are the post-processor's side
    assert vc.expected(b"abcd", b"ab") == _rec(E_VERIFY, 4, 2, b"abcd")
    assert vc.expected(b"ab", b"abcd") == _rec(E_VERIFY, 2, 2, b"ab")
    assert vc.expected(b"", b"a") == _rec(E_VERIFY, 0, 0, b"")
    assert vc.expected(b"a", b"") == _rec(E_VERIFY, 1, 0, b"a")
    assert hashlib.sha1(b"").hexdigest() == "da39a3ee5e6b4b0d3255bfef95601890afd80709"


@pytest.mark.parametrize("name", list(FORMS))
def test_every_form_round_trips_on_the_oracle(name):
    form = FORMS[name]
    assert form.sizes[:4] == [0, 1, 300, 5000] and form.sizes[4] == (140000 if form.wave else 20000)
    for n in form.sizes + [vc.TAMPER_N]:
        plain, pre, post = form.block(n, seed=int(n == vc.TAMPER_N))
        assert len(plain) == n and post == plain, (name, n)
    if "e8e9" in name:                                                         # the transform has something to undo
        assert vc.methods.e8e9_forward(form.block(5000)[0]) != form.block(5000)[0]


@pytest.mark.parametrize("ph", range(16))
def test_position_cases_differ_where_they_say(ph):
    assert POS_N == 3 * 4096 + 37
    singles = vc.flip_positions(ph)
    assert singles == sorted(set(singles)) and singles[0] == 0 and singles[-1] == POS_N - 1 and len(singles) == {14: 9, 15: 8}.get(ph, 10)
    for want in (0, 1, POS_N - 2, POS_N - 1):
        assert want in singles
    for at in (15, 16, 4095, 4096, 4097, 8192):                                # position + phase: the kernel's group arithmetic
        assert at - ph in singles
    pairs = vc.flip_pairs(ph)
    a, b = pairs[0]
    assert a < b and (a + ph) // 16 == (b + ph) // 16
    a, b = pairs[1]
    assert (a + ph) // 16 == 255 and (b + ph) // 16 == 256                     # the last lane of round 0, the first of round 1
    assert pairs[2] == (0, POS_N - 1)
    cases = vc.position_cases(ph)
    flips = [(p,) for p in singles] + pairs + [()]
    blocks = [(i, c) for i, c in enumerate(cases) if len(c.post) == POS_N]
    assert len(blocks) == len(flips)
    for (i, c), at in zip(blocks, flips):
        assert vc.phase_of(cases, i) == ph, c.name
        assert c.pre == c.post and len(c.orig) == POS_N
        assert [k for k in range(POS_N) if c.orig[k] != c.post[k]] == list(at), c.name
        assert c.want == _rec(E_VERIFY if at else 0, POS_N, at[0] if at else NONE, c.post), c.name
    for i, c in enumerate(cases):
        if len(c.post) != POS_N:
            assert c.orig == c.post and c.want["status"] == 0 and len(c.post) in (ph, vc.POS_PAD)
    # the device form's three: no leading filler, the phase comes from where the plaintext lies
    dev = vc.position_cases(ph, lead=False, flips=[(p,) for p in vc.device_positions(ph)])
    assert vc.device_positions(ph) == [0, 4096 - ph, POS_N - 1]
    big = [i for i, c in enumerate(dev) if len(c.post) == POS_N]
    assert len(big) == 4 and all(vc.phase_of(dev, i, start=ph) == ph for i in big)
    assert [dev[i].want["first_diff"] for i in big] == vc.device_positions(ph) + [NONE]


def test_neighbour_cases():
    clean, bad = vc.neighbour_cases(False), vc.neighbour_cases(True)
    assert [len(c.post) for c in clean] == list(range(34)) == [len(c.orig) for c in bad]
    assert {vc.phase_of(clean, i) for i in range(34)} == set(range(16))
    for n, (c, b) in enumerate(zip(clean, bad)):
        assert c.orig == c.post == c.pre == b.post and 0 not in c.post
        assert c.want == _rec(0, n, NONE, c.post)
        assert b.want == (_rec(E_VERIFY, n, n - 1, c.post) if n & 1 else c.want)


@pytest.mark.parametrize("name", list(FORMS))
def test_length_cases(name):
    form = FORMS[name]
    cut, ext = vc.length_cases(form)
    big = form.sizes[-1]
    assert [len(c.orig) for c in cut] == [0, 0, 1, 150, 299, 0, 1, 2500, 4999, 0, 1, big // 2, big - 1]
    assert [len(c.orig) - len(c.post) for c in ext] == [0, 1, 5000] + [1, 5000] * 4
    for c in cut:
        assert c.post.startswith(c.orig) and c.want == _rec(E_VERIFY, len(c.post), len(c.orig), c.post), c.name
    for c in ext[1:]:
        assert c.orig.startswith(c.post) and c.want == _rec(E_VERIFY, len(c.post), len(c.post), c.post), c.name
    assert ext[0].want == _rec(0, 0, NONE, b"") and ext[0].pre == form.pre(b"")
    assert ext[1].pre == ext[0].pre and len(ext[1].orig) == 1                 # the empty block against one byte
    for c, t in zip(cut, vc.true_cases(cut)):
        assert t.pre == c.pre and t.want == _rec(0, len(c.post), NONE, c.post)


def test_long_output_feeds_exceed_the_room_without_a_plaintext():
    cases = vc.long_output_cases()
    assert [c.name for c in cases] == ["lzpre-long", "lazy2-long"]
    for c, name, n in zip(cases, ("lzpre", "lazy2"), (1 + 200 * 75, 1 + 2 * 65536)):
        form = FORMS[name]
        assert c.post == b"q" * n and c.orig is None                           # by the oracle
        assert len(c.post) == len(lzcodes.expand(lzcodes.Info(form.method), [c.pre]))
        assert len(c.post) > vc.room_without_plaintext(form, c.pre) >= 4 * len(c.pre) + 4096
        assert c.want == _rec(0, n, NONE, c.post)


@pytest.mark.parametrize("method", ["x0,1,4,0,3,16", "x0,2,12,0,7,16"])
def test_lzcodes_catalogue_holds_long_output_feeds(method):
    """tests/test_gpu_verify.py::test_crafted_codes verifies these feeds without a plaintext: it has run the second round."""
    info = lzcodes.Info(method)
    segs = dict(lzcodes.catalogue(method))["len-65536-dist-1" if info.lazy else "ring-dist-131008"]
    feed = lzcodes.feed_of(info, segs[0])
    h = info.model.header
    post = oracle.run_pcomp(info.model.pcomp, feed, h[4], h[5], cap=1 << 18)
    assert len(segs) == 1 and len(post) > 4 * (len(feed) + 3 + len(info.model.pcomp)) + 4096


def test_tamper_cases_are_valid_codes_that_differ():
    cases = vc.tamper_cases()
    assert [c.name for c in cases] == [f"{f}-{w}-literal" for f in ("lazy2", "lazy2+e8e9", "lzpre", "lzpre+e8e9")
                                       for w in ("first", "last")] + ["store-byte"]
    for c in cases:
        form = FORMS[c.name.rsplit("-", 2)[0]]
        plain, pre, _ = form.block(vc.TAMPER_N, seed=1)
        assert c.orig == plain and len(c.pre) == len(pre)
        assert sum(bin(a ^ b).count("1") for a, b in zip(c.pre, pre)) == 1
        assert len(c.post) == len(plain) and c.post != plain                   # the same codes, one other value
        assert c.want["status"] == E_VERIFY and c.want["first_diff"] < len(plain)
        if "first" in c.name:
            assert c.want["first_diff"] == 0
        if c.name in ("lazy2-last-literal", "lzpre-last-literal", "store-byte"):
            where = [k for k in range(len(plain)) if c.post[k] != plain[k]]
            assert len(where) >= 1 and c.want["first_diff"] == where[0]
    # the walkers find what the model of the codes finds: every literal byte, in order
    for name in ("lazy2", "lzpre"):
        form = FORMS[name]
        plain, pre, _ = form.block(vc.TAMPER_N, seed=1)
        if name == "lazy2":
            v = int.from_bytes(pre, "little")
            lits = bytes((v >> b) & 255 for b in vc.lazy2_literals(pre, 0))
        else:
            lits = bytes(pre[i] for i in vc.lzpre_literals(pre))
        assert 0 < len(lits) < len(plain)
        it = iter(plain)
        assert all(any(x == y for y in it) for x in lits)                      # a subsequence of the plaintext


def test_batch_case():
    blocks, pre, tampered = vc.batch_case()
    form = FORMS["lzpre"]
    assert len(blocks) == 7 and vc.BATCH_BAD == (5, 6)
    assert vc.methods.model_of(vc.BATCH_METHOD)[0].pcomp == form.model.pcomp   # the modelled method's program is the form's
    for i, (b, p, t) in enumerate(zip(blocks, pre, tampered)):
        assert form.post(p) == b
        assert (t != p) == (i in vc.BATCH_BAD)
        assert (form.post(t) != b) == (i in vc.BATCH_BAD) and len(form.post(t)) == len(b)
