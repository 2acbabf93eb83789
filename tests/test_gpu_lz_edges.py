"""The edge catalogue of tests/lzcodes.py on the GPU: every crafted block decoded by the default kernel choice, by the generic
kernel and — blocks with a model — by the lane-per-component kernel, each result (output or error text) against the oracle's.
No instruction budget on either side and no exemption: the oracle finishes every case (tests/test_lz_edges.py shows it on the
CPU), so the device has to, with the same bytes."""
import pytest

import oracle
import zpaqsharp_amd as z
from tests import lzcodes

pytestmark = pytest.mark.gpu

# methods whose blocks zh_nibble.hip's kernels take (zpaqhip_stats.kernel_kind 3)
NIBBLE = set(lzcodes.DRAIN_METHODS) | {"x4,6,12,0,7,25,1c0,0,511i2"}


def _oracle(stream, cap):
    try:
        return oracle.decompress(stream, cap=cap), None
    except oracle.OracleError as e:
        return None, str(e)


def _device(ctx, stream, cap, kernel):
    try:
        return ctx.decompress(stream, out_cap=cap, kernel=kernel).tobytes(), None
    except z.ZpaqError as e:
        return None, str(e)


def _same(got, gerr, want, werr, what):
    assert (got is None) == (want is None), (what, werr, gerr)
    if want is not None:
        assert got == want, what
    else:
        assert werr.split(":")[-1].strip() in gerr or gerr.split(":")[-1].strip() in werr, (what, werr, gerr)


def _kernels(info):
    return (0, 1, 4) if info.modelled else (0, 1)


@pytest.mark.parametrize("method", lzcodes.METHODS)
def test_edge_catalogue_on_the_gpu(ctx, method):
    info = lzcodes.Info(method)
    cat = lzcodes.catalogue(method)
    compared = {k: 0 for k in _kernels(info)}
    for name, segs in cat:
        feeds = [lzcodes.feed_of(info, t) for t in segs]
        model = lzcodes.expand(info, feeds)
        s = lzcodes.block_of(info, feeds, plain=model)              # (a truthful size comment: the block is placed by it, one pass)
        want, werr = _oracle(s, len(model) + 4096)
        assert werr is None and want == model, (method, name, werr)
        cap = len(want) + 4096
        for kernel in _kernels(info):
            got, gerr = _device(ctx, s, cap, kernel)
            _same(got, gerr, want, werr, (method, name, kernel))
            st = ctx.stats()
            if kernel == 0 and method in lzcodes.STORE_METHODS:
                assert st.launches == 1, (method, name)            # zh_store.hip took the block: nothing was handed back
            if kernel != 1 and method in NIBBLE:
                assert st.kernel_kind == 3, (method, name, kernel)
            compared[kernel] += 1
    assert all(n == len(cat) for n in compared.values()), compared


@pytest.mark.parametrize("method", [m for m in lzcodes.METHODS if not lzcodes.Info(m).lazy])     # (lazy2's distance field starts at 1)
def test_ffffffff_offset_returns_with_the_oracles_bytes(ctx, method):
    """The block ADVICE r05 describes: a match code of C0 or more followed by FF FF FF FF (distance 0 by wrap-around), first in the
    stream and after literals."""
    info = lzcodes.Info(method)
    for toks in ([("match", info.minlen + 63, 0, 4), ("lit", b"and on"), ("match", info.minlen, 0, 4)],
                 [("lit", b"0123456789" * 30), ("match", info.minlen + 1, 0, 4), ("lit", b"!"), ("match", 40, 3)]):
        feed = lzcodes.feed_of(info, toks)
        assert b"\xff\xff\xff\xff" in feed and feed[feed.index(b"\xff\xff\xff\xff") - 1] >= 0xC0
        s = lzcodes.block_of(info, [feed])
        want = oracle.decompress(s, cap=1 << 16)
        assert want == lzcodes.expand(info, [feed])
        for kernel in _kernels(info):
            assert ctx.decompress(s, out_cap=len(want) + 64, kernel=kernel).tobytes() == want, (method, kernel)


@pytest.mark.parametrize("method", lzcodes.METHODS)
def test_seeded_sweep_on_the_gpu(ctx, method):
    """The sweep's blocks as ONE stream per method and kernel choice: the blocks of a launch run side by side."""
    info = lzcodes.Info(method)
    blocks, wants = [], []
    for toks in lzcodes.sweep(method):
        feed = lzcodes.feed_of(info, toks)
        s = lzcodes.block_of(info, [feed], plain=lzcodes.expand(info, [feed]))
        want, werr = _oracle(s, lzcodes.SWEEP_MAX_OUT + 4096)
        assert werr is None, werr
        blocks.append(s)
        wants.append(want)
    assert len(blocks) == lzcodes.SWEEP_STREAMS
    stream, want = b"".join(blocks), b"".join(wants)
    compared = 0
    for kernel in _kernels(info):
        got, gerr = _device(ctx, stream, len(want) + 4096, kernel)
        assert gerr is None, (method, kernel, gerr)
        if got != want:                                            # which block: the first whose bytes differ
            pos = 0
            for i, w in enumerate(wants):
                assert got[pos:pos + len(w)] == w, (method, kernel, "block", i)
                pos += len(w)
        assert got == want, (method, kernel)
        if kernel != 1 and method in NIBBLE:
            assert ctx.stats().kernel_kind == 3, (method, kernel)
        compared += len(blocks)
    assert compared == lzcodes.SWEEP_STREAMS * len(_kernels(info))
