"""zh_nibble.hip with opts.kernel == KERNEL_MODEL_E8: `lzpre` and `bwtrle` with E8E9 behind a model decoded with their
post-processor run wave-wide, the end-of-segment E8E9 loop as rounds of zh_e8e9_wave.h — against the oracle, the
plaintext and opts.kernel == 0; zpaqhip_stats.e8_wave_segs tells which path a segment took."""
import numpy as np
import pytest

import oracle
import zpaqsharp_amd as z
from tests import model_e8_cases as mc
from tests import store_e8_cases as cases
from tests import util
from tools import methods
from zpaqsharp_amd import synth

pytestmark = pytest.mark.gpu

K = z.KERNEL_MODEL_E8
SLICE, ROUND = 64, 4096


def _decode(ctx, s: bytes, kernel: int, cap=None, sha: bool = True):
    got = ctx.decompress(s, out_cap=cap, kernel=kernel, verify_sha1=sha).tobytes()
    return got, ctx.stats().e8_wave_segs


def _outcome(fn):
    try:
        return ("ok", fn())
    except (oracle.OracleError, z.ZpaqError) as e:
        return ("err", str(e))


@pytest.mark.parametrize("kind", ["X", "T"])
@pytest.mark.parametrize("method", mc.E8)
def test_the_three_methods_run_their_loop_wave_wide(ctx, method, kind):
    data = synth.plain(kind, 3, 65536).tobytes()
    s = methods.compress_block(method, data)
    assert oracle.decompress(s, cap=len(data) + 16) == data
    assert _decode(ctx, s, K) == (data, 1)
    assert _decode(ctx, s, 0) == (data, 0)


@pytest.mark.parametrize("method", mc.E8)
def test_pass_inputs_as_plaintexts_and_as_what_the_pass_runs_over(ctx, method):
    inputs = cases.pass_inputs(SLICE, ROUND)
    for name in [k for k in inputs if k.startswith(("dense", "run", "chain", "boundary", "tail"))]:
        x = inputs[name]
        s = methods.compress_block(method, x)
        assert oracle.decompress(s, cap=len(x) + 16) == x, name
        assert _decode(ctx, s, K) == (x, 1), name
        want = oracle.decompress(methods.compress_block(method, b"", pre=mc.pre_of(method, x)), cap=len(x) + 16)
        assert len(want) == len(x), name
        s = methods.compress_block(method, want, pre=mc.pre_of(method, x))       # (size comment and SHA-1 of what the program gives)
        assert _decode(ctx, s, K) == (want, 1), name


@pytest.mark.parametrize("method", mc.E8)
def test_short_plaintexts(ctx, method):
    for n in (0, 1, 4, 5, 6):
        data = bytes([0xE8, 0x10, 0x20, 0x30, 0xFF, 0xE9])[:n]
        s = methods.compress_block(method, data)
        assert oracle.decompress(s, cap=64) == data
        assert _decode(ctx, s, K, cap=64)[0] == data, n
        assert _decode(ctx, s, 0, cap=64) == (data, 0), n


def _device_block(ctx, stream: bytes, cap: int, kernel: int):
    import torch
    sc = z.scan(stream)
    a = np.frombuffer(stream + b"\0" * (-len(stream) % 4 + 4), np.uint8)
    d_in = torch.from_numpy(a.copy()).cuda()
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    rc, res = ctx.decode_blocks_device(d_in.data_ptr(), len(stream), sc, d_out.data_ptr(), [0], [cap], ids=[0], raise_on_error=False, kernel=kernel)
    return rc, [(r.status, r.out_len, r.out_off, r.pp_state, r.in_used) for r in res], d_out.cpu().numpy().tobytes()


@pytest.mark.parametrize("method", [mc.LZ3, mc.BWT])
def test_output_capacity_seven_bytes_short(ctx, method):
    data = synth.plain("X", 5, 9000).tobytes()
    s = methods.compress_block(method, data)
    want = oracle.decompress(s, cap=len(data) + 16)
    assert want == data
    cap = len(want) - 7
    rc, res, out = _device_block(ctx, s, cap, K)
    print(rc, res)
    assert res[0][0] == -20 and res[0][1] == len(want)       # ZPAQHIP_E_OUTPUT_FULL, the full length
    assert out[:cap] == want[:cap] and out[cap:] == bytes(64)  # counted, not written
    assert (rc, res, out) == _device_block(ctx, s, cap, 0)


def test_second_segment_reads_what_the_pass_left_in_m(ctx):
    s, n = mc.two_segments(1 << 20)
    want = oracle.decompress(s, cap=n + 64)
    assert len(want) == n
    assert _decode(ctx, s, K, cap=n, sha=False) == (want, 2)
    assert _decode(ctx, s, 0, cap=n, sha=False) == (want, 0)


def test_a_segment_longer_than_m_goes_back_to_the_program(ctx):
    s, n = mc.two_segments((1 << 20) + 1)
    want = oracle.decompress(s, cap=n + 64)
    assert len(want) == n
    assert _decode(ctx, s, K, cap=n, sha=False) == (want, 1)     # the second segment is short: its loop runs wave-wide


@pytest.mark.parametrize("method", mc.E8)
def test_a_changed_operand_of_the_loop_goes_back_to_the_program(ctx, method):
    other, args = mc.changed_loop(method)
    data = synth.plain("X", 7, 12000).tobytes()
    s = mc.modelled_block(other, [methods.preprocess(data, args)], sizes=[len(data)])
    want = oracle.decompress(s, cap=len(data) + 16)
    assert len(want) == len(data) and want != data
    assert _decode(ctx, s, K, cap=len(data), sha=False) == (want, 0)


@pytest.mark.parametrize("how", ["idx0", "not255"])
def test_a_block_the_inverse_bwt_refuses(ctx, how):
    x = synth.plain("X", 9, 5000).tobytes()
    pre = bytearray(methods.bwt_level3(x))
    idx = int.from_bytes(pre[-4:], "little")
    if how == "idx0":
        pre[-4:] = bytes(4)
    else:
        pre[idx] = 0x41
    s = methods.compress_block(mc.BWT, x, pre=bytes(pre))
    want = _outcome(lambda: oracle.decompress(s, cap=len(x) + 64))
    got = _outcome(lambda: ctx.decompress(s, out_cap=len(x) + 64, kernel=K).tobytes())
    got0 = _outcome(lambda: ctx.decompress(s, out_cap=len(x) + 64, kernel=0).tobytes())
    print(how, want[0], len(want[1]))
    assert got == want and got0 == want


def test_single_bit_damage_in_a_level_3_stream(ctx):
    rng = np.random.default_rng(78)
    good = methods.compress_block(mc.LZ3, synth.plain("X", 11, 40000).tobytes())
    g = z.scan(good).segments[0]
    for trial in range(6):
        dmg = bytearray(good)
        pos = int(g.data_off + rng.integers(40, g.data_len - 8))
        dmg[pos] ^= 1 << int(rng.integers(0, 8))
        want = _outcome(lambda: oracle.decompress(bytes(dmg), cap=1 << 20))
        got = _outcome(lambda: ctx.decompress(bytes(dmg), kernel=K).tobytes())
        got0 = _outcome(lambda: ctx.decompress(bytes(dmg), kernel=0).tobytes())
        assert got == want and got0 == want, (trial, pos)


def test_one_stream_of_every_kind_of_block(ctx):
    """Blocks whose launches hand the overlaid tables from one program to another: the three E8E9 methods, their twins
    without E8E9, the built-in min and mid, and two unmodelled E8E9 forms for the store kernel."""
    parts, n_e8 = [], 0
    for i in range(40):
        d = synth.plain("XT"[(i >> 2) & 1], i, 9000 + 37 * i).tobytes()
        m = mc.E8[i % 3]
        parts += [(methods.compress_block(m, d), d), (methods.compress_block(mc.TWIN[m], d[:3000 + i]), d[:3000 + i])]
        n_e8 += 1
    for i, name in enumerate(("min", "mid", "min", "mid")):
        d = util.text(4000 + 333 * i, seed=40 + i)
        parts.append((util.block(name, d), d))
    for m in ("x0,5,4,0,3,16", "x0,6,12,0,7,16"):
        d = synth.plain("X", 50, 20000).tobytes()
        parts.append((methods.compress_block(m, d), d))
    s, plain = b"".join(p for p, _ in parts), b"".join(d for _, d in parts)
    got = ctx.decompress(s, kernel=K, verify_sha1=True).tobytes()
    st = ctx.stats()
    at = 0
    for i, (_, d) in enumerate(parts):
        assert got[at:at + len(d)] == d, i
        at += len(d)
    assert at == len(got) and st.e8_wave_segs == n_e8
    launches = st.launches
    assert ctx.decompress(s, kernel=z.KERNEL_STORE_E8, verify_sha1=True).tobytes() == plain
    assert (ctx.stats().launches, ctx.stats().e8_wave_segs) == (launches, 0)
