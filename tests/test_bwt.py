"""The parts of the BWT (level 3) compression path that need no GPU: the new export, the opt-in of method.check_blocks with
its size limit, pre_bound for levels 3 / 7, the refusal of an oversized block before the device is touched, and the
closed forms the GPU tests use for degenerate blocks."""
import numpy as np
import pytest

from tools import methods
from zpaqsharp_amd import _lib, api, compressor, method


def test_bwt_export_is_declared_and_exported():
    assert "zpaqhip_bwt_blocks" in _lib.SYMBOLS
    assert hasattr(_lib.load(), "zpaqhip_bwt_blocks")
    with open(_lib.os.path.join(_lib._HERE, "..", "include", "zpaqhip.h")) as f:
        assert "int zpaqhip_bwt_blocks(" in f.read()


def test_level3_is_an_opt_in_with_its_own_size_limit():
    args = method.parse_args("x0,3ci1")[1]
    with pytest.raises(ValueError):
        method.check_blocks(args, [10])
    with pytest.raises(ValueError):
        method.check_blocks(args, [10], bwt=False)
    method.check_blocks(args, [10, (1 << 20) - 4096], bwt=True)
    with pytest.raises(ValueError):
        method.check_blocks(args, [10, (1 << 20) - 4095], bwt=True)
    # 2^(args[0] + 20) - 4096 holds for every args[0]: a 4 MiB block needs x3, not x2
    with pytest.raises(ValueError):
        method.check_blocks(method.parse_args("x2,7")[1], [1 << 22], bwt=True)
    method.check_blocks(method.parse_args("x3,7")[1], [1 << 22], bwt=True)
    method.check_blocks(method.parse_args("x12,3")[1], [(1 << 31) - 1], bwt=True)
    with pytest.raises(ValueError):
        method.check_blocks(method.parse_args("x12,3")[1], [1 << 31], bwt=True)
    # the other levels do not change with the keyword
    method.check_blocks(method.parse_args("x0,1,4,0,3,16")[1], [1 << 20], bwt=True)
    with pytest.raises(ValueError):
        method.check_blocks(method.parse_args("x0,1,4,0,3,16")[1], [(1 << 20) + 1], bwt=True)


def test_pre_bound_covers_the_reference_bwt():
    rng = np.random.default_rng(3)
    for m in ("x0,3", "x0,7", "x4,3ci1", "x0,7ci1"):
        args = method.parse_args(m)[1]
        for d in (b"", b"a", bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), b"ab" * 3000, bytes(5000),
                  bytes(rng.integers(0, 3, 4000, dtype=np.uint8))):
            assert len(methods.preprocess(d, args)) == len(d) + 5 <= method.pre_bound(args, len(d)), (m, len(d))


class _NoDevice(api.Context):
    """A Context whose C calls must not happen: the refusals come first."""

    def __init__(self):
        self._L = None
        self._h = None


def test_an_oversized_bwt_block_is_refused_before_the_device():
    ctx = _NoDevice()
    with pytest.raises(ValueError):
        ctx.compress_method("x0,3ci1", [b"x", bytes((1 << 20) - 4095)], bwt=True)
    with pytest.raises(ValueError):
        ctx.compress_method("x0,7", [bytes(1 << 20)], bwt=True)
    with pytest.raises(ValueError):                     # and without the keyword whatever the size
        ctx.compress_method("x0,3ci1", [b"x"])

    class R:
        def read(self, n):
            raise AssertionError("read before the check")
    with pytest.raises(ValueError):
        compressor.compress(R(), None, block_size=1 << 20, context=ctx, method="x0,3ci1", bwt=True)


def one_byte_bwt(z: int, n: int) -> bytes:
    """n >= 1 bytes of value z: every suffix is a prefix of the longer ones, so the suffix array is n-1, ..., 0; every
    suffix but the last in that order (position 0) has z in front of it: z * n, 255, idx = n."""
    return bytes([z]) * n + b"\xff" + n.to_bytes(4, "little")


def period2_bwt(x: int, y: int, m: int) -> bytes:
    """(x y) * m with x < y, n = 2m.  The suffixes at even positions are (xy)^k, those at odd positions y(xy)^k; all of
    the first kind sort below all of the second, and within a kind a shorter one is a prefix of a longer one, so the
    suffix array is n-2, n-4, ..., 0, n-1, n-3, ..., 1.  In front of the first m stands y (255 for position 0, the m-th:
    idx = m), in front of the last m stands x, and byte 0 is the last byte, y: y * m, 255, x * m, idx = m."""
    return bytes([y]) * m + b"\xff" + bytes([x]) * m + m.to_bytes(4, "little")


def test_closed_forms_of_the_degenerate_blocks():
    for n in (1, 2, 5, 4096):
        assert one_byte_bwt(122, n) == methods.bwt_level3(b"z" * n)
        assert one_byte_bwt(0, n) == methods.bwt_level3(bytes(n))
    for m in (1, 2, 3, 2048):
        assert period2_bwt(97, 98, m) == methods.bwt_level3(b"ab" * m)
        assert period2_bwt(0, 255, m) == methods.bwt_level3(b"\x00\xff" * m)
