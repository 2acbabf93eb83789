"""zpaqsharp_amd.method (the method-string generator the product uses for Context.compress_method) and the parts of the
method path that need no GPU: the generator is the object tools/methods re-exports, the new C exports are declared and
exported, and the ValueError refusals come before the device is touched."""
import pytest

from tests.test_methods import METHODS
from tools import methods
from zpaqsharp_amd import _lib, api, compressor, method


def test_tools_methods_reexports_the_product_generator():
    for name in ("parse_args", "make_config", "model_of", "_pcomp_lazy2", "_pcomp_lzpre", "_pcomp_bwtrle", "_E8E9_TAIL"):
        assert getattr(methods, name) is getattr(method, name), name


@pytest.mark.parametrize("m", METHODS + ["x0,2,1,0,7,16", "x0,2,3,0,7,16", "x0,2,64,0,7,16", "x2,6,33,0,7,22c0,0,511",
                                         "x4,1,12,0,3,24", "x0,4ci1,1,1,1,2am"])
def test_make_config_matches_the_tooling(m):
    assert method.make_config(m) == methods.make_config(m)
    assert method.parse_args(m) == methods.parse_args(m)
    assert method.model_of(m)[0].header == methods.model_of(m)[0].header


def test_new_exports_are_declared_and_exported():
    assert "zpaqhip_preprocess_blocks" in _lib.SYMBOLS and "zpaqhip_compress_method_blocks" in _lib.SYMBOLS
    L = _lib.load()
    assert hasattr(L, "zpaqhip_preprocess_blocks") and hasattr(L, "zpaqhip_compress_method_blocks")
    with open(_lib.os.path.join(_lib._HERE, "..", "include", "zpaqhip.h")) as f:
        h = f.read()
    assert "int zpaqhip_preprocess_blocks(" in h and "int zpaqhip_compress_method_blocks(" in h
    assert L.zpaqhip_version() == 1


def test_pre_bound_covers_the_reference_preprocessor():
    import numpy as np
    rng = np.random.default_rng(3)
    for m in ("x0,1,4,0,3,16", "x6,1,4,0,3,24", "x0,2,1,0,7,16", "x0,2,3,0,7,16", "x0,2,64,0,7,16", "x0,6,5,0,3,16"):
        args = method.parse_args(m)[1]
        for d in (b"", b"a", bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), b"ab" * 3000, bytes(5000),
                  bytes(rng.integers(0, 3, 4000, dtype=np.uint8))):
            assert len(methods.preprocess(d, args)) <= method.pre_bound(args, len(d)), (m, len(d))


class _NoDevice(api.Context):
    """A Context whose C calls must not happen: the refusals come first."""

    def __init__(self):
        self._L = None
        self._h = None


@pytest.mark.parametrize("m, size", [("x0,3ci1", 10), ("x2,7ci1", 10), ("x0,2,0,0,7,16", 10), ("x0,2,65,0,7,16", 10),
                                     ("x0,1,4,0,3,16", (1 << 20) + 1), ("x0,6,5,0,3,16c0,0,511", (1 << 20) + 1)])
def test_refusals_need_no_device(m, size):
    ctx = _NoDevice()
    blocks = [b"x", bytes(size)]
    with pytest.raises(ValueError):
        ctx.compress_method(m, blocks)
    with pytest.raises(ValueError):
        ctx.preprocess_blocks(m, blocks)


def test_level0_blocks_have_no_size_limit():
    method.check_blocks(method.parse_args("x0,4ci1")[1], [(1 << 20) + 1])
    method.check_blocks(method.parse_args("x0,1,4,0,3,16")[1], [1 << 20])


def test_compressor_refuses_a_block_size_beyond_the_pcomp_memory():
    class R:
        def read(self, n):
            raise AssertionError("read before the check")
    with pytest.raises(ValueError):
        compressor.compress(R(), None, block_size=(1 << 22) + 1, context=_NoDevice(), method="x2,1,4,0,3,22")
    with pytest.raises(ValueError):
        compressor.compress(R(), None, block_size=1 << 16, context=_NoDevice(), method="x2,3ci1")
