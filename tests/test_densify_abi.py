"""Adaptive density control without a GPU: the three entry points are exported and refuse NULL arguments before anything
touches a device (with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C

NAMES = ("lcgs_densify_accumulate", "lcgs_densify", "lcgs_opacity_reset")


def test_symbols_are_exported_and_listed(lcgs):
    lib = lcgs.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
    for method in ("densify_accumulate", "densify", "opacity_reset"):
        assert callable(getattr(lcgs.Renderer, method))


def test_null_arguments_are_refused_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    stats = lcgs.api._DensifyStats(None, None, None)
    pack = lcgs.api._Params(None, None, None, None, None)
    cfg = lcgs.api._DensifyConfig(2e-4, 0.01, 1.0, 0.005, 0, 0)
    n = C.c_int64(-1)
    p, s = C.byref(pack), C.byref(stats)
    fake_ctx = C.c_void_p(0)
    assert lib.lcgs_densify_accumulate(fake_ctx, 4, s) == 1  # LCGS_ERR_INVALID_ARG: NULL context
    assert b"NULL" in lib.lcgs_last_error()
    assert lib.lcgs_densify(fake_ctx, 4, 3, C.byref(cfg), s, p, p, p, p, p, p, p, s, 8, None, None, C.byref(n)) == 1
    assert lib.lcgs_opacity_reset(fake_ctx, 4, C.c_float(0.01), p, p, p, p) == 1
    # a NULL config / statistics / pack with a (never dereferenced) non-NULL context: refused by the first check too
    ctx = C.c_void_p(0x1000)
    assert lib.lcgs_densify(ctx, 4, 3, None, s, p, p, p, p, p, p, p, s, 8, None, None, C.byref(n)) == 1
    assert lib.lcgs_densify(ctx, 4, 3, C.byref(cfg), s, p, p, p, p, p, p, p, s, 8, None, None, None) == 1
    assert lib.lcgs_densify_accumulate(ctx, 4, None) == 1
    assert lib.lcgs_opacity_reset(ctx, 4, C.c_float(0.01), None, p, p, p) == 1
