"""The depth / alpha maps without a GPU: both entry points are exported, listed and declared, and refuse bad arguments before
anything touches a device (with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lcgs_render_maps", "lcgs_render_backward_maps")
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib = lcgs.load_library()
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+LCGS_DEPTH_Z\s+0\b", header) and re.search(r"#define\s+LCGS_DEPTH_INV_Z\s+1\b", header)
    assert (lcgs.DEPTH_Z, lcgs.DEPTH_INV_Z) == (0, 1)
    for method in ("render_maps", "backward_maps"):
        assert callable(getattr(lcgs.Renderer, method))
    assert callable(lcgs.render_autograd_maps)


def test_render_maps_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_render_maps
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)  # a non-NULL context that is never dereferenced
    depth, alpha = C.c_void_p(0x100000), C.c_void_p(0x200000)  # never dereferenced either
    assert fn(null, 0, depth, alpha) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    for mode in (-1, 2, 7):
        assert fn(ctx, mode, depth, alpha) == INVALID_ARG, mode
        assert b"mode" in lib.lcgs_last_error()
    assert fn(ctx, 0, null, null) == INVALID_ARG  # either output may be NULL, not both
    assert b"NULL" in lib.lcgs_last_error()


def test_render_backward_maps_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_render_backward_maps
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    dimg, dd, da = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000))
    g = lcgs.api._Grads(*[C.c_void_p(0x400000 + 0x100000 * k) for k in range(5)])
    assert fn(null, dimg, 0, dd, da, 0, C.byref(g)) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, dimg, 0, dd, da, 0, None) == INVALID_ARG  # no gradient struct
    for mode in (-1, 2):
        assert fn(ctx, dimg, mode, dd, da, 0, C.byref(g)) == INVALID_ARG, mode
        assert b"mode" in lib.lcgs_last_error()
    assert fn(ctx, null, 1, null, null, 0, C.byref(g)) == INVALID_ARG  # any of the three may be NULL, not all three
    assert b"all three" in lib.lcgs_last_error()
    for k in range(5):  # a NULL gradient buffer
        ptrs = [C.c_void_p(0x400000 + 0x100000 * j) for j in range(5)]
        ptrs[k] = null
        assert fn(ctx, null, 0, dd, null, 1, C.byref(lcgs.api._Grads(*ptrs))) == INVALID_ARG, k
        assert b"NULL gradient buffer" in lib.lcgs_last_error()
