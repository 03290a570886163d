"""The camera gradient without a GPU: the three entry points are exported, listed and declared, and refuse bad arguments before
anything touches a device (with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lcgs_camera_backward", "lcgs_render_backward_camera", "lcgs_camera_grad_to_twist")
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib = lcgs.load_library()
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header), name
    for method in ("camera_backward", "backward_camera"):
        assert callable(getattr(lcgs.Renderer, method))
    assert callable(lcgs.render_autograd_camera) and callable(lcgs.camera_grad_to_twist)
    # the gradient's order is the struct's: position, front, up, right are lcgs_camera's first four members
    assert tuple(f[0] for f in lcgs.Camera._fields_[:4]) == lcgs.api.CAM12_FIELDS == ("position", "front", "up", "right")
    assert re.search(r"float\s+position\[3\],\s*front\[3\],\s*up\[3\],\s*right\[3\];", header)


def test_camera_backward_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_camera_backward
    null, ctx, out = C.c_void_p(0), C.c_void_p(0x1000), C.c_void_p(0x100000)  # non-NULL values that are never dereferenced
    assert fn(null, out) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, null) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()


def test_render_backward_camera_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_render_backward_camera
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    dimg, dd, da, out = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000))
    assert fn(null, dimg, 0, dd, da, out) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, dimg, 0, dd, da, null) == INVALID_ARG  # no output
    assert b"NULL" in lib.lcgs_last_error()
    for mode in (-1, 2, 7):
        assert fn(ctx, dimg, mode, dd, da, out) == INVALID_ARG, mode
        assert b"mode" in lib.lcgs_last_error()
    assert fn(ctx, null, 1, null, null, out) == INVALID_ARG  # any of the three may be NULL, not all three
    assert b"all three" in lib.lcgs_last_error()
