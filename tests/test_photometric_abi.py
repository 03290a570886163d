"""The photometric loss without a GPU: both entry points are exported, listed and declared, and refuse bad arguments before
anything touches a device (with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lcgs_photometric_loss_backward", "lcgs_set_fit_loss")
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib = lcgs.load_library()
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+LCGS_LOSS_L2\s+0\b", header) and re.search(r"#define\s+LCGS_LOSS_PHOTOMETRIC\s+1\b", header)
    assert (lcgs.LOSS_L2, lcgs.LOSS_PHOTOMETRIC) == (0, 1)
    for method in ("photometric_loss_backward", "set_fit_loss"):
        assert callable(getattr(lcgs.Renderer, method))


def test_bad_arguments_are_refused_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_photometric_loss_backward
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)  # a non-NULL context that is never dereferenced
    img, tgt, dL, loss = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x400000))  # never dereferenced either
    assert fn(null, 4, 4, img, tgt, 0.2, dL, loss, None) == INVALID_ARG  # NULL context
    assert b"NULL" in lib.lcgs_last_error()
    for args in ((null, tgt, 0.2, dL, loss), (img, null, 0.2, dL, loss), (img, tgt, 0.2, dL, null)):
        assert fn(ctx, 4, 4, *args, None) == INVALID_ARG, args
        assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, 0, 4, img, tgt, 0.2, dL, loss, None) == INVALID_ARG  # width 0
    assert fn(ctx, 4, -1, img, tgt, 0.2, dL, loss, None) == INVALID_ARG
    for lam in (-0.1, 1.5, float("nan"), float("inf")):
        assert fn(ctx, 4, 4, img, tgt, lam, dL, loss, None) == INVALID_ARG, lam
        assert b"lambda" in lib.lcgs_last_error()
    # the gradient may not be written over either image (4 x 4 x 3 floats = 192 bytes each)
    assert fn(ctx, 4, 4, img, tgt, 0.2, img, loss, None) == INVALID_ARG
    assert fn(ctx, 4, 4, img, tgt, 0.2, C.c_void_p(0x200000 + 64), loss, None) == INVALID_ARG
    assert b"alias" in lib.lcgs_last_error()


def test_set_fit_loss_refuses_bad_arguments(lcgs):
    lib = lcgs.load_library()
    ctx = C.c_void_p(0x1000)
    assert lib.lcgs_set_fit_loss(C.c_void_p(0), 1, 0.2) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert lib.lcgs_set_fit_loss(ctx, 7, 0.2) == INVALID_ARG  # unknown kind
    assert lib.lcgs_set_fit_loss(ctx, -1, 0.2) == INVALID_ARG
    for lam in (-0.1, 1.5, float("nan")):
        assert lib.lcgs_set_fit_loss(ctx, 1, lam) == INVALID_ARG, lam
