"""The antialiased raster mode without a GPU: lcgs_set_raster_mode is exported, listed and declared, and refuses bad arguments
before anything touches a device (with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

INVALID_ARG = 1


def test_symbol_is_exported_listed_and_declared(lcgs):
    lib = lcgs.load_library()
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    name = "lcgs_set_raster_mode"
    assert hasattr(lib, name)
    assert name in lcgs.api.EXPORTED_SYMBOLS
    assert name in lcgs.api._signatures()
    assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(\s*lcgs_context\*\s*ctx\s*,\s*int\s+mode\s*\)", header)
    assert re.search(r"#define\s+LCGS_RASTER_CLASSIC\s+0\b", header) and re.search(r"#define\s+LCGS_RASTER_ANTIALIASED\s+1\b", header)
    assert (lcgs.RASTER_CLASSIC, lcgs.RASTER_ANTIALIASED) == (0, 1)
    assert callable(lcgs.Renderer.set_raster_mode)
    # what is not offered is said where the contract is
    for phrase in ("stage-level operators", "ownership step", "3-D smoothing filter", "per-call mode argument"):
        assert phrase in header, phrase


def test_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_set_raster_mode
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)  # a non-NULL context that is never dereferenced
    assert fn(null, 0) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(null, 1) == INVALID_ARG
    for mode in (2, -1, 7):
        assert fn(ctx, mode) == INVALID_ARG, mode
        assert b"LCGS_RASTER" in lib.lcgs_last_error()


def test_python_wrapper_refuses_unknown_names(lcgs):
    class _NoContext:  # the name is checked before the context is touched
        ctx = None

    with pytest.raises(ValueError):
        lcgs.Renderer.set_raster_mode(_NoContext(), "supersampled")
