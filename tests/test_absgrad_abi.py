"""lcgs_absgrad_accumulate without a GPU: the entry point is exported, listed and declared once, its contract and what is not
offered are said in the header, and it refuses bad arguments before anything touches a device (with tests/test_abi.py this pins
header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAME = "lcgs_absgrad_accumulate"
INVALID_ARG = 1
DEPTH_Z, DEPTH_INV_Z = 0, 1


def _addr(k):
    return C.c_void_p(0x100000 * (k + 1))  # never dereferenced


def test_symbol_is_exported_listed_and_declared(lcgs):
    lib = lcgs.load_library()
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    assert hasattr(lib, NAME)
    assert lcgs.api.EXPORTED_SYMBOLS.count(NAME) == 1
    assert len(re.findall(r"LCGS_API\s+lcgs_status\s+" + NAME + r"\s*\(", header)) == 1
    restype, argtypes = lcgs.api.SIGNATURES[NAME]
    assert restype is C.c_int and len(argtypes) == 8
    assert argtypes[6] is C.POINTER(lcgs.api.STRUCTS["lcgs_densify_stats"])
    assert callable(lcgs.Renderer.absgrad_accumulate)
    assert (lcgs.api.DEPTH_Z, lcgs.api.DEPTH_INV_Z) == (DEPTH_Z, DEPTH_INV_Z)
    # the definition, the order of operations and what is not offered are said where the contract is
    at = header.index("AbsGS densification statistics")
    text = " ".join(header[at:header.index(NAME + "(", at)].replace("*", " ").split())
    for phrase in ("summed per pixel FIRST", "then the absolute value", "sum_p |g_x(p, i)|", "ADDED at [2 i, 2 i + 1]", "NO preceding backward",
                   "the 0.99 cap passes nothing", "last layer behind the colour channels", "bit for bit", "about twice the 3DGS value",
                   "absgrad_walk, absgrad_rows"):
        assert phrase in text, phrase
    for phrase in ("distortion, normal and feature channels", "compact rows", "ownership step", "lcgs_fit_views", "lcgs-app flag",
                   "fused into the render-backward"):
        assert phrase in text[text.index("Not offered"):], phrase
    # the C++ mirror
    hpp = open(os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc", "lcgs", "lcgs.hpp")).read()
    assert re.search(r"void\s+absgrad_accumulate\s*\(", hpp) and NAME in hpp


def test_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = getattr(lib, NAME)
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)  # a non-NULL context that is never dereferenced
    stats = lcgs.api._DensifyStats(_addr(0), _addr(1), _addr(2))
    di, dd, da, out = _addr(3), _addr(4), _addr(5), _addr(6)
    assert fn(null, 10, di, DEPTH_Z, dd, da, C.byref(stats), out) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, 10, null, DEPTH_Z, null, null, C.byref(stats), out) == INVALID_ARG
    assert b"all three gradients" in lib.lcgs_last_error()
    assert fn(ctx, 10, di, DEPTH_Z, dd, da, None, null) == INVALID_ARG
    assert b"both outputs" in lib.lcgs_last_error()
    for k in range(3):  # a statistics set with a NULL member, one member at a time -- also when d_absgrad is given
        ptrs = [_addr(j) for j in range(3)]
        ptrs[k] = null
        for o in (out, null):
            assert fn(ctx, 10, di, DEPTH_Z, null, null, C.byref(lcgs.api._DensifyStats(*ptrs)), o) == INVALID_ARG, k
            assert b"statistics" in lib.lcgs_last_error()
    for mode in (-1, 2, 7):
        assert fn(ctx, 10, di, mode, dd, da, C.byref(stats), out) == INVALID_ARG
        assert b"mode" in lib.lcgs_last_error()
        assert fn(ctx, 10, di, mode, null, null, None, out) == INVALID_ARG  # (the mode is checked whether or not a map channel is given)
