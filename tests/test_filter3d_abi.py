"""The 3-D smoothing filter's four entry points without a GPU: exported, listed and declared as the header spells them, and every
bad argument refused before anything touches a device -- with a NULL context, or a non-NULL one that is never dereferenced
(with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

import filter3d_ref as R
from conftest import ROOT

NAMES = ("lcgs_filter3d_accumulate", "lcgs_filter3d_finalize", "lcgs_filter3d_apply", "lcgs_filter3d_backward")
OK, INVALID_ARG = 0, 1


def _addr(k):
    return C.c_void_p(0x100000 * (k + 1))  # never dereferenced


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib, api = lcgs.load_library(), lcgs.api
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    p, i, f = C.c_void_p, C.c_int, C.c_float
    expected = {"lcgs_filter3d_accumulate": [p, i, p, i, C.POINTER(api.Camera), p, p], "lcgs_filter3d_finalize": [p, i, p, f, p],
                "lcgs_filter3d_apply": [p, i, p, p, p, p, p], "lcgs_filter3d_backward": [p, i, p, p, p, p, p, p, p]}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(lcgs_context\* ctx, int num_gaussians,", header), name
        assert api.SIGNATURES[name] == (C.c_int, expected[name]), name
    for method in ("filter3d_accumulate", "filter3d_finalize", "filter3d_apply", "filter3d_backward"):
        assert callable(getattr(lcgs.Renderer, method)), method
    assert callable(lcgs.filter3d_autograd) and lcgs.filter3d_autograd is api.filter3d_autograd
    # the contract, the recipe and what is not offered are said where the declarations are
    for phrase in ("3-D smoothing filter", "Training recipe", "d_src_row", "lcgs_ply_write_raw", "lcgs_render_backward_adam",
                   "lcgs_fit_views", "ownership step", "filter_3D PLY property", "lcgs-app flag", "cannot underflow"):
        assert phrase in header, phrase
    # the accumulate pass's view chunk: one constant in the kernels' header, the binding and the restatement
    launch = open(os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc", "kernels", "launch.hpp")).read()
    chunk = int(re.search(r"constexpr int kFilter3dViewChunk = (\d+);", launch).group(1))
    assert chunk == api.LCGS_FILTER3D_VIEW_CHUNK == R.VIEW_CHUNK


def _refused(lib, status, needle):
    assert status == INVALID_ARG, status
    assert needle in lib.lcgs_last_error(), lib.lcgs_last_error()


def test_accumulate_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_filter3d_accumulate
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    cams = (lcgs.Camera * 2)(lcgs.get_lookat_cam([3, 0, 1], [0, 0, 0], [0, 0, 1]), lcgs.get_lookat_cam([0, 3, 1], [0, 0, 0], [0, 0, 1]))
    focal = C.c_float(7.0)
    good = [ctx, 10, _addr(0), 2, cams, _addr(1), C.byref(focal)]
    for k in (0, 2, 5, 6):  # context, positions, min_z, max_focal
        args = list(good)
        args[k] = null
        _refused(lib, fn(*args), b"NULL")
    args = list(good)
    args[4] = None  # views without cameras
    _refused(lib, fn(*args), b"NULL cameras")
    args[3] = -1
    _refused(lib, fn(*args), b"negative")
    args = list(good)
    args[1] = -1
    _refused(lib, fn(*args), b"negative")
    assert focal.value == 7.0


def test_finalize_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_filter3d_finalize
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    _refused(lib, fn(null, 10, _addr(0), 100.0, _addr(1)), b"NULL")
    _refused(lib, fn(ctx, 10, null, 100.0, _addr(1)), b"NULL")
    _refused(lib, fn(ctx, 10, _addr(0), 100.0, null), b"NULL")
    _refused(lib, fn(ctx, -1, _addr(0), 100.0, _addr(1)), b"negative")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _refused(lib, fn(ctx, 10, _addr(0), bad, _addr(1)), b"max_focal")


def test_apply_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_filter3d_apply
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    good = [ctx, 10, _addr(0), _addr(1), _addr(2), _addr(3), _addr(4)]
    for k in (0, 2, 3, 4, 5, 6):
        args = list(good)
        args[k] = null
        _refused(lib, fn(*args), b"NULL")
    args = list(good)
    args[1] = -1
    _refused(lib, fn(*args), b"negative")
    # aliased outputs: in place on the scale, on the opacity, onto the filter, a partial overlap, the outputs onto each other
    for out_s, out_o in ((good[2], good[6]), (good[5], good[3]), (good[5], good[4]), (C.c_void_p(good[2].value + 12 * 9), good[6]),
                         (good[5], C.c_void_p(good[5].value + 12 * 9)), (good[5], good[5])):
        _refused(lib, fn(ctx, 10, good[2], good[3], good[4], out_s, out_o), b"alias")
    _refused(lib, fn(ctx, 0, good[2], good[3], good[4], good[2], good[6]), b"alias")  # ... at any count


def test_backward_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_filter3d_backward
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    good = [ctx, 10, _addr(0), _addr(1), _addr(2), _addr(3), _addr(4), _addr(5), _addr(6)]
    for k in (0, 2, 3, 4, 7, 8):
        args = list(good)
        args[k] = null
        _refused(lib, fn(*args), b"NULL")
    args = list(good)
    args[1] = -1
    _refused(lib, fn(*args), b"negative")
    for k in (5, 6):  # exactly one of d_rows / d_count
        args = list(good)
        args[k] = null
        _refused(lib, fn(*args), b"d_rows and d_count")
