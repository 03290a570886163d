"""The depth-distortion map without a GPU: both entry points are exported, listed and declared with the header's signatures, and
refuse bad arguments before anything touches a device (with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <->
liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lcgs_render_distortion", "lcgs_render_backward_distortion")
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def _header():
    return open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib, header = lcgs.load_library(), _header()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header), name
    for method in ("render_distortion", "backward_distortion"):
        assert callable(getattr(lcgs.Renderer, method))
    assert callable(lcgs.render_autograd_distortion)
    # what the map is not, and what is not offered, is said where the contract is
    for phrase in ("NOT normalised", "NO background", "NOT clamped", "typical depth", "lcgs_render_backward_camera, in lcgs_fit_views",
                   "lcgs-app flag"):
        assert phrase in header, phrase


def test_binding_declares_the_headers_signatures(lcgs):
    """parameter by parameter: the header's C types against the ctypes the binding's one table gives the two symbols"""
    lib, api, header = lcgs.load_library(), lcgs.api, _header()
    grads = C.POINTER(api._Grads)
    ctype = {"lcgs_context*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "int": C.c_int, "float": C.c_float,
             "const lcgs_grads*": grads}
    for name in NAMES:
        params = re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        types = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(",")]
        restype, argtypes = api.SIGNATURES[name]
        assert getattr(lib, name).restype is restype
        assert [ctype[t] for t in types] == list(argtypes), (name, types, argtypes)
        assert list(getattr(lib, name).argtypes) == list(argtypes), name
    assert len(api.SIGNATURES["lcgs_render_distortion"][1]) == 4
    assert len(api.SIGNATURES["lcgs_render_backward_distortion"][1]) == 9


def test_render_distortion_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_render_distortion
    null, ctx, out = C.c_void_p(0), C.c_void_p(0x1000), C.c_void_p(0x100000)  # never dereferenced
    assert fn(null, 0, 0.0, out) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, 0, 0.0, null) == INVALID_ARG  # the output
    assert b"NULL" in lib.lcgs_last_error()
    for mode in (-1, 2, 7):
        assert fn(ctx, mode, 0.0, out) == INVALID_ARG, mode
        assert b"mode" in lib.lcgs_last_error()
    for center in (float("nan"), float("inf"), float("-inf")):
        assert fn(ctx, 1, center, out) == INVALID_ARG, center
        assert b"center" in lib.lcgs_last_error()


def test_render_backward_distortion_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_render_backward_distortion
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    dimg, dd, da, dq = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x380000))
    g = lcgs.api._Grads(*[C.c_void_p(0x400000 + 0x100000 * k) for k in range(5)])
    assert fn(null, dimg, 0, 0.0, dd, da, dq, 0, C.byref(g)) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, dimg, 0, 0.0, dd, da, dq, 0, None) == INVALID_ARG  # no gradient struct
    for mode in (-1, 2):
        assert fn(ctx, dimg, mode, 0.0, dd, da, dq, 0, C.byref(g)) == INVALID_ARG, mode
        assert b"mode" in lib.lcgs_last_error()
    for center in (float("nan"), float("inf")):
        assert fn(ctx, dimg, 0, center, dd, da, dq, 0, C.byref(g)) == INVALID_ARG, center
        assert b"center" in lib.lcgs_last_error()
    assert fn(ctx, null, 1, 2.5, null, null, null, 0, C.byref(g)) == INVALID_ARG  # any of the four may be NULL, not all four
    assert b"all four" in lib.lcgs_last_error()
    for k in range(5):  # a NULL gradient buffer
        ptrs = [C.c_void_p(0x400000 + 0x100000 * j) for j in range(5)]
        ptrs[k] = null
        assert fn(ctx, null, 0, 0.0, null, null, dq, 1, C.byref(lcgs.api._Grads(*ptrs))) == INVALID_ARG, k
        assert b"NULL gradient buffer" in lib.lcgs_last_error()
