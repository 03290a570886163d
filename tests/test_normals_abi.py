"""The normal map without a GPU: both entry points are exported, listed and declared with the header's signatures, refuse bad
arguments before anything touches a device, and the header says what the contract is (with tests/test_abi.py this pins
header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lcgs_render_normals", "lcgs_render_backward_normals")
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def _header():
    return open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib, header = lcgs.load_library(), _header()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header), name
    for method in ("render_normals", "backward_normals"):
        assert callable(getattr(lcgs.Renderer, method))
    assert callable(lcgs.render_autograd_normals)


def test_header_states_the_definition_the_contract_and_what_is_not_offered():
    header = " ".join(re.sub(r"\n \*", "\n", _header()).split())  # (a comment's lines joined, their leading " *" dropped)
    for phrase in (
            # the per-splat normal
            "k = 0; if (s[1] < s[k]) k = 1; if (s[2] < s[k]) k = 2;", "ties to the lower index", "NOT renormalised",
            "t = (c0 d0 + c1 d1) + c2 d2", "if (t > 0) c = -c", "t == 0 and NaN leave c as it is",
            "n = (right . c, up . c, front . c)", "(a0 b0 + a1 b1) + a2 b2", "scale_modifier plays no part",
            # the map and its backward
            "3*H*W floats, CHW", "sum_i fl(w_i n_i,c)", "the axis k and the flip are constants",
            "nothing goes to scale or pos from the normal's own value", "re-read the BOUND arrays",
            "needs no preceding lcgs_render_normals", "Any of the five incoming gradients may be NULL, not all five",
            "With d_dL_dnormal NULL the call is lcgs_render_backward_distortion",
            "lcgs_camera_backward behind a call that passed a non-NULL d_dL_dnormal returns LCGS_ERR_STATE",
            "behind any later backward of the frame it works as before", "sees the combined 2-D gradient",
            "LCGS_ERR_STATE without a keep_state frame, or after a frame of lcgs_owner_render",
            # not offered
            "world-space output", "lcgs_render_backward_camera, lcgs_render_backward_compact, lcgs_fit_views or the ownership step",
            "a fused normal-consistency loss", "an lcgs-app flag"):
        assert phrase in header, phrase


def test_binding_declares_the_headers_signatures(lcgs):
    """parameter by parameter: the header's C types against the ctypes the binding's one table gives the two symbols"""
    lib, api, header = lcgs.load_library(), lcgs.api, _header()
    grads = C.POINTER(api._Grads)
    ctype = {"lcgs_context*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "int": C.c_int, "float": C.c_float,
             "const lcgs_grads*": grads}
    for name in NAMES:
        params = re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        params = re.sub(r"/\*.*?\*/", "", params)
        types = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(",")]
        restype, argtypes = api.SIGNATURES[name]
        assert getattr(lib, name).restype is restype
        assert [ctype[t] for t in types] == list(argtypes), (name, types, argtypes)
        assert list(getattr(lib, name).argtypes) == list(argtypes), name
    assert len(api.SIGNATURES["lcgs_render_normals"][1]) == 2
    assert len(api.SIGNATURES["lcgs_render_backward_normals"][1]) == 10


def test_render_normals_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_render_normals
    null, ctx, out = C.c_void_p(0), C.c_void_p(0x1000), C.c_void_p(0x100000)  # never dereferenced
    assert fn(null, out) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, null) == INVALID_ARG  # the output
    assert b"NULL" in lib.lcgs_last_error()


def test_render_backward_normals_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_render_backward_normals
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    dimg, dd, da, dq, dn = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x380000, 0x3c0000))
    g = lcgs.api._Grads(*[C.c_void_p(0x400000 + 0x100000 * k) for k in range(5)])
    assert fn(null, dimg, 0, 0.0, dd, da, dq, dn, 0, C.byref(g)) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, dimg, 0, 0.0, dd, da, dq, dn, 0, None) == INVALID_ARG  # no gradient struct
    for mode in (-1, 2):
        assert fn(ctx, dimg, mode, 0.0, dd, da, dq, dn, 0, C.byref(g)) == INVALID_ARG, mode
        assert b"mode" in lib.lcgs_last_error()
    for center in (float("nan"), float("inf")):
        assert fn(ctx, dimg, 0, center, dd, da, dq, dn, 0, C.byref(g)) == INVALID_ARG, center
        assert b"center" in lib.lcgs_last_error()
    assert fn(ctx, null, 1, 2.5, null, null, null, null, 0, C.byref(g)) == INVALID_ARG  # any of the five may be NULL, not all
    assert b"all five" in lib.lcgs_last_error()
    for k in range(5):  # a NULL gradient buffer
        ptrs = [C.c_void_p(0x400000 + 0x100000 * j) for j in range(5)]
        ptrs[k] = null
        assert fn(ctx, null, 0, 0.0, null, null, null, dn, 1, C.byref(lcgs.api._Grads(*ptrs))) == INVALID_ARG, k
        assert b"NULL gradient buffer" in lib.lcgs_last_error()
