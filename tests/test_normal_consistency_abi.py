"""The normal-consistency loss without a GPU: the entry point is exported, listed and declared with the header's signature,
refuses bad arguments before anything touches a device, and the header says what the contract is (with tests/test_abi.py this
pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAME = "lcgs_normal_consistency_loss_backward"
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def _header():
    return open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()


def test_symbol_is_exported_listed_and_declared(lcgs):
    lib, header = lcgs.load_library(), _header()
    assert hasattr(lib, NAME)
    assert NAME in lcgs.api.EXPORTED_SYMBOLS
    assert re.search(r"LCGS_API\s+lcgs_status\s+" + NAME + r"\s*\(", header)
    assert callable(lcgs.Renderer.normal_consistency_loss_backward)
    assert callable(lcgs.normal_consistency_autograd) and lcgs.normal_consistency_autograd is lcgs.api.normal_consistency_autograd
    mirror = open(os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc", "lcgs", "lcgs.hpp")).read()
    assert "check(" + NAME + "(m_ctx, &cam," in mirror  # the C++ mirror's method


def test_binding_declares_the_headers_signature(lcgs):
    """parameter by parameter: the header's C types against the ctypes the binding's one table gives the symbol"""
    lib, api = lcgs.load_library(), lcgs.api
    ctype = {"lcgs_context*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "float": C.c_float,
             "const lcgs_camera*": C.POINTER(api.Camera)}
    params = re.search(r"LCGS_API\s+lcgs_status\s+" + NAME + r"\s*\(([^)]*)\)", _header()).group(1)
    types = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(",")]
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in params.split(",")]
    assert names == ["ctx", "camera", "d_depth", "d_alpha", "d_normal", "weight", "alpha_min", "d_dL_ddepth", "d_dL_dalpha",
                     "d_dL_dnormal", "d_loss"]
    restype, argtypes = api.SIGNATURES[NAME]
    assert restype is C.c_int and getattr(lib, NAME).restype is restype
    assert [ctype[t] for t in types] == list(argtypes), (types, argtypes)
    assert list(getattr(lib, NAME).argtypes) == list(argtypes)


def _cam(lcgs, W, H):
    cam = lcgs.api.Camera()
    cam.fov, cam.aspect_ratio, cam.width, cam.height = 50.0, W / H, W, H
    return cam


def test_bad_arguments_are_refused_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = getattr(lib, NAME)
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)  # a non-NULL context that is never dereferenced
    # 8 x 8: planes of 256 bytes, the normal map and its gradient 768; none of these is ever dereferenced
    d, a, n, gd, ga, gn, loss = (C.c_void_p(x) for x in (0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000))
    cam = C.byref(_cam(lcgs, 8, 8))

    def refused(word, *args):
        assert fn(*args) == INVALID_ARG, args
        assert word in lib.lcgs_last_error(), (word, lib.lcgs_last_error())

    refused(b"NULL", null, cam, d, a, n, 0.05, 1e-3, gd, ga, gn, loss)
    refused(b"NULL", ctx, None, d, a, n, 0.05, 1e-3, gd, ga, gn, loss)  # no camera
    for k in range(3):  # a NULL input
        ins = [d, a, n]
        ins[k] = null
        refused(b"NULL", ctx, cam, *ins, 0.05, 1e-3, gd, ga, gn, loss)
    refused(b"NULL", ctx, cam, d, a, n, 0.05, 1e-3, gd, ga, gn, null)  # no loss
    refused(b"NULL", ctx, cam, d, a, n, 0.05, 1e-3, null, null, null, null)  # ... in an evaluation-only call either
    for W, H in ((2, 8), (8, 2), (0, 8), (8, -1)):  # no interior pixel
        refused(b"at least 3", ctx, C.byref(_cam(lcgs, W, H)), d, a, n, 0.05, 1e-3, gd, ga, gn, loss)
    for weight in (-0.1, float("nan"), float("inf"), -float("inf")):
        refused(b"weight", ctx, cam, d, a, n, weight, 1e-3, gd, ga, gn, loss)
    for alpha_min in (0.0, -1e-3, float("nan"), float("inf")):
        refused(b"alpha_min", ctx, cam, d, a, n, 0.05, alpha_min, gd, ga, gn, loss)
    for k in range(3):  # some but not all of the gradients
        one = [null, null, null]
        one[k] = (gd, ga, gn)[k]
        refused(b"all NULL or all non-NULL", ctx, cam, d, a, n, 0.05, 1e-3, *one, loss)
        two = [gd, ga, gn]
        two[k] = null
        refused(b"all NULL or all non-NULL", ctx, cam, d, a, n, 0.05, 1e-3, *two, loss)
    # a gradient over an input: the same address, the last float of the input, the input starting inside the gradient
    for k, size in enumerate((256, 256, 768)):
        base = (0x100000, 0x200000, 0x300000)[k]
        for addr in (base, base + size - 4, base - 252):
            for g in range(3):
                outs = [gd, ga, gn]
                outs[g] = C.c_void_p(addr)
                refused(b"alias an input", ctx, cam, d, a, n, 0.05, 1e-3, *outs, loss)
    # ... the byte behind an input is free; this call passes every check and fails on the context it then dereferences -- so it
    # is not made.  Two gradients over each other:
    refused(b"alias each other", ctx, cam, d, a, n, 0.05, 1e-3, gd, gd, gn, loss)
    refused(b"alias each other", ctx, cam, d, a, n, 0.05, 1e-3, gd, ga, C.c_void_p(0x400000 + 252), loss)
    refused(b"alias each other", ctx, cam, d, a, n, 0.05, 1e-3, gd, C.c_void_p(0x600000 + 764), gn, loss)


def test_header_states_the_definition_the_contract_and_what_is_not_offered():
    header = " ".join(re.sub(r"\n \*", "\n", _header()).split())  # (a comment's lines joined, their leading " *" dropped)
    for phrase in (
            "z_q = depth_q / max(alpha_q, alpha_min)", "m = ey x ex", "a fronto-parallel plane gives (0, 0, -1)",
            "s = sqrt(m.m + 1e-20)", "term_p = alpha_p - normal_p . nt", "loss = weight / ((W-2)(H-2)) * sum_p term_p",
            "binary64 sum in a fixed order; same inputs -> same bits", "All per-pixel algebra is binary64, uncontracted",
            "each output rounded to binary32 once", "the pose plays no part",
            "dL/dnormal_p = -c nt", "g_m = -c (normal_p / s - m (m . normal_p) / s^3)", "g_ey = ex x g_m", "g_ex = g_m x ey",
            "G_q = g_ex(q - x^) - g_ex(q + x^) + g_ey(q - y^) - g_ey(q + y^)", "dL/ddepth_q = g_z / max(alpha_q, alpha_min)",
            "(alpha_q >= alpha_min ? -g_z depth_q / alpha_q^2 : 0)", "nothing is detached",
            "The clamp passes its gradient at equality", "either all non-NULL or all NULL",
            "its bits equal the gradient call's loss", "overwritten, never accumulated", "zeros at the border included",
            "needs no kept frame", "reads nothing back", "width or height below 3",
            "a gradient buffer that overlaps any input or another gradient buffer",
            # not offered
            "the term inside lcgs_fit_views", "LCGS_DEPTH_INV_Z input", "world-space normals", "a median-depth surface",
            "a camera gradient",
            # the normals comment points here
            "lcgs_normal_consistency_loss_backward, below"):
        assert phrase in header, phrase
