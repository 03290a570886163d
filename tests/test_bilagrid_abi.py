"""The bilateral grid's three entry points without a GPU: exported, listed and declared with the header's signatures, refusing bad
arguments before anything touches a device, and the header says what the contract is (with tests/test_abi.py this pins
header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

SLICE, BACKWARD, TV = "lcgs_bilagrid_slice", "lcgs_bilagrid_backward", "lcgs_bilagrid_tv_loss_backward"
PARAMS = {
    SLICE: ["ctx", "width", "height", "d_grid", "gw", "gh", "gl", "d_img_chw", "d_out_chw"],
    BACKWARD: ["ctx", "width", "height", "d_grid", "gw", "gh", "gl", "d_img_chw", "d_dL_dout_chw", "d_dL_dimg_chw", "d_dL_dgrid"],
    TV: ["ctx", "d_grids", "num_grids", "gw", "gh", "gl", "weight", "d_dL_dgrids", "d_loss"],
}
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def _header():
    return open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib, header = lcgs.load_library(), _header()
    mirror = open(os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc", "lcgs", "lcgs.hpp")).read()
    for name in PARAMS:
        assert hasattr(lib, name)
        assert name in lcgs.api.EXPORTED_SYMBOLS
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header)
        assert callable(getattr(lcgs.Renderer, name[len("lcgs_"):]))
        assert "check(" + name + "(m_ctx, " in mirror  # the C++ mirror's method
    for fn in ("bilagrid_identity", "bilagrid_autograd", "bilagrid_tv_autograd"):
        assert callable(getattr(lcgs, fn)) and getattr(lcgs, fn) is getattr(lcgs.api, fn)
    makefile = open(os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc", "Makefile")).read()
    assert "kernels/bilagrid.hip" in makefile and "abi_bilagrid.cpp" in makefile


@pytest.mark.parametrize("name", list(PARAMS))
def test_binding_declares_the_headers_signature(lcgs, name):
    """parameter by parameter: the header's C types against the ctypes the binding's one table gives the symbol"""
    lib, api = lcgs.load_library(), lcgs.api
    ctype = {"lcgs_context*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "float": C.c_float, "int": C.c_int}
    params = re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(([^)]*)\)", _header()).group(1)
    types = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(",")]
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in params.split(",")]
    assert names == PARAMS[name]
    restype, argtypes = api.SIGNATURES[name]
    assert restype is C.c_int and getattr(lib, name).restype is restype
    assert [ctype[t] for t in types] == list(argtypes), (types, argtypes)
    assert list(getattr(lib, name).argtypes) == list(argtypes)


# an 8 x 8 image is 768 bytes, a (2, 2, 2) grid 384; none of these addresses is ever dereferenced
NULL, CTX = C.c_void_p(0), C.c_void_p(0x1000)
GRID, IMG, OUT, GOUT, GIMG, GGRID, LOSS = (0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000)
IMG_BYTES, GRID_BYTES = 3 * 8 * 8 * 4, 12 * 2 * 2 * 2 * 4
BAD_DIMS = ((1, 2, 2), (2, 1, 2), (2, 2, 1), (0, 2, 2), (2, -3, 2), (257, 2, 2), (2, 257, 2), (2, 2, 17))
BAD_SIZES = ((0, 8), (8, 0), (-1, 8), (8, -8))


def _refuser(lib, name):
    fn = getattr(lib, name)

    def refused(word, *args):
        args = [C.c_void_p(a) if isinstance(a, int) and a >= 0x1000 else a for a in args]
        assert fn(*args) == INVALID_ARG, args
        assert word in lib.lcgs_last_error(), (word, lib.lcgs_last_error())

    return refused


def test_slice_refuses_bad_arguments_before_any_device_work(lcgs):
    refused = _refuser(lcgs.load_library(), SLICE)
    refused(b"NULL", NULL, 8, 8, GRID, 2, 2, 2, IMG, OUT)
    for k in (3, 7, 8):  # a NULL grid, image, output
        args = [CTX, 8, 8, GRID, 2, 2, 2, IMG, OUT]
        args[k] = NULL
        refused(b"NULL", *args)
    for W, H in BAD_SIZES:
        refused(b"positive", CTX, W, H, GRID, 2, 2, 2, IMG, OUT)
    for gw, gh, gl in BAD_DIMS:
        refused(b"dimensions", CTX, 8, 8, GRID, gw, gh, gl, IMG, OUT)
    # in place, the last float of the image, the image starting inside the output; the same against the grid
    for addr in (IMG, IMG + IMG_BYTES - 4, IMG - IMG_BYTES + 4, GRID, GRID + GRID_BYTES - 4, GRID - IMG_BYTES + 4):
        refused(b"alias", CTX, 8, 8, GRID, 2, 2, 2, IMG, addr)
    refused(b"in-place slicing is not offered", CTX, 8, 8, GRID, 2, 2, 2, IMG, IMG)


def test_backward_refuses_bad_arguments_before_any_device_work(lcgs):
    refused = _refuser(lcgs.load_library(), BACKWARD)
    ok = [CTX, 8, 8, GRID, 2, 2, 2, IMG, GOUT, GIMG, GGRID]
    for k in (0, 3, 7, 8):  # a NULL context, grid, image, dL_dout
        args = list(ok)
        args[k] = NULL
        refused(b"NULL", *args)
    refused(b"both NULL", CTX, 8, 8, GRID, 2, 2, 2, IMG, GOUT, NULL, NULL)
    for W, H in BAD_SIZES:
        refused(b"positive", CTX, W, H, *ok[3:])
    for gw, gh, gl in BAD_DIMS:
        refused(b"dimensions", CTX, 8, 8, GRID, gw, gh, gl, *ok[7:])
    # either gradient over each input: the same address, the input's last float, the input starting inside the gradient
    for base, size in ((GRID, GRID_BYTES), (IMG, IMG_BYTES), (GOUT, IMG_BYTES)):
        for which, own in ((9, IMG_BYTES), (10, GRID_BYTES)):
            for addr in (base, base + size - 4, base - own + 4):
                for other in (ok[19 - which], NULL):  # with and without the other gradient
                    args = list(ok)
                    args[which], args[19 - which] = addr, other
                    refused(b"alias an input", *args)
    # the two gradients over each other
    refused(b"alias each other", *ok[:9], GIMG, GIMG)
    refused(b"alias each other", *ok[:9], GIMG, GIMG + IMG_BYTES - 4)
    refused(b"alias each other", *ok[:9], GGRID + GRID_BYTES - 4, GGRID)


def test_tv_refuses_bad_arguments_before_any_device_work(lcgs):
    refused = _refuser(lcgs.load_library(), TV)
    ok = [CTX, GRID, 3, 2, 2, 2, 10.0, GGRID, LOSS]
    for k in (0, 1, 8):  # a NULL context, grids, loss
        args = list(ok)
        args[k] = NULL
        refused(b"NULL", *args)
    refused(b"NULL", CTX, GRID, 3, 2, 2, 2, 10.0, NULL, NULL)  # ... in an evaluation-only call either
    for n in (0, -1):
        refused(b"num_grids", CTX, GRID, n, 2, 2, 2, 10.0, GGRID, LOSS)
    for gw, gh, gl in BAD_DIMS:
        refused(b"dimensions", CTX, GRID, 3, gw, gh, gl, 10.0, GGRID, LOSS)
    for weight in (-0.1, float("nan"), float("inf"), -float("inf")):
        refused(b"weight", CTX, GRID, 3, 2, 2, 2, weight, GGRID, LOSS)
    for addr in (GRID, GRID + 3 * GRID_BYTES - 4, GRID - 3 * GRID_BYTES + 4):  # three grids: 1152 bytes
        refused(b"alias", CTX, GRID, 3, 2, 2, 2, 10.0, addr, LOSS)
    refused(b"alias", CTX, GRID, 3, 2, 2, 2, 10.0, GGRID, GRID + 8)         # the loss inside the grids
    refused(b"alias", CTX, GRID, 3, 2, 2, 2, 10.0, GGRID, GGRID + 3 * GRID_BYTES - 4)  # ... inside the gradient
    refused(b"alias", CTX, GRID, 3, 2, 2, 2, 10.0, NULL, GRID)              # ... in an evaluation-only call


def test_header_states_the_definition_the_contract_and_what_is_not_offered():
    header = " ".join(re.sub(r"\n \*", "\n", _header()).split())  # (a comment's lines joined, their leading " *" dropped)
    for phrase in (
            "float32 [12][L][GH][GW], contiguous", "Channel c = 4 r + k is entry (row r, column k) of the 3 x 4 matrix",
            "column 3 is the offset", "[N][12][L][GH][GW]", "2 <= gw, gh <= 256 and 2 <= gl <= 16",
            "x = ((float)px + 0.5f) / W * (GW-1)", "x0 = min(floor(x), GW-2)", "fx = x - x0", "x and y never reach the border",
            "gray = 0.299f*r + 0.587f*g + 0.114f*b", "the three products summed in that order", "uncontracted",
            "zr = gray*(L-1)", "z = clamp(zr, 0, L-1)", "z0 = min((int)z, L-2)", "fz = z - z0",
            "nested lerps a + t*(b - a): along x, then y, then z", "out_r = A[4r]*r + A[4r+1]*g + A[4r+2]*b + A[4r+3]",
            "an identity grid returns a finite image bit for bit", "the sign of a zero aside",
            "num_grids is too large for one call",
            'mode="bilinear", padding_mode="border", align_corners=True', "coords = 2 (x/(GW-1), y/(GH-1), gray) - 1",
            "hat(t) = max(0, 1 - |t|)", "dL/dgrid[c=4r+k][l][j][i] = sum over pixels of hat(x-i) hat(y-j) hat(z-l) g_r (k<3 ? c_k : 1)",
            "dL/dc_k = sum_r A[4r+k] g_r + w_k (L-1) inside sum_r g_r (dA[4r..4r+3]/dz . (r,g,b,1))",
            "dA/dz = the xy-bilinear sample at level z0+1 minus the one at z0", "w = (0.299f, 0.587f, 0.114f)",
            "inside = (zr > 0 && zr < L-1)", "black background pixels pass none", "the cell is the one above (floor)",
            "no float atomics", "written as exact zeros", "more vertices than pixels is a legal call",
            "NULL: not wanted", "not both NULL",
            "loss = weight/N * sum over axis in {x,y,z} of sum (grid[v+e_axis] - grid[v])^2 / count_axis",
            "for x, 12 L GH (GW-1)", "The per-element algebra is binary64", "the sum is binary64 in a fixed order",
            "rounded to binary32 once", "evaluation only", "weight = 0 gives exact zeros",
            "All outputs are overwritten, never accumulated", "The same inputs give the same bits, across calls and across contexts",
            "needs a kept frame or reads anything back", "in-place slicing is not offered",
            # not offered
            "the grid inside lcgs_fit_views or lcgs-app", "a library optimiser for grids", "interpolation between views' grids",
            "slicing fused into the photometric loss", "guidance other than the input's luminance"):
        assert phrase in header, phrase


def test_python_methods_refuse_mismatched_buffers_before_the_call(lcgs):
    """the C ABI sees pointers only: shape, dtype and device of every buffer are checked in Python (never reaches the context)"""
    import types

    import torch

    me = types.SimpleNamespace(_bilagrid_buffers=lcgs.Renderer._bilagrid_buffers, ctx=None)
    grid, img = torch.zeros(12, 2, 3, 4), torch.zeros(3, 5, 7)
    for out in (torch.zeros(3, 5, 6), torch.zeros(3, 5, 7, dtype=torch.float64), torch.zeros(3, 7, 5)):
        with pytest.raises(ValueError, match="out"):
            lcgs.Renderer.bilagrid_slice(me, grid, img, out)
    with pytest.raises(ValueError, match="grid"):
        lcgs.Renderer.bilagrid_slice(me, torch.zeros(11, 2, 3, 4), img, torch.zeros(3, 5, 7))
    good = torch.zeros(3, 5, 7)
    for kw, name in (({"dL_dimg": torch.zeros(3, 5, 8)}, "dL_dimg"), ({"dL_dgrid": torch.zeros(12, 2, 3, 5)}, "dL_dgrid"),
                     ({"dL_dgrid": torch.zeros(12, 2, 3, 4, dtype=torch.float16)}, "dL_dgrid")):
        with pytest.raises(ValueError, match=name):
            lcgs.Renderer.bilagrid_backward(me, grid, img, good, **kw)
    with pytest.raises(ValueError, match="dL_dout"):
        lcgs.Renderer.bilagrid_backward(me, grid, img, torch.zeros(3, 5), dL_dimg=good)
    grids = torch.zeros(2, 12, 2, 3, 4)
    with pytest.raises(ValueError, match="dL_dgrids"):
        lcgs.Renderer.bilagrid_tv_loss_backward(me, grids, torch.zeros(1, 12, 2, 3, 4), torch.zeros(1))
    with pytest.raises(ValueError, match="loss"):
        lcgs.Renderer.bilagrid_tv_loss_backward(me, grids, None, torch.zeros(2))
