"""The depth-prior loss without a GPU: the entry point is exported, listed and declared with the header's signature, refuses bad
arguments before anything touches a device, and the header says what the contract is (with tests/test_abi.py this pins
header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAME = "lcgs_depth_prior_loss_backward"
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def _header():
    return open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()


def test_symbol_is_exported_listed_and_declared(lcgs):
    lib, header = lcgs.load_library(), _header()
    assert hasattr(lib, NAME)
    assert NAME in lcgs.api.EXPORTED_SYMBOLS
    assert re.search(r"LCGS_API\s+lcgs_status\s+" + NAME + r"\s*\(", header)
    assert callable(lcgs.Renderer.depth_prior_loss_backward)
    assert callable(lcgs.depth_prior_autograd) and lcgs.depth_prior_autograd is lcgs.api.depth_prior_autograd
    mirror = open(os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc", "lcgs", "lcgs.hpp")).read()
    assert "check(" + NAME + "(m_ctx, width, height," in mirror  # the C++ mirror's method
    makefile = open(os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc", "Makefile")).read()
    assert "kernels/depth_prior.hip" in makefile and "abi_depth_prior.cpp" in makefile
    for define, value in (("LCGS_DEPTH_PRIOR_PEARSON", 0), ("LCGS_DEPTH_PRIOR_L1", 1), ("LCGS_DEPTH_ALIGN_FIT", 0),
                          ("LCGS_DEPTH_ALIGN_GIVEN", 1)):
        assert re.search(r"#define\s+" + define + r"\s+" + str(value) + r"\b", header), define


def test_binding_declares_the_headers_signature(lcgs):
    """parameter by parameter: the header's C types against the ctypes the binding's one table gives the symbol; the config
    struct member by member"""
    lib, api = lcgs.load_library(), lcgs.api
    ctype = {"lcgs_context*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "const uint8_t*": C.c_void_p,
             "int": C.c_int, "const lcgs_depth_prior_config*": C.POINTER(api._DepthPriorConfig)}
    params = re.search(r"LCGS_API\s+lcgs_status\s+" + NAME + r"\s*\(([^)]*)\)", _header()).group(1)
    types = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(",")]
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in params.split(",")]
    assert names == ["ctx", "width", "height", "d_depth", "d_alpha", "d_prior", "d_mask", "cfg", "d_dL_ddepth", "d_dL_dalpha",
                     "d_loss", "d_stats"]
    restype, argtypes = api.SIGNATURES[NAME]
    assert restype is C.c_int and getattr(lib, NAME).restype is restype
    assert [ctype[t] for t in types] == list(argtypes), (types, argtypes)
    assert list(getattr(lib, NAME).argtypes) == list(argtypes)
    assert api.STRUCTS["lcgs_depth_prior_config"] is api._DepthPriorConfig
    assert api._DepthPriorConfig._fields_ == [("kind", C.c_int), ("align", C.c_int), ("scale", C.c_float), ("shift", C.c_float),
                                              ("weight", C.c_float), ("alpha_min", C.c_float), ("patch", C.c_int),
                                              ("patch_x", C.c_int), ("patch_y", C.c_int)]
    assert C.sizeof(api._DepthPriorConfig) == 36


PEARSON, L1, FIT, GIVEN = 0, 1, 0, 1


def test_bad_arguments_are_refused_before_any_device_work(lcgs):
    lib, api = lcgs.load_library(), lcgs.api
    fn = getattr(lib, NAME)
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)  # a non-NULL context that is never dereferenced
    # 8 x 8: planes of 256 bytes, a mask of 64; none of these is ever dereferenced
    base = dict(d=0x100000, a=0x200000, m=0x300000, k=0x400000, gd=0x500000, ga=0x600000, loss=0x700000, stats=0x800000)

    def config(kind=PEARSON, align=FIT, scale=1.0, shift=0.0, weight=1.0, alpha_min=1e-3, patch=0, px=0, py=0):
        return api._DepthPriorConfig(kind, align, scale, shift, weight, alpha_min, patch, px, py)

    def refused(word, cfg=None, ctx=ctx, W=8, H=8, no_cfg=False, **ptrs):
        p = {k: C.c_void_p(v) for k, v in dict(base, **ptrs).items()}
        c = None if no_cfg else C.byref(cfg or config())
        args = (ctx, W, H, p["d"], p["a"], p["m"], p["k"], c, p["gd"], p["ga"], p["loss"], p["stats"])
        assert fn(*args) == INVALID_ARG, (word, ptrs)
        assert word in lib.lcgs_last_error(), (word, lib.lcgs_last_error())

    refused(b"ctx is NULL", ctx=null)
    refused(b"cfg is NULL", no_cfg=True)
    for k in ("d", "a", "m", "loss"):  # a NULL input, no loss
        refused(b"NULL", **{k: 0})
    refused(b"NULL", gd=0, ga=0, loss=0)  # ... in an evaluation-only call either
    for W, H in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        refused(b"positive", W=W, H=H)
    for kind in (-1, 2, 7):
        refused(b"unknown kind", config(kind=kind))
    for align in (-1, 2):
        refused(b"unknown align", config(kind=L1, align=align))
    refused(b"L1 kind only", config(kind=PEARSON, align=GIVEN))
    for patch in (32, 64, 128):
        refused(b"takes no patch", config(kind=L1, align=GIVEN, patch=patch))
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(b"scale and shift", config(kind=L1, align=GIVEN, scale=bad))
        refused(b"scale and shift", config(kind=L1, align=GIVEN, shift=bad))
    for weight in (-0.1, float("nan"), float("inf"), -float("inf")):
        refused(b"weight", config(weight=weight))
    for alpha_min in (0.0, -1e-3, float("nan"), float("inf")):
        refused(b"alpha_min", config(alpha_min=alpha_min))
    for patch in (-32, 1, 16, 33, 96, 256):
        refused(b"patch must be", config(patch=patch))
    for patch, px, py in ((32, 32, 0), (32, 0, 32), (32, -1, 0), (64, 0, -1), (128, 128, 5), (64, 5, 64)):
        refused(b"[0, patch)", config(patch=patch, px=px, py=py))
    refused(b"both NULL or both non-NULL", gd=0)
    refused(b"both NULL or both non-NULL", ga=0)
    # an output over an input: the same address, the last byte of the input, the input starting inside the output
    for k, size in (("d", 256), ("a", 256), ("m", 256), ("k", 64)):
        for out, out_size in (("gd", 256), ("ga", 256), ("loss", 4), ("stats", 16)):
            for addr in (base[k], base[k] + size - 4, base[k] - out_size + 4):
                refused(b"alias an input", **{out: addr})
    # ... the byte behind an input is free; that call passes every check and fails on the context it then dereferences -- so it
    # is not made.  Two outputs over each other:
    refused(b"alias each other", ga=base["gd"])
    refused(b"alias each other", ga=base["gd"] + 252)
    refused(b"alias each other", loss=base["gd"] + 128)
    refused(b"alias each other", stats=base["ga"] + 252)
    refused(b"alias each other", stats=base["loss"])
    refused(b"alias each other", stats=base["loss"] - 12)
    # without a mask or stats their addresses are not looked at (0 bytes at NULL overlap nothing): the checks go on to the next
    refused(b"weight", config(weight=-1.0), k=0, stats=0)


def test_python_method_refuses_mismatched_buffers_before_the_context_is_touched(lcgs):
    """the C ABI sees pointers only: a buffer of another shape, dtype or layout would be an out-of-bounds device access"""
    import pytest
    import torch

    r = lcgs.Renderer.__new__(lcgs.Renderer)  # no context: anything that reached the library would raise AttributeError
    H, W = 5, 7
    ok = dict(depth=torch.zeros(H, W), alpha=torch.zeros(H, W), prior=torch.zeros(H, W), dL_ddepth=torch.zeros(H, W),
              dL_dalpha=torch.zeros(H, W), loss=torch.zeros(1))
    bad = dict(alpha=torch.zeros(H, W + 1), prior=torch.zeros(H, W, dtype=torch.float64), dL_ddepth=torch.zeros(W, H),
               dL_dalpha=torch.zeros(H, 2 * W)[:, ::2], mask=torch.zeros(H, W, dtype=torch.int32),
               loss=torch.zeros(1, dtype=torch.float64), stats=torch.zeros(3))
    with pytest.raises(ValueError, match="loss"):
        r.depth_prior_loss_backward(**dict(ok, loss=None))
    for stats in (torch.zeros(4, dtype=torch.float64), torch.zeros(8)[::2], torch.zeros(5)):
        with pytest.raises(ValueError, match="stats"):
            r.depth_prior_loss_backward(**ok, stats=stats)
    for name, t in bad.items():
        with pytest.raises(ValueError, match=name):
            r.depth_prior_loss_backward(**dict(ok, **{name: t}))
    for kw in (dict(kind="l2"), dict(align="median")):
        with pytest.raises(ValueError, match="kind must be one of"):
            r.depth_prior_loss_backward(**ok, **kw)
    with pytest.raises(AttributeError):  # ... and good buffers (a bool mask among them) go on to the context
        r.depth_prior_loss_backward(**ok, mask=torch.zeros(H, W, dtype=torch.bool))


def test_header_states_the_definition_the_contract_and_what_is_not_offered():
    header = " ".join(re.sub(r"\n \*", "\n", _header()).split())  # (a comment's lines joined, their leading " *" dropped)
    for phrase in (
            "v_p = depth_p / max(alpha_p, alpha_min)", "(d_mask == NULL or mask_p != 0) and isfinite(prior_p)",
            "anchored at pixel (-patch_x, -patch_y), cut at the image border", "a group that holds at least 2 valid pixels",
            "1 valid pixel suffices", "G = the number of counted groups", "N_c = the number of valid pixels in counted groups",
            "the means first, then centred sums (two passes, not raw moments)", "eps = 1e-12",
            "mu_v = sum v / n", "var_v = sum (v - mu_v)^2 / n", "cov = sum (v - mu_v)(m - mu_m) / n",
            "r = cov / sqrt((var_v + eps)(var_m + eps))", "s = cov / (var_m + eps)", "t = mu_v - s mu_m",
            "a constant prior gives m - mu_m = 0 exactly", "loss = weight / G * sum_g (1 - r_g)", "(0 if G == 0)",
            "g_v(p) = -weight / (G n) * [ (m_p - mu_m) - cov (v_p - mu_v) / (var_v + eps) ] / sqrt((var_v + eps)(var_m + eps))",
            "res_p = v_p - (s_g m_p + t_g)", "loss = weight / N_c * sum |res_p|", "g_v(p) = weight / N_c * sign(res_p), sign(0) = 0",
            "they are detached", "computes no statistics", "every other pixel gets an exact zero",
            "dL/ddepth_p = g_v / max(alpha_p, alpha_min)", "(alpha_p >= alpha_min ? -g_v depth_p / alpha_p^2 : 0)",
            "binary64, uncontracted, the inputs widened exactly", "rounded to binary32 once", "no float atomics",
            "same inputs -> same bits, across calls and contexts", "both non-NULL or both NULL",
            "its bits equal the gradient call's loss", "overwritten, never accumulated", "{ N_c, G, s, t }",
            "zeros for s and t in patch mode", "needs no kept frame", "reads nothing back",
            "LCGS_DEPTH_ALIGN_GIVEN with the Pearson kind or with patch != 0", "a patch that is not 0, 32, 64 or 128",
            "an offset outside [0, patch)", "exactly one gradient pointer NULL",
            "that overlaps any input or another output",
            # not offered
            "FSGS's min over two depth transforms", "random or overlapping patches", "a non-detached alignment",
            "the term inside lcgs_fit_views", "an lcgs-app flag for it", "a camera gradient"):
        assert phrase in header, phrase
