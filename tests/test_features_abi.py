"""The feature channels without a GPU: both entry points are exported, listed and declared with the header's signatures, refuse
bad arguments before anything touches a device, and the header says what the contract is (with tests/test_abi.py this pins
header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ("lcgs_render_features", "lcgs_render_backward_features")
INVALID_ARG = 1  # LCGS_ERR_INVALID_ARG


def _header():
    return open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib, header = lcgs.load_library(), _header()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header), name
    for method in ("render_features", "backward_features"):
        assert callable(getattr(lcgs.Renderer, method))
    assert callable(lcgs.render_autograd_features)
    api = lcgs.api
    assert api.STRUCTS["lcgs_feature_channel"] is api._FeatureChannel
    assert api._FeatureChannel._fields_ == [("channels", C.c_int), ("d_features", C.c_void_p), ("d_dL_dfeature_map", C.c_void_p),
                                            ("d_dL_dfeatures", C.c_void_p)]
    assert C.sizeof(api._FeatureChannel) == 32
    assert re.search(r"#define\s+LCGS_FEATURES_MAX\s+256\s*$", header, re.M)


def test_header_states_the_definition_the_contract_and_what_is_not_offered():
    header = " ".join(re.sub(r"\n \*", "\n", _header()).split())  # (a comment's lines joined, their leading " *" dropped)
    for phrase in (
            # the map
            "P x K floats, row-major", "the context's row order", "sum_i fl(w_i f_i,c)", "K*H*W floats, CHW",
            "the multiply and the add separate operations", "an f32 MFMA is an fmaf chain",
            "The map is NOT normalised (divide by alpha), NO background is blended in and it is NOT clamped",
            "is 0 in all K channels", "works on antialiased and LOD frames unchanged", "num_gaussians must be the bound scene's P",
            # the backward
            "dL/df_i,c = sum_p w_i dL/dfeature_map[c][p] goes to d_dL_dfeatures", "Nothing reaches sh",
            "nothing reaches pos, scale or rotq from the feature's own value", "summed by float atomics in unspecified order",
            "With feat NULL the call is lcgs_render_backward_normals", "the features are frozen", "the frozen-geometry mode",
            "the frame's 2-D gradient rows are left as they were", "Both NULL is an argument error",
            "`accumulate` holds for the rows of `grads` and for d_dL_dfeatures alike", "exact zeros in both",
            "a caller-supplied feature has no direct camera term", "the refusal behind a non-NULL d_dL_dnormal stays",
            "LCGS_ERR_STATE without a keep_state frame, or after a frame of lcgs_owner_render",
            # not offered
            "Not offered: compact rows", "lcgs_render_backward_camera, lcgs_fit_views or the ownership step", "an lcgs-app flag",
            "f16 features"):
        assert phrase in header, phrase


def test_binding_declares_the_headers_signatures(lcgs):
    """parameter by parameter: the header's C types against the ctypes the binding's one table gives the two symbols"""
    lib, api, header = lcgs.load_library(), lcgs.api, _header()
    ctype = {"lcgs_context*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "int": C.c_int, "float": C.c_float,
             "const lcgs_grads*": C.POINTER(api._Grads), "const lcgs_feature_channel*": C.POINTER(api._FeatureChannel)}
    for name in NAMES:
        params = re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        params = re.sub(r"/\*.*?\*/", "", params)
        types = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in params.split(",")]
        restype, argtypes = api.SIGNATURES[name]
        assert getattr(lib, name).restype is restype
        assert [ctype[t] for t in types] == list(argtypes), (name, types, argtypes)
        assert list(getattr(lib, name).argtypes) == list(argtypes), name
    assert len(api.SIGNATURES["lcgs_render_features"][1]) == 5
    assert len(api.SIGNATURES["lcgs_render_backward_features"][1]) == 11
    assert api.SIGNATURES["lcgs_render_backward_features"][1][8] is C.POINTER(api._FeatureChannel)


def test_render_features_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_render_features
    null, ctx, rows, out = C.c_void_p(0), C.c_void_p(0x1000), C.c_void_p(0x100000), C.c_void_p(0x200000)  # never dereferenced
    for args in ((null, 10, 3, rows, out), (ctx, 10, 3, null, out), (ctx, 10, 3, rows, null)):
        assert fn(*args) == INVALID_ARG
        assert b"NULL" in lib.lcgs_last_error()
    for K in (0, -1, 257, 1 << 20):
        assert fn(ctx, 10, K, rows, out) == INVALID_ARG, K
        assert b"channels" in lib.lcgs_last_error()


def test_render_backward_features_refuses_bad_arguments_before_any_device_work(lcgs):
    lib, api = lcgs.load_library(), lcgs.api
    fn = lib.lcgs_render_backward_features
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)
    dimg, dd, da, dq, dn = (C.c_void_p(a) for a in (0x100000, 0x200000, 0x300000, 0x380000, 0x3c0000))
    g = api._Grads(*[C.c_void_p(0x400000 + 0x100000 * k) for k in range(5)])

    def feat(K=5, rows=0xa00000, gmap=0xb00000, grows=0xc00000):
        return api._FeatureChannel(K, C.c_void_p(rows), C.c_void_p(gmap), C.c_void_p(grows))

    def refused(word, *args):
        assert fn(*args) == INVALID_ARG, (word, args)
        assert word in lib.lcgs_last_error(), (word, lib.lcgs_last_error())

    ft = feat()
    refused(b"NULL", null, dimg, 0, 0.0, dd, da, dq, dn, C.byref(ft), 0, C.byref(g))
    refused(b"NULL", ctx, dimg, 0, 0.0, dd, da, dq, dn, None, 0, None)  # neither a feature channel nor gradient arrays
    for mode in (-1, 2):
        refused(b"mode", ctx, dimg, mode, 0.0, dd, da, dq, dn, C.byref(ft), 0, C.byref(g))
    for center in (float("nan"), float("inf")):
        refused(b"center", ctx, dimg, 0, center, dd, da, dq, dn, C.byref(ft), 0, C.byref(g))
    # feat NULL: lcgs_render_backward_normals' rule -- any of the five may be NULL, not all
    refused(b"all five", ctx, null, 1, 2.5, null, null, null, null, None, 0, C.byref(g))
    for K in (0, -3, 257):
        bad = feat(K=K)
        refused(b"channels", ctx, null, 0, 0.0, null, null, null, null, C.byref(bad), 0, C.byref(g))
    for kw in (dict(rows=0), dict(gmap=0)):  # the rows and the map's gradient are what the channel is
        bad = feat(**kw)
        refused(b"NULL", ctx, null, 0, 0.0, null, null, null, null, C.byref(bad), 0, C.byref(g))
    frozen = feat(grows=0)
    refused(b"both NULL", ctx, null, 0, 0.0, null, null, null, null, C.byref(frozen), 0, None)  # nothing to write
    # the frozen-geometry mode takes no other incoming gradient
    for k in range(5):
        others = [null] * 5
        others[k] = C.c_void_p(0x100000)
        refused(b"frozen geometry", ctx, others[0], 0, 0.0, others[1], others[2], others[3], others[4], C.byref(ft), 0, None)
    for k in range(5):  # a NULL gradient buffer
        ptrs = [C.c_void_p(0x400000 + 0x100000 * j) for j in range(5)]
        ptrs[k] = null
        refused(b"NULL gradient buffer", ctx, null, 0, 0.0, null, null, null, null, C.byref(ft), 1, C.byref(api._Grads(*ptrs)))
