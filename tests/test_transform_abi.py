"""The scene similarity transform's four entry points without a GPU: exported, listed and declared as the header spells them; the
host-only plan and camera against tests/transform_ref.py; every bad argument refused before anything touches a device -- with a
NULL context, or a non-NULL one that is never dereferenced."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import transform_ref as T
from conftest import ROOT

NAMES = ("lcgs_similarity_plan_make", "lcgs_camera_transform", "lcgs_scene_transform", "lcgs_scene_box_keep_mask")
OK, INVALID_ARG = 0, 1
ROTATIONS = T.rotation_set()


def _addr(k):
    return C.c_void_p(0x1000000 * (k + 1))  # never dereferenced


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib, api = lcgs.load_library(), lcgs.api
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    p, i = C.c_void_p, C.c_int
    sim, plan, cam, params = (C.POINTER(t) for t in (api.Similarity, api.SimilarityPlan, api.Camera, api.STRUCTS["lcgs_params"]))
    expected = {"lcgs_similarity_plan_make": [sim, plan, p], "lcgs_camera_transform": [cam, sim, cam],
                "lcgs_scene_transform": [p, i, i, sim, params, params], "lcgs_scene_box_keep_mask": [p, i, p, sim, p, p]}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header), name
        assert api.SIGNATURES[name] == (C.c_int, expected[name]), name
    assert api.STRUCTS["lcgs_similarity"] is api.Similarity and api.STRUCTS["lcgs_similarity_plan"] is api.SimilarityPlan
    assert C.sizeof(api.Similarity) == 13 * 4 and C.sizeof(api.SimilarityPlan) == 100 * 4
    for method in ("scene_transform", "scene_box_keep_mask"):
        assert callable(getattr(lcgs.Renderer, method)), method
    for fn in ("similarity", "similarity_plan", "camera_transform"):
        assert callable(getattr(lcgs, fn)) and getattr(lcgs, fn) is getattr(api, fn)
    # the contract and what is not offered are said where the declarations are
    for phrase in ("new = scale * rot * old + trans", "Shepperd", "rot_from_quat", "LCGS_SH_TERMS", "B_l(R d) = D_l B_l(d)",
                   "(w, x, y, z)", "((M[i][0]*x + M[i][1]*y) + M[i][2]*z) + t[i]", "w' = ((W*w - X*x) - Y*y) - Z*z",
                   "j ascending", "bit copy", "not renormalised", "in place", "alias", "Only enqueues", "no atomics",
                   "lcgs_scene_modified", "f16 coefficient copy", "lcgs_ply_filter_rows", "+inf is legal",
                   "Not offered", "non-uniform scale", "reflections", "optimiser moments", "resets the moments", "lcgs-app flag",
                   "gradients with respect to the transform", "ownership step"):
        assert phrase in header, phrase
    launch = open(os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "csrc", "kernels", "launch.hpp")).read()
    assert int(re.search(r"constexpr int kTransformTileRows = (\d+);", launch).group(1)) == 64  # the GPU tests' counts sit around it


# ------------------------------------------------------------------------------------------------------ the plan, the camera
def _agree(got, want64, what):
    """got: binary32 values of the library; want64: the restatement's binary64 values.  Bit for bit the binary32 rounding of
    want64 -- except where the binary64 value itself is not defined to a binary32 ulp: the library and the restatement build D_l by
    different methods that agree to a few 1e-16 ABSOLUTE (1e-12 is asserted), so (a) an entry within that distance of a rounding
    boundary may round to either neighbour (1 ulp), and (b) an entry that is 0 up to such noise (a 90-degree turn given in binary32
    has cos = 6e-17) has no defined bits at all: both sides below 1e-12 there."""
    got, want64 = np.asarray(got, np.float32).reshape(-1), np.asarray(want64, np.float64).reshape(-1)
    want = want64.astype(np.float32)
    same = got.view(np.uint32) == want.view(np.uint32)
    one_ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1
    near_tie = np.abs(want64 - (got.astype(np.float64) + want.astype(np.float64)) / 2) <= 1e-12
    noise = (np.abs(want64) <= 1e-12) & (np.abs(got) <= 1e-12)
    ok = same | (one_ulp & near_tie) | noise
    assert ok.all(), (what, got[~ok], want[~ok])
    return int((~same).sum())


@pytest.mark.parametrize("k", range(len(ROTATIONS)))
def test_plan_is_the_restatements(lcgs, k):
    rot, scale, trans = ROTATIONS[k], (1.0, 2.5, 0.37)[k % 3], (0.7, -1.3, 2.1)
    p = T.plan64(rot, scale, trans)
    plan, D64 = lcgs.similarity_plan(lcgs.similarity(rot, scale, trans))
    for l in range(3):
        assert np.abs(D64[l] - p["D"][l]).max() <= 1e-12, l
    loose = 0
    # M, t, s, q come out of the same binary64 operations in the same order on both sides: no allowance
    for got, want in ((plan.M, p["M"]), (plan.t, p["t"]), ([plan.s], [p["s"]]), (plan.q, p["q"])):
        assert T.same_bits(np.asarray(list(got), np.float32), np.asarray(want, np.float64).reshape(-1).astype(np.float32))
    for got, want, what in ((plan.D1, p["D"][0], "D1"), (plan.D2, p["D"][1], "D2"), (plan.D3, p["D"][2], "D3")):
        loose += _agree(list(got), want, what)
    if k < 20:
        assert loose == 0  # (generic rotations: every entry's bits are the restatement's)
    if k == 20:  # the identity is the identity, exactly
        assert list(plan.M) == [float(np.float32(scale)) if i % 4 == 0 else 0.0 for i in range(9)] and list(plan.q) == [1, 0, 0, 0]
        for D, n in ((plan.D1, 3), (plan.D2, 5), (plan.D3, 7)):
            assert T.same_bits(np.asarray(list(D), np.float32).reshape(n, n), np.eye(n, dtype=np.float32))


def test_camera_is_the_restatements(lcgs):
    cam = lcgs.get_lookat_cam([3, 0.5, 1.2], [0, 0, 0.5], [0, 0, 1], width=96, height=64)
    for k, rot in enumerate(ROTATIONS):
        xf = lcgs.similarity(rot, (1.0, 2.5)[k % 2], (0.7, -1.3, 2.1))
        got = lcgs.camera_transform(cam, xf).to_dict()
        want = T.camera(cam.to_dict(), T.plan64(rot, (1.0, 2.5)[k % 2], (0.7, -1.3, 2.1)))
        for key in ("position", "front", "up", "right"):
            assert T.same_bits(np.asarray(got[key], np.float32), np.asarray(want[key], np.float64).astype(np.float32)), (k, key)
        for key in ("fov", "aspect_ratio", "width", "height"):
            assert got[key] == cam.to_dict()[key]
    same = lcgs.Camera.from_dict(cam.to_dict())  # out may be in
    assert lcgs.load_library().lcgs_camera_transform(C.byref(same), C.byref(xf), C.byref(same)) == OK
    assert same.to_dict() == got


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refused(lib, status, needle):
    assert status == INVALID_ARG, status
    assert needle in lib.lcgs_last_error(), lib.lcgs_last_error()


def _bad_similarities(lcgs):
    """(similarity, what lcgs_last_error must say) for every refusal of the plan"""
    good = T.random_rotation(np.random.default_rng(1)).astype(np.float64)
    out = []
    for bad in (float("nan"), float("inf")):
        r = good.copy()
        r[1, 2] = bad
        out += [(lcgs.similarity(r), b"non-finite"), (lcgs.similarity(good, bad), b"non-finite"),
                (lcgs.similarity(good, 1.0, (0.0, bad, 0.0)), b"non-finite")]
    out += [(lcgs.similarity(good, 0.0), b"scale must be > 0"), (lcgs.similarity(good, -2.0), b"scale must be > 0")]
    skew = good.copy()
    skew[0] *= 1.001  # rot rot^T - I = 2e-3 on the diagonal
    out += [(lcgs.similarity(skew), b"not a rotation"), (lcgs.similarity(2.0 * good), b"not a rotation"),
            (lcgs.similarity(np.zeros((3, 3))), b"not a rotation")]
    out += [(lcgs.similarity(np.diag([1.0, 1.0, -1.0]) @ good), b"det rot <= 0"), (lcgs.similarity(-good), b"det rot <= 0")]
    return out


def test_plan_and_camera_refuse_bad_arguments(lcgs):
    lib = lcgs.load_library()
    xf, plan, cam = lcgs.similarity(), lcgs.SimilarityPlan(), lcgs.get_lookat_cam([3, 0, 1], [0, 0, 0], [0, 0, 1])
    out = lcgs.Camera()
    assert lib.lcgs_similarity_plan_make(C.byref(xf), C.byref(plan), None) == OK  # D64 is nullable
    _refused(lib, lib.lcgs_similarity_plan_make(None, C.byref(plan), None), b"NULL")
    _refused(lib, lib.lcgs_similarity_plan_make(C.byref(xf), None, None), b"NULL")
    _refused(lib, lib.lcgs_camera_transform(None, C.byref(xf), C.byref(out)), b"NULL")
    _refused(lib, lib.lcgs_camera_transform(C.byref(cam), None, C.byref(out)), b"NULL")
    _refused(lib, lib.lcgs_camera_transform(C.byref(cam), C.byref(xf), None), b"NULL")
    for bad, needle in _bad_similarities(lcgs):
        _refused(lib, lib.lcgs_similarity_plan_make(C.byref(bad), C.byref(plan), None), needle)
        _refused(lib, lib.lcgs_camera_transform(C.byref(cam), C.byref(bad), C.byref(out)), needle)
    # the 1e-4 is an input check: a binary32 rotation composed a few times stays far inside it
    r = np.eye(3, dtype=np.float32)
    for rot in ROTATIONS[:8]:
        r = (r @ rot).astype(np.float32)
    assert lib.lcgs_similarity_plan_make(C.byref(lcgs.similarity(r)), C.byref(plan), None) == OK


@pytest.mark.parametrize("ctx", [0, 0x1000])
def test_scene_transform_refuses_bad_arguments_before_any_device_work(lcgs, ctx):
    lib, api = lcgs.load_library(), lcgs.api
    fn = lib.lcgs_scene_transform
    ctx = C.c_void_p(ctx)
    xf = lcgs.similarity(ROTATIONS[0], 2.0, (1, 2, 3))
    P = 10
    span = 48 * 4 * P  # bytes of the largest array
    a = [0x1000000 + k * 0x10000 for k in range(10)]
    pack = lambda v: api._Params(*[C.c_void_p(x) for x in v])
    src, dst = pack(a[:5]), pack(a[5:])
    assert span < 0x10000
    if not ctx.value:
        _refused(lib, fn(ctx, P, 3, C.byref(xf), C.byref(src), C.byref(dst)), b"NULL")
        return
    _refused(lib, fn(ctx, P, 3, None, C.byref(src), C.byref(dst)), b"NULL")
    _refused(lib, fn(ctx, P, 3, C.byref(xf), None, C.byref(dst)), b"NULL")
    _refused(lib, fn(ctx, P, 3, C.byref(xf), C.byref(src), None), b"NULL")
    _refused(lib, fn(ctx, -1, 3, C.byref(xf), C.byref(src), C.byref(dst)), b"negative")
    for deg in (-1, 4):
        _refused(lib, fn(ctx, P, deg, C.byref(xf), C.byref(src), C.byref(dst)), b"sh_degree")
    for k in range(5):  # an output whose input is NULL
        v = a[:5]
        v[k] = 0
        _refused(lib, fn(ctx, P, 3, C.byref(xf), C.byref(pack(v)), C.byref(dst)), b"input is NULL")
    for bad, needle in _bad_similarities(lcgs):
        _refused(lib, fn(ctx, P, 3, C.byref(bad), C.byref(src), C.byref(dst)), needle)
    # aliasing: a partial overlap of an output with its own input, an output on a different input, two outputs on each other
    rows = (12, 12, 16, 192, 4)  # bytes per row
    for k in range(5):
        v = a[5:]
        v[k] = a[k] + rows[k] * 3  # three rows into its own input
        _refused(lib, fn(ctx, P, 3, C.byref(xf), C.byref(src), C.byref(pack(v))), b"alias")
        v[k] = a[k] - rows[k] * 3
        _refused(lib, fn(ctx, P, 3, C.byref(xf), C.byref(src), C.byref(pack(v))), b"alias")
        v[k] = a[(k + 1) % 5]  # exactly another member's input
        _refused(lib, fn(ctx, P, 3, C.byref(xf), C.byref(src), C.byref(pack(v))), b"alias")
        v = a[5:]
        v[k] = a[5 + (k + 2) % 5] + 4  # into another output
        _refused(lib, fn(ctx, P, 3, C.byref(xf), C.byref(src), C.byref(pack(v))), b"alias")
    # ... at any count (two outputs on one address)
    v = a[5:]
    v[1] = v[0]
    _refused(lib, fn(ctx, 0, 3, C.byref(xf), C.byref(src), C.byref(pack(v))), b"alias")
    # an input that is not read (its output is NULL) may lie anywhere: no refusal is owed to it -- the call would go on to the
    # device, so only the refusal side is pinned here: the same overlap WITH the output given is refused
    v_in, v_out = a[:5], a[5:]
    v_in[3] = v_out[0]  # the coefficients' input on the positions' output
    _refused(lib, fn(ctx, P, 3, C.byref(xf), C.byref(pack(v_in)), C.byref(pack(v_out))), b"alias")


@pytest.mark.parametrize("ctx", [0, 0x1000])
def test_box_keep_mask_refuses_bad_arguments_before_any_device_work(lcgs, ctx):
    lib = lcgs.load_library()
    fn = lib.lcgs_scene_box_keep_mask
    ctx = C.c_void_p(ctx)
    xf = lcgs.similarity(ROTATIONS[2], 1.0, (0.1, 0.2, 0.3))
    half = (C.c_float * 3)(1.0, float("inf"), 0.0)
    good = [ctx, 10, _addr(0), C.byref(xf), half, _addr(1)]
    if not ctx.value:
        _refused(lib, fn(*good), b"NULL")
        return
    for k in (2, 3, 4, 5):
        args = list(good)
        args[k] = None
        _refused(lib, fn(*args), b"NULL")
    args = list(good)
    args[1] = -1
    _refused(lib, fn(*args), b"negative")
    for bad in (-1.0, float("nan"), float("-inf")):
        for k in range(3):
            h = (C.c_float * 3)(1.0, 1.0, 1.0)
            h[k] = bad
            args = list(good)
            args[4] = h
            _refused(lib, fn(*args), b"half_extent")
    for bad, needle in _bad_similarities(lcgs):
        args = list(good)
        args[3] = C.byref(bad)
        _refused(lib, fn(*args), needle)
