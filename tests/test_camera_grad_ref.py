"""The camera gradient's reference (tests/camera_grad_ref.py) checked on the CPU, and the host-only twist helper.

Finite differences: for fixed random 2-D rows g the per-row scalar S_i(cam) = gm_i . mean_i + gc_i . conic_i + gcol_i . colour_i +
gv_i v_i, evaluated by the f64 oracle's sh_process / project / allocate_tiles, is differentiated by central differences over each of
the twelve camera floats (h = 1e-6, times the camera's distance to the scene centre for the position) and compared ROW BY ROW
with `contributions`; tolerance 1e-6 x sum_s |C64[row, k, s] g[row, s]| (truncation O(h^2) and round-off 1e-16 / h sit orders
below).  A row whose colour-clamp mask or frustum-clamp flags differ between the +-h evaluations is left out; at most 1 % of the
on-screen rows may be.  Worst ratios observed: 0.07 (crowd), 0.26 (102), 0.38 (108); docs/TESTS.md.
Draw 105 is not among the draws: one near-singular needle of it sits at 2.5 of the tolerance at h = 1e-6, at 0.21 at h = 1e-5 and
at 4.0 at h = 1e-7 -- an error that grows as h shrinks is the round-off of differencing that row's conic, which this yardstick
cannot tell from a wrong derivative; the needles and giants of 102 and 108 stay below it."""
import ctypes as C

import numpy as np
import pytest

import camera_grad_ref as cgr
import maps_ref
from gpu_util import _oracles, random_draw

FD_DRAWS = ("crowd", 102, 108)  # 102, 108: anisotropic needles and a few giants


def _draw(key):
    if key == "crowd":
        scene, pose, W, H = maps_ref.crowd()
        return scene, pose, W, H, None, 1.0
    _, scene, W, H, pose, fov, _, sm = random_draw(key)
    return scene, pose, W, H, fov, sm


def _evaluate(o64, scene, cam, mode, sm):
    """per row: (mean [P, 2], conic [P, 3], colour [P, 3], v [P]), radii, the colour-clamp mask [P, 3] and the frustum flags"""
    P = scene["pos"].shape[0]
    color, raw = o64.sh_process(np.array(cam.position[:]), scene["pos"], np.asarray(scene["sh"]).reshape(P, -1), deg=3, want_raw=True)
    m2, depth, cov = o64.project(scene["pos"], scene["scale"], scene["rotq"], cam, scale_modifier=sm)
    means, conic, _, radii = o64.allocate_tiles(cam.width, cam.height, depth, m2, cov)
    with np.errstate(divide="ignore"):
        v = depth if mode == "z" else np.where(depth != 0, 1.0 / depth, 0.0)
    with np.errstate(all="ignore"):
        t = cgr.geometry_terms(o64, scene, cam, np.zeros((P, cgr.N2D)), sm)
    flags = np.concatenate([(raw > 0) & (raw < 1), (t["clx"] != 0)[:, None], (t["cly"] != 0)[:, None],
                            (t["clx"] > 0)[:, None], (t["cly"] > 0)[:, None]], axis=1)
    return (means, conic, color, v), radii, flags


def _scalar(vals, g):
    means, conic, color, v = vals
    return (g[:, 0:2] * means).sum(1) + (g[:, 2:5] * conic).sum(1) + (g[:, 6:9] * color).sum(1) + g[:, 9] * v


@pytest.mark.parametrize("mode", maps_ref.MODES)
@pytest.mark.parametrize("key", FD_DRAWS)
def test_contributions_against_finite_differences(oracle, key, mode):
    _, o64, _ = _oracles()
    scene, pose, W, H, fov, sm = _draw(key)
    P = scene["pos"].shape[0]
    cam = o64.convert_camera(oracle.lookat(*pose, width=W, height=H, fov=fov))
    g = np.random.default_rng(41).normal(size=(P, cgr.N2D))
    base, radii, flags0 = _evaluate(o64, scene, cam, mode, sm)
    on = radii > 0
    assert on.sum() >= 1
    Cg = cgr.contributions(o64, scene, cam, radii, g, mode, sm)
    scale = np.einsum("pks,ps->pk", np.abs(cgr.unit_jacobian(o64, scene, cam, radii, mode, sm)), np.abs(g))
    v0 = cgr.cam12(cam)
    dist = float(np.linalg.norm(v0[0:3] - np.asarray(scene["pos"], np.float64).mean(axis=0)))
    worst, left_out = 0.0, np.zeros(P, bool)
    for k in range(12):
        h = 1e-6 * (dist if k < 3 else 1.0)
        S, ok = [], on.copy()
        for sgn in (+1.0, -1.0):
            v = v0.copy()
            v[k] += sgn * h
            vals, r, flags = _evaluate(o64, scene, cgr.with_cam12(o64, cam, v), mode, sm)
            assert np.array_equal(r > 0, on), (key, k)  # no row enters or leaves the screen within h
            ok &= (flags == flags0).all(axis=1)
            S.append(_scalar(vals, g))
        fd = (S[0] - S[1]) / (2.0 * h)
        left_out |= on & ~ok
        err = np.abs(fd - Cg[:, k])[ok]
        tol = 1e-6 * scale[ok, k]
        assert (tol > 0).all()
        ratio = float((err / tol).max()) if err.size else 0.0
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{key} {mode} component {k}: worst row at {ratio:.3f} of its tolerance"
    print(f"[camera FD] {key} {mode}: {int(on.sum())} on-screen rows, {int(left_out.sum())} left out, worst err/tol {worst:.3e}")
    assert left_out.sum() <= 0.01 * on.sum(), (int(left_out.sum()), int(on.sum()))


@pytest.mark.parametrize("key", ("crowd", 102))
def test_position_columns_reproduce_the_oracles_dpos(oracle, key):
    _, o64, _ = _oracles()
    scene, pose, W, H, fov, sm = _draw(key)
    cam = o64.convert_camera(oracle.lookat(*pose, width=W, height=H, fov=fov))
    rng = np.random.default_rng(3)
    gi, gd, ga = rng.normal(size=(3, H, W)), rng.normal(size=(H, W)), rng.normal(size=(H, W))
    for mode in maps_ref.MODES:
        kw = dict(mode=mode, bg=(0.1, 0.2, 0.3), scale_modifier=sm)
        g, st = cgr.walk_rows(o64, scene, cam, gi, gd, ga, **kw)
        Cc = cgr.contributions(o64, scene, cam, st["radii"], g, mode, sm)
        want = cgr.oracle_dpos(o64, scene, cam, gi, gd, ga, **kw).sum(axis=0)
        got = -Cc[:, 0:3].sum(axis=0)
        assert np.linalg.norm(want) > 0
        assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want), (key, mode, got, want)
        # ... and reference() takes exactly those rows
        r, C2 = cgr.reference(o64, scene, cam, gi, gd, ga, **kw)
        assert np.array_equal(r[0:3], -cgr.oracle_dpos(o64, scene, cam, gi, gd, ga, **kw).sum(axis=0))
        assert np.array_equal(C2[:, 3:], Cc[:, 3:])


def test_contributions_are_linear_in_the_rows(oracle):
    _, o64, _ = _oracles()
    scene, pose, W, H, fov, sm = _draw(102)
    cam = o64.convert_camera(oracle.lookat(*pose, width=W, height=H, fov=fov))
    P = scene["pos"].shape[0]
    radii = _evaluate(o64, scene, cam, "inv_z", sm)[1]
    g = np.random.default_rng(8).normal(size=(P, cgr.N2D))
    J = cgr.unit_jacobian(o64, scene, cam, radii, "inv_z", sm)
    direct = cgr.contributions(o64, scene, cam, radii, g, "inv_z", sm)
    via = np.einsum("pks,ps->pk", J, g)
    assert np.abs(direct - via).max() <= 1e-12 * np.einsum("pks,ps->pk", np.abs(J), np.abs(g)).max()


# ---------------------------------------------------------------------------------------------------------- the twist helper
def _twist_f64(cam, g12):
    Rc = np.stack([np.array(cam.right[:], np.float64), np.array(cam.up[:], np.float64), np.array(cam.front[:], np.float64)], axis=1)
    g = np.asarray(g12, np.float64)
    gk = (g[9:12], g[6:9], g[3:6])  # g_right, g_up, g_front
    terms = [np.cross(np.eye(3)[k], Rc.T @ gk[k]) for k in range(3)]
    omega, tau = sum(terms), Rc.T @ g[0:3]
    mag = np.concatenate([sum(np.abs(Rc.T) @ np.abs(gk[k]) for k in range(3)), np.abs(Rc.T) @ np.abs(g[0:3])])
    return np.concatenate([omega, tau]), mag


@pytest.mark.parametrize("case", ("lookat", "not orthonormal"))
def test_twist_helper_on_the_host(lcgs, case):
    cam = lcgs.get_lookat_cam([1.6, 0.3, 0.9], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0], width=45, height=37)
    rng = np.random.default_rng(12)
    if case == "not orthonormal":
        cam = lcgs.camera_with_vectors(cam, rng.normal(size=12).astype(np.float32))
    for _ in range(20):
        g12 = (rng.normal(size=12) * 10.0 ** rng.uniform(-3, 3, size=12)).astype(np.float32)
        got = lcgs.camera_grad_to_twist(cam, g12)
        want, mag = _twist_f64(cam, g12)
        assert got.dtype == np.float32 and got.shape == (6,)
        # one binary32 rounding of the binary64 value (plus the binary64 evaluation's own order-dependent error)
        assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-15 * mag).all(), (case, got, want)


def test_twist_helper_refuses_null(lcgs):
    lib = lcgs.load_library()
    g, out = (C.c_float * 12)(), (C.c_float * 6)()
    cam = lcgs.get_lookat_cam([1, 0, 0], [0, 0, 0], [0, 0, 1])
    assert lib.lcgs_camera_grad_to_twist(None, g, out) == 1  # LCGS_ERR_INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert lib.lcgs_camera_grad_to_twist(C.byref(cam), None, out) == 1
    assert lib.lcgs_camera_grad_to_twist(C.byref(cam), g, None) == 1
