"""The antialiased mode's CPU reference (tests/antialias_ref.py) pinned without a GPU: its f64 gradient against central
differences of its own f64 forward -- the antialiased counterpart of test_oracle_backward.py::
test_backward_matches_finite_differences_f64, with that test's step and tolerance -- and the compensation's closed forms."""
import numpy as np

import antialias_ref
from conftest import make_scene

POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])


def test_reference_gradient_matches_finite_differences_f64(oracle64):
    """Smooth mode (alpha-skip / T-stop disabled in forward AND backward): the frame is a smooth function of the parameters.
    Positions, scales and rotations move rho, so the differences see the compensation's covariance term; the opacity sees
    dL/do' rho."""
    o = oracle64
    rng = np.random.default_rng(1)
    P = 36
    scene = {k: v.astype(np.float64) for k, v in make_scene(rng, P, spread=0.35, log_scale=(-2.6, 0.5)).items()}
    scene["opacity"] = np.clip(scene["opacity"], 0.05, 0.9)
    W, H = 64, 48
    cam = o.lookat(*POSE, width=W, height=H)
    wt = rng.normal(size=(3, H, W))
    bg = (0.2, 0.3, 0.1)
    o.set_smooth(True)
    try:
        loss = lambda sc: float((antialias_ref.forward_state(o, sc, cam, bg=bg, scale_modifier=1.1)["img"] * wt).sum())
        g, st, _ = antialias_ref.gradients(o, scene, cam, wt, bg=bg, scale_modifier=1.1)
        assert st["num_rendered"] > 0
        on = st["radii"] > 0
        # the premise: the compensation is at work on this scene (sub-pixel and pixel-sized splats), nothing is degenerate
        assert (st["aa"]["d0"][on] > 0).all() and (st["rho"][on] < 0.9).sum() >= 8 and (st["rho"][on] < 0.5).any()
        classic = o.render_backward_full(scene, cam, wt, bg=bg, scale_modifier=1.1)
        assert np.abs(g["scale"] - classic["scale"]).max() > 1e-3 * np.abs(classic["scale"]).max()  # another function
        for name in antialias_ref.KEYS:
            flat, gf = scene[name].reshape(-1), g[name].reshape(-1)
            scale_g = np.abs(gf).max()
            for i in rng.choice(flat.size, min(25, flat.size), replace=False):
                h = 1e-6 * max(1.0, abs(flat[i]))
                old = flat[i]
                flat[i] = old + h
                lp = loss(scene)
                flat[i] = old - h
                lm = loss(scene)
                flat[i] = old
                fd = (lp - lm) / (2 * h)
                assert abs(fd - gf[i]) <= 2e-5 * max(abs(fd), abs(gf[i])) + 1e-7 * scale_g, (name, i, fd, gf[i])
    finally:
        o.set_smooth(False)


def test_compensation_lies_in_the_unit_interval_and_tends_to_one(oracle, oracle64):
    rng = np.random.default_rng(5)
    scene = make_scene(rng, 4000, log_scale=(-5.0, 1.0))
    for o in (oracle, oracle64):
        cam = o.lookat(*POSE, width=640, height=480)
        _, depth, cov = o.project(scene["pos"], scene["scale"], scene["rotq"], cam)
        aa = antialias_ref.compensation(o, cov)
        rho = aa["rho"]
        assert rho.dtype == o.dtype and np.isfinite(rho).all()
        assert (rho >= 0).all() and (rho <= 1).all()
        assert rho.min() < 0.1 and rho.max() > 0.9
    # a splat many pixels wide keeps its opacity: 1 - rho ~ 0.3 tr / (2 det) -> 0
    for o in (oracle, oracle64):
        wide = np.array([[3.0e4, 1.0e3, 2.0e4], [5.0e5, 0.0, 5.0e5]])
        first_order = 0.3 * (wide[:, 0] + wide[:, 2]) / (2 * (wide[:, 0] * wide[:, 2] - wide[:, 1] ** 2))  # 1.3e-5, 6e-7
        big = antialias_ref.compensation(o, wide)["rho"].astype(np.float64)
        assert (big <= 1).all() and (1 - big <= 1.01 * first_order + 8 * float(np.finfo(o.dtype).eps)).all(), big
        mid = antialias_ref.compensation(o, np.array([[30.0, 0.0, 30.0]]))["rho"]
        assert 0.98 < mid[0] < 0.995
    # degenerate rows: a zero or negative determinant, a NaN quotient -> 0
    bad = antialias_ref.compensation(oracle, np.array([[1.0, 1.0, 1.0], [1.0, 1.2, 1.0], [np.nan, 0.0, 1.0], [0.0, 0.0, 0.0]]))
    assert (bad["rho"] == 0).all()


def test_isotropic_splat_gives_v_over_v_plus_dilation(oracle, oracle64):
    """An isotropic splat on the optical axis projects to v I: rho = sqrt(v^2 / (v + 0.3)^2) = v / (v + 0.3), to rounding"""
    for o in (oracle, oracle64):
        eps = float(np.finfo(o.dtype).eps)
        cam = o.lookat([0.0, -4.0, 0.5], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0], width=64, height=64)
        centre = np.array(cam.position[:], np.float64) + 4.0 * np.array(cam.front[:], np.float64)
        sizes = np.array([1e-3, 5e-3, 2e-2, 0.1, 0.5])
        pos = np.tile(centre, (sizes.size, 1))
        scale = np.repeat(sizes[:, None], 3, axis=1)
        rotq = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (sizes.size, 1))
        _, _, cov = o.project(pos, scale, rotq, cam)
        v = cov[:, 0].astype(np.float64)
        assert np.allclose(cov[:, 2], cov[:, 0], rtol=64 * eps) and (np.abs(cov[:, 1]) <= 64 * eps * v).all()
        assert v.min() < 0.01 and v.max() > 10  # from far below a pixel to several pixels
        rho = antialias_ref.compensation(o, cov)["rho"].astype(np.float64)
        k = float(np.float32(0.3))  # (the dilation is the binary32 literal in every build)
        assert np.allclose(rho, v / (v + k), rtol=256 * eps, atol=0), (rho, v / (v + k))

    # the forward state hands the walks opacity * rho, one multiply
    o = oracle
    rng = np.random.default_rng(9)
    scene = make_scene(rng, 300, log_scale=(-4.0, 0.8))
    cam = o.lookat(*POSE, width=96, height=64)
    st = antialias_ref.forward_state(o, scene, cam)
    assert np.array_equal(st["opacity_eff"], scene["opacity"].astype(np.float32) * st["rho"])
    classic = o.forward_state(scene, cam)
    assert np.array_equal(st["radii"], classic["radii"]) and np.array_equal(st["point_list"], classic["point_list"])
    assert np.abs(st["img"] - classic["img"]).max() > 1e-4
