"""The depth-distortion map's CPU reference (tests/distortion_ref.py) pinned without a GPU: the closed form against the pairwise
sum it stands for, and its f64 gradient against central differences of its own f64 forward, with the already-validated depth
channel of maps_ref.py through the identical procedure as the yardstick."""
import numpy as np

import distortion_ref
import maps_ref
from conftest import make_scene

POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])


def test_closed_form_is_the_pairwise_sum_and_so_are_its_derivatives():
    """A M2 - M1^2 = sum_{i<j} w_i w_j (u_i - u_j)^2, d/dw_i = M2 + u_i (A u_i - 2 M1) = sum_j w_j (u_i - u_j)^2,
    d/du_i = 2 w_i (A u_i - M1) = 2 w_i sum_j w_j (u_i - u_j), for any centre.  float64; every comparison relative 1e-12 of the
    sum of the magnitudes of the terms the closed form combines (its own cancellation is what `center` is there for)."""
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 17, 200):
        w, v = rng.uniform(0, 1, n) * rng.uniform(0, 1, n), rng.uniform(0.5, 6.0, n)
        for center in (0.0, 3.0, float(v.mean())):
            u = v - center
            A, M1, M2 = w.sum(), (w * u).sum(), (w * u * u).sum()
            d = u[:, None] - u[None, :]
            ww = w[:, None] * w[None, :]
            pair = np.triu(ww * d * d, 1).sum()
            mag = A * M2 + M1 * M1
            assert abs((A * M2 - M1 * M1) - pair) <= 1e-12 * mag, (n, center)
            dw = (w[None, :] * d * d).sum(axis=1)
            assert (np.abs(M2 + u * (A * u - 2 * M1) - dw) <= 1e-12 * (M2 + np.abs(u) * (A * np.abs(u) + 2 * abs(M1)))).all(), (n, center)
            du = 2 * w * (w[None, :] * d).sum(axis=1)
            assert (np.abs(2 * w * (A * u - M1) - du) <= 1e-12 * 2 * w * (A * np.abs(u) + abs(M1))).all(), (n, center)
    # the value does not depend on the centre
    u = v - 100.0
    A, M1, M2 = w.sum(), (w * u).sum(), (w * u * u).sum()
    assert abs((A * M2 - M1 * M1) - pair) <= 1e-12 * (A * M2 + M1 * M1)


def _central_differences(o, scene, cam, loss, state, grad, rng, per_attribute):
    """(largest |fd - g| / max |g| of the attribute over the components drawn, components drawn, components skipped): central
    differences of `loss` with the frame's own thresholds in place; a component whose perturbed frames decide differently
    (n_contrib or lists) is skipped, not counted"""
    base = state(scene)
    worst, drawn, skipped = 0.0, 0, 0
    for name in ("pos", "scale", "rotq", "opacity"):
        flat, gf = scene[name].reshape(-1), grad[name].reshape(-1)
        scale_g = np.abs(gf).max()
        assert scale_g > 0, name
        for i in rng.choice(flat.size, per_attribute, replace=False):
            h = 1e-6 * max(1.0, abs(flat[i]))
            old = flat[i]
            vals = []
            same = True
            for s in (+1, -1):
                flat[i] = old + s * h
                st = state(scene)
                same &= all(np.array_equal(st[k], base[k]) for k in ("n_contrib", "point_list", "ranges"))
                vals.append(loss(scene))
            flat[i] = old
            drawn += 1
            if not same:
                skipped += 1
                continue
            worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - gf[i]) / scale_g)
    return worst, drawn, skipped


def test_reference_gradient_matches_central_differences_like_the_depth_channel_does(oracle64):
    """distortion_ref.backward (f64) against central differences of distortion_ref.forward (f64), 40 splats at 24 x 20, eight
    components per attribute, in both modes about a centre near the scene's depth; the same components through
    maps_ref.backward's depth channel are the yardstick, and the distortion channel is held to 10 x its disagreement (a term
    quadratic in the weights carries more truncation than a linear one).
    Measured (largest |fd - g| / max |g|; no component of the 32 drawn per mode is skipped):
        z:     depth channel 5.3e-10, distortion channel 6.5e-10
        inv_z: depth channel 5.6e-10, distortion channel 1.5e-09"""
    o = oracle64
    P, W, H = 40, 24, 20
    scene = {k: v.astype(np.float64) for k, v in make_scene(np.random.default_rng(3), P, spread=0.35, log_scale=(-2.2, 0.5)).items()}
    scene["opacity"] = np.clip(scene["opacity"], 0.05, 0.9)
    cam = o.lookat(*POSE, width=W, height=H)
    wrng = np.random.default_rng(11)
    wd, wq = wrng.normal(size=(H, W)), wrng.normal(size=(H, W))
    state = lambda sc: o.forward_state(sc, cam)
    for mode, center in (("z", 3.75), ("inv_z", 0.25)):
        g_depth = maps_ref.backward(o, scene, cam, wd, None, mode=mode)
        g_dist = distortion_ref.backward(o, scene, cam, wq, mode=mode, center=center)
        assert not g_dist["sh"].any() and (distortion_ref.forward(o, scene, cam, mode, center)[0] > 0).any()
        loss_depth = lambda sc: float((maps_ref.forward(o, sc, cam, mode)[0] * wd).sum())
        loss_dist = lambda sc: float((distortion_ref.forward(o, sc, cam, mode, center)[0] * wq).sum())
        e_depth, drawn, skipped = _central_differences(o, scene, cam, loss_depth, state, g_depth, np.random.default_rng(5), 8)
        e_dist, drawn2, skipped2 = _central_differences(o, scene, cam, loss_dist, state, g_dist, np.random.default_rng(5), 8)
        print(f"[distortion reference vs central differences] {mode}: depth channel {e_depth:.3e}, distortion channel {e_dist:.3e}, "
              f"{skipped} of {drawn} components skipped")
        assert (drawn, skipped) == (drawn2, skipped2) and 4 * skipped <= drawn, (drawn, skipped)
        assert e_depth > 0 and e_dist <= 10 * e_depth, (mode, e_dist, e_depth)
