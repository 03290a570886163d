"""The maps reference (tests/maps_ref.py) on the CPU: the f64 composition of the unchanged oracle against central finite
differences of the f64 maps, the oracle yardstick's own consistency, and the premises of the GPU tests' crowd."""
import numpy as np
import pytest

import maps_ref
from conftest import make_scene

POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])


@pytest.mark.parametrize("mode", maps_ref.MODES)
def test_backward_matches_finite_differences_f64(oracle64, mode):
    """Smooth mode (alpha skip and T stop off in forward and backward, as in tests/test_oracle_backward.py): both maps are smooth
    in the parameters, so central differences validate the composition -- render_backward with the colour (v, 1, 0), the
    preprocess-backward, and the dL/dv dv/dz front term -- for every attribute."""
    o = oracle64
    rng = np.random.default_rng(11)
    scene = {k: v.astype(np.float64) for k, v in make_scene(rng, 300, spread=0.35, log_scale=(-2.6, 0.4)).items()}
    scene["opacity"] = np.clip(scene["opacity"], 0.05, 0.9)  # below the 0.99 cap everywhere
    W, H = 40, 28
    cam = o.lookat(*POSE, width=W, height=H)
    wd, wa = rng.normal(size=(H, W)), rng.normal(size=(H, W))
    o.set_smooth(True)
    try:
        def loss(sc):
            depth, alpha, _ = maps_ref.forward(o, sc, cam, mode, scale_modifier=1.1)
            return float((depth * wd).sum() + (alpha * wa).sum())

        g = maps_ref.backward(o, scene, cam, wd, wa, mode, scale_modifier=1.1)
        assert np.all(g["sh"] == 0) and np.abs(g["pos"]).max() > 0
        for name in ("pos", "scale", "rotq", "opacity"):
            flat, gf = scene[name].reshape(-1), g[name].reshape(-1)
            scale_g = np.abs(gf).max()
            for i in rng.choice(flat.size, 25, replace=False):
                h = 1e-6 * max(1.0, abs(flat[i]))
                old = flat[i]
                flat[i] = old + h
                lp = loss(scene)
                flat[i] = old - h
                lm = loss(scene)
                flat[i] = old
                fd = (lp - lm) / (2 * h)
                assert abs(fd - gf[i]) <= 2e-5 * max(abs(fd), abs(gf[i])) + 1e-7 * scale_g, (mode, name, i, fd, gf[i])
    finally:
        o.set_smooth(False)


def test_crowd_is_what_the_gpu_tests_claim(oracle):
    """The crowd's premises from the oracle alone, and the yardstick's consistency on it: compositing (depth, 1, 0) over a zero
    background walks exactly the frame's entries, so channel 1 is 1 - final_T up to rounding."""
    scene, pose, W, H = maps_ref.crowd()
    cam = oracle.lookat(*pose, width=W, height=H)
    depth, alpha, st = maps_ref.forward(oracle, scene, cam, "z")
    lens = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    assert lens.size == 9 and lens.max() > 512, lens
    assert (st["final_T"] < 1e-3).sum() >= 1 and (st["n_contrib"] == 0).sum() >= 1 and (W % 8, H % 8) != (0, 0)
    assert depth.dtype == alpha.dtype == np.float32
    assert np.abs(alpha.astype(np.float64) - (1.0 - st["final_T"].astype(np.float64))).max() < 2e-6
    empty = st["n_contrib"] == 0
    assert np.all(depth[empty] == 0) and np.all(alpha[empty] == 0) and (depth[~empty] > 0).all()
    # the inverse mode composites 1 / z of the same entries
    inv = maps_ref.forward(oracle, scene, cam, "inv_z")
    assert np.array_equal(inv[1], alpha) and np.all(inv[0][empty] == 0) and not np.array_equal(inv[0], depth)


def test_row_bound_covers_the_f32_oracle(oracle):
    """The bound is a bound for an honest binary32 evaluation: the f32 oracle's own rows lie inside it (K >= 1)."""
    from gpu_util import gradient_row_ratios

    rng = np.random.default_rng(3)
    scene = make_scene(rng, 400, spread=0.4, log_scale=(-3.0, 0.5))
    W, H = 37, 29
    cam = oracle.lookat(*POSE, width=W, height=H)
    gd, ga = rng.normal(size=(H, W)).astype(np.float32), rng.normal(size=(H, W)).astype(np.float32)
    for mode in maps_ref.MODES:
        B, r64 = maps_ref.row_bound(scene, cam, gd, ga, mode)
        got = maps_ref.backward(oracle, scene, cam, gd, ga, mode)
        for k, (w, row, bad) in gradient_row_ratios(got, B, r64).items():
            assert w <= 1.0, (mode, k, w, row)
        assert all(np.isfinite(B[k]).all() for k in B)
