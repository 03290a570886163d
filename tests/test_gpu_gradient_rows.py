"""`-m gpu`: frames aimed at the gradient rows a norm hides -- the tile row and column next to the unrasterised strip,
single-pixel splats at the radius floor, footprints either side of the render-backward's switch to f64 per-splat algebra,
one tile with thousands of entries (more than the walk stages at once), opacities on the 1/255 and 0.99 thresholds (the
backward's hardware exp against the forward's defined one), pixels whose T falls below 1e-4 mid-list, and scene sizes at
256-row boundaries.  Each case asserts on the oracle that the frame really holds what it aims at.  Every case is seeded and every row is held to its own bound (gpu_util.check_gradient_rows)."""
import numpy as np
import pytest
import torch

from conftest import make_scene
from gpu_util import DEV, check_gradient_rows, dev, upload_scene

pytestmark = pytest.mark.gpu
POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])


def _run(lcgs, oracle, scene, W, H, tag, bg=(0.1, 0.2, 0.3), seed=0, pose=POSE):
    P = scene["pos"].shape[0]
    cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
    ocam = oracle.lookat(*pose, width=W, height=H)
    r = lcgs.Renderer(lcgs.Context(0))
    d = upload_scene(scene)
    r.bind_scene(d["pos"], d["scale"], d["rotq"], d["sh"], d["opacity"])
    img = torch.zeros(3, H, W, device=DEV)
    n = r.forward(cam, img, bg=bg, keep_state=True, sync=True)
    ref = oracle.render(scene, ocam, bg=bg)
    assert n == ref["num_rendered"] and n > 0, tag
    dL = np.random.default_rng(seed).normal(size=(3, H, W)).astype(np.float32)
    g = {k: torch.full_like(d[k], 7.0) for k in ("pos", "scale", "rotq", "sh", "opacity")}
    r.backward(dev(dL), g["pos"], g["scale"], g["rotq"], g["sh"], g["opacity"])
    r.ctx.synchronize()
    check_gradient_rows(g, scene, ocam, dL, bg=bg, tag=tag)
    return ref


@pytest.mark.parametrize("res", [(100, 72), (333, 201), (17, 300)])
def test_rows_next_to_the_partial_tile_strip(lcgs, oracle, res):
    """small splats scattered over the whole frame, so that dozens have their centres in the last rasterised tile row /
    column and dozens in the partial strip behind it, which the forward never rasterises (the reference's behaviour,
    tests/test_reference_png.py): splats whose pixels all lie there must get rows of exactly 0 (their bound is 0)"""
    W, H = res
    rng = np.random.default_rng(W * 1000 + H)
    scene = make_scene(rng, 3000, spread=1.4, log_scale=(-5.0, 0.3))
    st = oracle.forward_state(scene, oracle.lookat(*POSE, width=W, height=H), bg=(0.1, 0.2, 0.3))
    on = st["radii"] > 0
    mx, my = st["means"][:, 0], st["means"][:, 1]
    xs, ys = W - W % 16, H - H % 16  # first column / row of the strip
    in_strip = on & (((mx >= xs) & (mx < W)) | ((my >= ys) & (my < H)))
    next_to = on & ~in_strip & ((mx >= xs - 16) | (my >= ys - 16)) & (mx >= 0) & (my >= 0) & (mx < W) & (my < H)
    assert in_strip.sum() >= 20 and next_to.sum() >= 20, (int(in_strip.sum()), int(next_to.sum()))
    ref = _run(lcgs, oracle, scene, W, H, f"{W}x{H}")
    assert not ref["n_contrib"][ys:].any() and not ref["n_contrib"][:, xs:].any()


def test_single_pixel_splats_at_the_radius_floor(lcgs, oracle):
    rng = np.random.default_rng(11)
    scene = make_scene(rng, 4000, spread=0.7, log_scale=(-7.5, 0.3))  # sub-pixel: the 0.3 px^2 low-pass sets the footprint
    scene["opacity"][:] = np.clip(scene["opacity"], 0.3, 0.99)
    ref = _run(lcgs, oracle, scene, 160, 120, "radius floor")
    assert (ref["radii"][ref["radii"] > 0] <= 3).mean() > 0.9  # the floor: ceil(3 sqrt(0.3 px^2 + a sub-pixel variance))


def _cov_trace(oracle, scene, ocam):
    """the trace of each splat's filtered 2-D covariance (px^2): what the preprocess-backward compares with
    kGiantCovTrace = 455 to take its per-splat algebra in f64 (backward.hip, geom_backward)"""
    _, _, cov = oracle.project(scene["pos"], scene["scale"], scene["rotq"], ocam)
    return cov[:, 0].astype(np.float64) + cov[:, 2] + 0.6  # + the 0.3 px^2 low-pass on both axes


GIANT_COV_TRACE = 455.0


def test_footprints_either_side_of_the_f64_switch(lcgs, oracle):
    """round splats around the target, sized so that the traces of their filtered 2-D covariances straddle the switch: at
    least 20 on-screen splats within 15 % below it and 20 within 15 % above it (radius ~45 px for a round splat)"""
    rng = np.random.default_rng(12)
    P = 400
    scene = make_scene(rng, P, spread=0.05)
    scene["scale"][:] = np.exp(rng.uniform(np.log(0.19), np.log(0.3), (P, 1))).astype(np.float32)
    scene["opacity"][:] = rng.uniform(0.05, 0.6, P).astype(np.float32)
    ocam = oracle.lookat(*POSE, width=320, height=240)
    tr = _cov_trace(oracle, scene, ocam)
    on = oracle.render(scene, ocam)["radii"] > 0
    below = on & (tr > GIANT_COV_TRACE / 1.15) & (tr <= GIANT_COV_TRACE)
    above = on & (tr > GIANT_COV_TRACE) & (tr <= GIANT_COV_TRACE * 1.15)
    assert below.sum() >= 20 and above.sum() >= 20, (int(below.sum()), int(above.sum()))
    _run(lcgs, oracle, scene, 320, 240, "f64 switch")


@pytest.mark.parametrize("depths", ["coplanar", "staggered"])
def test_one_tile_with_thousands_of_entries(lcgs, oracle, depths):
    """5000 splats inside ONE 16 x 16 tile (the frame's centre, pixel 40 of 80, is that tile's centre): longer than one
    staging round of the walk, and T falls below 1e-4 in the middle of the list"""
    rng = np.random.default_rng(13 if depths == "coplanar" else 14)
    P, W = 5000, 80
    scene = make_scene(rng, P, log_scale=(-2.6, 0.1))
    target = np.array(POSE[1], np.float64)
    eye = np.array(POSE[0], np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0, 0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    off = rng.uniform(-0.02, 0.02, (P, 2))
    along = np.zeros(P) if depths == "coplanar" else rng.uniform(-0.3, 0.3, P)
    scene["pos"][:] = (target + off[:, :1] * right + off[:, 1:] * up + along[:, None] * fwd).astype(np.float32)
    scene["opacity"][:] = rng.uniform(0.05, 0.6, P).astype(np.float32)
    st = oracle.forward_state(scene, oracle.lookat(*POSE, width=W, height=W), bg=(0.1, 0.2, 0.3))
    lengths = st["ranges"][:, 1] - st["ranges"][:, 0]
    assert lengths.max() >= 4000 and np.sort(lengths)[-2] <= 0.05 * lengths.max(), np.sort(lengths)[-4:]
    tile = int(np.argmax(lengths))
    gx = (W + 15) // 16
    ty, tx = divmod(tile, gx)
    blk = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
    # the walk ended these pixels before the middle of the list: the next entry would have taken T below 1e-4
    stopped = (st["final_T"][blk] < 1e-3) & (st["n_contrib"][blk] > 0) & (st["n_contrib"][blk] < lengths[tile] // 2)
    assert stopped.sum() >= 16, int(stopped.sum())
    _run(lcgs, oracle, scene, W, W, f"one tile, {depths}")


def test_opacities_on_the_blend_thresholds(lcgs, oracle):
    """opacities CONSTRUCTED onto the two thresholds: for each splat the pixel nearest its centre is chosen, the binary32
    power there evaluated, and the opacity set so that o G lies within +-2 ulp of 1/255 (half the splats) or of 0.99 (those
    whose G there exceeds 0.992).  These are the entries the backward's hardware exp and the forward's defined exp may decide
    apart; the bound's flip term F must fire on them (asserted on the oracle first, then every row held to the bound)"""
    from gpu_util import _oracles
    from oracle import gradient_row_terms

    rng = np.random.default_rng(15)
    P, W, H = 3000, 200, 150
    scene = make_scene(rng, P, log_scale=(-3.0, 0.3))
    ocam = oracle.lookat(*POSE, width=W, height=H)
    st = oracle.forward_state(scene, ocam)
    m, cn = st["means"].astype(np.float32), st["conic"].astype(np.float32)
    pix = np.round(m).astype(np.float32)
    dx, dy = m[:, 0] - pix[:, 0], m[:, 1] - pix[:, 1]
    power = np.float32(-0.5) * (cn[:, 0] * dx * dx + cn[:, 2] * dy * dy) - cn[:, 1] * dx * dy  # the forward's expression
    G = oracle.blend_exp(np.minimum(power, 0))
    inside = (st["radii"] > 0) & (power <= 0) & (pix[:, 0] >= 0) & (pix[:, 0] < W - W % 16) & (pix[:, 1] >= 0) & \
        (pix[:, 1] < H - H % 16)
    k = rng.integers(-2, 3, P).astype(np.float32) * np.float32(2.0 ** -23)
    lo = inside & (np.arange(P) % 2 == 0)
    hi = inside & (np.arange(P) % 2 == 1) & (G > 0.992)
    scene["opacity"][lo] = (np.float32(1.0 / 255.0) / G[lo]) * (1 + k[lo])
    scene["opacity"][hi] = (np.float32(0.99) / G[hi]) * (1 + k[hi])
    dL = np.random.default_rng(0).normal(size=(3, H, W)).astype(np.float32)
    o32, o64, _ = _oracles()
    F = gradient_row_terms(o32, o64, scene, o32.convert_camera(ocam), dL, bg=(0.1, 0.2, 0.3))["F"]
    n_lo, n_hi = int((F[lo] > 0).any(axis=1).sum()), int((F[hi] > 0).any(axis=1).sum())
    print(f"[threshold opacities] F fires on {n_lo} of {int(lo.sum())} rows at 1/255, {n_hi} of {int(hi.sum())} at 0.99, "
          f"{int((F > 0).any(axis=1).sum())} rows in all")
    assert n_lo >= 0.5 * lo.sum() >= 500 and n_hi >= 0.5 * hi.sum() >= 100
    _run(lcgs, oracle, scene, W, H, "threshold opacities")


@pytest.mark.parametrize("P", [256, 257, 511, 512, 767])
def test_scene_sizes_at_256_row_boundaries(lcgs, oracle, P):
    rng = np.random.default_rng(16 + P)
    scene = make_scene(rng, P, log_scale=(-3.5, 0.7))
    _run(lcgs, oracle, scene, 96, 80, f"P={P}")
