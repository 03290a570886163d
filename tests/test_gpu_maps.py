"""`-m gpu`: the depth / alpha maps of a keep-state frame (lcgs_render_maps) and their backward (lcgs_render_backward_maps).

Forward: both maps equal the f32 oracle's composition bit for bit (tests/maps_ref.py: the frame's own state composited with the
colour (v, 1, 0)), in both depth modes -- the crowd (lists of five rounds, saturated and empty pixels, an image that is no
multiple of 8), eight random draws, a context-owned scene in spatial order, each output alone, a frame that draws nothing.
Backward: every component of every row inside maps_ref's bound (gpu_util.check_gradient_rows' formula and constants), no row
excluded -- depth only, alpha only, both, both with an image gradient, both modes, the crowd and four random draws;
accumulation over two views; overwritten arrays and exact zeros; the plain backward afterwards; the autograd wrapper."""
import numpy as np
import pytest
import torch

import luisacomputegaussiansplatting_amd as L
import maps_ref
from conftest import make_scene
from gpu_util import BG, DEV, KEYS, View, cached, check_gradient_rows, dev, random_draw, sevens, upload_scene

pytestmark = pytest.mark.gpu
FORWARD_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)       # 0, 3, 6: anisotropic needles and a few giants
BACKWARD_FRAMES = ("crowd", 100, 101, 102, 103)  # 102: needles and giants
VARIANTS = ("depth", "alpha", "both", "both+img")
POSE2 = ([-1.2, 1.1, 1.4], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])
AWAY = ([1.6, 0.3, 0.9], [5.0, 1.0, 1.3], [0.0, 0.0, 1.0])  # the crowd behind the camera


class Frame:
    """one (scene, pose, resolution, fov, bg, scale modifier) with the oracle's maps and the incoming gradients, computed once"""

    def __init__(self, oracle, key, pose=None):
        if key == "crowd":
            self.scene, p, self.W, self.H = maps_ref.crowd()
            self.pose, self.fov, self.bg, self.sm = pose or p, None, BG, 1.0
            rng = np.random.default_rng(17)
        else:
            rng, self.scene, self.W, self.H, self.pose, self.fov, self.bg, self.sm = random_draw(key)
        self.key, self.oracle = key, oracle
        self.P = self.scene["pos"].shape[0]
        self.ocam = oracle.lookat(*self.pose, width=self.W, height=self.H, fov=self.fov)
        shape = (self.H, self.W)
        self.gd, self.ga = rng.normal(size=shape).astype(np.float32), rng.normal(size=shape).astype(np.float32)
        self.gi = rng.normal(size=(3,) + shape).astype(np.float32)
        self._maps, self._bounds = {}, {}

    def cam(self):
        return L.get_lookat_cam(*self.pose, width=self.W, height=self.H, fov=self.fov)

    def maps(self, mode):
        if mode not in self._maps:
            self._maps[mode] = maps_ref.forward(self.oracle, self.scene, self.ocam, mode, scale_modifier=self.sm)
        return self._maps[mode]

    def incoming(self, variant):
        """(dL_dimg, dL_ddepth, dL_dalpha) of a variant; None = NULL"""
        return (self.gi if variant == "both+img" else None, None if variant == "alpha" else self.gd,
                None if variant == "depth" else self.ga)

    def bound(self, variant, mode):
        if (variant, mode) not in self._bounds:
            gi, gd, ga = self.incoming(variant)
            kw = dict(mode=mode, scale_modifier=self.sm)
            self._bounds[variant, mode] = (maps_ref.row_bound(self.scene, self.ocam, gd, ga, **kw) if gi is None else
                                           maps_ref.row_bound_with_image(self.scene, self.ocam, gi, gd, ga, bg=self.bg, **kw))
        return self._bounds[variant, mode]

    def renderer(self, keep=True):
        """a fresh context with the scene bound and the frame rendered; -> (renderer, device scene, image)"""
        r = L.Renderer(L.Context(0))
        d = upload_scene(self.scene)
        r.bind_scene(*[d[k] for k in KEYS])
        return (r, d) + ((self.render(r),) if keep else ())

    def render(self, r):
        img = torch.full((3, self.H, self.W), -1.0, device=DEV)
        n = r.forward(self.cam(), img, bg=self.bg, scale_modifier=self.sm, keep_state=True, sync=True)
        assert n > 0, self.key
        return img


def _frame(oracle, key, pose=None):
    return cached(("maps", key, str(pose)), lambda: Frame(oracle, key, pose))


def _maps(r, H, W, mode, depth=True, alpha=True):
    d = torch.full((H, W), 7.0, device=DEV) if depth else None
    a = torch.full((H, W), 7.0, device=DEV) if alpha else None
    r.render_maps(d, a, mode=mode)
    r.ctx.synchronize()
    return (None if d is None else d.cpu().numpy()), (None if a is None else a.cpu().numpy())


def _assert_maps(got, ref, tag):
    for name, g, e in (("depth", got[0], ref[0]), ("alpha", got[1], ref[1])):
        assert g.dtype == e.dtype == np.float32 and g.shape == e.shape
        assert np.array_equal(g, e), (f"{tag} {name}: {int((g != e).sum())} of {g.size} pixels differ from the oracle, max |diff| "
                                      f"{np.abs(g.astype(np.float64) - e).max():.3e}")


def _d(a):
    return None if a is None else dev(a)


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("mode", maps_ref.MODES)
def test_forward_crowd(lcgs, oracle, mode):
    f = _frame(oracle, "crowd")
    depth, alpha, st = f.maps(mode)
    lens = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    # a milder scene cannot replace the crowd unnoticed: several rounds, a saturated and an empty pixel
    assert lens.max() > 512 and (st["final_T"] < 1e-3).any() and (st["n_contrib"] == 0).any(), lens
    r, _, img = f.renderer()
    _assert_maps(_maps(r, f.H, f.W, mode), (depth, alpha), f"crowd {mode}")
    assert np.array_equal(img.cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])  # the colour frame is untouched


@pytest.mark.parametrize("seed", FORWARD_SEEDS)
def test_forward_random_draws(lcgs, oracle, seed):
    f = _frame(oracle, seed)
    r, _, _ = f.renderer()
    for mode in maps_ref.MODES:
        _assert_maps(_maps(r, f.H, f.W, mode), f.maps(mode)[:2], f"seed {seed} {mode}")


def test_forward_scene_in_spatial_order(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r = L.Renderer(L.Context(0))
    r.upload_scene(f.scene)  # context-owned, along a Morton curve
    assert r.permutation() is not None
    f.render(r)
    for mode in maps_ref.MODES:
        _assert_maps(_maps(r, f.H, f.W, mode), f.maps(mode)[:2], f"spatial order {mode}")


def test_forward_each_output_alone(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _, _ = f.renderer()
    for mode in maps_ref.MODES:
        depth, alpha, _ = f.maps(mode)
        d, none = _maps(r, f.H, f.W, mode, alpha=False)
        assert none is None and np.array_equal(d, depth), mode
        none, a = _maps(r, f.H, f.W, mode, depth=False)
        assert none is None and np.array_equal(a, alpha), mode


def test_forward_frame_that_draws_nothing(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer(keep=False)
    img = torch.full((3, f.H, f.W), -1.0, device=DEV)
    cam = L.get_lookat_cam(*AWAY, width=f.W, height=f.H)
    assert r.forward(cam, img, bg=f.bg, keep_state=True, sync=True) == 0
    for mode in maps_ref.MODES:
        d, a = _maps(r, f.H, f.W, mode)
        assert np.all(d == 0) and np.all(a == 0), mode
    assert bool((img == -1.0).all())  # the colour buffer keeps its poison; the maps are written
    # ... and its backward writes exact zeros
    g = sevens(f.scene)
    r.backward_maps(None, dev(f.gd), dev(f.ga), *[g[k] for k in KEYS])
    r.ctx.synchronize()
    assert all(bool((g[k] == 0).all()) for k in KEYS)


# ----------------------------------------------------------------------------------------------------------------- backward
def _backward(r, f, variant, mode, g=None, accumulate=False):
    g = g if g is not None else sevens(f.scene)
    gi, gd, ga = f.incoming(variant)
    r.backward_maps(_d(gi), _d(gd), _d(ga), *[g[k] for k in KEYS], mode=mode, accumulate=accumulate)
    r.ctx.synchronize()
    return g


@pytest.mark.parametrize("mode", maps_ref.MODES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("key", BACKWARD_FRAMES)
def test_backward_rows(lcgs, oracle, key, variant, mode):
    f = _frame(oracle, key)
    r, _, _ = f.renderer()
    g = _backward(r, f, variant, mode)  # onto arrays pre-filled with 7
    check_gradient_rows(g, None, None, None, bound=f.bound(variant, mode), tag=f"{key} {variant} {mode}")
    if variant != "both+img":  # no image gradient: nothing reaches the colours
        assert bool((g["sh"] == 0).all())


def test_backward_overwrites_and_leaves_exact_zeros_off_screen(lcgs, oracle):
    def make():
        scene = make_scene(np.random.default_rng(23), 2000, spread=0.4, log_scale=(-3.4, 0.5))
        scene["pos"][500:900] += 100.0  # off screen
        return View(oracle, scene, ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1]), 101, 75, seed=4)
    v = cached(("maps", "offscreen"), make)
    assert not v.on[500:900].any() and v.V >= 500
    r = L.Renderer(L.Context(0))
    d = upload_scene(v.scene)
    r.bind_scene(*[d[k] for k in KEYS])
    img = torch.zeros(3, v.H, v.W, device=DEV)
    r.forward(v.cam(), img, bg=v.bg, keep_state=True, sync=True)
    rows = v.survivors(r)
    off = np.ones(v.P, bool)
    off[rows] = False
    assert off[500:900].all()
    rng = np.random.default_rng(5)
    gd, ga = (rng.normal(size=(v.H, v.W)).astype(np.float32) for _ in range(2))
    for mode in maps_ref.MODES:
        g = sevens(v.scene)
        r.backward_maps(None, dev(gd), dev(ga), *[g[k] for k in KEYS], mode=mode)
        r.ctx.synchronize()
        for k in KEYS:
            a = g[k].cpu().numpy().reshape(v.P, -1)
            assert np.all(a[off] == 0), (mode, k)
        assert bool((g["sh"] == 0).all()) and bool((g["pos"] != 7.0).all())
        check_gradient_rows(g, None, None, None, bound=maps_ref.row_bound(v.scene, v.ocam, gd, ga, mode), tag=f"off screen {mode}")


@pytest.mark.parametrize("mode", maps_ref.MODES)
def test_backward_accumulates_over_two_views(lcgs, oracle, mode):
    f0, f1 = _frame(oracle, "crowd"), _frame(oracle, "crowd", POSE2)
    assert not np.array_equal(f0.maps(mode)[0], f1.maps(mode)[0])
    r, _, _ = f0.renderer()
    g = _backward(r, f0, "both+img", mode)
    f1.render(r)
    _backward(r, f1, "both", mode, g=g, accumulate=True)
    bound = maps_ref.sum_row_bounds([f0.bound("both+img", mode), f1.bound("both", mode)])
    check_gradient_rows(g, None, None, None, bound=bound, tag=f"two views {mode}")


def test_plain_backward_after_a_maps_backward(lcgs, oracle):
    scene, pose, W, H = maps_ref.crowd()
    v = cached(("maps", "crowd view"), lambda: View(oracle, scene, pose, W, H, seed=2))
    f = _frame(oracle, "crowd")
    r, _, _ = f.renderer()
    _backward(r, f, "both", "inv_z")
    g = sevens(scene)
    r.backward(dev(v.dL), *[g[k] for k in KEYS])  # the same frame: the maps' sums must not leak into it
    r.ctx.synchronize()
    check_gradient_rows(g, None, None, None, bound=v.bound(), tag="plain backward after maps")
    # ... and a maps backward after it starts from cleared rows again
    check_gradient_rows(_backward(r, f, "depth", "z"), None, None, None, bound=f.bound("depth", "z"), tag="maps after plain")


# ----------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("case", ("direct", "frame between", "depth only"))
def test_autograd(lcgs, oracle, case):
    f = _frame(oracle, "crowd")
    mode = "inv_z" if case == "frame between" else "z"
    r = L.Renderer(L.Context(0))
    t = {k: dev(f.scene[k]).requires_grad_(True) for k in KEYS}
    img, depth, alpha = L.render_autograd_maps(r, f.cam(), *[t[k] for k in KEYS], bg=f.bg, depth_mode=mode)
    assert np.array_equal(depth.detach().cpu().numpy(), f.maps(mode)[0]) and np.array_equal(alpha.detach().cpu().numpy(), f.maps(mode)[1])
    if case == "frame between":  # another view's frame replaces the renderer's state: the backward re-renders its own
        other = torch.zeros(3, f.H, f.W, device=DEV)
        r.forward(L.get_lookat_cam(*POSE2, width=f.W, height=f.H), other, keep_state=True, sync=True)
    if case == "depth only":  # the unused outputs arrive as None: passed as NULL
        (depth * dev(f.gd)).sum().backward()
        variant = "depth"
    else:
        ((img * dev(f.gi)).sum() + (depth * dev(f.gd)).sum() + (alpha * dev(f.ga)).sum()).backward()
        variant = "both+img"
    torch.cuda.synchronize()
    check_gradient_rows({k: t[k].grad for k in KEYS}, None, None, None, bound=f.bound(variant, mode), tag=f"autograd {case}")


# -------------------------------------------------------------------------------------------------------------------- state
def test_state_and_argument_errors(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, d = f.renderer(keep=False)
    g = sevens(f.scene)
    out = torch.zeros(f.H, f.W, device=DEV)

    def refused(status, fn, *a, **kw):
        with pytest.raises(L.LcgsError) as e:
            fn(*a, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))

    grads = [g[k] for k in KEYS]
    # no frame at all, then a frame without kept state
    refused(L.api.LCGS_ERR_STATE, r.render_maps, out, out.clone())
    refused(L.api.LCGS_ERR_STATE, r.backward_maps, None, dev(f.gd), None, *grads)
    img = torch.zeros(3, f.H, f.W, device=DEV)
    r.forward(f.cam(), img, bg=f.bg, keep_state=False, sync=True)
    refused(L.api.LCGS_ERR_STATE, r.render_maps, out, None)
    refused(L.api.LCGS_ERR_STATE, r.backward_maps, None, None, dev(f.ga), *grads)
    # a kept frame: all three gradients NULL is an argument error, and so are two NULL outputs
    f.render(r)
    refused(1, r.backward_maps, None, None, None, *grads)
    refused(1, r.render_maps, None, None)
    r.render_maps(out, None)
    # a frame drawn from received records is not this context's own
    rows, recs = r.owner_project(0, f.cam(), 0, f.P, keep_state=True)
    r.owner_render(f.cam(), rows, recs, img, bg=f.bg, keep_state=True)
    refused(L.api.LCGS_ERR_STATE, r.render_maps, out, None)
    refused(L.api.LCGS_ERR_STATE, r.backward_maps, dev(f.gi), dev(f.gd), dev(f.ga), *grads)
    r.ctx.synchronize()
