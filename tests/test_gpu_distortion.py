"""`-m gpu`: the depth-distortion map of a keep-state frame (lcgs_render_distortion) and its backward
(lcgs_render_backward_distortion), on the frames of test_gpu_maps.py.

Forward: the map equals the f32 oracle's composition bit for bit (tests/distortion_ref.py: the frame's own state composited with
the colour (u, 1, u^2), dist = A M2 - M1 M1), no pixel excluded, in both depth modes, about 0 and about the crowd's mean view
depth -- the crowd, eight random draws, a context-owned scene in spatial order, an antialiased frame, a frame that draws nothing.
Backward: every component of every row inside distortion_ref's bound (gpu_util.check_gradient_rows' formula and constants), no
row excluded -- the distortion channel alone, with depth and alpha, with an image gradient as well; accumulation over two views;
exact zeros; a NULL distortion gradient; the plain backward afterwards; the camera gradient and the densification statistics
behind it; the autograd wrapper; state and argument errors."""
import numpy as np
import pytest
import torch

import luisacomputegaussiansplatting_amd as L
import antialias_ref
import distortion_ref
import maps_ref
from conftest import make_scene
from gpu_util import DEV, KEYS, View, cached, check_gradient_rows, dev, sevens, upload_scene
from test_gpu_maps import AWAY, POSE2, _frame

pytestmark = pytest.mark.gpu
CROWD_DEPTH = 1.6665548  # the mean view z of the crowd's splats from its pose, a binary32 number
CENTERS = (0.0, CROWD_DEPTH)
FORWARD_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
BACKWARD_FRAMES = ("crowd", 100, 101, 102, 103)
VARIANTS = ("dist", "dist+maps", "all")  # the distortion channel alone; with depth and alpha; with an image gradient as well
MAPS_VARIANT = {"dist+maps": "both", "all": "both+img"}  # what test_gpu_maps.py calls the rest of the call


class DFrame:
    """a frame of test_gpu_maps.py (shared with it: its maps, incoming gradients and bounds are computed once) with the
    distortion map's incoming gradient, references and bounds"""

    def __init__(self, oracle, key, pose=None):
        self.f = _frame(oracle, key, pose)
        self.gq = np.random.default_rng(29).normal(size=(self.f.H, self.f.W)).astype(np.float32)
        self._dist, self._bounds = {}, {}

    def dist(self, mode, center):
        """(dist, forward state) of the f32 oracle"""
        if (mode, center) not in self._dist:
            f = self.f
            self._dist[mode, center] = distortion_ref.forward(f.oracle, f.scene, f.ocam, mode, center, scale_modifier=f.sm)
        return self._dist[mode, center]

    def incoming(self, variant):
        """(dL_dimg, dL_ddepth, dL_dalpha, dL_ddist); None = NULL"""
        return ((None, None, None) if variant == "dist" else self.f.incoming(MAPS_VARIANT[variant])) + (self.gq,)

    def bound(self, variant, mode, center):
        f = self.f
        if ("dist", mode, center) not in self._bounds:
            self._bounds["dist", mode, center] = distortion_ref.row_bound(f.scene, f.ocam, self.gq, mode=mode, center=center,
                                                                          scale_modifier=f.sm)
        if (variant, mode, center) not in self._bounds:
            self._bounds[variant, mode, center] = distortion_ref.sum_row_bounds(
                [self._bounds["dist", mode, center], f.bound(MAPS_VARIANT[variant], mode)])
        return self._bounds[variant, mode, center]


def _dframe(oracle, key, pose=None):
    return cached(("distortion", key, str(pose)), lambda: DFrame(oracle, key, pose))


def _dist(r, H, W, mode, center):
    out = torch.full((H, W), 7.0, device=DEV)
    r.render_distortion(out, mode=mode, center=center)
    r.ctx.synchronize()
    return out.cpu().numpy()


def _assert_dist(got, ref, tag):
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got, ref), (f"{tag}: {int((got != ref).sum())} of {got.size} pixels differ from the oracle, max |diff| "
                                      f"{np.abs(got.astype(np.float64) - ref).max():.3e}")


def _d(a):
    return None if a is None else dev(a)


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("center", CENTERS)
@pytest.mark.parametrize("mode", distortion_ref.MODES)
def test_forward_crowd(lcgs, oracle, mode, center):
    df = _dframe(oracle, "crowd")
    f = df.f
    ref, st = df.dist(mode, center)
    lens = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    # a milder scene cannot replace the crowd unnoticed: a list of more than two rounds, spread-out and empty pixels
    assert lens.max() > 512 and (ref > 0).any() and (st["n_contrib"] == 0).any(), lens
    assert ref.max() > 1e-3 and np.all(ref[st["n_contrib"] == 0] == 0)
    r, _, img = f.renderer()
    _assert_dist(_dist(r, f.H, f.W, mode, center), ref, f"crowd {mode} {center}")
    assert np.array_equal(img.cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])  # the colour frame is untouched


@pytest.mark.parametrize("seed", FORWARD_SEEDS)
def test_forward_random_draws(lcgs, oracle, seed):
    df = _dframe(oracle, seed)
    r, _, _ = df.f.renderer()
    for mode in distortion_ref.MODES:
        for center in CENTERS:
            _assert_dist(_dist(r, df.f.H, df.f.W, mode, center), df.dist(mode, center)[0], f"seed {seed} {mode} {center}")


def test_forward_scene_in_spatial_order(lcgs, oracle):
    df = _dframe(oracle, "crowd")
    f = df.f
    r = L.Renderer(L.Context(0))
    r.upload_scene(f.scene)  # context-owned, along a Morton curve
    assert r.permutation() is not None
    f.render(r)
    for mode in distortion_ref.MODES:
        for center in CENTERS:
            _assert_dist(_dist(r, f.H, f.W, mode, center), df.dist(mode, center)[0], f"spatial order {mode} {center}")


def test_forward_antialiased_frame(lcgs, oracle):
    df = _dframe(oracle, "crowd")
    f = df.f
    st = cached(("distortion", "crowd antialiased"), lambda: antialias_ref.forward_state(oracle, f.scene, f.ocam))
    r = L.Renderer(L.Context(0))
    d = upload_scene(f.scene)
    r.bind_scene(*[d[k] for k in KEYS])
    r.set_raster_mode("antialiased")
    img = torch.zeros(3, f.H, f.W, device=DEV)
    assert r.forward(f.cam(), img, keep_state=True, sync=True) == st["num_rendered"] > 0
    for mode in distortion_ref.MODES:
        v = maps_ref._value(oracle, f.scene, f.ocam, mode, 1.0)[0]
        for center in CENTERS:
            ref = distortion_ref.compose(oracle, st, f.ocam, v, center)[0]
            assert not np.array_equal(ref, df.dist(mode, center)[0])  # (the compensated opacity: another map)
            _assert_dist(_dist(r, f.H, f.W, mode, center), ref, f"antialiased {mode} {center}")


def test_forward_frame_that_draws_nothing(lcgs, oracle):
    df = _dframe(oracle, "crowd")
    f = df.f
    r, _ = f.renderer(keep=False)
    img = torch.full((3, f.H, f.W), -1.0, device=DEV)
    cam = L.get_lookat_cam(*AWAY, width=f.W, height=f.H)
    assert r.forward(cam, img, bg=f.bg, keep_state=True, sync=True) == 0
    for mode in distortion_ref.MODES:
        for center in CENTERS:
            assert np.all(_dist(r, f.H, f.W, mode, center) == 0), (mode, center)
    assert bool((img == -1.0).all())  # the colour buffer keeps its poison; the map is written
    # ... and its backward writes exact zeros
    g = sevens(f.scene)
    r.backward_distortion(None, None, None, dev(df.gq), *[g[k] for k in KEYS], center=CROWD_DEPTH)
    r.ctx.synchronize()
    assert all(bool((g[k] == 0).all()) for k in KEYS)


# ----------------------------------------------------------------------------------------------------------------- backward
def _backward(r, df, variant, mode, center, g=None, accumulate=False):
    g = g if g is not None else sevens(df.f.scene)
    r.backward_distortion(*[_d(a) for a in df.incoming(variant)], *[g[k] for k in KEYS], mode=mode, center=center,
                          accumulate=accumulate)
    r.ctx.synchronize()
    return g


@pytest.mark.parametrize("center", CENTERS)
@pytest.mark.parametrize("mode", distortion_ref.MODES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("key", BACKWARD_FRAMES)
def test_backward_rows(lcgs, oracle, key, variant, mode, center):
    df = _dframe(oracle, key)
    r, _, _ = df.f.renderer()
    g = _backward(r, df, variant, mode, center)  # onto arrays pre-filled with 7, without a preceding lcgs_render_distortion
    check_gradient_rows(g, None, None, None, bound=df.bound(variant, mode, center), tag=f"{key} {variant} {mode} {center}")
    if variant != "all":  # no image gradient: nothing reaches the colours
        assert bool((g["sh"] == 0).all())


def test_backward_overwrites_and_leaves_exact_zeros_off_screen(lcgs, oracle):
    def make():
        scene = make_scene(np.random.default_rng(23), 2000, spread=0.4, log_scale=(-3.4, 0.5))
        scene["pos"][500:900] += 100.0  # off screen
        return View(oracle, scene, ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1]), 101, 75, seed=4)
    v = cached(("distortion", "offscreen"), make)
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
    gq = np.random.default_rng(5).normal(size=(v.H, v.W)).astype(np.float32)
    for mode, center in (("z", 3.75), ("inv_z", 0.0)):
        g = sevens(v.scene)
        r.backward_distortion(None, None, None, dev(gq), *[g[k] for k in KEYS], mode=mode, center=center)
        r.ctx.synchronize()
        for k in KEYS:
            a = g[k].cpu().numpy().reshape(v.P, -1)
            assert np.all(a[off] == 0), (mode, k)
        assert bool((g["sh"] == 0).all()) and bool((g["pos"] != 7.0).all())
        check_gradient_rows(g, None, None, None, bound=distortion_ref.row_bound(v.scene, v.ocam, gq, mode=mode, center=center),
                            tag=f"off screen {mode}")


@pytest.mark.parametrize("mode", distortion_ref.MODES)
def test_backward_accumulates_over_two_views(lcgs, oracle, mode):
    d0, d1 = _dframe(oracle, "crowd"), _dframe(oracle, "crowd", POSE2)
    assert not np.array_equal(d0.dist(mode, 0.0)[0], d1.dist(mode, 0.0)[0])
    r, _, _ = d0.f.renderer()
    g = _backward(r, d0, "all", mode, CROWD_DEPTH)
    d1.f.render(r)
    _backward(r, d1, "dist", mode, 0.0, g=g, accumulate=True)
    bound = distortion_ref.sum_row_bounds([d0.bound("all", mode, CROWD_DEPTH), d1.bound("dist", mode, 0.0)])
    check_gradient_rows(g, None, None, None, bound=bound, tag=f"two views {mode}")


def test_null_distortion_gradient_is_backward_maps(lcgs, oracle):
    """The same launches, so the same rows bit for bit -- where bits are defined.  The maps walk sums an entry's terms over a
    tile with LDS float atomics, one per 16-lane row, and a row's tiles with global float atomics, both in order of arrival:
    0 + a + b does not depend on that order, three terms do (on the crowd two lcgs_render_backward_maps calls differ in the
    last bits of a few rows, measured: 18 of 4500 dL/dpos components).  So the bit-for-bit comparison runs on draw 7, which
    lists no splat on more than two tiles, with incoming gradients that are zero except on two covered pixels of every tile
    and no image gradient; on the crowd, with full gradients and an image gradient, the call is held to backward_maps' bound."""
    df = _dframe(oracle, 7)
    f = df.f
    st = f.maps("z")[2]
    lists = np.bincount(st["point_list"], minlength=f.P)
    assert lists.max() == 2 and (lists > 0).sum() >= 16, lists.max()
    keep = np.zeros((f.H, f.W), bool)
    for ty in range(0, f.H, 16):
        for tx in range(0, f.W, 16):
            ys, xs = np.nonzero(st["n_contrib"][ty:ty + 16, tx:tx + 16])
            for j in {0, len(ys) - 1} if len(ys) else ():
                keep[ty + ys[j], tx + xs[j]] = True
    assert keep.sum() >= 12
    r, _, _ = f.renderer()
    for variant in ("both", "depth", "alpha"):
        gi, gd, ga = f.incoming(variant)
        assert gi is None
        gd, ga = (None if x is None else np.where(keep, x, np.float32(0.0)) for x in (gd, ga))
        a, b = sevens(f.scene), sevens(f.scene)
        r.backward_maps(None, _d(gd), _d(ga), *[a[k] for k in KEYS], mode="inv_z")
        r.backward_distortion(None, _d(gd), _d(ga), None, *[b[k] for k in KEYS], mode="inv_z", center=CROWD_DEPTH)
        r.ctx.synchronize()
        assert int((a["opacity"] != 0).sum()) >= 8
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (variant, k, int((a[k] != b[k]).sum()))
    df = _dframe(oracle, "crowd")
    f = df.f
    r, _, _ = f.renderer()
    for variant, mode in (("both+img", "inv_z"), ("both", "z")):
        gi, gd, ga = f.incoming(variant)
        g = sevens(f.scene)
        r.backward_distortion(_d(gi), _d(gd), _d(ga), None, *[g[k] for k in KEYS], mode=mode, center=CROWD_DEPTH)
        r.ctx.synchronize()
        check_gradient_rows(g, None, None, None, bound=f.bound(variant, mode), tag=f"NULL distortion gradient, crowd {variant} {mode}")


def test_plain_backward_after_a_distortion_backward(lcgs, oracle):
    scene, pose, W, H = maps_ref.crowd()
    v = cached(("maps", "crowd view"), lambda: View(oracle, scene, pose, W, H, seed=2))
    df = _dframe(oracle, "crowd")
    r, _, _ = df.f.renderer()
    _backward(r, df, "dist+maps", "inv_z", CROWD_DEPTH)
    g = sevens(scene)
    r.backward(dev(v.dL), *[g[k] for k in KEYS])  # the same frame: the distortion channel's sums must not leak into it
    r.ctx.synchronize()
    check_gradient_rows(g, None, None, None, bound=v.bound(), tag="plain backward after distortion")
    # ... and a distortion backward after it starts from cleared rows again
    check_gradient_rows(_backward(r, df, "dist", "z", 0.0), None, None, None, bound=df.bound("dist", "z", 0.0),
                        tag="distortion after plain")


@pytest.mark.parametrize("mode", distortion_ref.MODES)
def test_camera_gradient_and_densify_statistics_behind_a_distortion_backward(lcgs, oracle, mode):
    df = _dframe(oracle, "crowd")
    f = df.f
    r, _, _ = f.renderer()
    g = _backward(r, df, "dist", mode, CROWD_DEPTH)  # the value slot's mode is set by the distortion channel alone
    out = torch.full((12,), 7.0, device=DEV)
    r.camera_backward(out)
    r.ctx.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    # the position numbers are minus the column sums of dL/dpos, to the column sums of the rows' own bounds
    B, _ = df.bound("dist", mode, CROWD_DEPTH)
    want = -g["pos"].double().sum(dim=0).cpu().numpy()
    tol = B["pos"].astype(np.float64).sum(axis=0)
    print(f"[distortion camera] {mode}: |got - want| / bound", np.array2string(np.abs(got[0:3] - want) / tol, precision=3))
    assert np.abs(want).max() > 0 and (np.abs(got[0:3] - want) <= tol).all(), (got[0:3], want, tol)
    # lcgs_densify_accumulate counts the frame on exactly its on-screen rows
    stats = {"grad_accum": torch.zeros(f.P, device=DEV), "denom": torch.zeros(f.P, dtype=torch.int32, device=DEV),
             "max_radii": torch.zeros(f.P, dtype=torch.int32, device=DEV)}
    r.densify_accumulate(stats)
    r.ctx.synchronize()
    on = torch.zeros(f.P, dtype=torch.bool, device=DEV)
    on[r.visible_rows().long()] = True
    assert 0 < int(on.sum()) and torch.equal(stats["denom"] == 1, on) and bool((stats["denom"][~on] == 0).all())
    assert bool((stats["grad_accum"][~on] == 0).all()) and bool((stats["grad_accum"][on] > 0).any())


# ----------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("case", ("direct", "frame between"))
def test_autograd(lcgs, oracle, case):
    df = _dframe(oracle, "crowd")
    f = df.f
    mode, center = ("inv_z", 0.0) if case == "frame between" else ("z", CROWD_DEPTH)
    r = L.Renderer(L.Context(0))
    t = {k: dev(f.scene[k]).requires_grad_(True) for k in KEYS}
    img, depth, alpha, dist = L.render_autograd_distortion(r, f.cam(), *[t[k] for k in KEYS], bg=f.bg, depth_mode=mode, center=center)
    assert np.array_equal(depth.detach().cpu().numpy(), f.maps(mode)[0]) and np.array_equal(alpha.detach().cpu().numpy(), f.maps(mode)[1])
    assert np.array_equal(dist.detach().cpu().numpy(), df.dist(mode, center)[0])
    assert np.array_equal(img.detach().cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])
    if case == "frame between":  # another view's frame replaces the renderer's state: the backward re-renders its own
        other = torch.zeros(3, f.H, f.W, device=DEV)
        r.forward(L.get_lookat_cam(*POSE2, width=f.W, height=f.H), other, keep_state=True, sync=True)
        (dist * dev(df.gq)).sum().backward()  # the unused outputs arrive as None: passed as NULL
        variant = "dist"
    else:
        ((img * dev(f.gi)).sum() + (depth * dev(f.gd)).sum() + (alpha * dev(f.ga)).sum() + (dist * dev(df.gq)).sum()).backward()
        variant = "all"
    torch.cuda.synchronize()
    check_gradient_rows({k: t[k].grad for k in KEYS}, None, None, None, bound=df.bound(variant, mode, center), tag=f"autograd {case}")


# -------------------------------------------------------------------------------------------------------------------- state
def test_state_and_argument_errors(lcgs, oracle):
    df = _dframe(oracle, "crowd")
    f = df.f
    r, d = f.renderer(keep=False)
    g = sevens(f.scene)
    out = torch.zeros(f.H, f.W, device=DEV)

    def refused(status, fn, *a, **kw):
        with pytest.raises(L.LcgsError) as e:
            fn(*a, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))

    grads = [g[k] for k in KEYS]
    # no frame at all, then a frame without kept state
    refused(L.api.LCGS_ERR_STATE, r.render_distortion, out)
    refused(L.api.LCGS_ERR_STATE, r.backward_distortion, None, None, None, dev(df.gq), *grads)
    img = torch.zeros(3, f.H, f.W, device=DEV)
    r.forward(f.cam(), img, bg=f.bg, keep_state=False, sync=True)
    refused(L.api.LCGS_ERR_STATE, r.render_distortion, out, center=CROWD_DEPTH)
    refused(L.api.LCGS_ERR_STATE, r.backward_distortion, None, dev(f.gd), None, dev(df.gq), *grads)
    # a kept frame: all four gradients NULL is an argument error, and so are a NULL output and a centre that is not finite
    f.render(r)
    refused(1, r.backward_distortion, None, None, None, None, *grads)
    refused(1, r.render_distortion, None)
    refused(1, r.render_distortion, out, center=float("nan"))
    refused(1, r.backward_distortion, None, None, None, dev(df.gq), *grads, center=float("inf"))
    r.render_distortion(out)
    # a frame drawn from received records is not this context's own
    rows, recs = r.owner_project(0, f.cam(), 0, f.P, keep_state=True)
    r.owner_render(f.cam(), rows, recs, img, bg=f.bg, keep_state=True)
    refused(L.api.LCGS_ERR_STATE, r.render_distortion, out)
    refused(L.api.LCGS_ERR_STATE, r.backward_distortion, dev(f.gi), dev(f.gd), dev(f.ga), dev(df.gq), *grads)
    r.ctx.synchronize()
