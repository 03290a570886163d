"""`-m gpu`: the antialiased raster mode's gradients held ROW BY ROW -- every component of every row against the f64 reference
within tests/antialias_ref.py's bound (gpu_util.check_gradient_rows' formula and constants, carried through the mode's
augmentation; tests/test_antialias_ref.py proves it on the CPU) -- on every route and in every kernel instantiation the mode has:

  dense, compact and autograd on draws 123, 121, 113, 127, the sub-pixel crowd and the needle crowd;
  k_preprocess_backward<true> (degrees 0, 1, 2; degree 3 with dL_dsh one float past a 16-byte boundary), survivor counts at wave
  and block boundaries, the sliced launch (LCGS_GRAD_SLICES), an under-hinted grid, the profiling path;
  the depth, alpha and distortion channels of lcgs_render_backward_maps / lcgs_render_backward_distortion on an antialiased frame,
  accumulated over two views and through the autograd wrappers;
  the camera gradient, with and without the kept Jacobian (k_camera_grad<true, true> / <false, true>), held to
  antialias_ref.camera_bound;
  rows whose compensation is 0 (rank-1 covariances);
  lcgs_densify_accumulate behind an antialiased maps backward.

Every gradient array starts at 7.0; no row is excluded; sums of views are held to the sum of the views' bounds; every frame is
first asserted bit-identical to the reference state.  Each (scene, pose, gradient) computes its references and bounds once."""
import numpy as np
import pytest
import torch

import luisacomputegaussiansplatting_amd as L
import antialias_ref
import distortion_ref
import maps_ref
from conftest import make_scene
from gpu_util import (BG, DEV, GRAD_ROW_CU, GRAD_ROW_K, KEYS, U32, _oracles, assert_image_parity, cached, check_gradient_rows,
                      dev, random_draw, sevens)
from test_gpu_backward_paths import FEW_POSE, POSE, POSE2, slice_counts
from test_gpu_distortion import CROWD_DEPTH
from test_gpu_maps import POSE2 as CROWD_POSE2

pytestmark = pytest.mark.gpu
DRAWS = (123, 121, 113, 127)
CROWDS = ("sub-pixel crowd", "needle crowd")
MAP_FRAMES = CROWDS + (121, 127)
MAP_VARIANTS = ("depth", "alpha", "both", "both+img")
DIST_VARIANTS = ("dist", "dist+maps", "all")
CENTERS = (0.0, CROWD_DEPTH)  # 0 and the crowd's mean view depth


def _d(a):
    return None if a is None else dev(a)


class AFrame:
    """One (scene, pose, resolution, fov, background, scale modifier, degree) under the mode: the reference state, the incoming
    gradients, and the references and bounds of every call, each computed once and left unchanged"""

    def __init__(self, scene, pose, W, H, fov=None, bg=BG, sm=1.0, sh_deg=3, dL=None, seed=0):
        o32, o64, _ = _oracles()
        self.scene, self.pose, self.W, self.H, self.fov, self.bg, self.sm, self.sh_deg = scene, pose, W, H, fov, bg, sm, sh_deg
        self.P = scene["pos"].shape[0]
        self.ocam = o32.lookat(*pose, width=W, height=H, fov=fov)
        self.cam64 = o64.lookat(*pose, width=W, height=H, fov=fov)
        self.kw = dict(bg=bg, scale_modifier=sm, sh_deg=sh_deg)
        self.state = antialias_ref.forward_state(o32, scene, self.ocam, **self.kw)
        m2, depth, cov = o32.project(scene["pos"], scene["scale"], scene["rotq"], self.ocam, scale_modifier=sm)
        self.on = o32.allocate_tiles(W, H, depth, m2, cov)[2] > 0  # (gpu_util.View.on)
        self.dL = dL if dL is not None else np.random.default_rng(seed).normal(size=(3, H, W)).astype(np.float32)
        rng = np.random.default_rng(17)
        self.gd, self.ga, self.gq = (rng.normal(size=(H, W)).astype(np.float32) for _ in range(3))
        self._c = {}

    def _once(self, key, make):
        if key not in self._c:
            self._c[key] = make()
        return self._c[key]

    def cam(self):
        return L.get_lookat_cam(*self.pose, width=self.W, height=self.H, fov=self.fov)

    @property
    def hit(self):
        """rows that reach a pixel of the reference frame (gpu_util.View.hit)"""
        def make():
            g = antialias_ref.gradients(_oracles()[0], self.scene, self.ocam, self.dL, **self.kw)[0]
            return (g["opacity"] != 0) | (g["sh"].reshape(self.P, -1) != 0).any(axis=1)
        return self._once("hit", make)

    # ---- bounds: (B, ref64) each
    def bound(self):
        return self._once("image", lambda: antialias_ref.row_bound(self.scene, self.ocam, self.dL, cam64=self.cam64, **self.kw))

    def incoming(self, variant):
        """(dL_dimg, dL_ddepth, dL_dalpha) of a maps variant; None = NULL"""
        return (self.dL if variant == "both+img" else None, None if variant == "alpha" else self.gd,
                None if variant == "depth" else self.ga)

    def maps_bound(self, variant, mode):
        if variant == "both+img":
            return self._once((variant, mode), lambda: antialias_ref.sum_row_bounds([self.maps_bound("both", mode), self.bound()]))
        _, gd, ga = self.incoming(variant)
        return self._once((variant, mode), lambda: antialias_ref.maps_row_bound(self.scene, self.ocam, gd, ga, mode, self.sm,
                                                                                self.sh_deg))

    def dist_incoming(self, variant):
        """(dL_dimg, dL_ddepth, dL_dalpha, dL_ddist)"""
        return ((None, None, None) if variant == "dist" else self.incoming({"dist+maps": "both", "all": "both+img"}[variant])) + \
            (self.gq,)

    def dist_bound(self, variant, mode, center):
        if variant == "dist":
            return self._once((variant, mode, center), lambda: antialias_ref.distortion_row_bound(
                self.scene, self.ocam, self.gq, mode=mode, center=center, scale_modifier=self.sm, sh_deg=self.sh_deg))
        rest = self.maps_bound({"dist+maps": "both", "all": "both+img"}[variant], mode)
        return self._once((variant, mode, center),
                          lambda: antialias_ref.sum_row_bounds([self.dist_bound("dist", mode, center), rest]))

    # ---- the device side
    def renderer(self, scene=None):
        r = L.Renderer(L.Context(0))
        d = {k: dev((scene or self.scene)[k]) for k in KEYS}
        r.bind_scene(*[d[k] for k in KEYS], sh_degree=self.sh_deg)
        r.set_raster_mode("antialiased")
        return r, d

    def render(self, r, sync=True, count=True):
        """the kept frame, asserted bit-identical to the reference state (an asynchronous frame: see `parity`)"""
        img = torch.full((3, self.H, self.W), -1.0, device=DEV)
        n = r.forward(self.cam(), img, bg=self.bg, scale_modifier=self.sm, keep_state=True, sync=sync)
        if sync:
            assert n > 0 and (not count or n == self.state["num_rendered"]), (n, self.state["num_rendered"])
            self.parity(img)
        return img

    def parity(self, img):
        assert_image_parity(img.cpu().numpy(), self.state)

    def survivors(self, r):
        """the frame's on-screen rows, between `hit` and `on` (gpu_util.View.survivors)"""
        rows = r.visible_rows().cpu().numpy()
        assert r.frame_stats()["num_visible"] == rows.size
        got = np.zeros(self.P, bool)
        got[rows] = True
        assert (rows[1:] > rows[:-1]).all() and not (got & ~self.on).any() and not (self.hit & ~got).any(), \
            (rows.size, int(self.on.sum()), int(self.hit.sum()))
        return rows


def _low_degree(scene, deg):
    scene = dict(scene)
    scene["sh"] = np.ascontiguousarray(scene["sh"][:, :(deg + 1) ** 2 * 3])
    return scene


def _frame(key, deg=3):
    def make():
        if key in CROWDS or key == "rank-1":
            scene, pose, W, H = {"sub-pixel crowd": antialias_ref.subpixel_crowd, "needle crowd": antialias_ref.needle_crowd,
                                 "rank-1": antialias_ref.rank1_crowd}[key]()
            return AFrame(_low_degree(scene, deg), pose, W, H, sh_deg=deg, seed=2)
        rng, scene, W, H, pose, fov, bg, sm = random_draw(key)
        dL = rng.normal(size=(3, H, W)).astype(np.float32)  # (test_gpu_antialias.py's Draw)
        return AFrame(_low_degree(scene, deg), pose, W, H, fov, bg, sm, sh_deg=deg, dL=dL)
    return cached(("antialias rows", key, deg), make)


def _rows(g, bound, tag, rows=None):
    return check_gradient_rows(g, None, None, None, bound=bound, rows=rows, tag=f"antialiased | {tag}")


def _exact_zeros(g, f, rows, tag):
    """rows the frame did not keep: written, and exactly 0"""
    off = np.ones(f.P, bool)
    off[rows] = False
    for k in KEYS:
        a = g[k].cpu().numpy().reshape(f.P, -1)
        assert np.all(a[off] == 0), (tag, k)


def _dense(r, f, tag, sh_offset=0, bound=None, g=None, **kw):
    g = g if g is not None else sevens(f.scene, sh_offset)
    r.backward(dev(f.dL), *[g[k] for k in KEYS], **kw)
    r.ctx.synchronize()
    rows = f.survivors(r)
    _rows(g, bound if bound is not None else f.bound(), f"{tag} dense")
    if not kw.get("accumulate"):
        _exact_zeros(g, f, rows, tag)
    return g, rows


def _compact(r, f, tag, sh_offset=0):
    rows = f.survivors(r)
    g = sevens(f.scene, sh_offset)
    r.backward(dev(f.dL), *[g[k] for k in KEYS], compact=True)
    r.ctx.synchronize()
    V = rows.size
    _rows({k: g[k].reshape(f.P, -1)[:V] for k in KEYS}, f.bound(), f"{tag} compact", rows=rows)
    assert all((g[k].reshape(f.P, -1)[V:] == 7.0).all() for k in KEYS)  # nothing written past row V
    return g


# ------------------------------------------------------------------------------------------------ dense, compact and autograd
@pytest.mark.parametrize("key", DRAWS + CROWDS)
def test_dense_and_compact_rows(lcgs, key):
    f = _frame(key)
    r, _ = f.renderer()
    f.render(r)
    _dense(r, f, f"routes | {key}")
    _compact(r, f, f"routes | {key}")


@pytest.mark.parametrize("key", DRAWS + CROWDS)
def test_autograd_rows(lcgs, key):
    f = _frame(key)
    r, d = f.renderer()
    leaves = [d[k].clone().requires_grad_(True) for k in KEYS]
    img = L.render_autograd(r, f.cam(), *leaves, bg=f.bg, scale_modifier=f.sm)
    f.parity(img.detach())
    (img * dev(f.dL)).sum().backward()
    torch.cuda.synchronize()
    _rows({k: t.grad for k, t in zip(KEYS, leaves)}, f.bound(), f"routes | {key} autograd")


# --------------------------------------------------------------------------------------------- the rows kernel in the mode
@pytest.mark.parametrize("deg", [0, 1, 2])
def test_low_degrees(lcgs, deg):
    """k_preprocess_backward<true>: no kept colour Jacobian below degree 3"""
    f = _frame("sub-pixel crowd", deg)
    r, _ = f.renderer()
    f.render(r)
    _dense(r, f, f"rows kernel | degree {deg}")
    _compact(r, f, f"rows kernel | degree {deg}")


def test_unaligned_sh_gradient(lcgs):
    """degree 3 with dL_dsh one float past a 16-byte boundary: k_preprocess_backward<true>, lane-wise SH rows"""
    f = _frame("sub-pixel crowd")
    r, _ = f.renderer()
    f.render(r)
    _dense(r, f, "rows kernel | unaligned dL_dsh", sh_offset=1)
    _compact(r, f, "rows kernel | unaligned dL_dsh", sh_offset=1)


def boundary_premise(V, deg=3):
    """test_gpu_backward_paths.py's case D under the mode: P = 1000 at 96 x 80 with exactly V rows on screen -- V of the rows
    that reach a pixel of the full scene's ANTIALIASED frame, every other row moved off screen"""
    def make():
        rng = np.random.default_rng(400)
        scene = _low_degree(make_scene(rng, 1000, spread=0.25, log_scale=(-3.5, 0.7)), deg)
        shown = np.nonzero(AFrame(dict(scene), POSE, 96, 80, sh_deg=deg, seed=8).hit)[0]
        assert shown.size >= V, shown.size
        keep = np.sort(rng.choice(shown, V, replace=False))
        off = np.ones(1000, bool)
        off[keep] = False
        scene["pos"] = scene["pos"].copy()
        scene["pos"][off] += 100.0
        f = AFrame(scene, POSE, 96, 80, sh_deg=deg, seed=8)
        assert int(f.on.sum()) == V and np.array_equal(np.nonzero(f.on)[0], keep) and np.array_equal(f.hit, f.on)
        assert (f.state["rho"][keep] < 0.9).sum() >= min(V, 8) // 2
        return f
    return cached(("antialias rows", "boundary", V, deg), make)


def _boundary(V, deg, tag, sh_offset=0):
    f = boundary_premise(V, deg)
    r, _ = f.renderer()
    f.render(r)
    _, rows = _dense(r, f, f"boundaries | V={V} {tag}", sh_offset=sh_offset)
    assert rows.size == V == r.frame_stats()["num_visible"]
    _compact(r, f, f"boundaries | V={V} {tag}", sh_offset=sh_offset)


@pytest.mark.parametrize("V", [1, 63, 64, 65, 255, 256, 257])
def test_survivor_counts_at_wave_and_block_boundaries(lcgs, V):
    _boundary(V, 3, "degree 3")


@pytest.mark.parametrize("V", [65, 257])
def test_boundary_counts_at_degree_2(lcgs, V):
    _boundary(V, 2, "degree 2")


@pytest.mark.parametrize("V", [65, 257])
def test_boundary_counts_with_an_unaligned_sh_gradient(lcgs, V):
    _boundary(V, 3, "unaligned dL_dsh", sh_offset=1)


# ------------------------------------------------------------------------------------------------------------------ sliced
def sliced_premise():
    """test_gpu_backward_paths.py's P4097 (200 x 150, rows [100, 137) off screen, row 0 on screen) with the scales shrunk so
    that the compensation is at work: at least 30 % of the rows that reach a pixel have rho < 0.5.  Two poses."""
    def make():
        P = 4097
        scene = make_scene(np.random.default_rng(200 + P + 5), P, spread=0.3)
        scene["scale"] *= np.float32(0.3)
        scene["pos"][0], scene["scale"][0], scene["opacity"][0] = [-1.5, -0.25, 1.4], 0.02, 0.6
        scene["pos"][100:137] += 100.0
        f0, f1 = AFrame(scene, POSE, 200, 150, seed=4), AFrame(scene, POSE2, 200, 150, seed=5)
        for f in (f0, f1):
            assert not f.on[100:137].any() and (f.state["rho"][f.hit] < 0.5).mean() >= 0.30, (f.state["rho"][f.hit] < 0.5).mean()
        for rows in (f0.on, f0.hit):
            for K in (2, 4, 16):
                c = slice_counts(rows, P, K)
                assert min(c) > 0 and any(n % 64 for n in c) and rows[0], (K, c)
        assert min(slice_counts(f1.hit, P, 4)) > 0
        return f0, f1
    return cached(("antialias rows", "sliced"), make)


def _comm_renderer(monkeypatch, f, K):
    """test_gpu_backward_paths._comm_renderer's recipe: a world-size-1 communicator that asks for K gradient slices"""
    monkeypatch.setenv("LCGS_GRAD_SLICES", str(K))
    r, _ = f.renderer()
    return r, L.Comm(r.ctx, 0, 1)


@pytest.mark.parametrize("K", [2, 16])
def test_sliced_backward(lcgs, monkeypatch, K):
    f, _ = sliced_premise()
    r, comm = _comm_renderer(monkeypatch, f, K)
    try:
        f.render(r)
        _dense(r, f, f"sliced | {K} slices")
    finally:
        comm.close()


def test_sliced_backward_accumulates_two_views(lcgs, monkeypatch):
    f0, f1 = sliced_premise()
    r, comm = _comm_renderer(monkeypatch, f0, 4)
    try:
        f0.render(r)
        g, _ = _dense(r, f0, "sliced | 4 slices, first view")
        f1.render(r)
        _dense(r, f1, "sliced | 4 slices, two views accumulated", g=g, accumulate=True,
               bound=antialias_ref.sum_row_bounds([f0.bound(), f1.bound()]))
    finally:
        comm.close()


# ------------------------------------------------------------------------------------------------------- an under-hinted grid
def strided_premise():
    """test_gpu_backward_paths.py's case C under the mode: 30 000 splats at 400 x 300, 150 of them in a far cluster"""
    def make():
        rng = np.random.default_rng(300)
        scene = make_scene(rng, 30000)
        scene["pos"][::200] = (rng.normal(0, 0.3, (150, 3)) + np.array(FEW_POSE[1])).astype(np.float32)
        few, many = AFrame(scene, FEW_POSE, 400, 300, seed=6), AFrame(scene, POSE, 400, 300, seed=7)
        V = int(few.on.sum())
        assert few.state["num_rendered"] > 0 and V <= 150, V
        blocks = (V + V // 4 + 4096 + 255) // 256  # the hint the synchronous frame leaves, as blocks of 256 rows
        assert many.hit.sum() > 3 * 256 * blocks, (int(many.hit.sum()), blocks)  # the loops take at least 4 passes
        return few, many
    return cached(("antialias rows", "strided"), make)


@pytest.mark.parametrize("path", ["dense", "compact"])
def test_strided_backward_behind_an_under_hinted_frame(lcgs, path):
    few, many = strided_premise()
    r, _ = many.renderer()
    few.render(r)  # synchronous: sets the launch hint from its handful of survivors
    img = many.render(r, sync=False)  # asynchronous: the hint stays
    if path == "dense":
        _dense(r, many, "under-hinted |")
    else:
        r.ctx.synchronize()
        _compact(r, many, "under-hinted |")
    many.parity(img)


# ------------------------------------------------------------------------------------------------------------- profiling on
def test_frame_under_profiling(lcgs):
    """the memset fill and launch_zero_grads2d in the mode: rows the frame does not keep are overwritten with zeros"""
    def make():
        scene, pose, W, H = antialias_ref.subpixel_crowd()
        scene["pos"][700:800] += 100.0
        f = AFrame(scene, pose, W, H, seed=3)
        assert not f.on[700:800].any() and f.hit.sum() >= 1000
        return f
    f = cached(("antialias rows", "profiling"), make)
    r, _ = f.renderer()
    r.set_profiling(True)
    f.render(r)
    g, rows = _dense(r, f, "profiling | on")
    assert all(bool((g[k][700:800] == 0).all()) for k in KEYS)
    names = [n for n in r.stage_times() if n in ("zero_grads", "render_backward", "preprocess_backward")]
    assert names == ["zero_grads", "render_backward", "preprocess_backward"], names
    _compact(r, f, "profiling | on")


# ------------------------------------------------------------------------------------------------------------- map channels
def _maps_forward_checked(r, f, mode):
    depth, alpha = (torch.full((f.H, f.W), 7.0, device=DEV) for _ in range(2))
    r.render_maps(depth, alpha, mode=mode)
    r.ctx.synchronize()
    want = f._once(("maps forward", mode), lambda: antialias_ref.maps_forward(_oracles()[0], f.scene, f.ocam, mode, f.sm, f.sh_deg))
    assert np.array_equal(depth.cpu().numpy(), want[0]) and np.array_equal(alpha.cpu().numpy(), want[1]), mode


def _dist_forward_checked(r, f, mode, center):
    out = torch.full((f.H, f.W), 7.0, device=DEV)
    r.render_distortion(out, mode=mode, center=center)
    r.ctx.synchronize()
    o32 = _oracles()[0]
    v = maps_ref._value(o32, f.scene, f.ocam, mode, f.sm)[0]
    want = f._once(("dist forward", mode, center), lambda: distortion_ref.compose(o32, f.state, f.ocam, v, center)[0])
    assert np.array_equal(out.cpu().numpy(), want), (mode, center)


def _no_image_zeros(g, f, r, tag):
    assert bool((g["sh"] == 0).all()), tag  # no image gradient: nothing reaches the colours
    _exact_zeros(g, f, f.survivors(r), tag)


@pytest.mark.parametrize("mode", maps_ref.MODES)
@pytest.mark.parametrize("key", MAP_FRAMES)
def test_maps_backward_rows(lcgs, key, mode):
    f = _frame(key)
    r, _ = f.renderer()
    f.render(r)
    _maps_forward_checked(r, f, mode)
    for variant in MAP_VARIANTS:
        g = sevens(f.scene)
        r.backward_maps(*[_d(a) for a in f.incoming(variant)], *[g[k] for k in KEYS], mode=mode)
        r.ctx.synchronize()
        _rows(g, f.maps_bound(variant, mode), f"maps | {key} {variant} {mode}")
        if variant != "both+img":
            _no_image_zeros(g, f, r, (key, variant, mode))


@pytest.mark.parametrize("center", CENTERS)
@pytest.mark.parametrize("mode", maps_ref.MODES)
@pytest.mark.parametrize("key", MAP_FRAMES)
def test_distortion_backward_rows(lcgs, key, mode, center):
    f = _frame(key)
    r, _ = f.renderer()
    f.render(r)
    _dist_forward_checked(r, f, mode, center)
    for variant in DIST_VARIANTS:
        g = sevens(f.scene)
        r.backward_distortion(*[_d(a) for a in f.dist_incoming(variant)], *[g[k] for k in KEYS], mode=mode, center=center)
        r.ctx.synchronize()
        _rows(g, f.dist_bound(variant, mode, center), f"distortion | {key} {variant} {mode} {center:.2f}")
        if variant != "all":
            _no_image_zeros(g, f, r, (key, variant, mode, center))


@pytest.mark.parametrize("mode", maps_ref.MODES)
def test_map_channels_accumulate_over_two_views(lcgs, mode):
    f0 = _frame("sub-pixel crowd")
    f1 = cached(("antialias rows", "sub-pixel crowd, second pose"),
                lambda: AFrame(f0.scene, CROWD_POSE2, f0.W, f0.H, seed=5))
    assert not np.array_equal(f0.state["img"], f1.state["img"]) and f1.hit.sum() >= 500
    r, _ = f0.renderer()
    f0.render(r)
    g = sevens(f0.scene)
    r.backward_distortion(*[_d(a) for a in f0.dist_incoming("all")], *[g[k] for k in KEYS], mode=mode, center=CROWD_DEPTH)
    f1.render(r)
    r.backward_maps(*[_d(a) for a in f1.incoming("both")], *[g[k] for k in KEYS], mode=mode, accumulate=True)
    r.ctx.synchronize()
    bound = antialias_ref.sum_row_bounds([f0.dist_bound("all", mode, CROWD_DEPTH), f1.maps_bound("both", mode)])
    _rows(g, bound, f"maps | two views accumulated {mode}")


@pytest.mark.parametrize("key", CROWDS)
def test_map_channels_through_autograd(lcgs, key):
    f = _frame(key)
    for wrapper, mode in (("maps", "inv_z"), ("distortion", "z")):
        r, d = f.renderer()
        t = {k: d[k].clone().requires_grad_(True) for k in KEYS}
        if wrapper == "maps":
            img, depth, alpha = L.render_autograd_maps(r, f.cam(), *[t[k] for k in KEYS], bg=f.bg, scale_modifier=f.sm,
                                                       depth_mode=mode)
            loss = (img * dev(f.dL)).sum() + (depth * dev(f.gd)).sum() + (alpha * dev(f.ga)).sum()
            bound = f.maps_bound("both+img", mode)
        else:
            img, depth, alpha, dist = L.render_autograd_distortion(r, f.cam(), *[t[k] for k in KEYS], bg=f.bg, depth_mode=mode,
                                                                   center=CROWD_DEPTH, scale_modifier=f.sm)
            loss = (img * dev(f.dL)).sum() + (depth * dev(f.gd)).sum() + (alpha * dev(f.ga)).sum() + (dist * dev(f.gq)).sum()
            bound = f.dist_bound("all", mode, CROWD_DEPTH)
        f.parity(img.detach())
        loss.backward()
        torch.cuda.synchronize()
        _rows({k: t[k].grad for k in KEYS}, bound, f"maps | {key} autograd {wrapper} {mode}")


# ------------------------------------------------------------------------------------------------------------------ camera
CAMERA_CASES = ("image", "image, degree 1", "image + maps")


@pytest.mark.parametrize("case", CAMERA_CASES)
@pytest.mark.parametrize("key", (127, "sub-pixel crowd"))
def test_camera_gradient(lcgs, key, case):
    """lcgs_render_backward_camera, and lcgs_camera_backward behind the parameter pass, held to antialias_ref.camera_bound:
    degree 3 runs k_camera_grad<true, true> (the kept Jacobian), degree 1 k_camera_grad<false, true>"""
    f = _frame(key, 1 if case.endswith("degree 1") else 3)
    gd, ga = (f.gd, f.ga) if case == "image + maps" else (None, None)
    mode = "inv_z" if case == "image + maps" else "z"
    rows_bound = f.maps_bound("both+img", mode) if gd is not None else f.bound()
    B, r64 = f._once(("camera", case), lambda: antialias_ref.camera_bound(f.scene, f.ocam, f.dL, gd, ga, mode, f.bg, f.sm,
                                                                          f.sh_deg, pos_bound=rows_bound[0]["pos"]))
    r, _ = f.renderer()
    f.render(r)
    out = torch.full((12,), 7.0, device=DEV)
    r.backward_camera(dev(f.dL), _d(gd), _d(ga), out, mode=mode)
    r.ctx.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    print(f"[gradient rows vs f64] antialiased | camera | {key} {case} walks: |got - r64| / bound "
          f"{np.array2string(np.abs(got - r64) / B, precision=3)}")
    assert np.isfinite(got).all() and (np.abs(got - r64) <= B).all(), (got, r64, B)
    # behind the parameter pass: the same twelve numbers, and minus the column sums of its dL/dpos rows
    g = sevens(f.scene)
    if gd is None:
        r.backward(dev(f.dL), *[g[k] for k in KEYS])
    else:
        r.backward_maps(dev(f.dL), _d(gd), _d(ga), *[g[k] for k in KEYS], mode=mode)
    out2 = torch.full((12,), 7.0, device=DEV)
    r.camera_backward(out2)
    r.ctx.synchronize()
    _rows(g, rows_bound, f"camera | {key} {case} rows")
    got2 = out2.cpu().numpy().astype(np.float64)
    print(f"[gradient rows vs f64] antialiased | camera | {key} {case} behind the rows: |got - r64| / bound "
          f"{np.array2string(np.abs(got2 - r64) / B, precision=3)}")
    assert (np.abs(got2 - r64) <= B).all(), (got2, r64, B)
    want = -g["pos"].double().sum(dim=0).cpu().numpy()
    for numbers in (got, got2):
        assert (np.abs(numbers[0:3] - want) <= B[0:3]).all(), (numbers[0:3], want, B[0:3])


# --------------------------------------------------------------------------------------------------------------- rho = 0 rows
@pytest.mark.parametrize("deg", [3, 1])
def test_rank_one_rows(lcgs, deg):
    """40 rows with a rank-1 covariance among normal rows: the forward's `q > 0 ? sqrt : 0`, the cull of a row whose compensated
    opacity is 0, the backward's `rho > 0` guard in front of the division by rho"""
    f = _frame("rank-1", deg)
    flat = antialias_ref.RANK1_ROWS
    assert (f.state["rho"][flat] == 0).sum() >= 10 and (f.state["opacity_eff"][flat] < 1 / 255).all() and f.on[flat].sum() >= 20
    assert not f.hit[flat].any() and f.hit.sum() >= 1000
    r, _ = f.renderer()
    f.render(r, count=False)
    g, rows = _dense(r, f, f"rho = 0 | degree {deg}")
    assert not np.isin(flat, rows).any()  # num_visible does not count them
    for k in KEYS:
        a = g[k].cpu().numpy().reshape(f.P, -1)
        assert np.isfinite(a).all() and not a[flat].any(), k
    gc = _compact(r, f, f"rho = 0 | degree {deg}")
    assert all(bool(torch.isfinite(gc[k]).all()) for k in KEYS)


# --------------------------------------------------------------------------------- consumers behind an antialiased backward
def test_densify_statistics_behind_a_maps_backward(lcgs):
    """lcgs_densify_accumulate after lcgs_render_backward_maps of the sub-pixel crowd: denom == 1 on exactly the on-screen rows,
    grad_accum within test_gpu_densify.py's statistics bound formed from the antialiased references"""
    o32, o64, _ = _oracles()
    f = _frame("sub-pixel crowd")
    mode = "z"
    r, _ = f.renderer()
    f.render(r)
    g = sevens(f.scene)
    r.backward_maps(dev(f.dL), dev(f.gd), dev(f.ga), *[g[k] for k in KEYS], mode=mode)
    stats = {"grad_accum": torch.zeros(f.P, device=DEV), "denom": torch.zeros(f.P, dtype=torch.int32, device=DEV),
             "max_radii": torch.zeros(f.P, dtype=torch.int32, device=DEV)}
    r.densify_accumulate(stats)
    r.ctx.synchronize()
    rows = f.survivors(r)
    on = np.zeros(f.P, bool)
    on[rows] = True
    got = {k: t.cpu().numpy() for k, t in stats.items()}
    assert np.array_equal(got["denom"] == 1, on) and not got["denom"][~on].any() and not got["grad_accum"][~on].any()
    assert np.array_equal(got["max_radii"], np.where(on, f.state["radii"], 0))
    kw = dict(mode=mode, bg=f.bg, scale_modifier=f.sm, sh_deg=f.sh_deg)
    gm32 = antialias_ref.camera_rows(o32, f.scene, f.ocam, f.dL, f.gd, f.ga, **kw)[0][:, 0:2].astype(np.float64)
    gm64 = antialias_ref.camera_rows(o64, f.scene, f.cam64, f.dL, f.gd, f.ga, **kw)[0][:, 0:2].astype(np.float64)
    A, _ = antialias_ref.walk_budgets(f.state, f.scene, f.ocam, f.dL, f.gd, f.ga, mode, f.bg, f.sm)
    half = np.array([f.W / 2, f.H / 2])
    want = np.sqrt(((gm32 * half) ** 2).sum(axis=1))
    bound = ((GRAD_ROW_K * np.abs(gm32 - gm64) + GRAD_ROW_CU * U32 * A[:, 0:2]) * half).sum(axis=1)
    diff = np.abs(got["grad_accum"].astype(np.float64) - np.where(on, want, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    print(f"[gradient rows vs f64] antialiased | densify | grad_accum worst diff/bound {ratio.max():.3f} (row {int(ratio.argmax())})")
    assert ratio.max() <= 1.0, (int(ratio.argmax()), float(ratio.max()), int((ratio > 1).sum()))
    assert (got["grad_accum"][on] > 0).mean() > 0.5
