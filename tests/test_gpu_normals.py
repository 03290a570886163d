"""`-m gpu`: the view-space normal map of a keep-state frame (lcgs_render_normals) and its backward
(lcgs_render_backward_normals), on the frames of test_gpu_maps.py.

Forward: the map equals the f32 reference's composition bit for bit (tests/normals_ref.py: the frame's own state composited with
the colour n, the per-splat normal restated in binary32 with the kernel's operation order), no pixel excluded -- the crowd, eight
random draws, a context-owned scene in spatial order, an antialiased frame, a frame that draws nothing.  Over those frames every
axis and both flip states occur among the rows some pixel blends (asserted on the reference).
Backward: every component of every row inside normals_ref's bound (gpu_util.check_gradient_rows' formula and constants), no row
excluded -- the normal channel alone, with depth, alpha and distortion, with an image gradient as well, both depth modes; the
gradients of a 2DGS-style consistency term; accumulation over two views; exact zeros; a NULL normal gradient; the plain backward
afterwards; the densification statistics behind it; the camera gradient refused behind it; the autograd wrapper; state and
argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import luisacomputegaussiansplatting_amd as L
import antialias_ref
import maps_ref
import normals_ref
from conftest import ROOT, make_scene
from gpu_util import DEV, KEYS, View, cached, check_gradient_rows, dev, sevens, upload_scene
from test_gpu_distortion import CROWD_DEPTH, _dframe
from test_gpu_maps import AWAY, POSE2

pytestmark = pytest.mark.gpu
FORWARD_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
BACKWARD_FRAMES = ("crowd", 100, 101, 102, 103)
# the normal channel alone (no depth channel: the mode plays no part); with depth, alpha and distortion; with an image gradient too
CASES = (("nrm", "z"), ("nrm+maps", "z"), ("nrm+maps", "inv_z"), ("all", "z"), ("all", "inv_z"))
DIST_VARIANT = {"nrm+maps": "dist+maps", "all": "all"}  # what test_gpu_distortion.py calls the rest of the call
CENTER = {"z": CROWD_DEPTH, "inv_z": 0.0}


class NFrame:
    """a frame of test_gpu_maps.py (shared with it and with test_gpu_distortion.py: maps, incoming gradients and bounds are
    computed once) with the normal map's incoming gradient, reference and bounds"""

    def __init__(self, oracle, key, pose=None):
        self.df = _dframe(oracle, key, pose)
        self.f = self.df.f
        self.gn = np.random.default_rng(31).normal(size=(3, self.f.H, self.f.W)).astype(np.float32)
        self._normal, self._bounds = None, {}

    def normal(self):
        """(normal [3, H, W], forward state, (n, k, flip)) of the f32 reference"""
        if self._normal is None:
            f = self.f
            self._normal = normals_ref.forward(f.oracle, f.scene, f.ocam, scale_modifier=f.sm)
        return self._normal

    def incoming(self, variant):
        """(dL_dimg, dL_ddepth, dL_dalpha, dL_ddist, dL_dnormal); None = NULL"""
        return ((None,) * 4 if variant == "nrm" else self.df.incoming(DIST_VARIANT[variant])) + (self.gn,)

    def bound(self, variant, mode):
        f = self.f
        if "nrm" not in self._bounds:
            self._bounds["nrm"] = normals_ref.row_bound(f.scene, f.ocam, self.gn, scale_modifier=f.sm)
        if variant == "nrm":
            return self._bounds["nrm"]
        if (variant, mode) not in self._bounds:
            self._bounds[variant, mode] = normals_ref.sum_row_bounds(
                [self._bounds["nrm"], self.df.bound(DIST_VARIANT[variant], mode, CENTER[mode])])
        return self._bounds[variant, mode]


def _nframe(oracle, key, pose=None):
    return cached(("normals", key, str(pose)), lambda: NFrame(oracle, key, pose))


def _normal(r, H, W):
    out = torch.full((3, H, W), 7.0, device=DEV)
    r.render_normals(out)
    r.ctx.synchronize()
    return out.cpu().numpy()


def _assert_normal(got, ref, tag):
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got, ref), (f"{tag}: {int((got != ref).sum())} of {got.size} values differ from the reference, max |diff| "
                                      f"{np.abs(got.astype(np.float64) - ref).max():.3e}")


def _d(a):
    return None if a is None else dev(a)


# ------------------------------------------------------------------------------------------------------------------ forward
def test_forward_crowd(lcgs, oracle):
    nf = _nframe(oracle, "crowd")
    f = nf.f
    ref, st, _ = nf.normal()
    lens = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    # a milder scene cannot replace the crowd unnoticed: a list of more than two rounds, covered and empty pixels
    assert lens.max() > 512 and (st["n_contrib"] == 0).any() and np.all(ref[:, st["n_contrib"] == 0] == 0)
    assert all(np.abs(ref[c]).max() > 1e-2 for c in range(3))
    r, _, img = f.renderer()
    _assert_normal(_normal(r, f.H, f.W), ref, "crowd")
    assert np.array_equal(img.cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])  # the colour frame is untouched


@pytest.mark.parametrize("seed", FORWARD_SEEDS)
def test_forward_random_draws(lcgs, oracle, seed):
    nf = _nframe(oracle, seed)
    r, _, _ = nf.f.renderer()
    _assert_normal(_normal(r, nf.f.H, nf.f.W), nf.normal()[0], f"seed {seed}")


def test_forward_frames_cover_every_axis_and_both_flips(oracle):
    """over the forward frames, among the rows some pixel blends: every axis k, each both unflipped and flipped (the reference's
    own decisions -- what the bit-for-bit comparisons above then hold the kernel to)"""
    seen = set()
    for key in ("crowd",) + FORWARD_SEEDS:
        nf = _nframe(oracle, key)
        _, st, (_, k, flip) = nf.normal()
        on = normals_ref.blended_rows(oracle, st, nf.f.ocam)
        seen |= set(zip(k[on].tolist(), flip[on].tolist()))
    assert seen == {(k, fl) for k in (0, 1, 2) for fl in (False, True)}, sorted(seen)


def test_forward_scene_in_spatial_order(lcgs, oracle):
    nf = _nframe(oracle, "crowd")
    f = nf.f
    r = L.Renderer(L.Context(0))
    r.upload_scene(f.scene)  # context-owned, along a Morton curve
    assert r.permutation() is not None
    f.render(r)
    _assert_normal(_normal(r, f.H, f.W), nf.normal()[0], "spatial order")


def test_forward_antialiased_frame(lcgs, oracle):
    nf = _nframe(oracle, "crowd")
    f = nf.f
    st = cached(("distortion", "crowd antialiased"), lambda: antialias_ref.forward_state(oracle, f.scene, f.ocam))
    r = L.Renderer(L.Context(0))
    d = upload_scene(f.scene)
    r.bind_scene(*[d[k] for k in KEYS])
    r.set_raster_mode("antialiased")
    img = torch.zeros(3, f.H, f.W, device=DEV)
    assert r.forward(f.cam(), img, keep_state=True, sync=True) == st["num_rendered"] > 0
    ref = normals_ref.compose(oracle, st, f.ocam, nf.normal()[2][0])
    assert not np.array_equal(ref, nf.normal()[0])  # (the compensated opacity: another map)
    _assert_normal(_normal(r, f.H, f.W), ref, "antialiased")


def test_forward_frame_that_draws_nothing(lcgs, oracle):
    nf = _nframe(oracle, "crowd")
    f = nf.f
    r, _ = f.renderer(keep=False)
    img = torch.full((3, f.H, f.W), -1.0, device=DEV)
    cam = L.get_lookat_cam(*AWAY, width=f.W, height=f.H)
    assert r.forward(cam, img, bg=f.bg, keep_state=True, sync=True) == 0
    assert np.all(_normal(r, f.H, f.W) == 0)
    assert bool((img == -1.0).all())  # the colour buffer keeps its poison; the map is written
    # ... and its backward writes exact zeros
    g = sevens(f.scene)
    r.backward_normals(None, None, None, None, dev(nf.gn), *[g[k] for k in KEYS])
    r.ctx.synchronize()
    assert all(bool((g[k] == 0).all()) for k in KEYS)


# ----------------------------------------------------------------------------------------------------------------- backward
def _backward(r, nf, variant, mode, g=None, accumulate=False):
    g = g if g is not None else sevens(nf.f.scene)
    r.backward_normals(*[_d(a) for a in nf.incoming(variant)], *[g[k] for k in KEYS], mode=mode, center=CENTER[mode],
                       accumulate=accumulate)
    r.ctx.synchronize()
    return g


@pytest.mark.parametrize("variant,mode", CASES)
@pytest.mark.parametrize("key", BACKWARD_FRAMES)
def test_backward_rows(lcgs, oracle, key, variant, mode):
    nf = _nframe(oracle, key)
    r, _, _ = nf.f.renderer()
    g = _backward(r, nf, variant, mode)  # onto arrays pre-filled with 7, without a preceding lcgs_render_normals
    check_gradient_rows(g, None, None, None, bound=nf.bound(variant, mode), tag=f"{key} {variant} {mode}")
    if variant != "all":  # no image gradient: nothing reaches the colours
        assert bool((g["sh"] == 0).all())
    assert bool((g["rotq"] != 0).any())


def _consistency_gradients(D, A, N, ocam):
    """(dL_ddepth, dL_dalpha, dL_dnormal) of the 2DGS-style term mean(A - N . nt(D / A)), nt the unit normal of the rendered
    depth surface (central differences of the back-projected points, turned to face the camera), by torch CPU autograd from the
    reference maps"""
    H, W = A.shape
    tany = np.tan(np.float64(ocam.fov) / 180.0 * np.pi * 0.5)
    tanx = tany * np.float64(ocam.aspect_ratio)
    D, A, N = (torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(True) for x in (D, A, N))
    z = D / A.clamp_min(1e-3)
    xs = ((torch.arange(W, dtype=torch.float64) + 0.5) / W * 2 - 1) * tanx
    ys = ((torch.arange(H, dtype=torch.float64) + 0.5) / H * 2 - 1) * tany
    pts = torch.stack([xs[None, :] * z, ys[:, None] * z, z])  # [3, H, W], view space
    dx = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2]
    dy = pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    cr = -torch.cross(dx, dy, dim=0)  # (towards the camera: negative view z)
    nt = cr / torch.sqrt((cr * cr).sum(dim=0, keepdim=True) + 1e-20)
    loss = (A[1:-1, 1:-1] - (N[:, 1:-1, 1:-1] * nt).sum(dim=0)).mean()
    loss.backward()
    return tuple(x.grad.float().numpy() for x in (D, A, N))


def test_backward_rows_under_a_normal_consistency_loss(lcgs, oracle):
    nf = _nframe(oracle, "crowd")
    f = nf.f

    def make():
        D, A, _ = f.maps("z")
        gd, ga, gn = _consistency_gradients(D, A, nf.normal()[0], f.ocam)
        assert all(np.isfinite(x).all() and np.abs(x).max() > 0 for x in (gd, ga, gn))
        return gd, ga, gn, normals_ref.row_bound(f.scene, f.ocam, gn, None, gd, ga, mode="z", scale_modifier=f.sm)
    gd, ga, gn, bound = cached(("normals", "consistency"), make)
    r, _, _ = f.renderer()
    g = sevens(f.scene)
    r.backward_normals(None, dev(gd), dev(ga), None, dev(gn), *[g[k] for k in KEYS], mode="z")
    r.ctx.synchronize()
    check_gradient_rows(g, None, None, None, bound=bound, tag="crowd, normal-consistency gradients")
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
    gn = np.random.default_rng(5).normal(size=(3, v.H, v.W)).astype(np.float32)
    g = sevens(v.scene)
    r.backward_normals(None, None, None, None, dev(gn), *[g[k] for k in KEYS])
    r.ctx.synchronize()
    for k in KEYS:
        a = g[k].cpu().numpy().reshape(v.P, -1)
        assert np.all(a[off] == 0), k
    assert bool((g["sh"] == 0).all()) and bool((g["rotq"] != 7.0).all()) and bool((g["pos"] != 7.0).all())
    check_gradient_rows(g, None, None, None, bound=normals_ref.row_bound(v.scene, v.ocam, gn), tag="off screen")


@pytest.mark.parametrize("mode", normals_ref.MODES)
def test_backward_accumulates_over_two_views(lcgs, oracle, mode):
    n0, n1 = _nframe(oracle, "crowd"), _nframe(oracle, "crowd", POSE2)
    assert not np.array_equal(n0.normal()[0], n1.normal()[0])
    r, _, _ = n0.f.renderer()
    g = _backward(r, n0, "all", mode)
    n1.f.render(r)
    _backward(r, n1, "nrm", mode, g=g, accumulate=True)
    bound = normals_ref.sum_row_bounds([n0.bound("all", mode), n1.bound("nrm", mode)])
    check_gradient_rows(g, None, None, None, bound=bound, tag=f"two views {mode}")


def test_null_normal_gradient_is_backward_distortion(lcgs, oracle):
    """The same launches, so the same rows bit for bit -- where bits are defined: on draw 7, which lists no splat on more than
    two tiles, with incoming gradients that are zero except on two covered pixels of every tile and no image gradient, for the
    reason test_gpu_distortion.py::test_null_distortion_gradient_is_backward_maps gives (float atomics in order of arrival: two
    terms commute, three do not)."""
    nf = _nframe(oracle, 7)
    f = nf.f
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
    gq = nf.df.gq
    for gd, ga, gq_ in ((f.gd, f.ga, gq), (f.gd, None, None), (None, f.ga, gq)):
        gd, ga, gq_ = (None if x is None else np.where(keep, x, np.float32(0.0)) for x in (gd, ga, gq_))
        a, b = sevens(f.scene), sevens(f.scene)
        r.backward_distortion(None, _d(gd), _d(ga), _d(gq_), *[a[k] for k in KEYS], mode="inv_z", center=CROWD_DEPTH)
        r.backward_normals(None, _d(gd), _d(ga), _d(gq_), None, *[b[k] for k in KEYS], mode="inv_z", center=CROWD_DEPTH)
        r.ctx.synchronize()
        assert int((a["opacity"] != 0).sum()) >= 8
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


def test_plain_backward_after_a_normals_backward(lcgs, oracle):
    scene, pose, W, H = maps_ref.crowd()
    v = cached(("maps", "crowd view"), lambda: View(oracle, scene, pose, W, H, seed=2))
    nf = _nframe(oracle, "crowd")
    r, _, _ = nf.f.renderer()
    _backward(r, nf, "nrm+maps", "inv_z")
    g = sevens(scene)
    r.backward(dev(v.dL), *[g[k] for k in KEYS])  # the same frame: the normal channel's sums must not leak into it
    r.ctx.synchronize()
    check_gradient_rows(g, None, None, None, bound=v.bound(), tag="plain backward after normals")
    # ... and a normals backward after it starts from cleared rows again
    check_gradient_rows(_backward(r, nf, "nrm", "z"), None, None, None, bound=nf.bound("nrm", "z"), tag="normals after plain")


def test_densify_statistics_behind_and_camera_gradient_refused(lcgs, oracle):
    nf = _nframe(oracle, "crowd")
    f = nf.f
    r, _, _ = f.renderer()
    _backward(r, nf, "nrm", "z")
    # lcgs_densify_accumulate counts the frame on exactly its on-screen rows
    stats = {"grad_accum": torch.zeros(f.P, device=DEV), "denom": torch.zeros(f.P, dtype=torch.int32, device=DEV),
             "max_radii": torch.zeros(f.P, dtype=torch.int32, device=DEV)}
    r.densify_accumulate(stats)
    r.ctx.synchronize()
    on = torch.zeros(f.P, dtype=torch.bool, device=DEV)
    on[r.visible_rows().long()] = True
    assert 0 < int(on.sum()) and torch.equal(stats["denom"] == 1, on) and bool((stats["denom"][~on] == 0).all())
    assert bool((stats["grad_accum"][~on] == 0).all()) and bool((stats["grad_accum"][on] > 0).any())
    # the camera gradient lacks the normal channel's direct term: refused, and the poison stays
    out = torch.full((12,), 7.0, device=DEV)

    def refused():
        with pytest.raises(L.LcgsError) as e:
            r.camera_backward(out)
        assert e.value.status == L.api.LCGS_ERR_STATE and "normal" in str(e.value)
        r.ctx.synchronize()
        assert bool((out == 7.0).all())

    def accepted():
        r.camera_backward(out)
        r.ctx.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got).all() and np.abs(got).max() > 0 and not (got == 7.0).any()
        out.fill_(7.0)

    refused()
    # a NULL normal gradient is no normal channel; nor is a plain backward of the frame
    g = sevens(f.scene)
    r.backward_normals(None, dev(f.gd), None, None, None, *[g[k] for k in KEYS])
    accepted()
    _backward(r, nf, "all", "z")
    refused()
    r.backward(dev(f.gi), *[g[k] for k in KEYS])
    accepted()


# ----------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("case", ("direct", "frame between"))
def test_autograd(lcgs, oracle, case):
    nf = _nframe(oracle, "crowd")
    f, df = nf.f, nf.df
    mode = "inv_z" if case == "frame between" else "z"
    center = CENTER[mode]
    r = L.Renderer(L.Context(0))
    t = {k: dev(f.scene[k]).requires_grad_(True) for k in KEYS}
    img, depth, alpha, dist, normal = L.render_autograd_normals(r, f.cam(), *[t[k] for k in KEYS], bg=f.bg, depth_mode=mode,
                                                                center=center)
    assert np.array_equal(depth.detach().cpu().numpy(), f.maps(mode)[0]) and np.array_equal(alpha.detach().cpu().numpy(), f.maps(mode)[1])
    assert np.array_equal(dist.detach().cpu().numpy(), df.dist(mode, center)[0])
    assert np.array_equal(normal.detach().cpu().numpy(), nf.normal()[0])
    assert np.array_equal(img.detach().cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])
    if case == "frame between":  # another view's frame replaces the renderer's state: the backward re-renders its own
        other = torch.zeros(3, f.H, f.W, device=DEV)
        r.forward(L.get_lookat_cam(*POSE2, width=f.W, height=f.H), other, keep_state=True, sync=True)
        (normal * dev(nf.gn)).sum().backward()  # the unused outputs arrive as None: passed as NULL
        variant = "nrm"
    else:
        ((img * dev(f.gi)).sum() + (depth * dev(f.gd)).sum() + (alpha * dev(f.ga)).sum() + (dist * dev(df.gq)).sum() +
         (normal * dev(nf.gn)).sum()).backward()
        variant = "all"
    torch.cuda.synchronize()
    check_gradient_rows({k: t[k].grad for k in KEYS}, None, None, None, bound=nf.bound(variant, mode), tag=f"autograd {case}")


# -------------------------------------------------------------------------------------------------------------------- state
def test_state_and_argument_errors(lcgs, oracle):
    nf = _nframe(oracle, "crowd")
    f = nf.f
    r, d = f.renderer(keep=False)
    g = sevens(f.scene)
    out = torch.zeros(3, f.H, f.W, device=DEV)

    def refused(status, fn, *a, **kw):
        with pytest.raises(L.LcgsError) as e:
            fn(*a, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))

    grads = [g[k] for k in KEYS]
    # no frame at all, then a frame without kept state
    refused(L.api.LCGS_ERR_STATE, r.render_normals, out)
    refused(L.api.LCGS_ERR_STATE, r.backward_normals, None, None, None, None, dev(nf.gn), *grads)
    img = torch.zeros(3, f.H, f.W, device=DEV)
    r.forward(f.cam(), img, bg=f.bg, keep_state=False, sync=True)
    refused(L.api.LCGS_ERR_STATE, r.render_normals, out)
    refused(L.api.LCGS_ERR_STATE, r.backward_normals, None, dev(f.gd), None, None, dev(nf.gn), *grads)
    # a kept frame: all five gradients NULL is an argument error, and so are a NULL output and a centre that is not finite
    f.render(r)
    refused(1, r.backward_normals, None, None, None, None, None, *grads)
    refused(1, r.render_normals, None)
    refused(1, r.backward_normals, None, None, None, None, dev(nf.gn), *grads, center=float("inf"))
    r.render_normals(out)
    # a frame drawn from received records is not this context's own
    rows, recs = r.owner_project(0, f.cam(), 0, f.P, keep_state=True)
    r.owner_render(f.cam(), rows, recs, img, bg=f.bg, keep_state=True)
    refused(L.api.LCGS_ERR_STATE, r.render_normals, out)
    refused(L.api.LCGS_ERR_STATE, r.backward_normals, dev(f.gi), dev(f.gd), dev(f.ga), dev(nf.df.gq), dev(nf.gn), *grads)
    r.ctx.synchronize()


def test_forward_and_backward_with_poisoned_workspace():
    """the crowd's and the draws' forward and the crowd's backward rows once more in a process whose library fills every fresh
    workspace allocation with garbage (LCGS_POISON=1, tests/test_gpu_poisoned_workspace.py): the per-row pass writes every normal
    a walk reads and clears every dL/dn slot the walk adds to"""
    env = dict(os.environ, LCGS_POISON="1")
    pick = "test_forward_crowd or test_forward_random_draws or test_forward_scene_in_spatial_order or (test_backward_rows and crowd)"
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", pick,
                          "tests/test_gpu_normals.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "\n15 passed" in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]
