"""`-m gpu`: caller-supplied per-splat feature channels blended over a keep-state frame (lcgs_render_features) and their backward
(lcgs_render_backward_features), on the frames of test_gpu_maps.py.

K values, the smallest that can still go wrong under the kernels' chunk widths of 4 / 8 / 16 channels: 1 and 3 (one chunk of 4,
padded), 7 (one chunk of 8, padded), 17 (two walks of 16 and a tail of one channel; rows of odd K are not 16-byte aligned),
and LCGS_FEATURES_MAX once, forward only.
Forward: the map equals the f32 reference's composition bit for bit (tests/features_ref.py: the frame's own state composited
once per zero-padded triple of feature columns), no pixel excluded.
Backward: every component of every row of pos / scale / rotq / opacity and of dL/dfeatures inside features_ref's bound
(gpu_util.check_gradient_rows' formula and constants), no row excluded, outputs pre-filled with 7."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import luisacomputegaussiansplatting_amd as L
import antialias_ref
import features_ref
import maps_ref
from conftest import ROOT, make_scene
from features_ref import FKEY
from gpu_util import DEV, KEYS, View, cached, check_gradient_rows, dev, random_draw, sevens, upload_scene
from test_gpu_camera import _check as _check_camera
from test_gpu_camera import _frame as _camera_frame
from test_gpu_maps import AWAY, POSE2
from test_gpu_normals import CASES, CENTER, _nframe

pytestmark = pytest.mark.gpu
KS = (1, 3, 7, 17)
KM = 17  # the multi-chunk K
FORWARD_SEEDS = (0, 1, 2, 3)
BACKWARD_DRAWS = (100, 101, 102, 103)  # test_gpu_maps.py's; 102: needles and giants
K_MAX = L.api.LCGS_FEATURES_MAX


def _features(P, K, seed=41):
    return np.random.default_rng(seed + K).normal(size=(P, K)).astype(np.float32)


class FFrame:
    """a frame of test_gpu_maps.py (shared with it, test_gpu_distortion.py and test_gpu_normals.py: maps, incoming gradients and
    bounds of the other channels are computed once) with feature rows, the feature map's incoming gradient, references and
    bounds per K"""

    def __init__(self, oracle, key, pose=None):
        self.nf = _nframe(oracle, key, pose)
        self.f = self.nf.f
        self._map, self._bounds = {}, {}

    def feats(self, K):
        return _features(self.f.P, K)

    def gF(self, K):
        return np.random.default_rng(43 + K).normal(size=(K, self.f.H, self.f.W)).astype(np.float32)

    def map(self, K):
        """(feature map [K, H, W], forward state) of the f32 reference"""
        if K not in self._map:
            f = self.f
            self._map[K] = features_ref.forward(f.oracle, f.scene, f.ocam, self.feats(K), scale_modifier=f.sm)
        return self._map[K]

    def bound(self, K, variant=None, mode="z"):
        """variant None: the feature channel alone; else test_gpu_normals.py's name of the rest of the call"""
        f = self.f
        if K not in self._bounds:
            self._bounds[K] = features_ref.row_bound(f.scene, f.ocam, self.feats(K), self.gF(K), scale_modifier=f.sm)
        if variant is None:
            return self._bounds[K]
        if (K, variant, mode) not in self._bounds:
            self._bounds[K, variant, mode] = features_ref.sum_row_bounds([self._bounds[K], self.nf.bound(variant, mode)])
        return self._bounds[K, variant, mode]


def _fframe(oracle, key, pose=None):
    return cached(("features", key, str(pose)), lambda: FFrame(oracle, key, pose))


def _render(r, feats, H, W):
    out = torch.full((feats.shape[1], H, W), 7.0, device=DEV)
    r.render_features(feats if torch.is_tensor(feats) else dev(feats), out)
    r.ctx.synchronize()
    return out.cpu().numpy()


def _assert_map(got, ref, tag):
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got, ref), (f"{tag}: {int((got != ref).sum())} of {got.size} values differ from the reference, max |diff| "
                                      f"{np.abs(got.astype(np.float64) - ref).max():.3e}")


def _d(a):
    return None if a is None else dev(a)


def _fsevens(scene, K):
    g = sevens(scene)
    g[FKEY] = torch.full((scene["pos"].shape[0], K), 7.0, device=DEV)
    return g


def _backward(r, ff, K, variant=None, mode="z", g=None, accumulate=False, rows=True, frows=True):
    """variant None: no other incoming gradient; rows False: grads NULL (frozen geometry); frows False: d_dL_dfeatures NULL"""
    g = g if g is not None else _fsevens(ff.f.scene, K)
    incoming = (None,) * 5 if variant is None else ff.nf.incoming(variant)
    r.backward_features(*[_d(a) for a in incoming], dev(ff.feats(K)), dev(ff.gF(K)), g[FKEY] if frows else None,
                        *([g[k] for k in KEYS] if rows else [None] * 5), mode=mode, center=CENTER[mode], accumulate=accumulate)
    r.ctx.synchronize()
    return g


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("K", KS)
def test_forward_crowd(lcgs, oracle, K):
    ff = _fframe(oracle, "crowd")
    f = ff.f
    ref, st = ff.map(K)
    lens = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    # a milder scene cannot replace the crowd unnoticed: a list of more than two rounds, covered and empty pixels
    assert lens.max() > 512 and (st["n_contrib"] == 0).any() and np.all(ref[:, st["n_contrib"] == 0] == 0)
    assert all(np.abs(ref[c]).max() > 1e-2 for c in range(K))
    r, _, img = f.renderer()
    _assert_map(_render(r, ff.feats(K), f.H, f.W), ref, f"crowd K = {K}")
    assert np.array_equal(img.cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])  # the colour frame is untouched


@pytest.mark.parametrize("seed", FORWARD_SEEDS)
def test_forward_random_draws(lcgs, oracle, seed):
    ff = _fframe(oracle, seed)
    r, _, _ = ff.f.renderer()
    _assert_map(_render(r, ff.feats(KM), ff.f.H, ff.f.W), ff.map(KM)[0], f"seed {seed}")


def test_forward_at_the_largest_channel_count(lcgs, oracle):
    """LCGS_FEATURES_MAX channels, sixteen walks, on the random draw of the fewest pixels"""
    assert K_MAX == 256
    seed = min(FORWARD_SEEDS, key=lambda s: (lambda d: d[2] * d[3])(random_draw(s)))
    ff = _fframe(oracle, seed)
    r, _, _ = ff.f.renderer()
    _assert_map(_render(r, ff.feats(K_MAX), ff.f.H, ff.f.W), ff.map(K_MAX)[0], f"seed {seed}, K = {K_MAX}")


def test_forward_scene_in_spatial_order(lcgs, oracle):
    ff = _fframe(oracle, "crowd")
    f = ff.f
    r = L.Renderer(L.Context(0))
    r.upload_scene(f.scene)  # context-owned, along a Morton curve: the caller's rows follow the context's order
    perm = r.permutation()
    assert perm is not None and not torch.equal(perm.cpu().long(), torch.arange(f.P))
    f.render(r)
    feats = dev(ff.feats(KM))[perm.long()].contiguous()
    _assert_map(_render(r, feats, f.H, f.W), ff.map(KM)[0], "spatial order")


def test_forward_antialiased_frame(lcgs, oracle):
    ff = _fframe(oracle, "crowd")
    f = ff.f
    st = cached(("distortion", "crowd antialiased"), lambda: antialias_ref.forward_state(oracle, f.scene, f.ocam))
    r = L.Renderer(L.Context(0))
    d = upload_scene(f.scene)
    r.bind_scene(*[d[k] for k in KEYS])
    r.set_raster_mode("antialiased")
    img = torch.zeros(3, f.H, f.W, device=DEV)
    assert r.forward(f.cam(), img, keep_state=True, sync=True) == st["num_rendered"] > 0
    ref = features_ref.compose(oracle, st, f.ocam, ff.feats(KM))
    assert not np.array_equal(ref, ff.map(KM)[0])  # (the compensated opacity: another map)
    _assert_map(_render(r, ff.feats(KM), f.H, f.W), ref, "antialiased")


def test_one_channel_of_ones_is_the_alpha_map_and_the_rows_normals_give_the_normal_map(lcgs, oracle):
    ff = _fframe(oracle, "crowd")
    f = ff.f
    r, _, _ = f.renderer()
    alpha = torch.full((f.H, f.W), 7.0, device=DEV)
    r.render_maps(None, alpha)
    one = torch.full((1, f.H, f.W), 7.0, device=DEV)
    r.render_features(torch.ones(f.P, 1, device=DEV), one)
    normal = torch.full((3, f.H, f.W), 7.0, device=DEV)
    r.render_normals(normal)
    fn = torch.full((3, f.H, f.W), 7.0, device=DEV)
    r.render_features(dev(ff.nf.normal()[2][0]), fn)  # the reference's per-splat normals: the kernel's own, bit for bit
    r.ctx.synchronize()
    assert float(alpha.max()) > 0.5 and torch.equal(one[0], alpha)
    assert bool((normal != 0).any()) and torch.equal(fn, normal)


def test_forward_frame_that_draws_nothing(lcgs, oracle):
    ff = _fframe(oracle, "crowd")
    f = ff.f
    r, _ = f.renderer(keep=False)
    img = torch.full((3, f.H, f.W), -1.0, device=DEV)
    cam = L.get_lookat_cam(*AWAY, width=f.W, height=f.H)
    assert r.forward(cam, img, bg=f.bg, keep_state=True, sync=True) == 0
    assert np.all(_render(r, ff.feats(KM), f.H, f.W) == 0)
    assert bool((img == -1.0).all())  # the colour buffer keeps its poison; the map is written
    # ... and its backward writes exact zeros to the rows and to dL/dfeatures
    g = _backward(r, ff, KM)
    assert all(bool((g[k] == 0).all()) for k in KEYS + (FKEY,))
    g = _backward(r, ff, KM, rows=False)
    assert bool((g[FKEY] == 0).all()) and all(bool((g[k] == 7.0).all()) for k in KEYS)


# ----------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("K", KS)
def test_backward_rows_features_alone(lcgs, oracle, K):
    ff = _fframe(oracle, "crowd")
    r, _, _ = ff.f.renderer()
    g = _backward(r, ff, K)  # onto arrays pre-filled with 7
    check_gradient_rows(g, None, None, None, bound=ff.bound(K), tag=f"crowd K = {K}")
    assert bool((g["sh"] == 0).all()) and bool((g[FKEY] != 0).any()) and bool((g["pos"] != 0).any())


@pytest.mark.parametrize("key", BACKWARD_DRAWS)
def test_backward_rows_random_draws(lcgs, oracle, key):
    ff = _fframe(oracle, key)
    r, _, _ = ff.f.renderer()
    g = _backward(r, ff, KM)
    check_gradient_rows(g, None, None, None, bound=ff.bound(KM), tag=f"draw {key} K = {KM}")
    assert bool((g["sh"] == 0).all())


@pytest.mark.parametrize("variant,mode", [c for c in CASES if c[0] != "nrm"])
def test_backward_rows_with_the_other_channels(lcgs, oracle, variant, mode):
    """features with depth, alpha, distortion and normals ("nrm+maps"), with an image gradient as well ("all"), both depth modes"""
    ff = _fframe(oracle, "crowd")
    r, _, _ = ff.f.renderer()
    g = _backward(r, ff, KM, variant, mode)
    check_gradient_rows(g, None, None, None, bound=ff.bound(KM, variant, mode), tag=f"crowd K = {KM} + {variant} {mode}")
    if variant != "all":  # no image gradient: nothing reaches the colours
        assert bool((g["sh"] == 0).all())


def test_frozen_geometry_mode_leaves_the_2d_rows_and_what_reads_them_alone(lcgs, oracle):
    """grads NULL: dL/dfeatures inside the same bound; lcgs_camera_backward and lcgs_densify_accumulate behind it give what they
    gave before the call, bit for bit (the 2-D rows are neither cleared nor added to)"""
    ff = _fframe(oracle, "crowd")
    f = ff.f
    r, _, _ = f.renderer()
    g = sevens(f.scene)
    r.backward_maps(dev(f.gi), dev(f.gd), dev(f.ga), *[g[k] for k in KEYS], mode="inv_z")

    def behind():
        cam12 = torch.full((12,), 7.0, device=DEV)
        r.camera_backward(cam12)
        stats = {"grad_accum": torch.zeros(f.P, device=DEV), "denom": torch.zeros(f.P, dtype=torch.int32, device=DEV),
                 "max_radii": torch.zeros(f.P, dtype=torch.int32, device=DEV)}
        r.densify_accumulate(stats)
        r.ctx.synchronize()
        return cam12, stats

    cam_a, stats_a = behind()
    for K in (3, KM):
        gf = _backward(r, ff, K, rows=False)
        B, R = ff.bound(K)
        check_gradient_rows({FKEY: gf[FKEY]}, None, None, None, bound=({FKEY: B[FKEY]}, {FKEY: R[FKEY]}), tag=f"grads NULL, K = {K}")
        assert all(bool((gf[k] == 7.0).all()) for k in KEYS)
    cam_b, stats_b = behind()
    assert bool((cam_a != 7.0).all()) and torch.equal(cam_a, cam_b)
    assert bool((stats_a["grad_accum"] > 0).any()) and all(torch.equal(stats_a[k], stats_b[k]) for k in stats_a)
    # ... and it adds to dL/dfeatures when asked to
    twice = _backward(r, ff, KM, rows=False, g=_backward(r, ff, KM, rows=False), accumulate=True)
    B, R = ff.bound(KM)
    check_gradient_rows({FKEY: twice[FKEY]}, None, None, None, bound=({FKEY: 2 * B[FKEY]}, {FKEY: 2 * R[FKEY]}), tag="grads NULL, twice")


def test_frozen_features_write_the_geometry_rows_alone(lcgs, oracle):
    ff = _fframe(oracle, "crowd")
    r, _, _ = ff.f.renderer()
    g = _backward(r, ff, KM, frows=False)
    check_gradient_rows({k: g[k] for k in KEYS}, None, None, None, bound=features_ref.geometry_only(ff.bound(KM)),
                        tag="d_dL_dfeatures NULL")
    assert bool((g[FKEY] == 7.0).all())


@pytest.mark.parametrize("mode", maps_ref.MODES)
def test_backward_accumulates_over_two_views(lcgs, oracle, mode):
    f0, f1 = _fframe(oracle, "crowd"), _fframe(oracle, "crowd", POSE2)
    assert not np.array_equal(f0.map(KM)[0], f1.map(KM)[0])
    r, _, _ = f0.f.renderer()
    g = _backward(r, f0, KM, "all", mode)
    f1.f.render(r)
    _backward(r, f1, KM, None, mode, g=g, accumulate=True)
    bound = features_ref.sum_row_bounds([f0.bound(KM, "all", mode), f1.bound(KM)])
    check_gradient_rows(g, None, None, None, bound=bound, tag=f"two views {mode}")


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
    feats, gF = _features(v.P, KM), np.random.default_rng(5).normal(size=(KM, v.H, v.W)).astype(np.float32)
    g = _fsevens(v.scene, KM)
    r.backward_features(None, None, None, None, None, dev(feats), dev(gF), g[FKEY], *[g[k] for k in KEYS])
    r.ctx.synchronize()
    for k in KEYS + (FKEY,):
        a = g[k].cpu().numpy().reshape(v.P, -1)
        assert np.all(a[off] == 0), k
    assert bool((g["sh"] == 0).all()) and bool((g[FKEY] != 7.0).all()) and bool((g["pos"] != 7.0).all())
    check_gradient_rows(g, None, None, None, bound=features_ref.row_bound(v.scene, v.ocam, feats, gF), tag="off screen")


def test_null_feature_channel_is_backward_normals(lcgs, oracle):
    """The same launches, so the same rows bit for bit -- where bits are defined: the two-term frame of
    test_gpu_normals.py::test_null_normal_gradient_is_backward_distortion (draw 7, no splat on more than two tiles, gradients
    zero except on two covered pixels of every tile, no image gradient)."""
    ff = _fframe(oracle, 7)
    nf, f = ff.nf, ff.f
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
    gd, ga, gq = (np.where(keep, x, np.float32(0.0)) for x in (f.gd, f.ga, nf.df.gq))
    gn = np.where(keep[None], nf.gn, np.float32(0.0))
    a, b = sevens(f.scene), sevens(f.scene)
    r.backward_normals(None, _d(gd), _d(ga), _d(gq), _d(gn), *[a[k] for k in KEYS], mode="inv_z", center=CENTER["inv_z"])
    r.backward_features(None, _d(gd), _d(ga), _d(gq), _d(gn), None, None, None, *[b[k] for k in KEYS], mode="inv_z",
                        center=CENTER["inv_z"])
    r.ctx.synchronize()
    assert int((a["opacity"] != 0).sum()) >= 8
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


def test_plain_backward_after_a_features_backward(lcgs, oracle):
    scene, pose, W, H = maps_ref.crowd()
    v = cached(("maps", "crowd view"), lambda: View(oracle, scene, pose, W, H, seed=2))
    ff = _fframe(oracle, "crowd")
    r, _, _ = ff.f.renderer()
    _backward(r, ff, KM, "nrm+maps", "inv_z")
    g = sevens(scene)
    r.backward(dev(v.dL), *[g[k] for k in KEYS])  # the same frame: the feature channel's sums must not leak into it
    r.ctx.synchronize()
    check_gradient_rows(g, None, None, None, bound=v.bound(), tag="plain backward after features")
    # ... and a features backward after it starts from cleared rows again
    check_gradient_rows(_backward(r, ff, 3), None, None, None, bound=ff.bound(3), tag="features after plain")


def test_camera_gradient_and_densify_statistics_behind_a_features_backward(lcgs, oracle):
    """a caller-supplied feature has no direct camera term: lcgs_camera_backward is accepted, and with one channel of ones and
    the gradient g it is the camera gradient of <g, alpha> -- held to test_gpu_camera.py's own bound of that"""
    cf = _camera_frame(oracle, "crowd")
    r, _ = cf.renderer()
    g = _fsevens(cf.scene, 1)
    r.backward_features(None, None, None, None, None, torch.ones(cf.P, 1, device=DEV), dev(cf.ga[None]), g[FKEY],
                        *[g[k] for k in KEYS])
    out = torch.full((12,), 7.0, device=DEV)
    r.camera_backward(out)
    r.ctx.synchronize()
    bound = cf.bound("alpha", "z")
    assert np.abs(bound[1]).max() > 0
    _check_camera(out.cpu().numpy(), bound, "crowd, one channel of ones, backward_features + camera_backward")
    fast = torch.full((12,), 7.0, device=DEV)
    r.backward_camera(None, None, dev(cf.ga), fast)
    r.ctx.synchronize()
    _check_camera(fast.cpu().numpy(), bound, "crowd alpha, render_backward_camera")
    # lcgs_densify_accumulate counts the frame on exactly its on-screen rows
    ff = _fframe(oracle, "crowd")
    f = ff.f
    r, _, _ = f.renderer()
    _backward(r, ff, KM)
    stats = {"grad_accum": torch.zeros(f.P, device=DEV), "denom": torch.zeros(f.P, dtype=torch.int32, device=DEV),
             "max_radii": torch.zeros(f.P, dtype=torch.int32, device=DEV)}
    r.densify_accumulate(stats)
    r.ctx.synchronize()
    on = torch.zeros(f.P, dtype=torch.bool, device=DEV)
    on[r.visible_rows().long()] = True
    assert 0 < int(on.sum()) and torch.equal(stats["denom"] == 1, on) and bool((stats["denom"][~on] == 0).all())
    assert bool((stats["grad_accum"][~on] == 0).all()) and bool((stats["grad_accum"][on] > 0).any())
    # the refusal behind a normal gradient stays, with a feature channel in the same call or without
    _backward(r, ff, KM, "nrm+maps", "z")
    with pytest.raises(L.LcgsError) as e:
        r.camera_backward(out)
    assert e.value.status == L.api.LCGS_ERR_STATE and "normal" in str(e.value)
    _backward(r, ff, 3)
    r.camera_backward(out)
    r.ctx.synchronize()


# ----------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("case", ("direct", "frame between"))
def test_autograd(lcgs, oracle, case):
    ff = _fframe(oracle, "crowd")
    f = ff.f
    r = L.Renderer(L.Context(0))
    t = {k: dev(f.scene[k]).requires_grad_(True) for k in KEYS}
    t[FKEY] = dev(ff.feats(KM)).requires_grad_(True)
    img, alpha, fmap = L.render_autograd_features(r, f.cam(), *[t[k] for k in KEYS], t[FKEY], bg=f.bg)
    assert np.array_equal(alpha.detach().cpu().numpy(), f.maps("z")[1])
    assert np.array_equal(fmap.detach().cpu().numpy(), ff.map(KM)[0])
    assert np.array_equal(img.detach().cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])
    if case == "frame between":  # another view's frame replaces the renderer's state: the backward re-renders its own
        other = torch.zeros(3, f.H, f.W, device=DEV)
        r.forward(L.get_lookat_cam(*POSE2, width=f.W, height=f.H), other, keep_state=True, sync=True)
        (fmap * dev(ff.gF(KM))).sum().backward()  # the unused outputs arrive as None: passed as NULL
        bound = ff.bound(KM)
    else:
        ((img * dev(f.gi)).sum() + (alpha * dev(f.ga)).sum() + (fmap * dev(ff.gF(KM))).sum()).backward()
        bound = cached(("features", "autograd bound"), lambda: features_ref.sum_row_bounds(
            [ff.bound(KM), maps_ref.row_bound_with_image(f.scene, f.ocam, f.gi, None, f.ga, bg=f.bg, scale_modifier=f.sm)]))
    torch.cuda.synchronize()
    check_gradient_rows({k: t[k].grad for k in KEYS + (FKEY,)}, None, None, None, bound=bound, tag=f"autograd {case}")


# -------------------------------------------------------------------------------------------------------------------- state
def test_state_and_argument_errors(lcgs, oracle):
    ff = _fframe(oracle, "crowd")
    f = ff.f
    r, d = f.renderer(keep=False)
    K = 3
    g = _fsevens(f.scene, K)
    feats, gF = dev(ff.feats(K)), dev(ff.gF(K))
    out = torch.zeros(K, f.H, f.W, device=DEV)

    def refused(status, fn, *a, **kw):
        with pytest.raises(L.LcgsError) as e:
            fn(*a, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))

    grads = [g[k] for k in KEYS]
    none5 = (None,) * 5
    # no frame at all, then a frame without kept state
    refused(L.api.LCGS_ERR_STATE, r.render_features, feats, out)
    refused(L.api.LCGS_ERR_STATE, r.backward_features, *none5, feats, gF, g[FKEY], *grads)
    refused(L.api.LCGS_ERR_STATE, r.backward_features, *none5, feats, gF, g[FKEY])
    img = torch.zeros(3, f.H, f.W, device=DEV)
    r.forward(f.cam(), img, bg=f.bg, keep_state=False, sync=True)
    refused(L.api.LCGS_ERR_STATE, r.render_features, feats, out)
    refused(L.api.LCGS_ERR_STATE, r.backward_features, None, dev(f.gd), None, None, None, feats, gF, g[FKEY], *grads)
    # a kept frame: argument errors
    f.render(r)
    refused(1, r.render_features, feats[:-1].contiguous(), out)  # rows that are not the bound scene's
    refused(1, r.render_features, feats, None)
    refused(1, r.render_features, torch.zeros(f.P, 0, device=DEV), out)
    refused(1, r.render_features, torch.zeros(f.P, K_MAX + 1, device=DEV), out)
    refused(1, r.backward_features, *none5, None, None, None, *grads)  # every gradient NULL
    refused(1, r.backward_features, *none5, feats, None, g[FKEY], *grads)  # a channel without its map gradient
    refused(1, r.backward_features, *none5, feats, gF, None)  # nothing to write
    refused(1, r.backward_features, None, dev(f.gd), None, None, None, feats, gF, g[FKEY])  # frozen geometry takes no other gradient
    refused(1, r.backward_features, *none5, feats, gF, g[FKEY], *grads, center=float("inf"))
    r.render_features(feats, out)
    # a frame drawn from received records is not this context's own
    rows, recs = r.owner_project(0, f.cam(), 0, f.P, keep_state=True)
    r.owner_render(f.cam(), rows, recs, img, bg=f.bg, keep_state=True)
    refused(L.api.LCGS_ERR_STATE, r.render_features, feats, out)
    refused(L.api.LCGS_ERR_STATE, r.backward_features, *none5, feats, gF, g[FKEY], *grads)
    refused(L.api.LCGS_ERR_STATE, r.backward_features, *none5, feats, gF, g[FKEY])
    r.ctx.synchronize()


def test_forward_and_backward_with_poisoned_workspace():
    """the crowd's forward, the spatial order and one backward case once more in a process whose library fills every fresh
    workspace allocation with garbage (LCGS_POISON=1, tests/test_gpu_poisoned_workspace.py): the walks read nothing they or the
    frame did not write"""
    env = dict(os.environ, LCGS_POISON="1")
    pick = "test_forward_crowd or test_forward_scene_in_spatial_order or (test_backward_rows_features_alone and 17)"
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", pick,
                          "tests/test_gpu_features.py"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "\n6 passed" in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]
