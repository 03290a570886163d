"""`-m gpu`: the camera gradient (lcgs_camera_backward, lcgs_render_backward_camera, kernels/camera_grad.hip).

All twelve components, none excluded anywhere, against tests/camera_grad_ref.py's f64 reference within its bound: the crowd and
random draws 100 - 103 (102: giants, the f64 branch) x {colour, depth, alpha, all three} x both depth modes, each through a
backward + lcgs_camera_backward and again through lcgs_render_backward_camera; frames of 1, 255, 256, 257 and 513 on-screen rows
(the block boundaries of the reduction); a frame that draws nothing; same rows -> same bits; consistency with the parameter
pass's dL/dpos; behind the compact and the fused-Adam backward, a degree-1 scene (the SH-row path), a context-owned scene in
spatial order; the fast path writes no parameter rows and leaves the next backward alone; state errors; the autograd wrapper.
Worst diff / bound seen: docs/TESTS.md."""
import numpy as np
import pytest
import torch

import camera_grad_ref as cgr
import luisacomputegaussiansplatting_amd as L
import maps_ref
from gpu_util import BG, DEV, KEYS, View, cached, check_gradient_rows, dev, gradient_row_bound, random_draw, sevens, upload_scene

pytestmark = pytest.mark.gpu
FRAMES = ("crowd", 100, 101, 102, 103)  # 102: needles and giants
VARIANTS = ("colour", "depth", "alpha", "all")
AWAY = ([1.6, 0.3, 0.9], [5.0, 1.0, 1.3], [0.0, 0.0, 1.0])  # the crowd behind the camera
BLOCK_ROWS = (1, 255, 256, 257, 513)


class Frame:
    """one (scene, pose, resolution, fov, bg, scale modifier) with its incoming gradients; bounds computed once and shared"""

    def __init__(self, oracle, key, scene=None, sh_deg=3):
        if key == "crowd":
            self.scene, self.pose, self.W, self.H = maps_ref.crowd()
            self.fov, self.bg, self.sm = None, BG, 1.0
            rng = np.random.default_rng(17)
        else:
            rng, self.scene, self.W, self.H, self.pose, self.fov, self.bg, self.sm = random_draw(key)
        if scene is not None:
            self.scene = scene
        self.key, self.oracle, self.sh_deg = key, oracle, sh_deg
        self.P = self.scene["pos"].shape[0]
        self.ocam = oracle.lookat(*self.pose, width=self.W, height=self.H, fov=self.fov)
        shape = (self.H, self.W)
        self.gd, self.ga = rng.normal(size=shape).astype(np.float32), rng.normal(size=shape).astype(np.float32)
        self.gi = rng.normal(size=(3,) + shape).astype(np.float32)
        self._bounds, self._rows = {}, {}

    def cam(self):
        return L.get_lookat_cam(*self.pose, width=self.W, height=self.H, fov=self.fov)

    def incoming(self, variant):
        """(dL_dimg, dL_ddepth, dL_dalpha) of a variant; None = NULL"""
        return (self.gi if variant in ("colour", "all") else None, self.gd if variant in ("depth", "all") else None,
                self.ga if variant in ("alpha", "all") else None)

    def _key(self, variant, mode):
        return (variant, "z" if variant == "colour" else mode)  # (without a map gradient the mode is not read)

    def rows_bound(self, variant, mode):
        """the per-row bound of the parameter gradients of the same call (gpu_util / maps_ref)"""
        k = self._key(variant, mode)
        if k not in self._rows:
            gi, gd, ga = self.incoming(variant)
            kw = dict(scale_modifier=self.sm, sh_deg=self.sh_deg)
            if gd is None and ga is None:
                self._rows[k] = gradient_row_bound(self.scene, self.ocam, gi, bg=self.bg, **kw)
            elif gi is None:
                self._rows[k] = maps_ref.row_bound(self.scene, self.ocam, gd, ga, mode=k[1], **kw)
            else:
                self._rows[k] = maps_ref.row_bound_with_image(self.scene, self.ocam, gi, gd, ga, mode=k[1], bg=self.bg, **kw)
        return self._rows[k]

    def bound(self, variant, mode):
        k = self._key(variant, mode)
        if k not in self._bounds:
            self._bounds[k] = cgr.bound(self.scene, self.ocam, *self.incoming(variant), mode=k[1], bg=self.bg,
                                        scale_modifier=self.sm, sh_deg=self.sh_deg, pos_bound=self.rows_bound(variant, mode)[0]["pos"])
        return self._bounds[k]

    def renderer(self, keep=True, owned=False):
        """a fresh context with the scene bound (owned: uploaded, in spatial order) and the frame rendered"""
        r = L.Renderer(L.Context(0))
        if owned:
            r.upload_scene(self.scene, sh_degree=self.sh_deg)
            d = None
        else:
            d = upload_scene(self.scene)
            r.bind_scene(*[d[k] for k in KEYS], sh_degree=self.sh_deg)
        if keep:
            self.render(r)
        return r, d

    def render(self, r, cam=None, expect_drawn=True):
        img = torch.full((3, self.H, self.W), -1.0, device=DEV)
        n = r.forward(cam or self.cam(), img, bg=self.bg, scale_modifier=self.sm, keep_state=True, sync=True)
        assert (n > 0) == expect_drawn, self.key
        return img


def _frame(oracle, key):
    return cached(("camera", key), lambda: Frame(oracle, key))


def _d(a):
    return None if a is None else dev(a)


def _out(fill=7.0):
    return torch.full((12,), fill, device=DEV)


def _via_backward(r, f, variant, mode, compact=False):
    """a backward that writes parameter rows, then lcgs_camera_backward -> (the twelve floats, the rows)"""
    gi, gd, ga = f.incoming(variant)
    g = sevens(f.scene)
    if gd is None and ga is None:
        r.backward(_d(gi), *[g[k] for k in KEYS], compact=compact)
    else:
        assert not compact
        r.backward_maps(_d(gi), _d(gd), _d(ga), *[g[k] for k in KEYS], mode=mode)
    out = _out()
    r.camera_backward(out)
    r.ctx.synchronize()
    return out.cpu().numpy(), g


def _fast(r, f, variant, mode, fill=7.0):
    out = _out(fill)
    r.backward_camera(*[_d(a) for a in f.incoming(variant)], out, mode=mode)
    r.ctx.synchronize()
    return out.cpu().numpy()


def _check(got, bound, tag):
    B, r64 = bound
    assert got.dtype == np.float32 and got.shape == (12,) and np.isfinite(got).all(), (tag, got)
    diff = np.abs(got.astype(np.float64) - r64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(B > 0, diff / B, np.where(diff > 0, np.inf, 0.0))
    k = int(np.argmax(ratio))
    print(f"[camera gradient vs f64] {tag}: worst diff/bound {ratio[k]:.3f} (component {k}: {got[k]:.6e} vs {r64[k]:.6e}, "
          f"bound {B[k]:.2e}); |r64| {np.abs(r64).min():.2e} .. {np.abs(r64).max():.2e}")
    assert (ratio <= 1.0).all(), f"{tag}: components {np.nonzero(ratio > 1.0)[0].tolist()} over their bound, ratios {ratio.round(3).tolist()}"
    return float(ratio[k])


# ------------------------------------------------------------------------------------------------- the crowd and random draws
@pytest.mark.parametrize("mode", maps_ref.MODES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("key", FRAMES)
def test_camera_gradient(lcgs, oracle, key, variant, mode):
    f = _frame(oracle, key)
    r, _ = f.renderer()
    bound = f.bound(variant, mode)
    assert np.abs(bound[1]).max() > 0
    got, _ = _via_backward(r, f, variant, mode)
    _check(got, bound, f"{key} {variant} {mode}, backward + camera_backward")
    _check(_fast(r, f, variant, mode), bound, f"{key} {variant} {mode}, render_backward_camera")


# ------------------------------------------------------------------------------------------ block boundaries of the reduction
@pytest.mark.parametrize("rows", BLOCK_ROWS)
def test_block_boundaries_of_the_reduction(lcgs, oracle, rows):
    full = _frame(oracle, "crowd")

    def visible():
        r, _ = full.renderer()
        return r.visible_rows().cpu().numpy()
    vis = cached(("camera", "crowd visible"), visible)
    n = int(vis[rows - 1]) + 1  # the shortest prefix of the crowd with `rows` on-screen splats (the cull is per splat)
    f = cached(("camera", "prefix", rows), lambda: Frame(oracle, "crowd", scene={k: full.scene[k][:n].copy() for k in KEYS}))
    r, _ = f.renderer()
    assert r.frame_stats()["num_visible"] == rows
    bound = f.bound("all", "inv_z")
    got, _ = _via_backward(r, f, "all", "inv_z")
    _check(got, bound, f"{rows} on-screen rows, backward_maps + camera_backward")
    _check(_fast(r, f, "all", "inv_z"), bound, f"{rows} on-screen rows, render_backward_camera")


def test_frame_that_draws_nothing(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer(keep=False)
    f.render(r, L.get_lookat_cam(*AWAY, width=f.W, height=f.H), expect_drawn=False)
    assert r.frame_stats()["num_visible"] == 0
    for variant in ("colour", "all"):
        got = _fast(r, f, variant, "z")
        assert np.array_equal(got, np.zeros(12, np.float32)), (variant, got)  # twelve exact zeros over the 7.0-filled buffer
    got, _ = _via_backward(r, f, "all", "inv_z")
    assert np.array_equal(got, np.zeros(12, np.float32)), got


def test_same_rows_same_bits(lcgs, oracle):
    f = _frame(oracle, 102)
    r, _ = f.renderer()
    first, _ = _via_backward(r, f, "all", "z")
    again, other = _out(7.0), _out(-3.0)
    r.camera_backward(again)
    r.camera_backward(other)
    r.ctx.synchronize()
    assert np.array_equal(first, again.cpu().numpy()) and np.array_equal(first, other.cpu().numpy())
    assert np.abs(first).min() > 0


@pytest.mark.parametrize("variant,mode", (("colour", "z"), ("all", "z"), ("all", "inv_z")))
def test_position_agrees_with_the_parameter_pass(lcgs, oracle, variant, mode):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer()
    got, g = _via_backward(r, f, variant, mode)
    want = -g["pos"].double().sum(dim=0).cpu().numpy()
    B = f.bound(variant, mode)[0][0:3]
    assert (np.abs(got[0:3].astype(np.float64) - want) <= B).all(), (got[0:3], want, B)


# ---------------------------------------------------------------------------------------------------- other backward variants
def test_behind_the_compact_backward(lcgs, oracle):
    f = _frame(oracle, 101)
    r, _ = f.renderer()
    got, _ = _via_backward(r, f, "colour", "z", compact=True)
    _check(got, f.bound("colour", "z"), "101 colour, backward_compact + camera_backward")


def _activate(raw):
    return {"pos": raw["pos"], "scale": torch.exp(raw["scale"]), "sh": raw["sh"], "opacity": torch.sigmoid(raw["opacity"]),
            "rotq": raw["rotq"] / raw["rotq"].norm(dim=1, keepdim=True)}


def test_behind_the_fused_adam_backward(lcgs, oracle):
    """lcgs_camera_backward re-evaluates geometry from the bound arrays, so behind lcgs_render_backward_adam it sees the scene
    AFTER the step.  All learning rates are zero here: the step rewrites the activated arrays from the raw ones (scale = exp,
    opacity = sigmoid, rotq normalised: the same values to within an ulp) and nothing else, so the reference of the frame still
    applies; a second context runs the plain backward on the same frame."""
    f = _frame(oracle, "crowd")
    s = f.scene
    raw = {"pos": dev(s["pos"]), "scale": torch.log(dev(s["scale"])), "rotq": dev(s["rotq"]), "sh": dev(s["sh"]),
           "opacity": torch.logit(dev(s["opacity"]))}
    act = {k: dev(s[k]) for k in KEYS}
    act["pos"], act["sh"] = raw["pos"], raw["sh"]  # identity activations: one array
    m, v = ({k: torch.zeros_like(raw[k]) for k in KEYS} for _ in range(2))
    r = L.Renderer(L.Context(0))
    r.bind_scene(*[act[k] for k in KEYS])
    f.render(r)
    lr = {k: 0.0 for k in ("pos", "sh_dc", "sh_rest", "opacity", "scale", "rot")}
    r.backward_adam(dev(f.gi), raw, m, v, act, 1, lr, eps=1e-8)
    out = _out()
    r.camera_backward(out)
    r.ctx.synchronize()
    # the step moved nothing beyond the activations' own rounding: exp(fl(log s)) is off by about |log s| u <= 7 u here (plus
    # an ulp or two of log and exp themselves), logit -> sigmoid likewise
    for k in ("scale", "rotq", "opacity"):
        assert torch.allclose(act[k], dev(s[k]), rtol=2e-6, atol=0.0), k
    bound = f.bound("colour", "z")
    _check(out.cpu().numpy(), bound, "crowd colour, backward_adam (zero rates) + camera_backward")
    r2, _ = f.renderer()
    got2, _ = _via_backward(r2, f, "colour", "z")
    _check(got2, bound, "crowd colour, plain backward in a second context")


def test_degree_one_scene_takes_the_sh_row_path(lcgs, oracle):
    full = _frame(oracle, 100)
    scene = {k: (full.scene[k][:, :12].copy() if k == "sh" else full.scene[k]) for k in KEYS}  # (flat rows: 4 coefficients x 3)
    f = cached(("camera", "degree 1"), lambda: Frame(oracle, 100, scene=scene, sh_deg=1))
    r, _ = f.renderer()
    got, _ = _via_backward(r, f, "all", "z")
    _check(got, f.bound("all", "z"), "degree 1, backward_maps + camera_backward")
    _check(_fast(r, f, "colour", "z"), f.bound("colour", "z"), "degree 1, render_backward_camera")


def test_context_owned_scene_in_spatial_order(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer(owned=True)
    assert r.permutation() is not None
    _check(_fast(r, f, "all", "inv_z"), f.bound("all", "inv_z"), "spatial order, render_backward_camera")
    out = _out()
    r.camera_backward(out)  # the fast path counts as a backward of the frame
    r.ctx.synchronize()
    _check(out.cpu().numpy(), f.bound("all", "inv_z"), "spatial order, camera_backward behind the fast path")


# ------------------------------------------------------------------------------------- the fast path writes no parameter rows
def test_fast_path_leaves_the_next_backward_alone(lcgs, oracle):
    scene, pose, W, H = maps_ref.crowd()
    v = cached(("camera", "crowd view"), lambda: View(oracle, scene, pose, W, H, seed=2))
    f = _frame(oracle, "crowd")
    r, _ = f.renderer()
    _check(_fast(r, f, "all", "inv_z"), f.bound("all", "inv_z"), "fast path before a plain backward")
    stats = {"grad_accum": torch.zeros(f.P, device=DEV), "denom": torch.zeros(f.P, dtype=torch.int32, device=DEV),
             "max_radii": torch.zeros(f.P, dtype=torch.int32, device=DEV)}
    r.densify_accumulate(stats)  # the fast path counts as a backward of the frame
    r.ctx.synchronize()
    assert int(stats["denom"].sum()) == r.frame_stats()["num_visible"] and float(stats["grad_accum"].sum()) > 0
    g = sevens(scene)
    r.backward(dev(v.dL), *[g[k] for k in KEYS])  # the same frame: the rows it gives in a fresh context
    r.ctx.synchronize()
    check_gradient_rows(g, None, None, None, bound=v.bound(), tag="plain backward after the camera fast path")


# -------------------------------------------------------------------------------------------------------------------- state
def test_state_errors(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer(keep=False)
    out = _out()

    def refused(fn, *a, **kw):
        with pytest.raises(L.LcgsError) as e:
            fn(*a, **kw)
        assert e.value.status == L.api.LCGS_ERR_STATE, (e.value.status, str(e.value))

    refused(r.camera_backward, out)  # no frame
    refused(r.backward_camera, dev(f.gi), None, None, out)
    img = torch.zeros(3, f.H, f.W, device=DEV)
    r.forward(f.cam(), img, bg=f.bg, keep_state=False, sync=True)  # a frame without kept state
    refused(r.camera_backward, out)
    refused(r.backward_camera, dev(f.gi), None, None, out)
    f.render(r)
    refused(r.camera_backward, out)  # no backward of the frame yet
    g = sevens(f.scene)
    r.backward(dev(f.gi), *[g[k] for k in KEYS])
    r.camera_backward(out)
    f.render(r)  # a new forward: its rows are only zeros again
    refused(r.camera_backward, out)
    r.backward_camera(None, None, dev(f.ga), out)
    r.camera_backward(out)
    # a frame drawn from received records is not this context's own
    rows, recs = r.owner_project(0, f.cam(), 0, f.P, keep_state=True)
    r.owner_render(f.cam(), rows, recs, img, bg=f.bg, keep_state=True)
    refused(r.camera_backward, out)
    refused(r.backward_camera, dev(f.gi), None, None, out)
    r.ctx.synchronize()
    assert bool((out != 7.0).all())


# ----------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("case", ("camera only", "camera and scene"))
def test_autograd(lcgs, oracle, case):
    f = _frame(oracle, "crowd")
    mode = "inv_z"
    r = L.Renderer(L.Context(0))
    with_scene = case == "camera and scene"
    t = {k: dev(f.scene[k]).requires_grad_(with_scene) for k in KEYS}
    cam = f.cam()
    c12 = torch.tensor(cgr.cam12(cam), dtype=torch.float32).requires_grad_(True)
    img, depth, alpha = L.render_autograd_camera(r, cam, c12, *[t[k] for k in KEYS], bg=f.bg, mode=mode)
    assert np.array_equal(img.detach().cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])
    ((img * dev(f.gi)).sum() + (depth * dev(f.gd)).sum() + (alpha * dev(f.ga)).sum()).backward()
    torch.cuda.synchronize()
    assert c12.grad is not None and c12.grad.shape == (12,)
    _check(c12.grad.numpy(), f.bound("all", mode), f"autograd, {case}")
    if with_scene:
        check_gradient_rows({k: t[k].grad for k in KEYS}, None, None, None, bound=f.rows_bound("all", mode), tag="autograd, scene rows")
    else:
        assert all(t[k].grad is None for k in KEYS)
