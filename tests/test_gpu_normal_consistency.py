"""`-m gpu`: lcgs_normal_consistency_loss_backward (csrc/kernels/loss.hip) against the float64 restatement of the term in
tests/normal_consistency_ref.py, its determinism, the evaluation-only call, the autograd wrapper behind render_autograd_normals,
and a short training run driven by its gradients.

Every output array (loss, dL_ddepth, dL_dalpha, dL_dnormal) is held element by element, no element excluded, to

    |got - f64| <= 3 E32 + 4 u S

E32: the largest |float32 autograd restatement - float64| over that array on that input, S: the largest |float64 value| in it,
u = 2^-24 (photometric_ref.bound).  Where the bound is 0 (dL_ddepth of a frame whose depth is 0) the array must equal the
reference.  weight and alpha_min cross the C ABI as binary32 numbers, so the restatements are evaluated at float(float32(.)).
Outputs are pre-filled with NaN: a pixel the call does not write fails.  The worst diff / bound per input class is printed and
recorded in docs/TESTS.md."""
import numpy as np
import pytest
import torch

import normal_consistency_ref as R
from conftest import make_scene
from gpu_util import DEV, KEYS, upload_scene

pytestmark = pytest.mark.gpu

TW, TH = 32, 16  # the kernel's tile (csrc/kernels/loss.hip: kTW x kTH)
SIZES = [(3, 3), (4, 3), (5, 7), (37, 53), (320, 240),
         (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (TW + 2, TH + 2)]  # (W, H); the last four: every halo case
CLASSES = R.CLASSES + ("rendered",)
WEIGHT, ALPHA_MIN = 0.05, 1e-3
POSE = ([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])
NAMES = ("loss", "dL_ddepth", "dL_dalpha", "dL_dnormal")


def _cam(lcgs, W, H):
    """the lcgs_camera of R.camera(W, H): the call reads width, height, fov and aspect ratio only"""
    c, cam = R.camera(W, H), lcgs.api.Camera()
    cam.fov, cam.aspect_ratio, cam.width, cam.height = c.fov, c.aspect_ratio, W, H
    assert (float(cam.fov), float(cam.aspect_ratio)) == (c.fov, c.aspect_ratio)
    return cam


def _rendered(lcgs, W, H):
    """the maps of a real frame: a make_scene scene through render_maps and render_normals.  Frames of 16 pixels and less are
    the centre of a 64 x 64 frame (at such sizes most splats fall below the renderer's radius floor)."""
    rw, rh = (W, H) if min(W, H) > 16 else (64, 64)
    scene = make_scene(np.random.default_rng(11 + W), 3000, log_scale=(-3.2, 0.6) if rw * rh > 4096 else (-2.4, 0.6))
    r = lcgs.Renderer(lcgs.Context(0))
    d = upload_scene(scene)
    r.bind_scene(*[d[k] for k in KEYS])
    img = torch.zeros(3, rh, rw, device=DEV)
    r.forward(lcgs.get_lookat_cam(*POSE, width=rw, height=rh), img, keep_state=True, sync=True)
    D, A, N = torch.zeros(rh, rw, device=DEV), torch.zeros(rh, rw, device=DEV), torch.zeros(3, rh, rw, device=DEV)
    r.render_maps(D, A, mode="z")
    r.render_normals(N)
    r.ctx.synchronize()
    assert (A > 0).any(), "the scene must reach the frame"
    y0, x0 = (rh - H) // 2, (rw - W) // 2
    return tuple(t[..., y0:y0 + H, x0:x0 + W].contiguous() for t in (D, A, N))


def _inputs(lcgs, kind, W, H):
    if kind == "rendered":
        return _rendered(lcgs, W, H)
    return tuple(t.to(DEV) for t in R.inputs(kind, W, H, ALPHA_MIN))


def _call(lcgs, r, D, A, N, weight=WEIGHT, alpha_min=ALPHA_MIN, with_grad=True):
    """(loss, dL_ddepth, dL_dalpha, dL_dnormal) onto NaN"""
    H, W = A.shape
    grads = [torch.full_like(t, float("nan")) if with_grad else None for t in (D, A, N)]
    loss = torch.full((1,), float("nan"), device=DEV)
    r.normal_consistency_loss_backward(_cam(lcgs, W, H), D, A, N, *grads, loss, weight, alpha_min)
    r.ctx.synchronize()
    torch.cuda.synchronize()
    return (loss, *grads)


def _held(got, ref64, ref32, tag):
    """worst |got - f64| / bound over one output array"""
    got, ref64 = got.detach().cpu().double().reshape(-1), ref64.double().reshape(-1)
    assert torch.isfinite(got).all(), tag
    b = R.bound(ref64, ref32.reshape(-1))
    return ((got - ref64).abs().max().item() / b) if b > 0 else (0.0 if torch.equal(got, ref64) else float("inf"))


def _check_against_the_restatement(lcgs, r, D, A, N, tag):
    H, W = A.shape
    w32, a32, cam = R.abi32(WEIGHT), R.abi32(ALPHA_MIN), R.camera(W, H)
    ref64 = R.autograd(D, A, N, cam, w32, a32, torch.float64)
    ref32 = R.autograd(D, A, N, cam, w32, a32, torch.float32)
    got = _call(lcgs, r, D, A, N)
    ratios = {name: _held(g, a, b, f"{tag} {name}") for name, g, a, b in zip(NAMES, got, ref64, ref32)}
    print(f"[normal consistency vs f64] {tag}: diff/bound " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()) +
          f" (loss {got[0].item():.7f})")
    for k, v in ratios.items():
        assert v <= 1.0, f"{tag}: {k} at {v:.3f} x its bound"
    return got, ref64


@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("W,H", SIZES)
def test_loss_and_gradients_against_the_float64_restatement(lcgs, W, H, kind):
    r = lcgs.Renderer(lcgs.Context(0))
    D, A, N = _inputs(lcgs, kind, W, H)
    got, ref64 = _check_against_the_restatement(lcgs, r, D, A, N, f"{kind} {W}x{H}")
    if kind == "degenerate":  # m = 0 everywhere: everything finite (checked above), nothing reaches the depth
        assert bool((got[1] == 0).all()) and bool((ref64[1] == 0).all())
    if kind == "holes":
        assert bool((A == 0).any()) and bool((A == R.abi32(ALPHA_MIN)).any())
        assert W * H < 1000 or 0.25 < (A < R.abi32(ALPHA_MIN)).float().mean().item() < 0.35


def test_evaluation_only_gives_the_same_loss_and_writes_no_gradient(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    D, A, N = _inputs(lcgs, "noisy", 320, 240)
    loss, *grads = _call(lcgs, r, D, A, N)
    assert all(torch.isfinite(g).all() for g in grads)
    for g in grads:
        g.fill_(-123.0)  # the buffers of the call before: an evaluation-only call must not remember them
    loss_e = _call(lcgs, r, D, A, N, with_grad=False)[0]
    assert torch.equal(loss_e, loss)
    assert all(torch.equal(g, torch.full_like(g, -123.0)) for g in grads)
    # ... and on a fresh context
    loss_f = _call(lcgs, lcgs.Renderer(lcgs.Context(0)), D, A, N, with_grad=False)[0]
    assert torch.equal(loss_f, loss)


def test_two_calls_give_the_same_bits(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    D, A, N = _inputs(lcgs, "noisy", 1920, 1080)
    a, b = _call(lcgs, r, D, A, N), _call(lcgs, r, D, A, N)
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)


def test_a_small_call_after_a_large_one_is_not_reached_by_the_stale_workspace(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    _call(lcgs, r, *_inputs(lcgs, "noisy", 1920, 1080))
    D, A, N = _inputs(lcgs, "noisy", 37, 53)
    got, _ = _check_against_the_restatement(lcgs, r, D, A, N, "noisy 37x53 after 1920x1080")
    fresh = _call(lcgs, lcgs.Renderer(lcgs.Context(0)), D, A, N)
    for u, v in zip(got, fresh):
        assert torch.equal(u, v)


def test_weight_zero_gives_exact_zeros(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    for kind in ("noisy", "holes", "degenerate"):
        for out in _call(lcgs, r, *_inputs(lcgs, kind, 37, 53), weight=0.0):
            assert bool((out == 0).all()), kind


def _grads_agree(got, want, tag):
    """tests/test_gpu_photometric.py::_grads_agree: relative norm 2e-4 and the same zero pattern (the render backward sums with
    float atomics: bit equality is not on offer)"""
    for k in KEYS:
        num, den = (got[k] - want[k]).double().norm().item(), want[k].double().norm().item()
        print(f"[normal consistency end to end] {tag} {k}: |got - want| / |want| = {num / max(den, 1e-300):.2e}")
        assert num <= 2e-4 * den + 1e-12, (tag, k, num, den)
        assert torch.equal(got[k] == 0, want[k] == 0), (tag, k)


def test_autograd_end_to_end_equals_the_reference_gradients_through_backward_normals(lcgs):
    """render_autograd_normals -> normal_consistency_autograd -> backward(): the parameter gradients against those of the float64
    restatement's three gradients fed to Renderer.backward_normals on the same frame"""
    import maps_ref

    scene, pose, W, H = maps_ref.crowd()
    cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
    r = lcgs.Renderer(lcgs.Context(0))
    t = {k: v.requires_grad_(True) for k, v in upload_scene(scene).items()}
    _, depth, alpha, _, normal = lcgs.render_autograd_normals(r, cam, *[t[k] for k in KEYS])
    loss = lcgs.normal_consistency_autograd(r, cam, depth, alpha, normal, WEIGHT, ALPHA_MIN)
    assert loss.dim() == 0 and loss.requires_grad
    (2.0 * loss).backward()  # (the incoming scalar scales the stored gradients)
    torch.cuda.synchronize()
    got = {k: t[k].grad.clone() for k in KEYS}
    ref = R.autograd(depth, alpha, normal, cam, R.abi32(WEIGHT), R.abi32(ALPHA_MIN))
    assert abs(loss.item() - ref[0].item()) <= 1e-5 * abs(ref[0].item()) + 1e-9
    gd, ga, gn = ((2.0 * g).float().to(DEV).contiguous() for g in ref[1:])
    assert all(bool((g != 0).any()) for g in (gd, ga, gn))
    r2 = lcgs.Renderer(lcgs.Context(0))
    d = upload_scene(scene)
    r2.bind_scene(*[d[k] for k in KEYS])
    r2.forward(cam, torch.zeros(3, H, W, device=DEV), keep_state=True, sync=True)
    want = {k: torch.full_like(d[k], 7.0) for k in KEYS}
    r2.backward_normals(None, gd, ga, None, gn, *[want[k] for k in KEYS], mode="z")
    r2.ctx.synchronize()
    assert bool((want["rotq"] != 0).any()) and bool((want["pos"] != 0).any())
    _grads_agree(got, want, "crowd")


TRAIN_LR = {"pos": 0.0, "sh_dc": 0.0, "sh_rest": 0.0, "opacity": 0.0, "scale": 0.0, "rot": 2e-2}


def train(lcgs, lr, steps=30):
    """`steps` Adam steps on the normal-consistency loss alone (weight 1), driven from Python through backward_normals -> losses"""
    P, W, H = 20000, 320, 240
    scene = lcgs.synth_scene(0, 1001, P)
    cam = lcgs.get_lookat_cam(*POSE, width=W, height=H)
    r = lcgs.Renderer(lcgs.Context(0))
    op = np.clip(scene["opacity"], 1e-6, 1 - 1e-6)
    raw = {"pos": scene["pos"], "scale": np.log(scene["scale"]), "rotq": scene["rotq"], "sh": scene["sh"], "opacity": np.log(op / (1 - op))}
    raw = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV) for k, v in raw.items()}
    act = {"pos": raw["pos"], "scale": torch.exp(raw["scale"]), "rotq": raw["rotq"].clone(), "sh": raw["sh"],
           "opacity": torch.sigmoid(raw["opacity"])}
    m = {k: torch.zeros_like(raw[k]) for k in KEYS}
    v = {k: torch.zeros_like(raw[k]) for k in KEYS}
    g = {k: torch.zeros_like(raw[k]) for k in KEYS}
    r.bind_scene(*[act[k] for k in KEYS])
    img = torch.zeros(3, H, W, device=DEV)
    D, A, N = torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV), torch.zeros(3, H, W, device=DEV)
    gd, ga, gn = torch.zeros_like(D), torch.zeros_like(A), torch.zeros_like(N)
    loss_all = torch.zeros(steps, device=DEV)
    for step in range(1, steps + 1):
        r.forward(cam, img, keep_state=True, sync=False)
        r.render_maps(D, A, mode="z")
        r.render_normals(N)
        r.normal_consistency_loss_backward(cam, D, A, N, gd, ga, gn, loss_all[step - 1:step], 1.0, ALPHA_MIN)
        r.backward_normals(None, gd, ga, None, gn, *[g[k] for k in KEYS], mode="z")
        r.adam_step(g, raw, m, v, act, step, lr)
    r.ctx.synchronize()
    return loss_all.cpu().tolist()


def test_thirty_adam_steps_on_the_normal_consistency_gradient_train(lcgs):
    losses = train(lcgs, TRAIN_LR)
    print(f"[normal consistency training] loss {losses[0]:.6f} -> {losses[-1]:.6f} (ratio {losses[-1] / losses[0]:.3f}); "
          f"min of the first five {min(losses[:5]):.6f}, of the last five {min(losses[-5:]):.6f}")
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0] and min(losses[-5:]) < min(losses[:5]), losses
