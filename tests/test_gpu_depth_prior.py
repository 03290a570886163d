"""`-m gpu`: lcgs_depth_prior_loss_backward (csrc/kernels/depth_prior.hip) against the float64 restatement of the two terms in
tests/depth_prior_ref.py, its determinism, the evaluation-only call, the autograd wrapper behind render_autograd_maps, and a
short training run driven by its gradients.

Every output array (loss, dL_ddepth, dL_dalpha, stats[2:4]) is held element by element to

    |got - f64| <= 3 E32 + 4 u S

E32: the largest |float32 autograd restatement - float64| over that array on that input, S: the largest |float64 value| in it,
u = 2^-24 (photometric_ref.bound).  Where the bound is 0 the array must equal the reference; stats[0:2] (N_c, G) are exact.
weight, alpha_min, scale and shift cross the C ABI as binary32 numbers, so the restatements are evaluated at abi32(.).  Outputs
are pre-filled with NaN: a pixel the call does not write fails.

The L1 gradient is weight / N_c sign(res): a pixel whose residual is smaller than what binary32 resolves has no decided sign.
Such a pixel, |res| <= tau with tau = 3 E32(res) + 4 u max|res| (the same bound, applied to the float64 residual array), is left
out of the element-wise comparison (E32 is then taken over the remaining pixels) but must still satisfy |dL/ddepth| <=
weight / (N_c max(alpha, alpha_min)) and |dL/dalpha| <= weight |depth| / (N_c alpha^2), plus their rounding; at most 1 % of
the counted pixels may be left out.  tau == 0 leaves nothing out: every residual is then 0 in binary32 and binary64 alike.
On class "affine" EVERY residual of the fitted alignment is rounding (the fit finds the planted pair), and so it is on a 2 x 1
frame (a line fitted to two points passes through both): only the loss bound and the magnitude bounds are asserted there
(depth_prior_ref.fit_is_exact).
The worst diff / bound per input class is printed and recorded in docs/TESTS.md."""
import functools

import numpy as np
import pytest
import torch

import depth_prior_ref as R
from gpu_util import DEV, KEYS, upload_scene

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 1), (5, 7), (37, 53), (31, 15), (32, 16), (33, 17), (320, 240)]  # (W, H); 32 x 16 is the kernels' tile
PATCHES = [(33, 17, 32, (0, 0)), (33, 17, 32, (1, 1)), (33, 17, 32, (31, 31)), (320, 240, 64, (0, 0)), (320, 240, 64, (17, 40)),
           (320, 240, 128, (0, 0)),
           (29, 31, 32, (0, 0)), (100, 100, 128, (0, 0))]  # (W, H, patch, offset); the last two: a patch grid of ONE group
WEIGHT, ALPHA_MIN = 0.7, 1e-3
W32, A32 = R.abi32(WEIGHT), R.abi32(ALPHA_MIN)
VARIANTS = {"pearson": dict(kind="pearson"), "l1_fit": dict(kind="l1"),
            "l1_given": dict(kind="l1", align="given", scale=R.abi32(0.37), shift=R.abi32(1.9))}
POSE = ([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])
_RENDERER = {}


def _renderer(lcgs):
    """one context for the comparisons (the tests about contexts make their own)"""
    if "r" not in _RENDERER:
        _RENDERER["r"] = lcgs.Renderer(lcgs.Context(0))
    return _RENDERER["r"]


@functools.lru_cache(maxsize=None)
def _case(kind, W, H, variant, patch=0, offset=(0, 0)):
    """the inputs of one case and its two restatements, computed once"""
    D, A, M, mask = R.inputs(kind, W, H, ALPHA_MIN)
    kw = dict(weight=W32, alpha_min=A32, patch=patch, patch_offset=offset, **VARIANTS[variant])
    ref64, ref32 = R.autograd(D, A, M, mask, **kw), R.autograd(D, A, M, mask, dtype=torch.float32, **kw)
    counted = R.counted_pixels(A, M, mask, kw.get("align", "fit"), patch, offset)
    return (D, A, M, mask), ref64, ref32, counted


def _call(r, D, A, M, mask, variant, weight=WEIGHT, patch=0, offset=(0, 0), with_grad=True):
    """(loss, dL_ddepth, dL_dalpha, stats) onto NaN; inputs anywhere, moved to the device"""
    D, A, M = (t.to(DEV) for t in (D, A, M))
    mask = None if mask is None else mask.to(DEV)
    grads = [torch.full_like(t, float("nan")) if with_grad else None for t in (D, A)]
    loss, stats = torch.full((1,), float("nan"), device=DEV), torch.full((4,), float("nan"), device=DEV)
    r.depth_prior_loss_backward(D, A, M, *grads, loss, mask=mask, weight=weight, alpha_min=ALPHA_MIN, patch=patch,
                                patch_offset=offset, stats=stats, **VARIANTS[variant])
    r.ctx.synchronize()
    torch.cuda.synchronize()
    return (loss, *grads, stats)


def _held(got, ref64, ref32, tag):
    """worst |got - f64| / bound over one output array"""
    got, ref64 = got.detach().cpu().double().reshape(-1), ref64.double().reshape(-1)
    assert torch.isfinite(got).all(), tag
    if got.numel() == 0:
        return 0.0
    b = R.bound(ref64, ref32.reshape(-1))
    return ((got - ref64).abs().max().item() / b) if b > 0 else (0.0 if torch.equal(got, ref64) else float("inf"))


def _check_against_the_restatement(r, kind, W, H, variant, patch=0, offset=(0, 0)):
    (D, A, M, mask), ref64, ref32, counted = _case(kind, W, H, variant, patch, offset)
    tag = f"{kind} {variant} {W}x{H}" + (f" patch {patch} at -{offset}" if patch else "")
    got = _call(r, D, A, M, mask, variant, patch=patch, offset=offset)
    loss, gd, ga, stats = (g.cpu().double() for g in got)
    assert all(torch.isfinite(g).all() for g in (loss, gd, ga, stats)), tag
    assert torch.equal(stats[:2], ref64[3][:2]), (tag, stats, ref64[3])
    ratios = {"loss": _held(loss, ref64[0], ref32[0], tag), "stats[2:4]": _held(stats[2:], ref64[3][2:], ref32[3][2:], tag)}
    assert bool((gd[~counted] == 0).all()) and bool((ga[~counted] == 0).all()), tag  # exact zeros off the counted pixels
    left_out = torch.zeros_like(counted)
    if variant != "pearson":
        n_c = max(int(counted.sum()), 1)
        tau = R.tau(ref64[4], ref32[4])
        rounding_only = R.fit_is_exact(kind, VARIANTS[variant].get("align", "fit"), int(counted.sum()), patch)
        left_out = R.sign_undecided(ref64[4], ref32[4], counted, rounding_only)
        # what a pixel's gradients can be at most, whatever its sign: (1 + 4u) covers the rounding of k = weight / N_c, of the
        # division or the product chain behind it and of the binary32 result
        A64, D64 = A.double(), D.double()
        cap_d = W32 / (n_c * A64.clamp_min(A32)) * (1 + 4 * R.U32)
        cap_a = torch.where(A64 >= A32, W32 * D64.abs() / (n_c * A64 * A64), torch.zeros_like(A64)) * (1 + 4 * R.U32)
        assert bool((gd.abs() <= cap_d)[left_out].all()) and bool((ga.abs() <= cap_a)[left_out].all()), tag
        assert rounding_only or int(left_out.sum()) <= 0.01 * n_c, (tag, int(left_out.sum()), n_c, tau)
    keep = ~left_out
    ratios["dL_ddepth"] = _held(gd[keep], ref64[1][keep], ref32[1][keep], tag)
    ratios["dL_dalpha"] = _held(ga[keep], ref64[2][keep], ref32[2][keep], tag)
    print(f"[depth prior vs f64] {tag}: diff/bound " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()) +
          f" (loss {loss.item():.7f}, N_c {int(stats[0])}, G {int(stats[1])}, left out {int(left_out.sum())})")
    for k, v in ratios.items():
        assert v <= 1.0, f"{tag}: {k} at {v:.3f} x its bound"
    return got, ref64


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", R.CLASSES)
@pytest.mark.parametrize("W,H", SIZES)
def test_loss_and_gradients_against_the_float64_restatement(lcgs, W, H, kind, variant):
    (D, A, M, mask), _, _, counted = _case(kind, W, H, variant)
    got, ref64 = _check_against_the_restatement(_renderer(lcgs), kind, W, H, variant)
    loss, gd, ga, stats = got
    if kind == "constant_prior" and variant == "pearson":  # m - mu_m = 0 exactly: r = 0, nothing reaches the maps
        assert bool((gd == 0).all()) and bool((ga == 0).all())
        assert W * H < 2 or loss.item() == float(np.float32(WEIGHT))
    if kind in ("none_valid", "one_valid") and variant != "l1_given":  # no counted group
        assert loss.item() == 0 and bool((gd == 0).all()) and bool((ga == 0).all()) and bool((stats[:2] == 0).all())
    if kind == "one_valid" and variant == "l1_given":  # ... but one valid pixel suffices for a given alignment
        assert stats[:2].tolist() == [1.0, 1.0] and int((gd != 0).sum()) == 1
    if kind == "holes" and W * H >= 1000:
        assert bool((A == 0).any()) and bool((A == A32).any()) and bool(torch.isnan(M).any()) and bool(torch.isinf(M).any())
        assert 0.25 < (A < A32).float().mean().item() < 0.35 and 0.25 < (mask == 0).float().mean().item() < 0.35
        assert 0.5 * W * H < int(counted.sum()) < 0.75 * W * H


@pytest.mark.parametrize("variant", ("pearson", "l1_fit"))
@pytest.mark.parametrize("kind", ("noisy", "holes"))
@pytest.mark.parametrize("W,H,patch,offset", PATCHES)
def test_patch_mode_against_the_float64_restatement(lcgs, W, H, patch, offset, kind, variant):
    got, ref64 = _check_against_the_restatement(_renderer(lcgs), kind, W, H, variant, patch, offset)
    groups = ((W + offset[0] + patch - 1) // patch) * ((H + offset[1] + patch - 1) // patch)
    assert 0 < got[3][1].item() <= groups  # (G itself is held to the restatement's; at -(31, 31) the first group is one pixel)
    assert bool((got[3][2:] == 0).all())  # no fit reported in patch mode, not even by a grid that has one group on this image
    if groups == 1:  # ... whose loss and gradients are the image's
        (D, A, M, mask), _, _, _ = _case(kind, W, H, variant, patch, offset)
        whole = _call(_renderer(lcgs), D, A, M, mask, variant)
        assert all(torch.equal(u, v) for u, v in zip(got[:3], whole[:3])) and torch.equal(got[3][:2], whole[3][:2])
        assert bool((whole[3][2:] != 0).all())


CALLS = [("pearson", 0, (0, 0)), ("pearson", 64, (17, 40)), ("l1_fit", 0, (0, 0)), ("l1_fit", 32, (3, 5)), ("l1_given", 0, (0, 0))]


@pytest.mark.parametrize("variant,patch,offset", CALLS)
def test_evaluation_only_gives_the_same_loss_and_writes_no_gradient(lcgs, variant, patch, offset):
    r = _renderer(lcgs)
    D, A, M, mask = (None if t is None else t.to(DEV) for t in R.inputs("holes", 320, 240, ALPHA_MIN))
    loss, gd, ga, stats = _call(r, D, A, M, mask, variant, patch=patch, offset=offset)
    assert torch.isfinite(gd).all() and torch.isfinite(ga).all() and loss.item() > 0
    for g in (gd, ga):
        g.fill_(-123.0)  # the buffers of the call before: an evaluation-only call must not remember them
    loss_e, _, _, stats_e = _call(r, D, A, M, mask, variant, patch=patch, offset=offset, with_grad=False)
    assert torch.equal(loss_e, loss) and torch.equal(stats_e, stats)
    assert all(torch.equal(g, torch.full_like(g, -123.0)) for g in (gd, ga))
    # ... and on a fresh context
    loss_f = _call(lcgs.Renderer(lcgs.Context(0)), D, A, M, mask, variant, patch=patch, offset=offset, with_grad=False)[0]
    assert torch.equal(loss_f, loss)


@pytest.mark.parametrize("variant,patch", [("pearson", 64), ("l1_fit", 0)])
def test_two_calls_give_the_same_bits(lcgs, variant, patch):
    r = _renderer(lcgs)
    D, A, M, mask = R.inputs("noisy", 1920, 1080, ALPHA_MIN)
    a, b = (_call(r, D, A, M, mask, variant, patch=patch, offset=(5, 9) if patch else (0, 0)) for _ in range(2))
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    assert bool((a[1] != 0).all())


def test_a_small_call_after_a_large_one_is_not_reached_by_the_stale_workspace(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    big = R.inputs("noisy", 1920, 1080, ALPHA_MIN)
    for variant, patch in (("pearson", 32), ("l1_fit", 0)):
        _call(r, *big, variant, patch=patch)
        for small_patch in (0, 32):
            got, _ = _check_against_the_restatement(r, "holes", 37, 53, variant, small_patch, (0, 0))
            fresh = _call(lcgs.Renderer(lcgs.Context(0)), *_case("holes", 37, 53, variant, small_patch, (0, 0))[0], variant,
                          patch=small_patch)
            for u, v in zip(got, fresh):
                assert torch.equal(u, v)


def test_weight_zero_gives_exact_zeros(lcgs):
    r = _renderer(lcgs)
    for kind in ("noisy", "holes", "flat_render"):
        for variant, patch in (("pearson", 0), ("pearson", 32), ("l1_fit", 0), ("l1_fit", 32), ("l1_given", 0)):
            for out in _call(r, *R.inputs(kind, 37, 53, ALPHA_MIN), variant, weight=0.0, patch=patch)[:3]:
                assert bool((out == 0).all()), (kind, variant, patch)


def _grads_agree(got, want, tag):
    """tests/test_gpu_normal_consistency.py::_grads_agree: relative norm 2e-4 and the same zero pattern (the render backward sums
    with float atomics: bit equality is not on offer)"""
    for k in KEYS:
        num, den = (got[k] - want[k]).double().norm().item(), want[k].double().norm().item()
        print(f"[depth prior end to end] {tag} {k}: |got - want| / |want| = {num / max(den, 1e-300):.2e}")
        assert num <= 2e-4 * den + 1e-12, (tag, k, num, den)
        assert torch.equal(got[k] == 0, want[k] == 0), (tag, k)


@pytest.mark.parametrize("variant", ("pearson", "l1_fit"))
def test_autograd_end_to_end_equals_the_reference_gradients_through_backward_maps(lcgs, variant):
    """render_autograd_maps -> depth_prior_autograd -> backward(): the parameter gradients against those of the float64
    restatement's two gradients fed to Renderer.backward_maps on the same frame"""
    import maps_ref

    scene, pose, W, H = maps_ref.crowd()
    cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
    r = lcgs.Renderer(lcgs.Context(0))
    t = {k: v.requires_grad_(True) for k, v in upload_scene(scene).items()}
    _, depth, alpha = lcgs.render_autograd_maps(r, cam, *[t[k] for k in KEYS], depth_mode="inv_z")
    # a prior that is neither the rendered depth nor unrelated to it; the crowd's empty pixels are masked out
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    v = (depth / alpha.clamp_min(A32)).detach().cpu()
    prior = (1.7 * v + 0.2 + 0.05 * torch.sin(0.9 * x + 0.4 * y)).to(DEV)
    mask = (alpha.detach() > 0.05).to(torch.uint8)
    kw = dict(weight=WEIGHT, alpha_min=ALPHA_MIN, **VARIANTS[variant])
    loss = lcgs.depth_prior_autograd(r, depth, alpha, prior, mask, **kw)
    assert loss.dim() == 0 and loss.requires_grad
    (2.0 * loss).backward()  # (the incoming scalar scales the stored gradients)
    torch.cuda.synchronize()
    got = {k: t[k].grad.clone() for k in KEYS}
    ref = R.autograd(depth, alpha, prior, mask, **dict(kw, weight=W32, alpha_min=A32))
    assert abs(loss.item() - ref[0].item()) <= 1e-5 * abs(ref[0].item()) + 1e-9
    gd, ga = ((2.0 * g).float().to(DEV).contiguous() for g in ref[1:3])
    assert bool((gd != 0).any()) and bool((ga != 0).any())
    r2 = lcgs.Renderer(lcgs.Context(0))
    d = upload_scene(scene)
    r2.bind_scene(*[d[k] for k in KEYS])
    r2.forward(cam, torch.zeros(3, H, W, device=DEV), keep_state=True, sync=True)
    want = {k: torch.full_like(d[k], 7.0) for k in KEYS}
    r2.backward_maps(None, gd, ga, *[want[k] for k in KEYS], mode="inv_z")
    r2.ctx.synchronize()
    assert bool((want["pos"] != 0).any())
    _grads_agree(got, want, f"crowd {variant}")


TRAIN_LR = {"pos": 2e-3, "sh_dc": 0.0, "sh_rest": 0.0, "opacity": 0.0, "scale": 0.0, "rot": 0.0}


def train(lcgs, variant, steps=30):
    """`steps` Adam steps on the depth-prior loss alone (weight 1), driven from Python through backward_maps: the prior is
    2.5 v + 0.3 of the scene's own inverse depth, the splats start displaced along the view axis"""
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
    D, A = torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV)
    r.forward(cam, img, keep_state=True, sync=True)
    r.render_maps(D, A, mode="inv_z")
    r.ctx.synchronize()
    prior = 2.5 * (D / A.clamp_min(ALPHA_MIN)) + 0.3
    mask = (A > 0.5).to(torch.uint8)
    # the displacement: up to 0.15 along the view axis, per splat
    eye, target = (np.asarray(p, dtype=np.float64) for p in POSE[:2])
    axis = torch.from_numpy(((target - eye) / np.linalg.norm(target - eye)).astype(np.float32)).to(DEV)
    shift = torch.from_numpy(np.random.default_rng(3).uniform(-0.15, 0.15, (P, 1)).astype(np.float32)).to(DEV)
    raw["pos"] += shift * axis  # (the activated positions are the raw ones: one tensor)
    r.bind_scene(*[act[k] for k in KEYS])
    gd, ga = torch.zeros_like(D), torch.zeros_like(A)
    loss_all = torch.zeros(steps, device=DEV)
    for step in range(1, steps + 1):
        r.forward(cam, img, keep_state=True, sync=False)
        r.render_maps(D, A, mode="inv_z")
        r.depth_prior_loss_backward(D, A, prior, gd, ga, loss_all[step - 1:step], mask=mask, weight=1.0, alpha_min=ALPHA_MIN,
                                    **VARIANTS[variant])
        r.backward_maps(None, gd, ga, *[g[k] for k in KEYS], mode="inv_z")
        r.adam_step(g, raw, m, v, act, step, TRAIN_LR)
    r.ctx.synchronize()
    return loss_all.cpu().tolist()


@pytest.mark.parametrize("variant", ("pearson", "l1_fit"))
def test_thirty_adam_steps_on_the_depth_prior_gradient_train(lcgs, variant):
    losses = train(lcgs, variant)
    print(f"[depth prior training] {variant}: loss {losses[0]:.6f} -> {losses[-1]:.6f} (ratio {losses[-1] / losses[0]:.3f}); "
          f"min of the first five {min(losses[:5]):.6f}, of the last five {min(losses[-5:]):.6f}")
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0] and min(losses[-5:]) < min(losses[:5]), losses
