"""`-m gpu`: lcgs_photometric_loss_backward (csrc/kernels/loss.hip) against the float64 restatement of the 3DGS loss in
tests/photometric_ref.py, its determinism, the evaluation-only call, lcgs_fit_views with the loss selected, and a short
training run driven by its gradient.

Every output array (loss, terms, dL_dimg) is held element by element to

    |got - f64| <= 3 E32 + 4 u S

E32: the largest |float32 autograd restatement - float64| over that array on that input, S: the largest |float64 value| in it,
u = 2^-24 (photometric_ref.bound).  lambda crosses the C ABI as a binary32 number, so the restatements are evaluated at
float(float32(lambda)): the loss the library was asked for.  The worst diff / bound per input class is printed and recorded in
docs/TESTS.md."""
import numpy as np
import pytest
import torch

import photometric_ref as R
from conftest import make_scene
from gpu_util import DEV, upload_scene

pytestmark = pytest.mark.gpu

SIZES = [(1920, 1080), (800, 800), (320, 240), (37, 53), (16, 16), (11, 11), (7, 5), (1, 1)]  # (W, H)
LAMBDAS = (0.0, 0.2, 1.0)
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
POSE = ([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])


def _lam32(lam):
    return float(np.float32(lam))


def _render_pair(lcgs, W, H, seed):
    """A frame of a make_scene scene (the target) and the frame of a perturbed copy of it (what training sees).  Frames
    of 16 pixels and less are the centre of a 64 x 64 frame (at such sizes most splats fall below the renderer's radius floor
    and the frame comes out empty)."""
    rw, rh = (W, H) if min(W, H) > 16 else (64, 64)
    rng = np.random.default_rng(seed)
    scene = make_scene(rng, 20000 if rw * rh > 100000 else 3000, log_scale=(-3.2, 0.6) if rw * rh > 4096 else (-2.4, 0.6))
    moved = {k: v.copy() for k, v in scene.items()}
    moved["opacity"] = (moved["opacity"] * 0.7).astype(np.float32)
    moved["sh"][:, :3] += rng.normal(0, 0.15, (moved["sh"].shape[0], 3)).astype(np.float32)
    cam = lcgs.get_lookat_cam(*POSE, width=rw, height=rh)
    frames = []
    for s in (moved, scene):
        r = lcgs.Renderer(lcgs.Context(0))
        d = upload_scene(s)
        r.bind_scene(*[d[k] for k in KEYS])
        img = torch.zeros(3, rh, rw, device=DEV)
        r.forward(cam, img)
        r.ctx.synchronize()
        assert (img > 0).any(), "the scene must reach the frame"
        y0, x0 = (rh - H) // 2, (rw - W) // 2
        frames.append(img[:, y0:y0 + H, x0:x0 + W].contiguous())
    return frames[0], frames[1]


def _inputs(lcgs, kind, W, H):
    g = torch.Generator().manual_seed(1000 * W + H)
    a, b = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    if kind == "uniform":
        return a.to(DEV), b.to(DEV)
    if kind == "rendered":
        return _render_pair(lcgs, W, H, 5 + W)
    if kind == "constant":  # flat regions: sigma^2 = G*x^2 - mu^2 is a difference of equal numbers
        return torch.full((3, H, W), 0.5).to(DEV), b.to(DEV)
    if kind == "half_equal":  # sign(0) = 0 on half the pixels
        mask = torch.rand(3, H, W, generator=g) < 0.5
        return torch.where(mask, b, a).to(DEV), b.to(DEV)
    raise ValueError(kind)


def _held(got, ref64, ref32, tag):
    """worst |got - f64| / bound over one output array"""
    got, ref64 = got.detach().cpu().double().reshape(-1), ref64.double().reshape(-1)
    assert torch.isfinite(got).all(), tag
    b = R.bound(ref64, ref32.reshape(-1))
    return ((got - ref64).abs().max().item() / b) if b > 0 else (0.0 if torch.equal(got, ref64) else float("inf"))


def _call(r, x, y, lam, with_grad=True):
    dL = torch.full_like(x, float("nan")) if with_grad else None
    loss, terms = torch.full((1,), float("nan"), device=DEV), torch.full((2,), float("nan"), device=DEV)
    r.photometric_loss_backward(x, y, dL, loss, lam, terms)
    r.ctx.synchronize()
    torch.cuda.synchronize()
    return loss, terms, dL


def _check_against_the_restatement(r, x, y, tag, lambdas=LAMBDAS):
    parts = R.closed_form(x, y)
    worst = {}
    for lam in lambdas:
        lam32 = _lam32(lam)
        loss64, terms64, grad64 = R.combine(parts, lam32)
        loss32, terms32, grad32 = R.autograd(x, y, lam32, torch.float32)
        loss, terms, dL = _call(r, x, y, lam)
        ratios = {"loss": _held(loss, loss64, loss32, tag), "terms": _held(terms, terms64, terms32, tag),
                  "dL": _held(dL, grad64, grad32, tag)}
        print(f"[photometric vs f64] {tag} lambda {lam}: diff/bound loss {ratios['loss']:.3f} terms {ratios['terms']:.3f} "
              f"dL {ratios['dL']:.3f} (loss {loss.item():.6f}, L1 {terms[0].item():.6f}, SSIM {terms[1].item():.6f})")
        for k, v in ratios.items():
            assert v <= 1.0, f"{tag} lambda {lam}: {k} at {v:.3f} x its bound"
            worst[k] = max(worst.get(k, 0.0), v)
        if lam == 0.0:  # the L1 term alone: exactly sign(x - y) / n, no rounded 0 x (anything) added
            assert torch.equal(dL, torch.sign(x - y) / x.numel()), tag
    return worst


@pytest.mark.parametrize("kind", ["uniform", "rendered", "constant", "half_equal"])
@pytest.mark.parametrize("W,H", SIZES)
def test_loss_terms_and_gradient_against_the_float64_restatement(lcgs, W, H, kind):
    r = lcgs.Renderer(lcgs.Context(0))
    x, y = _inputs(lcgs, kind, W, H)
    worst = _check_against_the_restatement(r, x, y, f"{kind} {W}x{H}")
    print(f"[photometric worst] {kind} {W}x{H}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_evaluation_only_gives_the_same_loss_and_writes_no_gradient(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    x, y = _inputs(lcgs, "uniform", 320, 240)
    loss, terms, dL = _call(r, x, y, 0.2)
    assert torch.isfinite(dL).all()
    dL.fill_(-123.0)  # the buffer of the call before: an evaluation-only call must not remember it
    loss_e, terms_e, _ = _call(r, x, y, 0.2, with_grad=False)
    assert torch.equal(loss_e, loss) and torch.equal(terms_e, terms)
    assert torch.equal(dL, torch.full_like(dL, -123.0))
    # ... and on a fresh context, whose workspace never held the planes of a gradient call
    loss_f, terms_f, _ = _call(lcgs.Renderer(lcgs.Context(0)), x, y, 0.2, with_grad=False)
    assert torch.equal(loss_f, loss) and torch.equal(terms_f, terms)


def test_two_calls_give_the_same_bits(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    x, y = _inputs(lcgs, "uniform", 1920, 1080)
    a, b = _call(r, x, y, 0.2), _call(r, x, y, 0.2)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_a_small_call_after_a_large_one_is_not_reached_by_the_stale_workspace(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    _call(r, *_inputs(lcgs, "uniform", 1920, 1080), 0.2)
    x, y = _inputs(lcgs, "uniform", 37, 53)
    _check_against_the_restatement(r, x, y, "uniform 37x53 after 1920x1080", lambdas=(0.2, 1.0))
    fresh = _call(lcgs.Renderer(lcgs.Context(0)), x, y, 0.2)
    for u, v in zip(_call(r, x, y, 0.2), fresh):
        assert torch.equal(u, v)


def test_lambda_zero_is_the_l1_term_alone(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    _call(r, *_inputs(lcgs, "uniform", 320, 240), 1.0)  # leaves planes in the workspace that lambda = 0 must not read
    x, y = _inputs(lcgs, "half_equal", 320, 240)
    loss, terms, dL = _call(r, x, y, 0.0)
    assert torch.equal(dL, torch.sign(x - y) / x.numel())
    l1 = (x.double() - y.double()).abs().mean().cpu()
    l1_32 = (x.cpu() - y.cpu()).abs().mean()
    assert abs(loss.item() - l1.item()) <= R.bound(l1, l1_32)
    assert torch.equal(loss.cpu(), terms[:1].cpu())


def _fit_setup(lcgs, n_views):
    from bench import view_pose

    rng = np.random.default_rng(77)  # the scene and poses of tests/test_gpu_train.py's fit-views test
    P, W, H = 40000, 320, 240
    d = upload_scene(make_scene(rng, P, spread=1.5, log_scale=(-3.6, 0.6)))
    cams = [lcgs.get_lookat_cam(*view_pose(k), width=W, height=H) for k in range(n_views)]
    g = torch.Generator().manual_seed(3)
    targets = [torch.rand(3, H, W, generator=g).to(DEV) for _ in range(n_views)]
    shapes = {"pos": (P, 3), "scale": (P, 3), "rotq": (P, 4), "sh": (P, 48), "opacity": (P,)}
    return d, cams, targets, shapes, (W, H)


def _grads_agree(got, want, tag):
    """The agreement tests/test_gpu_train.py asks of two evaluations of the same gradient sums.  Not torch.equal: the
    render-backward adds its pixel-to-splat sums with float atomics, so two backward passes of ONE frame on ONE context
    already differ in the last bits (tests/test_gpu_train.py, the fused-Adam test's docstring); nothing the loss or the
    two-context overlap does enters into it."""
    bit_equal = True
    for k in KEYS:
        num, den = (got[k] - want[k]).double().norm().item(), want[k].double().norm().item()
        assert num <= 2e-4 * den + 1e-12, (tag, k, num, den)
        assert torch.equal(got[k] == 0, want[k] == 0), (tag, k)
        bit_equal = bit_equal and torch.equal(got[k], want[k])
    print(f"[fit_views] {tag}: gradients bit-equal: {bit_equal}")


def test_fit_views_with_the_photometric_loss_equals_the_hand_written_loop(lcgs):
    """losses: bit for bit (the forward and this loss are deterministic, whichever of the two contexts runs the view);
    gradients: see _grads_agree."""
    n_views = 3
    d, cams, targets, shapes, (W, H) = _fit_setup(lcgs, n_views)
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[d[k] for k in KEYS])
    want = {k: torch.full(shapes[k], 7.0, device=DEV) for k in KEYS}
    want_loss = torch.zeros(n_views, device=DEV)
    img, dL = torch.zeros(3, H, W, device=DEV), torch.zeros(3, H, W, device=DEV)
    for j, cam in enumerate(cams):
        r.forward(cam, img, keep_state=True, sync=False)
        r.photometric_loss_backward(img, targets[j], dL, want_loss[j:j + 1], 0.2)
        r.backward(dL, *[want[k] for k in KEYS], accumulate=j > 0)
    r.ctx.synchronize()
    r2 = lcgs.Renderer(lcgs.Context(0))
    r2.bind_scene(*[d[k] for k in KEYS])
    r2.set_fit_loss(lcgs.LOSS_PHOTOMETRIC, 0.2)
    for rep in range(2):  # (the second step starts from stale arrays and a warm sibling)
        got = {k: torch.full(shapes[k], -3.0, device=DEV) for k in KEYS}
        got_loss = torch.full((n_views,), -1.0, device=DEV)
        torch.cuda.synchronize()
        r2.fit_views(cams, targets, *[got[k] for k in KEYS], got_loss)
        r2.ctx.synchronize()
        assert torch.equal(got_loss, want_loss), (rep, got_loss, want_loss)
        _grads_agree(got, want, f"photometric, step {rep}")
    assert (want_loss > 0.3).all()  # random targets: far from the frames (an MSE would be ~0.2 here)


def test_fit_views_default_loss_is_unchanged(lcgs):
    """Without lcgs_set_fit_loss -- and with LCGS_LOSS_L2 set explicitly, or set back after the photometric loss was
    selected -- fit_views is the L2 step it was.  The L2 loss is ONE atomic float sum and the gradients are atomic sums too
    (_grads_agree), so two evaluations agree to rounding, not bit for bit: the bars are those of tests/test_gpu_train.py."""
    n_views = 3
    d, cams, targets, shapes, _ = _fit_setup(lcgs, n_views)
    out = []
    for mode in ("never", "explicit", "restored"):
        r = lcgs.Renderer(lcgs.Context(0))
        r.bind_scene(*[d[k] for k in KEYS])
        if mode == "explicit":
            r.set_fit_loss(lcgs.LOSS_L2, 0.7)
        if mode == "restored":
            r.set_fit_loss(lcgs.LOSS_PHOTOMETRIC, 0.2)
            r.set_fit_loss(lcgs.LOSS_L2)
        g = {k: torch.full(shapes[k], -3.0, device=DEV) for k in KEYS}
        losses = torch.full((n_views,), -1.0, device=DEV)
        r.fit_views(cams, targets, *[g[k] for k in KEYS], losses)
        r.ctx.synchronize()
        out.append((g, losses))
    img = torch.zeros_like(targets[0])
    r.forward(cams[0], img)
    assert torch.allclose(out[0][1][:1], ((img - targets[0]) ** 2).mean().reshape(1), rtol=1e-5)  # it IS the MSE
    for g, losses in out[1:]:
        assert torch.allclose(losses, out[0][1], rtol=1e-5, atol=0.0)
        _grads_agree(g, out[0][0], "default loss")


def test_thirty_adam_steps_on_the_photometric_gradient_train(lcgs):
    """The perturbed start of test_lcgs_app_fit_trains_through_the_c_abi_only (lcgs_app.cpp --fit: every opacity logit one
    lower, the base colours shifted; Adam on opacity and base colour only), driven from Python with the photometric gradient."""
    P, W, H = 20000, 320, 240
    scene = lcgs.synth_scene(0, 1001, P)
    cam = lcgs.get_lookat_cam(*POSE, width=W, height=H)
    r = lcgs.Renderer(lcgs.Context(0))
    d = upload_scene(scene)
    r.bind_scene(*[d[k] for k in KEYS])
    target = torch.zeros(3, H, W, device=DEV)
    r.forward(cam, target)
    op = np.clip(scene["opacity"], 1e-6, 1 - 1e-6)
    sh = scene["sh"].copy()
    idx = np.arange(P)[:, None] * 3 + np.arange(3)[None, :]
    sh[:, :3] += (0.3 * ((idx % 7).astype(np.float32) / 3.0 - 1.0)).astype(np.float32)
    raw = {"pos": scene["pos"], "scale": np.log(scene["scale"]), "rotq": scene["rotq"], "sh": sh,
           "opacity": np.log(op / (1 - op)) - 1.0}
    raw = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV) for k, v in raw.items()}
    act = {"pos": raw["pos"], "scale": torch.exp(raw["scale"]), "rotq": raw["rotq"].clone(), "sh": raw["sh"],
           "opacity": torch.sigmoid(raw["opacity"])}
    m = {k: torch.zeros_like(raw[k]) for k in KEYS}
    v = {k: torch.zeros_like(raw[k]) for k in KEYS}
    g = {k: torch.zeros_like(raw[k]) for k in KEYS}
    lr = {"pos": 0.0, "sh_dc": 2.5e-2, "sh_rest": 0.0, "opacity": 5e-2, "scale": 0.0, "rot": 0.0}
    r.bind_scene(*[act[k] for k in KEYS])
    img, dL = torch.zeros(3, H, W, device=DEV), torch.zeros(3, H, W, device=DEV)
    loss_all = torch.zeros(30, device=DEV)
    for step in range(1, 31):
        r.forward(cam, img, keep_state=True, sync=False)
        r.photometric_loss_backward(img, target, dL, loss_all[step - 1:step], 0.2)
        r.backward(dL, *[g[k] for k in KEYS])
        r.adam_step(g, raw, m, v, act, step, lr)
    r.ctx.synchronize()
    losses = loss_all.cpu().tolist()
    print(f"[photometric training] loss {losses[0]:.6f} -> {losses[-1]:.6f} (ratio {losses[-1] / losses[0]:.3f}); "
          f"min of the first five {min(losses[:5]):.6f}, of the last five {min(losses[-5:]):.6f}")
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0] and min(losses[-5:]) < min(losses[:5]), losses
