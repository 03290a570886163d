"""`-m gpu`: per-view bilateral-grid colour correction (lcgs_bilagrid_slice / _backward / _tv_loss_backward,
csrc/kernels/bilagrid.hip) against the float64 restatement in tests/bilagrid_ref.py, the identity grid, the exact zeros, its
determinism, the autograd wrappers behind render_autograd, and a short training run of one grid.

Every output array (out, dL_dimg, dL_dgrid, the TV loss and gradient) is held element by element to

    |got - f64| <= 3 E32 + 4 u S

E32: the largest |float32 autograd restatement - float64| over that array on that input, S: the largest |float64 value| in it,
u = 2^-24 (photometric_ref.bound).  Where the bound is 0 the array must equal the reference.  Outputs are pre-filled with NaN: an
element the call does not write fails.  In the constructed classes no element is excluded: their generator keeps every pixel's
float64 guidance coordinate zr exactly at 0, or 1e-3 clear of every integer and of the clamp (asserted on the reference side).
Class `knots` (every gray within 2 ulp of a level) holds out and dL_dgrid, both continuous in z, to the bound and asks dL_dimg
to be finite.  Class `rendered` (a real frame) may leave pixels whose float64 zr lies within 1e-4 of an integer in (0, L-1] out
of the dL_dimg check alone, at most 1 % of the frame.  The worst diff / bound per class is printed and recorded in
docs/TESTS.md."""
import functools

import numpy as np
import pytest
import torch

import bilagrid_ref as R
import photometric_ref as P
from conftest import make_scene
from gpu_util import DEV, KEYS, upload_scene

pytestmark = pytest.mark.gpu

TW, TH = 32, 16  # the per-pixel kernel's tile (csrc/kernels/launch.hpp: kBilagridTileW x kBilagridTileH)
SIZES = [(1, 1), (5, 7), (37, 53), (320, 240), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (TW + 2, TH + 2)]  # (W, H)
DIMS = [(16, 16, 8), (2, 2, 2), (3, 5, 2), (4, 3, 16)]  # (GW, GH, L)
POSE = ([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])
NAMES = ("out", "dL_dimg", "dL_dgrid")


@functools.lru_cache(maxsize=None)
def _rendered(W, H):
    """a real frame [3, H, W] on the CPU: a make_scene scene through Renderer.forward.  Frames of 16 pixels and less are the
    centre of a 64 x 64 frame (at such sizes most splats fall below the renderer's radius floor)."""
    import luisacomputegaussiansplatting_amd as lcgs

    rw, rh = (W, H) if min(W, H) > 16 else (64, 64)
    scene = make_scene(np.random.default_rng(11 + W), 3000, log_scale=(-3.2, 0.6) if rw * rh > 4096 else (-2.4, 0.6))
    r = lcgs.Renderer(lcgs.Context(0))
    d = upload_scene(scene)
    r.bind_scene(*[d[k] for k in KEYS])
    img = torch.zeros(3, rh, rw, device=DEV)
    assert r.forward(lcgs.get_lookat_cam(*POSE, width=rw, height=rh), img, sync=True) > 0
    assert bool((img != 0).any()), "the scene must reach the frame"
    y0, x0 = (rh - H) // 2, (rw - W) // 2
    return img[:, y0:y0 + H, x0:x0 + W].contiguous().cpu()


@functools.lru_cache(maxsize=None)
def _image(kind, W, H, L):
    return _rendered(W, H) if kind == "rendered" else R.image(kind, W, H, L)


@functools.lru_cache(maxsize=None)
def _g_out(W, H):
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(17 * W + H), dtype=torch.float64).float()


@functools.lru_cache(maxsize=16)
def _reference(grid_kind, img_kind, dims, W, H):
    """((out, dL_dimg, dL_dgrid) in float64, the same in float32): computed once, shared, never written"""
    grid, img, g = R.grid(grid_kind, dims), _image(img_kind, W, H, dims[2]), _g_out(W, H)
    return R.autograd(grid, img, g, torch.float64), R.autograd(grid, img, g, torch.float32)


def _nan(shape):
    return torch.full(tuple(shape), float("nan"), device=DEV)


def _slice(r, grid, img):
    out = _nan(img.shape)
    r.bilagrid_slice(grid, img, out)
    r.ctx.synchronize()
    return out


def _backward(r, grid, img, g, want_img=True, want_grid=True, fill=float("nan")):
    d_img, d_grid = torch.full_like(img, fill), torch.full_like(grid, fill)
    r.bilagrid_backward(grid, img, g, d_img if want_img else None, d_grid if want_grid else None)
    r.ctx.synchronize()
    return d_img, d_grid


def _held(got, ref64, ref32, tag, keep=None):
    """worst |got - f64| / bound over one output array (keep: a mask of the elements that take part)"""
    got, ref64, ref32 = got.detach().cpu().double(), ref64.double(), ref32.double()
    assert torch.isfinite(got).all(), tag
    if keep is not None:
        got, ref64, ref32 = got[keep], ref64[keep], ref32[keep]
    got, ref64, ref32 = got.reshape(-1), ref64.reshape(-1), ref32.reshape(-1)
    if got.numel() == 0:
        return 0.0
    b = R.bound(ref64, ref32)
    return ((got - ref64).abs().max().item() / b) if b > 0 else (0.0 if torch.equal(got, ref64) else float("inf"))


def _near_a_level(img, L, eps=1e-4):
    """pixels whose float64 zr lies within eps of an integer in (0, L - 1]"""
    z = R.zr64(img, L)
    k = torch.round(z)
    return ((z - k).abs() < eps) & (k >= 1) & (k <= L - 1)


def _check(lcgs, r, grid_kind, img_kind, dims, W, H):
    ref64, ref32 = _reference(grid_kind, img_kind, dims, W, H)
    grid, img, g = (t.to(DEV) for t in (R.grid(grid_kind, dims), _image(img_kind, W, H, dims[2]), _g_out(W, H)))
    out = _slice(r, grid, img)
    d_img, d_grid = _backward(r, grid, img, g)
    tag = f"{grid_kind}/{img_kind} {W}x{H} grid {dims}"
    keep = None
    if img_kind == "rendered":
        near = _near_a_level(img, dims[2])
        assert near.float().mean().item() <= 0.01, (tag, near.float().mean().item())
        keep = (~near)[None].expand(3, H, W)
    else:
        assert img_kind == "knots" or bool(R.well_placed(img, dims[2]).all())
    ratios = {"out": _held(out, ref64[0], ref32[0], tag), "dL_dgrid": _held(d_grid, ref64[2], ref32[2], tag)}
    if img_kind == "knots":
        assert torch.isfinite(d_img).all(), tag
    else:
        ratios["dL_dimg"] = _held(d_img, ref64[1], ref32[1], tag, keep)
    print(f"[bilagrid vs f64] {tag}: diff/bound " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, f"{tag}: {k} at {v:.3f} x its bound"
    if grid_kind == "identity":  # every lerp is a + t * 0: the image comes back bit for bit
        assert torch.equal(out, img), tag
    return ratios


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("W,H", SIZES)
def test_slice_and_gradients_against_the_float64_restatement(lcgs, W, H, dims):
    r = lcgs.Renderer(lcgs.Context(0))
    worst = {}
    for grid_kind in R.GRID_CLASSES:
        for img_kind in R.IMAGE_CLASSES + ("rendered",):
            for k, v in _check(lcgs, r, grid_kind, img_kind, dims, W, H).items():
                worst[(grid_kind, img_kind, k)] = v
    top = max(worst, key=worst.get)
    print(f"[bilagrid vs f64] {W}x{H} grid {dims}: worst {worst[top]:.4f} ({'/'.join(top)})")


def test_unreached_vertices_are_exact_zeros_and_each_gradient_alone_has_the_same_bits(lcgs):
    """5 x 7 pixels under 16 x 16 x 8: more vertices than pixels.  A vertex no pixel reaches is written, as an exact zero."""
    dims, W, H = (16, 16, 8), 5, 7
    r = lcgs.Renderer(lcgs.Context(0))
    grid, img, g = (t.to(DEV) for t in (R.grid("random", dims), R.image("uniform", W, H, dims[2]), _g_out(W, H)))
    d_img, d_grid = _backward(r, grid, img, g)
    ref_grid = _reference("random", "uniform", dims, W, H)[0][2]
    unreached = (ref_grid == 0).to(DEV)
    assert unreached.float().mean().item() > 0.5 and bool((~unreached).any())
    assert bool((d_grid[unreached] == 0).all()) and bool((d_grid[~unreached] != 0).any())
    only_img, untouched_grid = _backward(r, grid, img, g, want_grid=False, fill=-123.0)
    untouched_img, only_grid = _backward(r, grid, img, g, want_img=False, fill=-123.0)
    assert torch.equal(only_img, d_img) and torch.equal(only_grid, d_grid)
    assert bool((untouched_grid == -123.0).all()) and bool((untouched_img == -123.0).all())
    # ... and at a size with many tiles and a grid whose footprints are split into row slices
    dims, W, H = (3, 5, 2), 320, 240
    grid, img, g = (t.to(DEV) for t in (R.grid("random", dims), R.image("overrange", W, H, dims[2]), _g_out(W, H)))
    d_img, d_grid = _backward(r, grid, img, g)
    assert torch.equal(_backward(r, grid, img, g, want_grid=False, fill=-123.0)[0], d_img)
    assert torch.equal(_backward(r, grid, img, g, want_img=False, fill=-123.0)[1], d_grid)


def _all_three(r, grid, img, g):
    return (_slice(r, grid, img), *_backward(r, grid, img, g))


def test_two_calls_and_a_fresh_context_give_the_same_bits_and_no_stale_workspace_leaks(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    W, H = 1920, 1080
    g = _g_out(W, H).to(DEV)
    for dims in ((16, 16, 8), (2, 2, 2)):  # eight row slices a vertex column; 64 through the workspace
        grid, img = R.grid("random", dims).to(DEV), R.image("uniform", W, H, dims[2]).to(DEV)
        a, b = _all_three(r, grid, img, g), _all_three(r, grid, img, g)
        c = _all_three(lcgs.Renderer(lcgs.Context(0)), grid, img, g)
        for u, v, w in zip(a, b, c):
            assert torch.isfinite(u).all() and torch.equal(u, v) and torch.equal(u, w)
        if dims == (2, 2, 2):
            # ... and the bound where a lane's binary32 run of dL/dgrid is longest: 4 vertex columns, every footprint the whole
            # frame, 64 row slices of 17 rows x 1920 pixels over 256 lanes = about 130 pixels a lane
            ref64, ref32 = R.autograd(grid, img, g, torch.float64), R.autograd(grid, img, g, torch.float32)
            ratios = {n: _held(u, x, y, f"1920x1080 {n}") for n, u, x, y in zip(NAMES, a, ref64, ref32)}
            print(f"[bilagrid vs f64] random/uniform {W}x{H} grid {dims}: diff/bound " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
            for k, v in ratios.items():
                assert v <= 1.0, (k, v)
    # a 37 x 53 call after the 1080p ones equals a fresh context's
    W, H = 37, 53
    for dims in ((16, 16, 8), (2, 2, 2)):
        _check(lcgs, r, "random", "uniform", dims, W, H)
        args = [t.to(DEV) for t in (R.grid("random", dims), R.image("uniform", W, H, dims[2]), _g_out(W, H))]
        for u, v in zip(_all_three(r, *args), _all_three(lcgs.Renderer(lcgs.Context(0)), *args)):
            assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------------------ total variation
def _tv(r, grids, weight, with_grad=True, fill=float("nan")):
    grad, loss = torch.full_like(grids, fill), _nan((1,))
    r.bilagrid_tv_loss_backward(grids, grad if with_grad else None, loss, weight)
    r.ctx.synchronize()
    return loss, grad


@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("N", (1, 3))
def test_tv_loss_and_gradient_against_the_float64_restatement(lcgs, N, dims):
    r = lcgs.Renderer(lcgs.Context(0))
    weight = 10.0
    grids = torch.stack([R.grid("random", dims, seed=s) for s in range(N)])
    ref64, ref32 = R.tv(grids, R.abi32(weight), torch.float64), R.tv(grids, R.abi32(weight), torch.float32)
    loss, grad = _tv(r, grids.to(DEV), weight)
    ratios = {"loss": _held(loss, ref64[0], ref32[0], "tv loss"), "dL_dgrids": _held(grad, ref64[1], ref32[1], "tv gradient")}
    print(f"[bilagrid tv vs f64] N {N} grid {dims}: diff/bound " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()) +
          f" (loss {loss.item():.7f})")
    for k, v in ratios.items():
        assert v <= 1.0, (N, dims, k, v)
    # the identity has no variation
    loss, grad = _tv(r, lcgs.bilagrid_identity(N, dims, device=DEV), weight)
    assert loss.item() == 0.0 and bool((grad == 0).all())


def test_tv_weight_zero_evaluation_only_and_determinism(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    grids = torch.stack([R.grid("random", (16, 16, 8), seed=s) for s in range(5)]).to(DEV)
    for out in _tv(r, grids, 0.0):
        assert bool((out == 0).all())
    loss, grad = _tv(r, grids, 10.0)
    assert torch.isfinite(grad).all() and loss.item() > 0
    loss_e, untouched = _tv(r, grids, 10.0, with_grad=False, fill=-123.0)
    assert torch.equal(loss_e, loss) and bool((untouched == -123.0).all())
    for rr in (r, lcgs.Renderer(lcgs.Context(0))):
        again = _tv(rr, grids, 10.0)
        assert torch.equal(again[0], loss) and torch.equal(again[1], grad)


# ----------------------------------------------------------------------------------------------------------------- autograd
def _photometric_autograd(r, img, target, lam=0.2):
    """the photometric loss as a scalar torch can differentiate: one lcgs_photometric_loss_backward call"""

    class _Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, img):
            x = img.detach().contiguous()
            grad, loss = torch.empty_like(x), torch.empty(1, device=x.device)
            r.photometric_loss_backward(x, target, grad, loss, lam)
            ctx.save_for_backward(grad)
            return loss[0]

        @staticmethod
        def backward(ctx, g_loss):
            return ctx.saved_tensors[0] * g_loss

    return _Fn.apply(img)


def _photometric_ref(out, target, lam, dtype):
    l1 = (out - target).abs().mean()
    ssim = P.ssim_map(out, target, lambda t: P._conv2d(t, dtype)).mean()
    return (1.0 - lam) * l1 + lam * (1.0 - ssim)


def _grads_agree(got, want, tag):
    """tests/test_gpu_photometric.py::_grads_agree: relative norm 2e-4 and the same zero pattern (the render backward sums with
    float atomics: bit equality is not on offer)"""
    for k in KEYS:
        num, den = (got[k] - want[k]).double().norm().item(), want[k].double().norm().item()
        print(f"[bilagrid end to end] {tag} {k}: |got - want| / |want| = {num / max(den, 1e-300):.2e}")
        assert num <= 2e-4 * den + 1e-12, (tag, k, num, den)
        assert torch.equal(got[k] == 0, want[k] == 0), (tag, k)


def test_autograd_end_to_end_equals_the_reference_gradients_through_backward(lcgs):
    """render_autograd -> bilagrid_autograd -> photometric loss -> backward(): the scene gradients against those of the float64
    restatement's dL/dimg fed to Renderer.backward on the same frame; the grid's gradient against the bound"""
    import maps_ref

    scene, pose, W, H = maps_ref.crowd()
    dims, lam = (16, 16, 8), 0.2
    cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
    r = lcgs.Renderer(lcgs.Context(0))
    t = {k: v.requires_grad_(True) for k, v in upload_scene(scene).items()}
    grid = R.grid("random", dims).to(DEV).requires_grad_(True)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(9)).to(DEV)
    img = lcgs.render_autograd(r, cam, *[t[k] for k in KEYS])
    out = lcgs.bilagrid_autograd(r, grid, img)
    loss = _photometric_autograd(r, out, target, lam)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    got = {k: t[k].grad.clone() for k in KEYS}
    # the restatement from the same frame on
    ref = {}
    for dtype in (torch.float64, torch.float32):
        x = img.detach().to("cpu", dtype).requires_grad_(True)
        gr = grid.detach().to("cpu", dtype).requires_grad_(True)
        ref_loss = _photometric_ref(R.slice_apply(gr, x, dtype), target.to("cpu", dtype), lam, dtype)
        ref_loss.backward()
        ref[dtype] = (ref_loss.detach(), x.grad.detach(), gr.grad.detach())
    assert abs(loss.item() - ref[torch.float64][0].item()) <= 1e-5 * abs(ref[torch.float64][0].item())
    ratio = _held(grid.grad, ref[torch.float64][2], ref[torch.float32][2], "end to end dL_dgrid")
    print(f"[bilagrid end to end] crowd: dL_dgrid diff/bound {ratio:.4f}")
    assert ratio <= 1.0
    g_img = ref[torch.float64][1].float().to(DEV).contiguous()
    assert bool((g_img != 0).any())
    r2 = lcgs.Renderer(lcgs.Context(0))
    d = upload_scene(scene)
    r2.bind_scene(*[d[k] for k in KEYS])
    r2.forward(cam, torch.zeros(3, H, W, device=DEV), keep_state=True, sync=True)
    want = {k: torch.full_like(d[k], 7.0) for k in KEYS}
    r2.backward(g_img, *[want[k] for k in KEYS])
    r2.ctx.synchronize()
    assert bool((want["sh"] != 0).any()) and bool((want["pos"] != 0).any())
    _grads_agree(got, want, "crowd")
    # only the gradient autograd asks for is computed: the image alone, the grid alone
    x = img.detach().clone().requires_grad_(True)
    lcgs.bilagrid_autograd(r, grid.detach(), x).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    gr = grid.detach().clone().requires_grad_(True)
    lcgs.bilagrid_autograd(r, gr, img.detach()).sum().backward()
    assert gr.grad is not None and torch.isfinite(gr.grad).all()


def test_forty_adam_steps_on_one_grid_learn_a_views_colour_transform(lcgs):
    """one view rendered at 320 x 240; the target is the frame through a gain, an offset and a mild tone curve; torch's Adam
    steps ONE grid from the identity on the photometric loss + TV"""
    W, H, steps = 320, 240, 40
    scene = lcgs.synth_scene(0, 1001, 20000)
    r = lcgs.Renderer(lcgs.Context(0))
    d = upload_scene(scene)
    r.bind_scene(*[d[k] for k in KEYS])
    img = torch.zeros(3, H, W, device=DEV)
    assert r.forward(lcgs.get_lookat_cam(*POSE, width=W, height=H), img, sync=True) > 0
    gain = torch.tensor([1.3, 0.9, 0.8], device=DEV).view(3, 1, 1)
    offset = torch.tensor([0.02, 0.03, 0.05], device=DEV).view(3, 1, 1)
    target = ((gain * img + offset).clamp_min(0.0) ** 0.8).contiguous()
    grids = lcgs.bilagrid_identity(1, device=DEV).requires_grad_(True)
    assert grids.shape == (1, 12, 8, 16, 16)
    l1_identity = (lcgs.bilagrid_autograd(r, grids[0], img) - target).abs().mean().item()
    assert l1_identity == (img - target).abs().mean().item()
    opt = torch.optim.Adam([grids], lr=1e-2)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        out = lcgs.bilagrid_autograd(r, grids[0], img)
        loss = _photometric_autograd(r, out, target) + lcgs.bilagrid_tv_autograd(r, grids, 10.0)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().tolist()
    l1_final = (lcgs.bilagrid_autograd(r, grids[0], img) - target).abs().mean().item()
    print(f"[bilagrid training] loss {losses[0]:.6f} -> {losses[-1]:.6f}; min of the first five {min(losses[:5]):.6f}, of the "
          f"last five {min(losses[-5:]):.6f}; L1 to the target {l1_identity:.6f} -> {l1_final:.6f}")
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0] and min(losses[-5:]) < min(losses[:5]), losses
    assert l1_final < l1_identity
