"""The yardstick of lcgs_bilagrid_slice / _backward / _tv_loss_backward: per-view bilateral-grid colour correction restated in
torch (no GPU needed), as include/lcgs_hip.h defines it.

A view's grid is [12, L, GH, GW]: channel 4 r + k is entry (row r, column k) of a 3 x 4 affine colour transform.  The grid is
sliced at (pixel x, pixel y, luminance of the input pixel) -- exactly torch's grid_sample(mode="bilinear", padding_mode="border",
align_corners=True) with coords = 2 (x / (GW-1), y / (GH-1), gray) - 1 -- and the transform is applied to the input colour.

  autograd(grid, img, g_out, dtype)   the grid_sample form with torch's autograd -> (out, dL/dimg, dL/dgrid), in float64 (the
                                      yardstick) or float32 (what binary32 delivers on that input)
  hat_form(grid, img, g_out)          float64, independent: the trilinear weights written as products of hat functions, the
                                      gradients written out as the header writes them, with its `inside` mask
                                      (tests/test_bilagrid_ref.py pins the two at 1e-12)
  tv(grids, weight, dtype)            the total-variation term and its gradient by autograd

The luminance weights are binary32 constants in the kernel: float(float32(.)) in both precisions.  weight crosses the C ABI as
a binary32 number: callers evaluate tv at abi32(weight)."""
import numpy as np
import torch
import torch.nn.functional as F

from photometric_ref import bound  # noqa: F401  (3 E32 + 4 u S per output array)

LUMA = tuple(float(np.float32(w)) for w in (0.299, 0.587, 0.114))
GRID_CLASSES = ("identity", "random")
IMAGE_CLASSES = ("uniform", "overrange", "black_patches", "knots")
KNOT_MARGIN = 1e-3  # the constructed classes keep every pixel's float64 zr this far from every integer (or exactly at 0)


def abi32(v):
    """the binary32 number the library receives for a Python float"""
    return float(np.float32(v))


def _as(x, dtype):
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return x.detach().to("cpu", dtype).clone()


def identity_grid(dims, dtype=torch.float32):
    """[12, L, GH, GW], dims = (GW, GH, L): every cell the identity transform"""
    GW, GH, L = dims
    g = torch.zeros(12, L, GH, GW, dtype=dtype)
    g[(0, 5, 10), ...] = 1.0
    return g


def grid(kind, dims, seed=0):
    """a float32 grid of one class: `identity`, or `random` = identity + 0.3 N(0, 1)"""
    if kind not in GRID_CLASSES:
        raise ValueError(kind)
    g = identity_grid(dims, torch.float64)
    if kind == "random":
        gen = torch.Generator().manual_seed(104729 * seed + 31 * dims[0] + 7 * dims[1] + dims[2])
        g = g + 0.3 * torch.randn(g.shape, generator=gen, dtype=torch.float64)
    return g.float()


def zr64(img, L):
    """the float64 guidance coordinate gray (L - 1) of a float32 image [3, H, W]"""
    x = _as(img, torch.float64)
    return (LUMA[0] * x[0] + LUMA[1] * x[1] + LUMA[2] * x[2]) * (L - 1)


def well_placed(img, L):
    """per pixel: the float64 zr is exactly 0, or <= -margin, or >= L - 1 + margin, or inside (0, L - 1) and at least the margin
    away from every integer -- so that binary32 and binary64 agree on the cell and on the clamp"""
    z = zr64(img, L)
    interior = (z > 0) & (z < L - 1) & ((z - torch.round(z)).abs() >= KNOT_MARGIN)
    return (z == 0) | (z <= -KNOT_MARGIN) | (z >= L - 1 + KNOT_MARGIN) | interior


def image(kind, W, H, L, seed=0):
    """a float32 image [3, H, W] of one class:
    uniform        colours in [0, 1]
    overrange      colours in [-0.2, 1.4]: the guidance clamps on both sides
    black_patches  uniform, exact zeros over a third of the frame
    knots          every pixel's binary32 gray within 2 ulp of some l / (L - 1)
    Every class but `knots` is well_placed (offenders are nudged by three margins; asserted): no exact white, no pixel whose
    cell or clamp binary32 and binary64 could decide differently."""
    if kind not in IMAGE_CLASSES:
        raise ValueError(kind)
    gen = torch.Generator().manual_seed(7919 * W + 13 * H + 101 * L + seed)
    x = torch.rand(3, H, W, generator=gen, dtype=torch.float64)
    if kind == "knots":
        return _knots(W, H, L, gen)
    if kind == "overrange":
        x = -0.2 + 1.6 * x
    x = x.float()
    black = torch.zeros(H * W, dtype=torch.bool)
    if kind == "black_patches":
        n = H * W
        black[n // 3:n // 3 + (n + 2) // 3] = True
        x[:, black.view(H, W)] = 0.0
    for _ in range(4):
        bad = ~well_placed(x, L)
        if not bad.any():
            break
        x[:, bad] += np.float32(3.0 * KNOT_MARGIN / (L - 1))
    assert bool(well_placed(x, L).all())
    assert bool((x[:, black.view(H, W)] == 0).all()) and not bool((x == 1.0).all(dim=0).any())
    return x


def gray32(x):
    """the kernel's luminance: binary32, the three products summed in order"""
    x = x.float()
    w = [torch.tensor(v, dtype=torch.float32) for v in (0.299, 0.587, 0.114)]
    return (w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]


def _knots(W, H, L, gen):
    """r = g = b = v, v one of the binary32 neighbours of l / (L - 1) whose gray lands within 2 ulp of l / (L - 1)"""
    l = torch.randint(0, L, (H, W), generator=gen)
    pick = torch.randint(0, 3, (H, W), generator=gen)
    target = (l.double() / (L - 1)).float()
    ulp = torch.nextafter(target, torch.full_like(target, 2.0)) - target
    best = target.expand(3, H, W).contiguous()
    err = (gray32(best).double() - target.double()).abs() / ulp.double()
    for k, toward in enumerate((-1.0, 2.0)):
        v = torch.nextafter(target, torch.full_like(target, toward)).expand(3, H, W).contiguous()
        e = (gray32(v).double() - target.double()).abs() / ulp.double()
        use = (e <= 2.0) & ((pick == k + 1) | (err > 2.0))
        best = torch.where(use, v, best)
        err = torch.where(use, e, err)
    assert bool((err <= 2.0).all())
    return best


def coords(img, dims, dtype):
    """grid_sample's normalised coordinates [1, 1, H, W, 3] of an image [3, H, W] of `dtype` (differentiable in img)"""
    _, H, W = img.shape
    xs = 2 * ((torch.arange(W, dtype=dtype) + 0.5) / W) - 1  # 2 (x / (GW - 1)) - 1
    ys = 2 * ((torch.arange(H, dtype=dtype) + 0.5) / H) - 1
    gray = LUMA[0] * img[0] + LUMA[1] * img[1] + LUMA[2] * img[2]
    return torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W), 2 * gray - 1], dim=-1)[None, None]


def slice_apply(grid, img, dtype=torch.float64):
    """out [3, H, W]: tensors of `dtype`, differentiable"""
    _, H, W = img.shape
    GW, GH, L = grid.shape[3], grid.shape[2], grid.shape[1]
    A = F.grid_sample(grid[None], coords(img, (GW, GH, L), dtype), mode="bilinear", padding_mode="border",
                      align_corners=True)[0, :, 0].view(3, 4, H, W)
    return A[:, 0] * img[0] + A[:, 1] * img[1] + A[:, 2] * img[2] + A[:, 3]


def autograd(grid, img, g_out, dtype=torch.float64):
    """-> (out, dL/dimg, dL/dgrid) for dL/dout = g_out"""
    grid, img = (_as(t, dtype).requires_grad_(True) for t in (grid, img))
    out = slice_apply(grid, img, dtype)
    (out * _as(g_out, dtype)).sum().backward()
    return out.detach(), img.grad.detach(), grid.grad.detach()


def _hat(t):
    return (1 - t.abs()).clamp_min(0)


def hat_form(grid, img, g_out):
    """float64 -> (out, dL/dimg, dL/dgrid), the header's formulas: hat-function weights, the guidance's `inside` mask"""
    grid, img, g = (_as(t, torch.float64) for t in (grid, img, g_out))
    _, L, GH, GW = grid.shape
    _, H, W = img.shape
    x = (torch.arange(W, dtype=torch.float64) + 0.5) / W * (GW - 1)
    y = (torch.arange(H, dtype=torch.float64) + 0.5) / H * (GH - 1)
    zr = (LUMA[0] * img[0] + LUMA[1] * img[1] + LUMA[2] * img[2]) * (L - 1)
    z = zr.clamp(0, L - 1)
    wx = _hat(x[:, None] - torch.arange(GW, dtype=torch.float64)[None, :])             # [W, GW]
    wy = _hat(y[:, None] - torch.arange(GH, dtype=torch.float64)[None, :])             # [H, GH]
    wz = _hat(z[..., None] - torch.arange(L, dtype=torch.float64))                      # [H, W, L]
    A = torch.einsum("clji,hwl,hj,wi->chw", grid, wz, wy, wx).view(3, 4, H, W)
    c1 = torch.cat([img, torch.ones(1, H, W, dtype=torch.float64)])                     # (r, g, b, 1)
    out = (A * c1[None]).sum(dim=1)
    # dL/dgrid[4r + k] = sum_pixels hat hat hat g_r (k < 3 ? c_k : 1)
    d_grid = torch.einsum("rhw,khw,hwl,hj,wi->rklji", g, c1, wz, wy, wx).reshape(12, L, GH, GW)
    # dA/dz: the level above the cell's floor minus the level below, z0 = min(floor(z), L - 2)
    z0 = z.floor().clamp(max=L - 2).long()
    dwz = torch.zeros(H, W, L, dtype=torch.float64)
    dwz.scatter_(2, z0[..., None], -1.0)
    dwz.scatter_(2, z0[..., None] + 1, 1.0)
    dA = torch.einsum("clji,hwl,hj,wi->chw", grid, dwz, wy, wx).view(3, 4, H, W)
    inside = ((zr > 0) & (zr < L - 1)).double()
    through = (g * (dA * c1[None]).sum(dim=1)).sum(dim=0) * (L - 1) * inside
    d_img = (A[:, :3] * g[:, None]).sum(dim=0) + torch.tensor(LUMA, dtype=torch.float64)[:, None, None] * through
    return out, d_img, d_grid


def tv(grids, weight, dtype=torch.float64):
    """-> (loss, dL/dgrids) of grids [N, 12, L, GH, GW]: weight / N x the sum over the axes of the mean squared forward
    difference (the mean over ONE grid's differences along that axis, 12 channels included)"""
    g = _as(grids, dtype).requires_grad_(True)
    N = g.shape[0]
    dx, dy, dz = g[..., 1:] - g[..., :-1], g[..., 1:, :] - g[..., :-1, :], g[:, :, 1:] - g[:, :, :-1]
    loss = weight / N * sum((d * d).sum() / d[0].numel() for d in (dx, dy, dz))
    loss.backward()
    return loss.detach(), g.grad.detach()
