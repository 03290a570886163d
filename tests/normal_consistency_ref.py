"""The yardstick of lcgs_normal_consistency_loss_backward: the normal-consistency term of 2DGS-style training restated in torch
(no GPU needed), as include/lcgs_hip.h defines it.

    z = D / max(A, alpha_min),  P = (rx z, ry z, z) through the pixel centres,
    ex = P(x+1, y) - P(x-1, y),  ey = P(x, y+1) - P(x, y-1),  m = ey x ex,  nt = m / sqrt(m.m + 1e-20)
    loss = weight x mean over the INTERIOR pixels of (A - N . nt)

D, A: [H, W], N: [3, H, W]; cam: anything with fov (degrees), aspect_ratio, width and height.  Two evaluations:

  autograd(D, A, N, cam, weight, alpha_min, dtype)   the definition with torch's autograd, in float64 (the yardstick) or float32
                                                     (what binary32 delivers on that input)
  closed_form(D, A, N, cam, weight, alpha_min)       float64: the gradients written out as the header writes them, a gather of
                                                     g_ex, g_ey over every pixel's four neighbours
                                                     (tests/test_normal_consistency_ref.py pins it to autograd at 1e-12)

Both return (loss, dL_dD, dL_dA, dL_dN).  weight and alpha_min cross the C ABI as binary32 numbers: callers evaluate these at
float(np.float32(.)), see abi32()."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from photometric_ref import bound  # noqa: F401  (3 E32 + 4 u S per output array)

EPS = 1e-20


def abi32(v):
    """the binary32 number the library receives for a Python float"""
    return float(np.float32(v))


def camera(W, H, fov=50.0):
    """the four numbers of a camera the loss reads, as the binary32 members of lcgs_camera hold them"""
    from types import SimpleNamespace

    return SimpleNamespace(fov=abi32(fov), aspect_ratio=abi32(W / H), width=W, height=H)


CLASSES = ("smooth", "noisy", "holes", "degenerate")


def inputs(kind, W, H, alpha_min=1e-3):
    """(D [H, W], A [H, W], N [3, H, W]) float32 tensors of one input class:
    smooth      z = 3 + a gentle plane + a sinusoid, alpha in [0.2, 0.99], unit normals times alpha, D = z alpha
    noisy       the smooth z plus uniform noise of 0.5
    holes       smooth, 30 % of the pixels with alpha below alpha_min, one pixel exactly 0 and one exactly alpha_min
    degenerate  depth identically 0: m = 0 everywhere"""
    g = torch.Generator().manual_seed(7919 * W + H)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    z = 3.0 + 0.4 * x / W - 0.3 * y / H + 0.2 * torch.sin(5.0 * x / W + 3.0 * y / H)
    A = 0.2 + 0.79 * torch.rand(H, W, generator=g, dtype=torch.float64)
    n = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    n = n / n.norm(dim=0, keepdim=True)
    noise, hole, low = (torch.rand(H, W, generator=g, dtype=torch.float64) for _ in range(3))
    if kind == "noisy":
        z = z + 0.5 * noise
    if kind == "holes":
        A = torch.where(hole < 0.3, low * abi32(alpha_min) * 0.999, A)
        A.view(-1)[(W * H) // 2] = 0.0
        A.view(-1)[(W * H) // 3] = abi32(alpha_min)
    D = torch.zeros_like(z) if kind == "degenerate" else z * A
    if kind not in CLASSES:
        raise ValueError(kind)
    return D.float(), A.float(), (n * A).float()


def _tans(cam):
    tany = math.tan(float(cam.fov) / 180.0 * math.pi * 0.5)
    return tany * float(cam.aspect_ratio), tany


def _rays(cam, dtype):
    W, H = int(cam.width), int(cam.height)
    tanx, tany = _tans(cam)
    xs = ((torch.arange(W, dtype=dtype) + 0.5) / W * 2 - 1) * tanx
    ys = ((torch.arange(H, dtype=dtype) + 0.5) / H * 2 - 1) * tany
    return xs, ys


def _cross(a, b):
    return torch.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _as(x, dtype):
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return x.detach().to("cpu", dtype).clone()


def surface_normal(D, A, cam, alpha_min, dtype=torch.float64):
    """(ex, ey, m, s, nt) over the interior pixels, [3, H-2, W-2] each (s: [H-2, W-2]); D, A tensors of `dtype`"""
    xs, ys = _rays(cam, dtype)
    z = D / A.clamp_min(alpha_min)
    pts = torch.stack([xs[None, :] * z, ys[:, None] * z, z])
    ex = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2]
    ey = pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    m = _cross(ey, ex)
    s = torch.sqrt((m * m).sum(dim=0) + EPS)
    return ex, ey, m, s, m / s


def autograd(D, A, N, cam, weight, alpha_min, dtype=torch.float64):
    D, A, N = (_as(x, dtype).requires_grad_(True) for x in (D, A, N))
    nt = surface_normal(D, A, cam, alpha_min, dtype)[4]
    H, W = A.shape
    c = weight / ((W - 2) * (H - 2))
    loss = c * (A[1:-1, 1:-1] - (N[:, 1:-1, 1:-1] * nt).sum(dim=0)).sum()
    loss.backward()
    return loss.detach(), D.grad.detach(), A.grad.detach(), N.grad.detach()


def closed_form(D, A, N, cam, weight, alpha_min):
    D, A, N = (_as(x, torch.float64) for x in (D, A, N))
    H, W = A.shape
    c = weight / ((W - 2) * (H - 2))
    ex, ey, m, s, nt = surface_normal(D, A, cam, alpha_min)
    n = N[:, 1:-1, 1:-1]
    loss = c * (A[1:-1, 1:-1] - (n * nt).sum(dim=0)).sum()
    g_n = torch.zeros_like(N)
    g_n[:, 1:-1, 1:-1] = -c * nt
    g_m = -c * (n / s - m * (m * n).sum(dim=0) / s ** 3)
    # g_ex, g_ey on the whole frame (0 off the interior) inside a margin of one pixel, so that every pixel has four neighbours
    g_ex, g_ey = (F.pad(g, (2, 2, 2, 2)) for g in (_cross(g_m, ey), _cross(ex, g_m)))
    G = (g_ex[:, 1:-1, :-2] - g_ex[:, 1:-1, 2:]) + g_ey[:, :-2, 1:-1] - g_ey[:, 2:, 1:-1]
    xs, ys = _rays(cam, torch.float64)
    g_z = G[0] * xs[None, :] + G[1] * ys[:, None] + G[2]
    g_d = g_z / A.clamp_min(alpha_min)
    g_a = torch.where(A >= alpha_min, -g_z * D / (A * A), torch.zeros_like(A))
    g_a[1:-1, 1:-1] += c
    return loss, g_d, g_a, g_n
