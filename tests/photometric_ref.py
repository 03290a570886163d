"""The yardstick of lcgs_photometric_loss_backward: the published 3DGS training loss restated in torch (no GPU needed).

    loss = (1 - lam) mean|x - y| + lam (1 - SSIM(x, y)),   x, y: [3, H, W]

SSIM with the 11-tap Gaussian window (sigma 1.5) applied per channel with zero padding of 5, C1 = 0.01^2, C2 = 0.03^2 (the
contract in include/lcgs_hip.h).  Three evaluations:

  autograd(x, y, lam, dtype)   form (i): five conv2d(padding=5, groups=3) calls with the 11 x 11 window and torch's autograd,
                               in float64 (the yardstick) or float32 (what binary32 delivers on that input)
  closed_form(x, y)            form (ii), float64: the partial derivatives a, b, c of the per-pixel ssim written out and pushed
                               back through the (self-adjoint) zero-padded convolution, evaluated as two 1-D passes -- the same
                               sums in another order, 11 x cheaper in float64 on a CPU, which is what makes 1920 x 1080 affordable
                               in the GPU tests.  tests/test_photometric_ref.py pins (ii) to (i) at 1e-12.
  combine(parts, lam)          loss, (L1, SSIM) and gradient of form (ii) for one lambda
"""
import math

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
U32 = 2.0 ** -24


def window(dtype=torch.float64):
    """w[k] = exp(-(k - 5)^2 / (2 1.5^2)) / sum, k = 0..10, computed in float64"""
    w = torch.tensor([math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)], dtype=torch.float64)
    return (w / w.sum()).to(dtype)


def _conv2d(img, dtype):
    """G * img for img [C, H, W]: the 11 x 11 window, zero padding of 5, one group per channel"""
    c = img.shape[0]
    w = window(torch.float64)
    k = torch.outer(w, w).to(dtype).expand(c, 1, 11, 11).contiguous()
    return F.conv2d(img[None], k, padding=5, groups=c)[0]


def _conv_separable(img):
    """the same in float64 as a row pass and a column pass (zero padding on both)"""
    c = img.shape[0]
    w = window(torch.float64)
    t = F.conv2d(img[None], w.view(1, 1, 1, 11).expand(c, 1, 1, 11).contiguous(), padding=(0, 5), groups=c)
    return F.conv2d(t, w.view(1, 1, 11, 1).expand(c, 1, 11, 1).contiguous(), padding=(5, 0), groups=c)[0]


def ssim_map(x, y, conv):
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def autograd(x, y, lam, dtype=torch.float64):
    """form (i) -> (loss, terms [L1, SSIM], dL/dx), all in `dtype`"""
    x = x.detach().to("cpu", dtype).clone().requires_grad_(True)
    y = y.detach().to("cpu", dtype)
    l1 = (x - y).abs().mean()
    ssim = ssim_map(x, y, lambda t: _conv2d(t, dtype)).mean()
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    loss.backward()
    return loss.detach(), torch.stack([l1.detach(), ssim.detach()]), x.grad.detach()


def closed_form(x, y):
    """form (ii), float64 -> {"l1", "ssim" (scalars), "g_l1", "g_ssim" (d L1 / dx, d SSIM / dx)}"""
    x, y = x.detach().to("cpu", torch.float64), y.detach().to("cpu", torch.float64)
    n = x.numel()
    G = _conv_separable
    mu1, mu2 = G(x), G(y)
    s1, s2, s12 = G(x * x) - mu1 * mu1, G(y * y) - mu2 * mu2, G(x * y) - mu1 * mu2
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    ssim = A1 * A2 / (B1 * B2)
    b = -ssim / B2                                   # d ssim / d sigma1^2
    c = 2 * A1 / (B1 * B2)                           # d ssim / d sigma12
    a = 2 * mu2 * A2 / (B1 * B2) - 2 * mu1 * ssim / B1 - 2 * mu1 * b - mu2 * c  # d ssim / d mu1, sigmas expanded
    g_ssim = (G(a) + 2 * x * G(b) + y * G(c)) / n
    return {"l1": (x - y).abs().mean(), "ssim": ssim.mean(), "g_l1": torch.sign(x - y) / n, "g_ssim": g_ssim}


def combine(parts, lam):
    """-> (loss, terms [L1, SSIM], dL/dx) of form (ii) for one lambda"""
    loss = (1.0 - lam) * parts["l1"] + lam * (1.0 - parts["ssim"])
    return loss, torch.stack([parts["l1"], parts["ssim"]]), (1.0 - lam) * parts["g_l1"] - lam * parts["g_ssim"]


def bound(ref64, ref32):
    """3 x E32 + 4 u S for one output array: E32 = the largest |float32 restatement - float64| over the array, S = the
    largest |float64 value| in it, u = 2^-24.  The factor 3 is the project's standing margin over what binary32 itself loses
    (README "Gradients"); the 4 u S floor covers the rounding of the output where the restatement happens to be exact."""
    ref64 = ref64.double()
    e32 = (ref32.double() - ref64).abs().max().item()
    return 3.0 * e32 + 4.0 * U32 * ref64.abs().max().item()
