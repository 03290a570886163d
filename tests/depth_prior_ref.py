"""The yardstick of lcgs_depth_prior_loss_backward: the Pearson and aligned-L1 depth-prior losses restated in torch (no GPU
needed), as include/lcgs_hip.h defines them.

    v = D / max(A, alpha_min),  m = the prior;  valid: (no mask or mask != 0) and isfinite(m)
    group: the image (patch 0) or the patch x patch blocks of the grid anchored at (-patch_x, -patch_y); counted: >= 2 valid
    pixels (align "given": the image, >= 1)
    per counted group, means first, then centred sums:  r = cov / sqrt((var_v + eps)(var_m + eps)),  s = cov / (var_m + eps),
    t = mu_v - s mu_m,  eps = 1e-12
    pearson: loss = weight / G sum_g (1 - r_g)          l1: loss = weight / N_c sum |v - (s m + t)|, (s, t) detached

D, A, M: [H, W]; mask: [H, W] uint8 or None.  Two evaluations, both with centred sums:

  autograd(D, A, M, mask, ..., dtype)   the definition with torch's autograd, in float64 (the yardstick) or float32 (what
                                        binary32 delivers on that input)
  closed_form(D, A, M, mask, ...)       float64: the gradients written out as the header writes them
                                        (tests/test_depth_prior_ref.py pins it to autograd at 1e-9)

Both return (loss, dL_dD, dL_dA, stats, res): stats = [N_c, G, s, t] (s, t: the image's fit for patch 0, the given pair, zeros
in patch mode), res = the L1 residual per pixel (0 where the pixel is not a valid pixel of a counted group; zeros for pearson).
weight, alpha_min, scale and shift cross the C ABI as binary32 numbers: callers evaluate these at abi32(.)."""
import numpy as np
import torch
import torch.nn.functional as F

import normal_consistency_ref as NR
from photometric_ref import U32, bound  # noqa: F401  (3 E32 + 4 u S per output array)

EPS = 1e-12
abi32 = NR.abi32

CLASSES = ("smooth", "noisy", "offset", "holes", "constant_prior", "flat_render", "one_valid", "none_valid", "affine")
AFFINE_S, AFFINE_T = 0.5, 0.75  # the pair planted in class "affine": v = 0.5 m + 0.75, exactly


def inputs(kind, W, H, alpha_min=1e-3):
    """(D [H, W], A [H, W], M [H, W] float32, mask [H, W] uint8 or None) of one input class:
    smooth          z, A of normal_consistency_ref.inputs("smooth"), D = z A; prior = 0.37 z + 1.9 + 0.1 (uniform - 0.5)
    noisy           the same on the z of its class "noisy" (uniform noise of 0.5 on z)
    offset          the smooth z + 50
    holes           smooth; 30 % of the pixels masked out, another 5 % with a NaN or +-Inf prior, 30 % with alpha below alpha_min,
                    one alpha exactly 0 and one exactly alpha_min
    constant_prior  smooth, the prior 2.5 everywhere
    flat_render     D = 2 A: v = 2 exactly at every pixel
    one_valid       smooth, the mask 0 except at one pixel
    none_valid      smooth, the mask 0 everywhere
    affine          m a multiple of 1/64, alpha a power of two, v = 0.5 m + 0.75 exactly in binary32"""
    if kind not in CLASSES:
        raise ValueError(kind)
    g = torch.Generator().manual_seed(104729 * W + H)
    D, A, _ = NR.inputs("noisy" if kind == "noisy" else "smooth", W, H, alpha_min)
    D, A = D.double(), A.double()
    z = D / A  # (alpha >= 0.2 here)
    u, hole, bad, low, lowv = (torch.rand(H, W, generator=g, dtype=torch.float64) for _ in range(5))
    if kind == "offset":
        z = z + 50.0
    M = 0.37 * z + 1.9 + 0.1 * (u - 0.5)
    mask = None
    if kind == "holes":
        mask = (hole >= 0.3).to(torch.uint8)
        M = torch.where(bad < 0.05 / 3, torch.full_like(M, float("nan")), M)
        M = torch.where((bad >= 0.05 / 3) & (bad < 0.10 / 3), torch.full_like(M, float("inf")), M)
        M = torch.where((bad >= 0.10 / 3) & (bad < 0.05), torch.full_like(M, -float("inf")), M)
        A = torch.where(low < 0.3, lowv * abi32(alpha_min) * 0.999, A)
        A.view(-1)[(W * H) // 2] = 0.0
        A.view(-1)[(W * H) // 3] = abi32(alpha_min)
    if kind == "constant_prior":
        M = torch.full_like(M, 2.5)
    if kind == "one_valid":
        mask = torch.zeros(H, W, dtype=torch.uint8)
        mask.view(-1)[(2 * W * H) // 3] = 1
    if kind == "none_valid":
        mask = torch.zeros(H, W, dtype=torch.uint8)
    if kind == "affine":
        M = torch.floor(u * 512.0) / 64.0
        A = torch.tensor([0.25, 0.5, 1.0], dtype=torch.float64)[torch.floor(hole * 3.0).long().clamp(0, 2)]
        z = AFFINE_S * M + AFFINE_T
    D = 2.0 * A if kind == "flat_render" else z * A
    return D.float(), A.float(), M.float(), mask


def _as(x, dtype):
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return x.detach().to("cpu", dtype).clone()


def groups(W, H, patch=0, patch_offset=(0, 0)):
    """(gid [H, W] long, the number of groups)"""
    if not patch:
        return torch.zeros(H, W, dtype=torch.long), 1
    px, py = patch_offset
    gx, gy = (torch.arange(W) + px) // patch, (torch.arange(H) + py) // patch
    GX, GY = int(gx.max()) + 1, int(gy.max()) + 1
    return (gy[:, None] * GX + gx[None, :]).long(), GX * GY


def _group_sums(W, H, patch, patch_offset):
    """x [H, W] -> its sum per group [NG], with torch's own (pairwise) reduction: in float32 that is what binary32 delivers
    with some care, where one running sum over 1920 x 1080 terms would not be"""
    if not patch:
        return lambda x: x.sum().reshape(1)
    px, py = patch_offset
    GX, GY = (W + px + patch - 1) // patch, (H + py + patch - 1) // patch

    def gsum(x):
        x = F.pad(x, (px, GX * patch - W - px, py, GY * patch - H - py))
        return x.reshape(GY, patch, GX, patch).sum(dim=(1, 3)).reshape(-1)

    return gsum


def _statistics(v, M, mask, align, patch, patch_offset):
    """the per-group statistics of the definition; v may carry a graph"""
    H, W = v.shape
    dtype = v.dtype
    valid = torch.isfinite(M) & (torch.ones(H, W, dtype=torch.bool) if mask is None else _as(mask, torch.uint8) != 0)
    M0, vf = torch.where(valid, M, torch.zeros_like(M)), valid.to(dtype)
    gid, _ = groups(W, H, patch, patch_offset)
    gsum = _group_sums(W, H, patch, patch_offset)
    n = gsum(vf)
    counted = n >= (1 if align == "given" else 2)
    nn = n.clamp_min(1)
    mu_v, mu_m = gsum(v * vf) / nn, gsum(M0 * vf) / nn
    cv, cm = (v - mu_v[gid]) * vf, (M0 - mu_m[gid]) * vf
    var_v, var_m, cov = (gsum(x) / nn for x in (cv * cv, cm * cm, cv * cm))
    in_counted = vf * counted[gid].to(dtype)
    return dict(M0=M0, gid=gid, n=n, nn=nn, counted=counted, mu_v=mu_v, mu_m=mu_m, cv=cv, cm=cm, var_v=var_v, var_m=var_m,
                cov=cov, in_counted=in_counted, G=int(counted.sum()), N_c=int(n[counted].sum()))


def _fit(st, align, scale, shift, patch, dtype):
    """(s [NG], t [NG], the stats' pair)"""
    if align == "given":
        s, t = torch.full_like(st["mu_v"], scale), torch.full_like(st["mu_v"], shift)
        return s, t, (scale, shift)
    s = (st["cov"] / (st["var_m"] + EPS)).detach()
    t = (st["mu_v"] - s * st["mu_m"]).detach()
    pair = (s[0].item(), t[0].item()) if not patch and bool(st["counted"][0]) else (0.0, 0.0)
    return s, t, pair


def _stats(st, pair):
    return torch.tensor([float(st["N_c"]), float(st["G"]), pair[0], pair[1]], dtype=torch.float64)


def autograd(D, A, M, mask=None, kind="pearson", align="fit", scale=1.0, shift=0.0, weight=1.0, alpha_min=1e-3, patch=0,
             patch_offset=(0, 0), dtype=torch.float64):
    D, A = (_as(x, dtype).requires_grad_(True) for x in (D, A))
    M = _as(M, dtype)
    v = D / A.clamp_min(alpha_min)
    st = _statistics(v, M, mask, align, patch, patch_offset)
    s, t, pair = _fit(st, align, scale, shift, patch, dtype)
    res = torch.zeros_like(v)
    if kind == "pearson":
        r = st["cov"] / torch.sqrt((st["var_v"] + EPS) * (st["var_m"] + EPS))
        loss = (weight / max(st["G"], 1)) * ((1.0 - r) * st["counted"].to(dtype)).sum()
    else:
        res = (v - (s[st["gid"]] * st["M0"] + t[st["gid"]])) * st["in_counted"]
        loss = (weight / max(st["N_c"], 1)) * res.abs().sum()
    loss.backward()
    return loss.detach(), D.grad.detach(), A.grad.detach(), _stats(st, pair), res.detach()


def closed_form(D, A, M, mask=None, kind="pearson", align="fit", scale=1.0, shift=0.0, weight=1.0, alpha_min=1e-3, patch=0,
                patch_offset=(0, 0)):
    D, A, M = (_as(x, torch.float64) for x in (D, A, M))
    amax = A.clamp_min(alpha_min)
    v = D / amax
    st = _statistics(v, M, mask, align, patch, patch_offset)
    s, t, pair = _fit(st, align, scale, shift, patch, torch.float64)
    gid, G, N_c = st["gid"], st["G"], st["N_c"]
    res = torch.zeros_like(v)
    if kind == "pearson":
        root = torch.sqrt((st["var_v"] + EPS) * (st["var_m"] + EPS))
        loss = (weight / max(G, 1)) * ((1.0 - st["cov"] / root) * st["counted"].double()).sum()
        B = st["cov"] / (st["var_v"] + EPS)
        g_v = -(weight / max(G, 1)) / (st["nn"] * root)[gid] * (st["cm"] - B[gid] * st["cv"]) * st["in_counted"]
    else:
        res = (v - (s[gid] * st["M0"] + t[gid])) * st["in_counted"]
        loss = (weight / max(N_c, 1)) * res.abs().sum()
        g_v = (weight / max(N_c, 1)) * torch.sign(res)
    g_d = g_v / amax
    g_a = torch.where(A >= alpha_min, -g_v * D / (A * A), torch.zeros_like(A))
    return loss, g_d, g_a, _stats(st, pair), res


def counted_pixels(A, M, mask=None, align="fit", patch=0, patch_offset=(0, 0)):
    """[H, W] bool: the valid pixels of counted groups, the ones the loss is summed over"""
    st = _statistics(torch.zeros_like(_as(A, torch.float64)), _as(M, torch.float64), mask, align, patch, patch_offset)
    return st["in_counted"] != 0


def tau(res64, res32):
    """the residual below which binary32 does not decide the sign of an L1 residual: the bound, applied to the residual array"""
    return bound(res64, res32)


def fit_is_exact(kind, align, n_c, patch=0):
    """the L1 inputs on which EVERY residual of the fitted alignment is rounding, so that no sign is decided and only the loss
    and the gradients' magnitudes can be held: class "affine" (the fit finds the planted pair) and an image of two valid
    pixels (the fitted line passes through both).  The rule the loss was specified with names class "affine" alone; the
    two-pixel image is this suite's addition to it, for the same reason: with two counted pixels of rounding-only residuals a
    cap of 1 % of the counted pixels cannot be met by any implementation, the float64 restatement included.  Such a case keeps
    the loss bound, the exact zeros and both magnitude bounds."""
    return align == "fit" and (kind == "affine" or (not patch and n_c == 2))


def sign_undecided(res64, res32, counted, exact):
    """[H, W] bool: the counted pixels an L1 comparison leaves out of the element-wise check -- all of them where the fit is
    exact, else those with |res| <= tau; none where tau == 0 (every residual is then 0 in binary32 and binary64 alike: every
    sign is decided)"""
    if exact:
        return counted
    t = tau(res64, res32)
    return (counted & (res64.abs() <= t)) if t > 0 else torch.zeros_like(counted)
