"""Times the depth-prior losses on a 1920x1080 frame of the bicycle stand-in (its inverse-depth and alpha maps; the prior is
2.5 v + 0.3 of the frame's own v plus noise, the mask the covered pixels), same run.  Four variants, each with its gradients
and evaluation only:
    global Pearson, patch-64 Pearson, L1 with the fitted alignment, L1 with a given alignment
Every leg alternates with the same term composed in torch (binary32 on the device; forward + autograd backward, or the forward
under no_grad) and with lcgs_l2_loss_backward on the frame, the yardstick of a streaming pass: every round times the three once
(--reps calls after warm-up), a row is the median of the rounds' medians with the rounds' spread, and the fused call must beat
the composed one in EVERY round.  Whole calls are timed with events on the context's stream.
The floor quoted beside each leg is traffic: 13 B per pixel per statistics pass (depth, alpha, prior, mask), 21 B for the
gradient pass (the same + two gradients), 5 B for the given alignment's count of the valid pixels (prior, mask).
    python tools/depth_prior_bench.py [--out profiles/depth_prior_bench.txt] [--splats N] [--rounds 3]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--splats", type=int, default=2_000_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H, WARM = 1920, 1080, 5
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
WEIGHT, ALPHA_MIN, EPS, PATCH = 1.0, 1e-3, 1e-12, 64
GIVEN_S, GIVEN_T = 0.4, -0.12

scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
cam = L.get_lookat_cam([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0], width=W, height=H)  # bench.py's view 0
img = torch.zeros(3, H, W, device=dev)
depth, alpha = (torch.zeros(H, W, device=dev) for _ in range(2))
n = r.forward(cam, img, keep_state=True, sync=True)
r.render_maps(depth, alpha, mode="inv_z")
r.ctx.synchronize()
gen = torch.Generator(device=dev).manual_seed(1)
prior = 2.5 * (depth / alpha.clamp_min(ALPHA_MIN)) + 0.3 + 0.05 * (torch.rand(H, W, device=dev, generator=gen) - 0.5)
mask = (alpha > 0).to(torch.uint8)
maskf = mask.float()
g_d, g_a = torch.empty_like(depth), torch.empty_like(alpha)
loss, stats = torch.zeros(1, device=dev), torch.zeros(4, device=dev)
target = torch.rand(3, H, W, device=dev, generator=gen)
dL_img = torch.empty_like(img)
PH, PW = -(-H // PATCH) * PATCH, -(-W // PATCH) * PATCH


def patch_sums(x):
    """x [H, W] -> [GY, 1, GX, 1], the sums over the 64 x 64 blocks of the grid anchored at the first pixel"""
    return F.pad(x, (0, PW - W, 0, PH - H)).reshape(PH // PATCH, PATCH, PW // PATCH, PATCH).sum(dim=(1, 3), keepdim=True)


def spread(g):
    """[GY, 1, GX, 1] -> [H, W]"""
    return g.expand(-1, PATCH, -1, PATCH).reshape(PH, PW)[:H, :W]


def statistics_of(v, patch):
    """centred statistics per group, as the header defines them, in binary32: group-level tensors (0-dim for the image,
    [GY, 1, GX, 1] for patches) -- only the means go back to the pixels, for the centring -- and the way back"""
    gsum, to_pixels = (patch_sums, spread) if patch else ((lambda x: x.sum()), (lambda g: g))
    nn = gsum(maskf)
    counted = (nn >= 2).float()
    nn = nn.clamp_min(1.0)
    mu_v, mu_m = gsum(v * maskf) / nn, gsum(prior * maskf) / nn
    cv, cm = (v - to_pixels(mu_v)) * maskf, (prior - to_pixels(mu_m)) * maskf
    return counted, mu_v, mu_m, gsum(cv * cv) / nn, gsum(cm * cm) / nn, gsum(cv * cm) / nn, to_pixels


def composed(kind, align, patch, grad):
    def run():
        with torch.set_grad_enabled(grad):
            D, A = (t.detach().clone().requires_grad_(grad) for t in (depth, alpha))
            v = D / A.clamp_min(ALPHA_MIN)
            if kind == "pearson":  # reduced over the groups: [GY, GX] numbers, or one
                counted, _, _, var_v, var_m, cov, _ = statistics_of(v, patch)
                rr = cov / torch.sqrt((var_v + EPS) * (var_m + EPS))
                out = WEIGHT / counted.sum().clamp_min(1.0) * ((1.0 - rr) * counted).sum()
            else:
                if align == "given":
                    s, t, sel = GIVEN_S, GIVEN_T, maskf
                else:
                    with torch.no_grad():
                        counted, mu_v, mu_m, _, var_m, cov, to_pixels = statistics_of(v, patch)
                        s = cov / (var_m + EPS)
                        s, t, sel = to_pixels(s), to_pixels(mu_v - s * mu_m), maskf * to_pixels(counted)
                out = WEIGHT * ((v - (s * prior + t)).abs() * sel).sum() / sel.sum().clamp_min(1.0)
            if grad:
                out.backward()
            return out, D.grad, A.grad
    return run


def fused(kind, align, patch, grad):
    kw = dict(mask=mask, kind=kind, align=align, scale=GIVEN_S, shift=GIVEN_T, weight=WEIGHT, alpha_min=ALPHA_MIN, patch=patch, stats=stats)
    return lambda: r.depth_prior_loss_backward(depth, alpha, prior, g_d if grad else None, g_a if grad else None, loss, **kw)


def timed(fn):
    ms = []
    for i in range(args.reps + WARM):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARM:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


PX = W * H
# (name, kind, align, patch, bytes per pixel of the gradient call, of the evaluation-only call)
VARIANTS = [("global Pearson", "pearson", "fit", 0, 13 + 13 + 21, 13 + 13), ("patch-64 Pearson", "pearson", "fit", PATCH, 13 + 13 + 21, 13 + 13),
            ("L1, fitted alignment", "l1", "fit", 0, 13 + 13 + 21, 13 + 13 + 13), ("L1, given alignment", "l1", "given", 0, 5 + 21, 5 + 13)]
l2 = lambda: r.l2_loss_backward(img, target, dL_img, loss)
L2_BYTES = 9 * PX * 4  # img + target read, dL_dimg written

lines = [f"bicycle stand-in, {args.splats} splats, {W}x{H}: num_rendered {n}, {maskf.mean().item() * 100:.1f} % of the pixels covered "
         f"(the mask); {args.rounds} alternating rounds of {args.reps} calls after {WARM} warm-up calls; {torch.cuda.get_device_name(0)}, "
         f"clocks as the machine sets them (nothing pinned), nothing else on the stream"]
all_beat = True
for name, kind, align, patch, b_grad, b_eval in VARIANTS:
    for grad, per_px in ((True, b_grad), (False, b_eval)):
        legs = [("fused", fused(kind, align, patch, grad)), ("torch", composed(kind, align, patch, grad)), ("l2", l2)]
        res = {k: [] for k, _ in legs}
        for _ in range(args.rounds):
            for k, fn in legs:
                res[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in res.items()}
        beat = all(f < t for f, t in zip(res["fused"], res["torch"]))
        all_beat = all_beat and beat
        l2_rate = L2_BYTES / (med["l2"] * 1e-3)  # bytes per second
        floor_us = per_px * PX / l2_rate * 1e6
        lines.append(f"{name}, {'loss + two gradients' if grad else 'evaluation only'}")
        for k, label in (("fused", "lcgs_depth_prior_loss_backward"), ("torch", "torch float32 on the device, composed"), ("l2", "lcgs_l2_loss_backward on the frame")):
            lines.append(f"    {label:44s} median {med[k] * 1e3:9.1f} us   rounds {min(res[k]) * 1e3:9.1f} .. {max(res[k]) * 1e3:9.1f} us")
        lines.append(f"    traffic floor {per_px} B/pixel = {per_px * PX / 1e6:.1f} MB: {per_px * PX / (med['fused'] * 1e-3) / 1e12:.2f} TB/s achieved "
                     f"(L2 loss: {l2_rate / 1e12:.2f} TB/s); the floor at the L2 loss's rate is {floor_us:.1f} us, the call takes "
                     f"{med['fused'] * 1e3 / floor_us:.2f} x that; torch composed / fused = {med['torch'] / med['fused']:.1f} x; "
                     f"fused faster in every round: {'yes' if beat else 'NO'}")
        # the two agree (binary32 against binary64: loosely)
        fused(kind, align, patch, True)()
        ref = composed(kind, align, patch, True)()
        torch.cuda.synchronize()
        if grad:
            lines.append(f"    loss {loss.item():.7f} (torch float32 {ref[0].item():.7f}); largest gradient difference from torch float32: " +
                         ", ".join(f"{nm} {(a - b).abs().max().item():.2e} of {b.abs().max().item():.2e}"
                                   for nm, a, b in zip(("depth", "alpha"), (g_d, g_a), ref[1:])))
lines.append(f"every fused leg faster than its torch-composed counterpart in every round: {'yes' if all_beat else 'NO'}")

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
