"""Times the normal-consistency loss on a 1920x1080 frame of the bicycle stand-in (the frame of tools/normals_bench.py: its depth,
alpha and normal maps), same run:
    lcgs_normal_consistency_loss_backward        the fused call: loss + the three gradients, and evaluation only
    the same term composed in torch              binary32 on the device, forward + autograd backward (what a caller did before)
    lcgs_l2_loss_backward on the same frame      the yardstick of a streaming pass: 9 planes moved for the fused call's 10
Whole calls are timed with events on the context's stream.  The candidates alternate: every round times each of them once
(--reps calls after warm-up); a row is the median of the rounds' medians with the rounds' spread.
    python tools/normal_consistency_bench.py [--out profiles/normal_consistency_bench.txt] [--splats N] [--rounds 3]"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H, WARM = 1920, 1080, 5
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
WEIGHT, ALPHA_MIN = 0.05, 1e-3

scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
cam = L.get_lookat_cam([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0], width=W, height=H)  # bench.py's view 0
img = torch.zeros(3, H, W, device=dev)
depth, alpha = (torch.zeros(H, W, device=dev) for _ in range(2))
normal = torch.zeros(3, H, W, device=dev)
n = r.forward(cam, img, keep_state=True, sync=True)
r.render_maps(depth, alpha, mode="z")
r.render_normals(normal)
r.ctx.synchronize()
g_d, g_a, g_n = torch.empty_like(depth), torch.empty_like(alpha), torch.empty_like(normal)
loss = torch.zeros(1, device=dev)
target = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
dL_img = torch.empty_like(img)

tany = math.tan(float(cam.fov) / 180.0 * math.pi * 0.5)
tanx = tany * float(cam.aspect_ratio)
xs = (((torch.arange(W, device=dev, dtype=torch.float32) + 0.5) / W * 2 - 1) * tanx)[None, :]
ys = (((torch.arange(H, device=dev, dtype=torch.float32) + 0.5) / H * 2 - 1) * tany)[:, None]


def torch_composed():
    D, A, N = (t.detach().clone().requires_grad_(True) for t in (depth, alpha, normal))
    z = D / A.clamp_min(ALPHA_MIN)
    pts = torch.stack([xs * z, ys * z, z])
    ex = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2]
    ey = pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    m = torch.cross(ey, ex, dim=0)
    nt = m / torch.sqrt((m * m).sum(dim=0, keepdim=True) + 1e-20)
    out = WEIGHT * (A[1:-1, 1:-1] - (N[:, 1:-1, 1:-1] * nt).sum(dim=0)).mean()
    out.backward()
    return out, D.grad, A.grad, N.grad


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


FUSED, EVAL, L2, TORCH = ("lcgs_normal_consistency_loss_backward, loss + three gradients", "lcgs_normal_consistency_loss_backward, evaluation only",
                          "lcgs_l2_loss_backward on the frame", "torch float32 on the device: the composed term + autograd backward")
candidates = [
    (FUSED, lambda: r.normal_consistency_loss_backward(cam, depth, alpha, normal, g_d, g_a, g_n, loss, WEIGHT, ALPHA_MIN)),
    (EVAL, lambda: r.normal_consistency_loss_backward(cam, depth, alpha, normal, None, None, None, loss, WEIGHT, ALPHA_MIN)),
    (L2, lambda: r.l2_loss_backward(img, target, dL_img, loss)),
    (TORCH, torch_composed),
]
res = {name: [] for name, _ in candidates}
for _ in range(args.rounds):
    for name, fn in candidates:
        res[name].append(timed(fn))

lines = [f"bicycle stand-in, {args.splats} splats, {W}x{H}: num_rendered {n}, {(alpha > 0).float().mean().item() * 100:.1f} % of the pixels "
         f"covered; {args.rounds} alternating rounds of {args.reps} calls after {WARM} warm-up calls; {torch.cuda.get_device_name(0)}, "
         f"clocks as the machine sets them (nothing pinned), nothing else on the stream"]
med = {}
for name, ms in res.items():
    med[name] = statistics.median(ms)
    lines.append(f"{name:76s} median {med[name] * 1e3:9.1f} us   rounds {min(ms) * 1e3:9.1f} .. {max(ms) * 1e3:9.1f} us")
plane = W * H * 4
fused_bytes, l2_bytes = 10 * plane, 9 * plane  # 5 planes read + 5 written; img + target read, dL_dimg written
bw = lambda b, ms: b / (ms * 1e-3) / 1e9
lines.append(f"  fused call: {fused_bytes / 1e6:.1f} MB of 10-plane traffic in {med[FUSED] * 1e3:.1f} us = {bw(fused_bytes, med[FUSED]):.0f} GB/s;  "
             f"L2 loss: {l2_bytes / 1e6:.1f} MB of 9-plane traffic in {med[L2] * 1e3:.1f} us = {bw(l2_bytes, med[L2]):.0f} GB/s;  "
             f"time per byte, fused / L2 = {(med[FUSED] / fused_bytes) / (med[L2] / l2_bytes):.2f}")
lines.append(f"  torch composed / fused = {med[TORCH] / med[FUSED]:.1f} x")

r.normal_consistency_loss_backward(cam, depth, alpha, normal, g_d, g_a, g_n, loss, WEIGHT, ALPHA_MIN)
ref = torch_composed()
torch.cuda.synchronize()
lines.append(f"  loss {loss.item():.7f} (torch float32 {ref[0].item():.7f}); largest gradient difference from torch float32: " +
             ", ".join(f"{name} {(a - b).abs().max().item():.2e} of {b.abs().max().item():.2e}"
                       for name, a, b in zip(("depth", "alpha", "normal"), (g_d, g_a, g_n), ref[1:])))

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
