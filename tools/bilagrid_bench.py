"""Times the per-view bilateral grid (lcgs_bilagrid_slice / _backward / _tv_loss_backward, kernels/bilagrid.hip) on a 1920x1080
frame of the bicycle stand-in under a 16 x 16 x 8 grid, same run:
    slice                                         beside torch's grid_sample + affine apply (binary32 on the device, no autograd)
    backward: both gradients, dL/dgrid only,      beside the same step composed in torch: grid_sample forward + autograd backward
              dL/dimg only                        (torch has to run the forward to differentiate it: the library's slice + backward
                                                  is the like-for-like figure, the backward alone is listed too)
    TV over 200 grids                             beside the same term + autograd in torch
    lcgs_photometric_loss_backward on the frame   the loss the slice sits in front of
each with its traffic floor: slice 24 B a pixel, backward 36 B a pixel, TV 8 B a grid element.
Whole calls are timed with events on the context's stream.  The candidates alternate: every round times each of them once
(--reps calls after warm-up); a row is the median of the rounds' medians with the rounds' spread.
    python tools/bilagrid_bench.py [--out profiles/bilagrid_bench.txt] [--splats N] [--rounds 3]"""
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
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H, WARM = 1920, 1080, 5
DIMS, NUM_GRIDS, TV_WEIGHT = (16, 16, 8), 200, 10.0
KEYS = ("pos", "scale", "rotq", "sh", "opacity")

scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
cam = L.get_lookat_cam([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0], width=W, height=H)  # bench.py's view 0
img = torch.zeros(3, H, W, device=dev)
n = r.forward(cam, img, sync=True)
gen = torch.Generator(device=dev).manual_seed(1)
grids = L.bilagrid_identity(NUM_GRIDS, DIMS, device=dev)
grids += 0.05 * torch.randn(grids.shape, device=dev, generator=gen)
grid = grids[0]
target = torch.rand(3, H, W, device=dev, generator=gen)
g_out = torch.randn(3, H, W, device=dev, generator=gen)
out, d_img, d_grid, d_grids = torch.empty_like(img), torch.empty_like(img), torch.empty_like(grid), torch.empty_like(grids)
loss = torch.zeros(1, device=dev)

xs = (2 * ((torch.arange(W, device=dev, dtype=torch.float32) + 0.5) / W) - 1)[None, :].expand(H, W)
ys = (2 * ((torch.arange(H, device=dev, dtype=torch.float32) + 0.5) / H) - 1)[:, None].expand(H, W)


def torch_slice(grid, img):
    gray = 0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2]
    coords = torch.stack([xs, ys, 2 * gray - 1], dim=-1)[None, None]
    A = F.grid_sample(grid[None], coords, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].view(3, 4, H, W)
    return A[:, 0] * img[0] + A[:, 1] * img[1] + A[:, 2] * img[2] + A[:, 3]


def torch_forward():
    with torch.no_grad():
        return torch_slice(grid, img)


# the leaves torch differentiates with respect to are made once, outside the timed calls (a call only drops their old .grad)
leaf_img, leaf_grid, leaf_grids = (t.detach().clone().requires_grad_(True) for t in (img, grid, grids))


def torch_backward(want_img, want_grid):
    x, g = (leaf_img if want_img else img), (leaf_grid if want_grid else grid)
    leaf_img.grad = leaf_grid.grad = None
    torch_slice(g, x).backward(g_out)
    return leaf_img.grad, leaf_grid.grad


def torch_tv():
    g = leaf_grids
    g.grad = None
    dx, dy, dz = g[..., 1:] - g[..., :-1], g[..., 1:, :] - g[..., :-1, :], g[:, :, 1:] - g[:, :, :-1]
    t = TV_WEIGHT / NUM_GRIDS * sum((v * v).sum() / v[0].numel() for v in (dx, dy, dz))
    t.backward()
    return t, g.grad


def lib_step(want_img, want_grid):
    r.bilagrid_slice(grid, img, out)
    r.bilagrid_backward(grid, img, g_out, d_img if want_img else None, d_grid if want_grid else None)


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


SLICE, T_SLICE = "lcgs_bilagrid_slice", "torch: grid_sample + affine apply, no autograd"
B_BOTH, B_GRID, B_IMG = ("lcgs_bilagrid_backward, both gradients", "lcgs_bilagrid_backward, dL/dgrid only",
                         "lcgs_bilagrid_backward, dL/dimg only")
S_BOTH, S_GRID, S_IMG = ("slice + backward, both gradients", "slice + backward, dL/dgrid only", "slice + backward, dL/dimg only")
T_BOTH, T_GRID, T_IMG = ("torch: forward + autograd backward, both gradients", "torch: forward + autograd backward, dL/dgrid only",
                         "torch: forward + autograd backward, dL/dimg only")
TV, T_TV = f"lcgs_bilagrid_tv_loss_backward, {NUM_GRIDS} grids", f"torch: the TV term + autograd backward, {NUM_GRIDS} grids"
TV_EVAL = f"lcgs_bilagrid_tv_loss_backward, {NUM_GRIDS} grids, evaluation only"
PHOTO = "lcgs_photometric_loss_backward on the frame"
candidates = [
    (SLICE, lambda: r.bilagrid_slice(grid, img, out)),
    (T_SLICE, torch_forward),
    (B_BOTH, lambda: r.bilagrid_backward(grid, img, g_out, d_img, d_grid)),
    (B_GRID, lambda: r.bilagrid_backward(grid, img, g_out, None, d_grid)),
    (B_IMG, lambda: r.bilagrid_backward(grid, img, g_out, d_img, None)),
    (S_BOTH, lambda: lib_step(True, True)),
    (T_BOTH, lambda: torch_backward(True, True)),
    (S_GRID, lambda: lib_step(False, True)),
    (T_GRID, lambda: torch_backward(False, True)),
    (S_IMG, lambda: lib_step(True, False)),
    (T_IMG, lambda: torch_backward(True, False)),
    (TV, lambda: r.bilagrid_tv_loss_backward(grids, d_grids, loss, TV_WEIGHT)),
    (TV_EVAL, lambda: r.bilagrid_tv_loss_backward(grids, None, loss, TV_WEIGHT)),
    (T_TV, torch_tv),
    (PHOTO, lambda: r.photometric_loss_backward(img, target, d_img, loss)),
]
res = {name: [] for name, _ in candidates}
for _ in range(args.rounds):
    for name, fn in candidates:
        res[name].append(timed(fn))

lines = [f"bicycle stand-in, {args.splats} splats, {W}x{H}: num_rendered {n}, {(img != 0).any(dim=0).float().mean().item() * 100:.1f} % of "
         f"the pixels covered; grid {DIMS[0]} x {DIMS[1]} x {DIMS[2]}; {args.rounds} alternating rounds of {args.reps} calls after {WARM} "
         f"warm-up calls; {torch.cuda.get_device_name(0)}, clocks as the machine sets them (nothing pinned), nothing else on the stream"]
med = {}
for name, ms in res.items():
    med[name] = statistics.median(ms)
    lines.append(f"{name:76s} median {med[name] * 1e3:9.1f} us   rounds {min(ms) * 1e3:9.1f} .. {max(ms) * 1e3:9.1f} us")
px, cells = W * H, NUM_GRIDS * 12 * DIMS[0] * DIMS[1] * DIMS[2]
bw = lambda b, ms: b / (ms * 1e-3) / 1e9
lines.append(f"  traffic floors: slice {24 * px / 1e6:.1f} MB (24 B a pixel) in {med[SLICE] * 1e3:.1f} us = {bw(24 * px, med[SLICE]):.0f} GB/s;  "
             f"backward, both gradients {36 * px / 1e6:.1f} MB (36 B a pixel) in {med[B_BOTH] * 1e3:.1f} us = {bw(36 * px, med[B_BOTH]):.0f} GB/s;  "
             f"TV {8 * cells / 1e6:.1f} MB (8 B an element) in {med[TV] * 1e3:.1f} us = {bw(8 * cells, med[TV]):.0f} GB/s")
lines.append(f"  torch / library: slice {med[T_SLICE] / med[SLICE]:.1f} x;  slice + backward: both {med[T_BOTH] / med[S_BOTH]:.1f} x, "
             f"dL/dgrid only {med[T_GRID] / med[S_GRID]:.1f} x, dL/dimg only {med[T_IMG] / med[S_IMG]:.1f} x;  TV {med[T_TV] / med[TV]:.1f} x")
lines.append(f"  slice + backward (both) / lcgs_photometric_loss_backward = {med[S_BOTH] / med[PHOTO]:.2f}")

lib_step(True, True)
r.bilagrid_tv_loss_backward(grids, d_grids, loss, TV_WEIGHT)
ref_out, (ref_img, ref_grid), (ref_tv, ref_grids) = torch_forward(), torch_backward(True, True), torch_tv()
torch.cuda.synchronize()
lines.append("  largest difference from torch float32: " +
             ", ".join(f"{name} {(a - b).abs().max().item():.2e} of {b.abs().max().item():.2e}" for name, a, b in
                       (("out", out, ref_out), ("dL/dimg", d_img, ref_img), ("dL/dgrid", d_grid, ref_grid), ("TV gradient", d_grids, ref_grids))) +
             f"; TV loss {loss.item():.7f} (torch float32 {ref_tv.item():.7f})")

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
