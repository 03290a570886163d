"""Times lcgs_scene_transform on the 6.13 M-splat bicycle stand-in at degree 3 -- in place, out of place, and the coefficients
only -- against two yardsticks on the same arrays, same box, same run, the three ALTERNATING round by round:
  copy    a device-to-device copy of the same arrays (torch.Tensor.copy_): what moving the bytes costs and nothing else
  torch   the same transform composed in torch (a matmul for the positions, the quaternion product, one einsum per band)
    python tools/transform_bench.py [--out profiles/transform_bench.txt]
A round times --calls back-to-back calls between two device events; the figures are per call, per round, with their median.  The
traffic floor is 2 x 59 x 4 B per row (every float read once and written once; 2 x 48 x 4 B for the coefficients alone), stated
beside the achieved TB/s against the 8 TB/s HBM peak.  The library's figure over the copy's is the price of the arithmetic and of
staging the coefficient rows through LDS."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

P, dev, HBM = args.splats, torch.device("cuda", 0), 8.0e12
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
host = L.synth_scene(1, 2001, P)
src = {k: torch.from_numpy(host[k]).to(dev) for k in KEYS}
dst = {k: torch.empty_like(v) for k, v in src.items()}
work = {k: v.clone() for k, v in src.items()}  # the in-place leg's arrays

q = np.random.default_rng(1).normal(size=4)
q /= np.linalg.norm(q)
w, x, y, z = q
rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
xf = L.similarity(rot, 1.0, (0.7, -1.3, 2.1))  # (scale 1: the in-place leg applies it rounds x calls times over)
plan, _ = L.similarity_plan(xf)
t = lambda a, *shape: torch.tensor(list(a), device=dev).reshape(*shape)
M, tr, s, Q = t(plan.M, 3, 3), t(plan.t, 3), float(plan.s), list(plan.q)
D = (t(plan.D1, 3, 3), t(plan.D2, 5, 5), t(plan.D3, 7, 7))
r = L.Renderer(L.Context(0))


def torch_sh(sh):
    c = sh.view(P, 16, 3)
    return torch.cat([c[:, :1]] + [torch.einsum("kj,pjc->pkc", D[l - 1], c[:, l * l:(l + 1) * (l + 1)]) for l in (1, 2, 3)], dim=1)


def torch_all(a):
    W, X, Y, Z = Q
    w, x, y, z = a["rotq"].unbind(1)
    rq = torch.stack([W * w - X * x - Y * y - Z * z, W * x + X * w + Y * z - Z * y, W * y - X * z + Y * w + Z * x,
                      W * z + X * y - Y * x + Z * w], dim=1)
    return a["pos"] @ M.T + tr, s * a["scale"], rq, torch_sh(a["sh"]), a["opacity"].clone()


def copy_all(keys):
    for k in keys:
        dst[k].copy_(src[k])


LEGS = [  # name, bytes per row at the floor, library, copy, torch
    ("in place      ", 2 * 59 * 4, lambda: r.scene_transform(xf, work), lambda: copy_all(KEYS), lambda: torch_all(src)),
    ("out of place  ", 2 * 59 * 4, lambda: r.scene_transform(xf, src, dst), lambda: copy_all(KEYS), lambda: torch_all(src)),
    ("SH only       ", 2 * 48 * 4, lambda: r.scene_transform(xf, src, {"sh": dst["sh"]}), lambda: copy_all(("sh",)),
     lambda: torch_sh(src["sh"])),
]


def rounds(fns):
    """per side: ms per call of every round (2 warm-up rounds dropped), the sides taking turns inside each round"""
    ms = [[] for _ in fns]
    for i in range(args.rounds + 2):
        for side, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                out = fn()
            b.record()
            b.synchronize()
            del out
            if i >= 2:
                ms[side].append(a.elapsed_time(b) / args.calls)
    return ms


lines = [f"lcgs_scene_transform, {P} splats at degree 3 (bicycle stand-in); {args.rounds} rounds of {args.calls} calls between device "
         f"events, library / copy / torch alternating inside every round; ms per call"]
for name, per_row, lib, cp, tor in LEGS:
    ms = rounds((lib, cp, tor))
    med = [float(np.median(m)) for m in ms]
    gb = per_row * P / 1e9
    lines.append(f"{name} library {med[0]:7.3f} ms   copy {med[1]:7.3f} ms   torch {med[2]:7.3f} ms   library / copy {med[0] / med[1]:.2f}   "
                 f"torch / library {med[2] / med[0]:.1f}   floor {per_row} B per row = {gb:.3f} GB: library {gb / med[0]:.2f} TB/s "
                 f"({gb / med[0] / (HBM / 1e12) * 100:.0f} % of 8 TB/s), copy {gb / med[1]:.2f} TB/s")
    for side, m in zip(("library", "copy   ", "torch  "), ms):
        lines.append(f"    {side} per round: " + " ".join(f"{v:.3f}" for v in m) + f"   (min {min(m):.3f}, max {max(m):.3f})")
torch.cuda.synchronize()
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
