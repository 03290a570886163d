"""Times the 3-D smoothing filter's steps on the 6.13 M-splat bicycle stand-in's size -- lcgs_filter3d_accumulate over 8 views and
over a few hundred, lcgs_filter3d_finalize, lcgs_filter3d_apply, lcgs_filter3d_backward (dense rows) -- against the same steps
composed in torch (after Mip-Splatting's compute_3D_filter / get_scaling_with_3D_filter / get_opacity_with_3D_filter and autograd
through them), same box, same run, the two ALTERNATING repeat by repeat: hipEvent median of --reps each.
    python tools/filter3d_bench.py [--out profiles/filter3d_bench.txt]
Beside the times: the bytes apply and backward must move (36 and 52 per row) over their time against the 8 TB/s HBM peak, and
the accumulate pass's cost per (row, view) with the plain vector operations that is (26 per pair in the kernel's inner loop)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--views", type=int, default=256)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

P, dev = args.splats, torch.device("cuda", 0)
HBM, VALU = 8.0e12, 157.3e12 / 2  # bytes/s; plain f32 vector operations/s (the FMA peak counts two per operation)
PAIR_OPS = 26                     # v_mul / v_add / v_cmp / v_cndmask per (row, view) in k_filter3d_accumulate's inner loop
gen = torch.Generator(device=dev).manual_seed(1)
u = lambda *s: torch.rand(*s, device=dev, generator=gen)
rng = np.random.default_rng(1)

pos = (u(P, 3) * 2 - 1) * torch.tensor([4.0, 4.0, 1.5], device=dev)
scale = torch.exp(torch.randn(P, 3, device=dev, generator=gen) * 1.0 - 4.5)
opacity = 0.02 + 0.9 * u(P)
g_scale, g_opacity = torch.randn(P, 3, device=dev, generator=gen), torch.randn(P, device=dev, generator=gen)


def ring(n):
    cams = []
    for k in range(n):
        a, d = 2 * np.pi * k / n, rng.uniform(3.0, 6.0)
        cams.append(L.get_lookat_cam([d * np.cos(a), d * np.sin(a), rng.uniform(0.2, 2.0)], [0, 0, 0], [0, 0, 1],
                                     width=1245, height=825, fov=float(rng.uniform(40.0, 70.0))))
    return cams


cams = {8: ring(8), args.views: ring(args.views)}
r = L.Renderer(L.Context(0))


def view_tensors(cs):
    """per view: (R [3, 3], t [3], limx, limy) on the device, from the library's own host matrices"""
    out = []
    for c in cs:
        m = L.world_to_local_matrix(c)
        tany = float(np.tan(np.float32(c.fov) / np.float32(180.0) * np.float32(3.1415926536) * np.float32(0.5)))
        out.append((torch.tensor(m[:3, :3], device=dev), torch.tensor(m[:3, 3], device=dev), 1.3 * tany * c.aspect_ratio, 1.3 * tany))
    return out


def torch_accumulate(views, min_z):
    for R, t, limx, limy in views:
        v = pos @ R.T + t
        z = v[:, 2]
        seen = (z > 0.2) & (v[:, 0].abs() <= limx * z) & (v[:, 1].abs() <= limy * z)
        torch.minimum(min_z, torch.where(seen, z, torch.inf), out=min_z)


def torch_finalize(min_z, focal):
    finite = torch.isfinite(min_z)
    zmax = torch.where(finite, min_z, -torch.inf).max()
    return torch.where(finite, min_z, zmax) / focal * (0.2 ** 0.5)


def torch_apply(s, o, f):
    f2 = (f * f)[:, None]
    a = s * s
    b = a + f2
    return torch.sqrt(b), o * torch.sqrt(torch.prod(a / b, dim=1))


def alternate(lib_fn, torch_fn, prep=None):
    """(library ms, torch ms): medians of --reps repeats after 2 warm-ups, the two sides taking turns"""
    ms = ([], [])
    for i in range(args.reps + 2):
        for side, fn in enumerate((lib_fn, torch_fn)):
            if prep:
                prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            if i >= 2:
                ms[side].append(a.elapsed_time(b))
            del out
    return float(np.median(ms[0])), float(np.median(ms[1]))


min_z = torch.empty(P, device=dev)
filt = torch.empty(P, device=dev)
reset = lambda: min_z.fill_(float("inf"))
acc = {}
for n, cs in cams.items():
    vt = view_tensors(cs)
    acc[n] = alternate(lambda: r.filter3d_accumulate(pos, cs, min_z), lambda: torch_accumulate(vt, min_z), reset)
reset()
focal = r.filter3d_accumulate(pos, cams[args.views], min_z)
fin = alternate(lambda: r.filter3d_finalize(min_z, focal, filt), lambda: torch_finalize(min_z, focal))
r.filter3d_finalize(min_z, focal, filt)
r.ctx.synchronize()
seen_rows = int(torch.isfinite(min_z).sum())
s_out, o_out = torch.empty_like(scale), torch.empty_like(opacity)
app = alternate(lambda: r.filter3d_apply(scale, opacity, filt, s_out, o_out), lambda: torch_apply(scale, opacity, filt))
gs, go = g_scale.clone(), g_opacity.clone()
s_leaf, o_leaf = scale.clone().requires_grad_(True), opacity.clone().requires_grad_(True)
graph = []


def torch_forward():  # (outside the timed window: the library's backward re-derives the forward, autograd keeps it)
    graph[:] = torch_apply(s_leaf, o_leaf, filt)


def restore():
    gs.copy_(g_scale)
    go.copy_(g_opacity)
    torch_forward()


bwd = alternate(lambda: r.filter3d_backward(scale, opacity, filt, gs, go),
                lambda: torch.autograd.grad(graph, (s_leaf, o_leaf), (g_scale, g_opacity)), restore)

pairs = {n: P * n for n in cams}
lines = [f"3-D smoothing filter, {P} splats ({seen_rows} seen by one of {args.views} views), 1245 x 825 views; hipEvent median of "
         f"{args.reps}, library and torch alternating"]
for n in cams:
    hip, tor = acc[n]
    lines.append(f"lcgs_filter3d_accumulate, {n:3d} views {hip:9.3f} ms   torch composition {tor:9.3f} ms   ({tor / hip:.1f} x)   "
                 f"{hip * 1e9 / pairs[n]:.2f} ps per (row, view) = {PAIR_OPS * pairs[n] / (hip * 1e-3) / 1e12:.1f} T plain vector operations/s "
                 f"= {PAIR_OPS * pairs[n] / (hip * 1e-3) / VALU * 100:.0f} % of {VALU / 1e12:.1f} T/s; {16 * P / (hip * 1e-3) / 1e12:.2f} TB/s of its 16 B per row")
for name, (hip, tor), per_row in (("lcgs_filter3d_finalize ", fin, 12), ("lcgs_filter3d_apply    ", app, 36), ("lcgs_filter3d_backward ", bwd, 52)):
    lines.append(f"{name}            {hip:9.3f} ms   torch composition {tor:9.3f} ms   ({tor / hip:.1f} x)   {per_row} B per row: "
                 f"{per_row * P / 1e9:.3f} GB moved, {per_row * P / (hip * 1e-3) / 1e12:.2f} TB/s = {per_row * P / (hip * 1e-3) / HBM * 100:.0f} % of 8 TB/s")
lines.append("(finalize: two passes over min_z, 4 + 4 B read and 4 B written per row; the torch compositions' own traffic is not counted; the "
             "torch backward is autograd through a forward kept outside the timed window)")
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
