"""Times TSDF fusion and the mesh extraction on a 512^3 volume with colour: 64 views of the bicycle stand-in at 1920x1080, their
depth / alpha maps and images rendered once, then
    lcgs_tsdf_integrate, all views in one call        (ceil(64 / 42) = 2 launches: the state is read and written once per launch)
    lcgs_tsdf_integrate, one call per view            (64 launches)
    the same update composed in torch                 (projection, nearest-pixel index, masked running mean; per view)
    lcgs_tsdf_mesh_count / lcgs_tsdf_mesh_extract     (cell pass + counts; the whole extraction: + two scans, vertex and triangle pass)
same box, same run, the integrate legs ALTERNATING repeat by repeat; hipEvent medians.
    python tools/tsdf_bench.py [--out profiles/tsdf_bench.txt] [--resolution 512] [--views 64] [--reps 5]
Beside the times: the traffic floor of a launch (20 B read + 20 B written per sample, whatever the views in it) against the 8 TB/s
HBM peak, the batched / one-per-call ratio and the torch ratio."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resolution", type=int, default=512)
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
W, H, N, HBM = 1920, 1080, args.resolution, 8.0e12
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
rng = np.random.default_rng(3)
cams = []
for k in range(args.views):
    a, dist = 2 * np.pi * k / args.views, rng.uniform(3.0, 4.5)
    cams.append(L.get_lookat_cam([dist * np.cos(a), dist * np.sin(a), rng.uniform(0.6, 2.3)], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0],
                                 width=W, height=H))
maps = []
for cam in cams:
    img, depth, alpha = torch.zeros(3, H, W, device=dev), torch.zeros(H, W, device=dev), torch.zeros(H, W, device=dev)
    r.forward(cam, img, keep_state=True, sync=True)
    r.render_maps(depth, alpha, mode="z")
    maps.append((img, depth, alpha))
side = 8.0
origin, voxel = (-0.5 * side, -0.5 * side, 0.5 - 0.5 * side), side / (N - 1)
volume = L.TsdfVolume(origin, voxel, (N, N, N), rgb=True, device=dev)
n = N ** 3
cfg = dict(trunc=4 * voxel, depth_max=50.0, alpha_min=0.5)
depths, alphas, images = [m[1] for m in maps], [m[2] for m in maps], [m[0] for m in maps]


def batched():
    r.tsdf_integrate(volume, cams, depths, alphas, images, **cfg)


def one_per_call():
    for k, cam in enumerate(cams):
        r.tsdf_integrate(volume, [cam], depths[k:k + 1], alphas[k:k + 1], images[k:k + 1], **cfg)


# ---- the same update in torch: per view (R, t, 1 / tan) from the library's own host matrices
ax = [torch.tensor(np.float32(origin[c]) + np.float32(voxel) * np.arange(N, dtype=np.float32), device=dev) for c in range(3)]
X = torch.stack(torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")[::-1], dim=-1).reshape(n, 3)  # sample-major, (x, y, z)
view_t = []
for cam in cams:
    m = L.world_to_local_matrix(cam)
    tany = float(np.tan(np.float32(cam.fov) / np.float32(180.0) * np.float32(3.1415926536) * np.float32(0.5)))
    view_t.append((torch.tensor(m[:3, :3], device=dev), torch.tensor(m[:3, 3], device=dev), 1.0 / (tany * cam.aspect_ratio), 1.0 / tany))


def torch_integrate():
    tsdf, weight, rgb = volume.tsdf.view(n), volume.weight.view(n), volume.rgb.view(n, 3)
    for (R, t, itx, ity), (img, depth, alpha) in zip(view_t, maps):
        v = X @ R.T + t
        z = v[:, 2]
        ux, uy = (v[:, 0] / z * itx + 1.0) * (0.5 * W), (v[:, 1] / z * ity + 1.0) * (0.5 * H)
        ok = (z > 0) & (ux >= 0) & (ux < W) & (uy >= 0) & (uy < H)
        pix = (torch.floor(uy).clamp_(0, H - 1).long() * W + torch.floor(ux).clamp_(0, W - 1).long()).masked_fill_(~ok, 0)
        a = alpha.view(-1)[pix]
        dd = depth.view(-1)[pix] / a
        sdf = dd - z
        ok &= (a >= cfg["alpha_min"]) & torch.isfinite(dd) & (dd > 0) & (dd <= cfg["depth_max"]) & (sdf >= -cfg["trunc"])
        u = torch.clamp(sdf / cfg["trunc"], max=1.0)
        w1 = weight + 1.0
        tsdf.copy_(torch.where(ok, (tsdf * weight + u) / w1, tsdf))
        rgb.copy_(torch.where(ok[:, None], (rgb * weight[:, None] + img.view(3, -1)[:, pix].T) / w1[:, None], rgb))
        weight.copy_(torch.where(ok, w1, weight))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


legs = {"batched": batched, "one_per_call": one_per_call, "torch": torch_integrate}
ms = {k: [] for k in legs}
for i in range(args.reps + 1):  # (the first round warms up)
    for name, fn in legs.items():
        if name == "torch" and i > min(args.reps, 2):
            continue  # (seconds per repeat: three are enough for a median)
        t, _ = timed(fn)
        if i >= 1:
            ms[name].append(t)
med = {k: statistics.median(v) for k, v in ms.items()}

# ---- the mesh of a freshly fused volume (every view once)
volume.zero_()
batched()
r.ctx.synchronize()
seen = int((volume.weight > 0).sum())
count_ms, extract_ms = [], []
for i in range(args.reps + 1):
    t, (nv, nt) = timed(lambda: r.tsdf_mesh_count(volume, 1.0))
    verts = torch.empty((nv, 3), device=dev)
    cols = torch.empty((nv, 3), device=dev)
    tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    got = (C.c_uint64(0), C.c_uint64(0))
    vol = volume._struct()
    t2, st = timed(lambda: L.load_library().lcgs_tsdf_mesh_extract(r.ctx._h, C.byref(vol), 1.0, nv, nt, verts.data_ptr(), cols.data_ptr(),
                                                                    tris.data_ptr(), C.addressof(got[0]), C.addressof(got[1])))
    assert st == 0 and (got[0].value, got[1].value) == (nv, nt)
    if i >= 1:
        count_ms.append(t), extract_ms.append(t2)
cm, em = statistics.median(count_ms), statistics.median(extract_ms)

launches = -(-args.views // L.api.LCGS_TSDF_VIEW_CHUNK)
floor_bytes = 40.0 * n
lines = [
    f"TSDF fusion, {N}^3 volume with colour ({n} samples x 20 B), {args.views} views of the bicycle stand-in ({args.splats} splats) at "
    f"{W}x{H}; hipEvent medians of {args.reps} (torch: {len(ms['torch'])}), legs alternating",
    f"traffic floor per launch: 20 B read + 20 B written per sample = {floor_bytes / 1e9:.2f} GB = {floor_bytes / HBM * 1e3:.2f} ms at 8 TB/s",
    f"lcgs_tsdf_integrate, {args.views} views in one call ({launches} launches)   {med['batched']:10.3f} ms   "
    f"{launches * floor_bytes / (med['batched'] * 1e-3) / 1e12:.2f} TB/s of the floor's bytes = {launches * floor_bytes / (med['batched'] * 1e-3) / HBM * 100:.0f} % of 8 TB/s; "
    f"{med['batched'] * 1e9 / (n * args.views):.2f} ps per (sample, view)",
    f"lcgs_tsdf_integrate, one call per view ({args.views} launches)        {med['one_per_call']:10.3f} ms   "
    f"{args.views * floor_bytes / (med['one_per_call'] * 1e-3) / 1e12:.2f} TB/s of the floor's bytes; one-per-call / batched = {med['one_per_call'] / med['batched']:.2f}",
    f"the same update composed in torch (per view)              {med['torch']:10.3f} ms   torch / batched = {med['torch'] / med['batched']:.1f}",
    f"mesh of the fused volume ({seen} samples seen): {nv} vertices, {nt} triangles",
    f"lcgs_tsdf_mesh_count   (clear, cell pass, counts, read-back)   {cm:10.3f} ms",
    f"lcgs_tsdf_mesh_extract (the same + two scans, vertex pass, triangle pass) {em:10.3f} ms   scans + vertex + triangle passes = {em - cm:.3f} ms",
    "(the floor counts every sample as written; the kernel stores only the samples a view of the launch touched)",
]
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
