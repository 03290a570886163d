"""A triangle mesh out of a trained scene, file to file: TSDF fusion of the views' rendered depth maps, then marching tetrahedra.
    python tools/extract_mesh.py in.ply cameras.txt mesh.ply [--width 1920 --height 1080] [--resolution 256 | --voxel V]
                                 [--origin X Y Z --size SX SY SZ] [--trunc T] [--depth-max D] [--alpha-min A] [--weight-min W]
                                 [--chunk 16] [--no-colour]
cameras.txt is lcgs-app's --cameras file (tools/prune_ply.py reads the same): `px py pz tx ty tz ux uy uz [fov]` per line.  The
volume is the cube of lcgs_scene_extent (the cameras' centre, 1.1 x their largest distance from it) cut into --resolution voxels
a side, or the box --origin / --size at --voxel.  Every view is rendered once with keep_state; lcgs_render_maps(LCGS_DEPTH_Z)
gives its accumulated depth and opacity; lcgs_tsdf_integrate fuses --chunk views per call (colour from the rendered image);
lcgs_tsdf_mesh_extract takes the zero level set of the cells every sample of which some view has seen --weight-min times."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402
from tools.prune_ply import read_cameras  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_ply")
    ap.add_argument("cameras")
    ap.add_argument("out_ply")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--voxel", type=float, default=None)
    ap.add_argument("--origin", type=float, nargs=3, default=None)
    ap.add_argument("--size", type=float, nargs=3, default=None)
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance (default: 4 voxels)")
    ap.add_argument("--depth-max", type=float, default=None, help="default: the volume's diagonal plus the cameras' radius")
    ap.add_argument("--alpha-min", type=float, default=0.5)
    ap.add_argument("--weight-min", type=float, default=1.0)
    ap.add_argument("--chunk", type=int, default=16, help="views fused per lcgs_tsdf_integrate call")
    ap.add_argument("--no-colour", action="store_true")
    args = ap.parse_args(argv)
    if (args.origin is None) != (args.size is None):
        raise SystemExit("--origin and --size go together")
    cams = read_cameras(args.cameras, args.width, args.height)
    center, radius = L.scene_extent(cams)
    if args.origin is not None:
        origin, size = np.asarray(args.origin, np.float64), np.asarray(args.size, np.float64)
        voxel = args.voxel if args.voxel else float(size.max()) / args.resolution
    else:
        origin, size = center.astype(np.float64) - radius, np.full(3, 2.0 * radius)
        voxel = args.voxel if args.voxel else 2.0 * radius / args.resolution
    if not (voxel > 0 and np.isfinite(voxel)):
        raise SystemExit("the volume is empty: give --origin / --size / --voxel (one camera has no extent)")
    dims = [int(np.ceil(s / voxel)) + 1 for s in size]
    depth_max = args.depth_max if args.depth_max else float(np.linalg.norm(size)) + 2.0 * radius + 1.0

    dev = torch.device("cuda", 0)
    r = L.Renderer(L.Context(0))
    P = r.load_ply(args.in_ply)
    volume = L.TsdfVolume(origin, voxel, dims, rgb=not args.no_colour, device=dev)
    H, W = args.height, args.width
    slots = [(torch.zeros(3, H, W, device=dev), torch.zeros(H, W, device=dev), torch.zeros(H, W, device=dev))
             for _ in range(max(1, min(args.chunk, len(cams))))]
    for first in range(0, len(cams), len(slots)):
        batch = cams[first:first + len(slots)]
        for cam, (img, depth, alpha) in zip(batch, slots):
            r.forward(cam, img, keep_state=True, sync=True)
            r.render_maps(depth, alpha, mode="z")
        n = len(batch)
        r.tsdf_integrate(volume, batch, [s[1] for s in slots[:n]], [s[2] for s in slots[:n]],
                         None if args.no_colour else [s[0] for s in slots[:n]], trunc=args.trunc, depth_max=depth_max,
                         alpha_min=args.alpha_min)
    vertices, rgb, triangles = r.tsdf_mesh(volume, weight_min=args.weight_min)
    r.ctx.synchronize()
    L.write_mesh_ply(args.out_ply, vertices, triangles, rgb)
    print(f"{args.out_ply}: {vertices.shape[0]} vertices, {triangles.shape[0]} triangles from {P} splats over {len(cams)} views; "
          f"volume {dims[0]} x {dims[1]} x {dims[2]} at voxel {voxel:.4g}, {int((volume.weight >= args.weight_min).sum())} samples seen")


if __name__ == "__main__":
    main()
