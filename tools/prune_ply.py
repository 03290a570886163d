"""Contribution-based pruning of a trained scene, file to file: the splats a set of views never uses (or hardly uses) are dropped.
    python tools/prune_ply.py in.ply cameras.txt out.ply [--min-weight-max 0.01] [--min-weight-sum S] [--min-pixels N]
                              [--min-views N] [--width 1920 --height 1080]
cameras.txt is lcgs-app's --cameras file: `px py pz tx ty tz ux uy uz [fov]` per line.  Every view is rendered once with
keep_state, lcgs_contrib_accumulate scores the splats by their blend weights, lcgs_contrib_keep_mask applies the minimums
(RadSplat's rule is the default: largest blend weight over the views >= 0.01) and lcgs_ply_filter_rows copies the kept vertex
records bit for bit.  The scene is loaded in FILE order, so the mask's rows are the file's rows."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402


def read_cameras(path, width, height):
    cams = []
    for line in open(path):
        v = [float(x) for x in line.split("#")[0].split()]
        if not v:
            continue
        if len(v) not in (9, 10):
            raise SystemExit(f"bad camera line in {path}: {line.strip()}")
        cams.append(L.get_lookat_cam(v[0:3], v[3:6], v[6:9], width=width, height=height, fov=v[9] if len(v) == 10 else None))
    if not cams:
        raise SystemExit(f"no cameras in {path}")
    return cams


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_ply")
    ap.add_argument("cameras")
    ap.add_argument("out_ply")
    ap.add_argument("--min-weight-max", type=float, default=None)
    ap.add_argument("--min-weight-sum", type=float, default=0.0)
    ap.add_argument("--min-pixels", type=int, default=0)
    ap.add_argument("--min-views", type=int, default=0)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    minimums = dict(min_weight_max=args.min_weight_max or 0.0, min_weight_sum=args.min_weight_sum, min_pixels=args.min_pixels,
                    min_views=args.min_views)
    if args.min_weight_max is None and not any(minimums.values()):
        minimums["min_weight_max"] = 0.01  # RadSplat's rule
    dev = torch.device("cuda", 0)
    r = L.Renderer(L.Context(0))
    P = r.load_ply(args.in_ply, order="file")
    cams = read_cameras(args.cameras, args.width, args.height)
    stats = {"weight_sum": torch.zeros(P, device=dev), "weight_max": torch.zeros(P, device=dev),
             "pixels": torch.zeros(P, dtype=torch.int32, device=dev), "views": torch.zeros(P, dtype=torch.int32, device=dev)}
    img = torch.zeros(3, args.height, args.width, device=dev)
    for cam in cams:
        r.forward(cam, img, keep_state=True, sync=True)
        r.contrib_accumulate(stats)
    keep = torch.zeros(P, dtype=torch.uint8, device=dev)
    r.contrib_keep_mask(stats, keep, **minimums)
    r.ctx.synchronize()
    L.ply_filter_rows(args.in_ply, args.out_ply, keep.cpu().numpy())
    rule = ", ".join(f"{k} = {v:g}" for k, v in minimums.items() if v)
    print(f"{args.out_ply}: {int(keep.sum())} of {P} splats kept over {len(cams)} views ({rule}); "
          f"{int((stats['views'] == 0).sum())} were blended by no pixel of any view")


if __name__ == "__main__":
    main()
