"""A similarity transform of a trained scene, file to file: new = scale * R * old + translate, with the SH bands rotated.
    python tools/transform_ply.py in.ply out.ply [--rotate AX AY AZ DEGREES | --quat W X Y Z] [--scale S] [--translate X Y Z]
                                  [--crop CX CY CZ HX HY HZ] [--also in2.ply [--also-rotate ... | --also-quat ...]
                                                                              [--also-scale S] [--also-translate X Y Z]]
The file goes through lcgs_scene_load_ply in FILE order, lcgs_scene_transform in place on the context's arrays,
lcgs_scene_download and lcgs_ply_write_raw; the file's raw properties are recovered in binary64 (log of the scale, logit of the
opacity; the rotation is written as the unit quaternion).  --crop keeps the rows whose NEW position lies in the axis-aligned box
with centre C and half extents H (inf: unbounded on that axis; faces included) through lcgs_scene_box_keep_mask.  --also appends
a second file's rows after that file's own transform (the merge of two captures: bring each into the common frame); the crop
applies to both.  Positions, scales and orientations move with the scene and so does the view-dependent colour: a transform that
leaves the degree-1 to degree-3 coefficients alone renders highlights nailed to the old axes."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402


def rotation_matrix(axis_angle=None, quat=None):
    """row-major 3 x 3, binary64, from `ax ay az degrees` or `w x y z` (either is normalised); neither: the identity"""
    if axis_angle is not None and quat is not None:
        raise SystemExit("give the rotation once: axis-angle or quaternion")
    if quat is None:
        if axis_angle is None:
            return np.eye(3)
        a = np.asarray(axis_angle[:3], np.float64)
        if not np.linalg.norm(a) > 0:
            raise SystemExit("the rotation axis is zero")
        half = np.radians(axis_angle[3]) / 2
        quat = [np.cos(half), *(np.sin(half) * a / np.linalg.norm(a))]
    q = np.asarray(quat, np.float64)
    if not np.linalg.norm(q) > 0:
        raise SystemExit("the quaternion is zero")
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def transformed(path, xf, box):
    """the file's rows after xf (host arrays of read_gs_ply's layout), cropped by box = (world_to_box, half extents) or None"""
    r = L.Renderer(L.Context(0))
    P = r.load_ply(path, order="file")
    if P == 0:
        return r.download_scene(), 0
    arrays = r.scene_tensors()
    r.scene_transform(xf, arrays)
    keep = None
    if box is not None:
        keep = torch.zeros(P, dtype=torch.uint8, device=arrays["pos"].device)
        r.scene_box_keep_mask(arrays["pos"], box[0], box[1], keep)
    scene = r.download_scene()  # (synchronises the context's stream)
    if keep is not None:
        rows = keep.cpu().numpy() != 0
        scene = {k: v[rows] for k, v in scene.items()}
    r.ctx.close()
    return scene, P


def write_raw(path, scene):
    """lcgs_ply_write_raw from ACTIVATED arrays: the raw properties recovered in binary64"""
    P = scene["pos"].shape[0]
    sh = scene["sh"].reshape(P, 16, 3)
    with np.errstate(divide="ignore"):
        o = scene["opacity"].astype(np.float64)
        L.write_ply_raw(path, scene["pos"], sh[:, 0, :], sh[:, 1:, :].transpose(0, 2, 1).reshape(P, 45), np.log(o / (1.0 - o)),
                        np.log(scene["scale"].astype(np.float64)), scene["rotq"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("in_ply")
    ap.add_argument("out_ply")
    for prefix in ("", "also-"):
        ap.add_argument(f"--{prefix}rotate", type=float, nargs=4, metavar=("AX", "AY", "AZ", "DEGREES"))
        ap.add_argument(f"--{prefix}quat", type=float, nargs=4, metavar=("W", "X", "Y", "Z"))
        ap.add_argument(f"--{prefix}scale", type=float, default=1.0)
        ap.add_argument(f"--{prefix}translate", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--crop", type=float, nargs=6, metavar=("CX", "CY", "CZ", "HX", "HY", "HZ"))
    ap.add_argument("--also", metavar="IN2_PLY")
    args = ap.parse_args()
    box = None
    if args.crop:
        box = (L.similarity(None, 1.0, [-c for c in args.crop[:3]]), args.crop[3:])
    xf = L.similarity(rotation_matrix(args.rotate, args.quat), args.scale, args.translate)
    scene, P = transformed(args.in_ply, xf, box)
    counts = [(args.in_ply, P, scene["pos"].shape[0])]
    if args.also:
        xf2 = L.similarity(rotation_matrix(args.also_rotate, args.also_quat), args.also_scale, args.also_translate)
        more, P2 = transformed(args.also, xf2, box)
        counts.append((args.also, P2, more["pos"].shape[0]))
        scene = {k: np.concatenate([scene[k], more[k]]) for k in scene}
    write_raw(args.out_ply, scene)
    print(f"{args.out_ply}: {scene['pos'].shape[0]} splats (" +
          "; ".join(f"{kept} of {n} from {p}" for p, n, kept in counts) + ")")


if __name__ == "__main__":
    main()
