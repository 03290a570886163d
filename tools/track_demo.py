"""Camera tracking against a fixed scene -- a demonstration of the camera gradient, not a test.
Renders a target from a pose, perturbs the pose, then runs gradient steps on a twist in the camera's own frame: each step
renders through render_autograd_camera, takes the photometric loss (L1 + D-SSIM, lcgs_photometric_loss_backward), backpropagates
to the twelve camera numbers (lcgs_render_backward_camera: no parameter rows), chains them onto the twist
(lcgs_camera_grad_to_twist), and applies an Adam step to the six numbers.  Prints the pose error per step.
    python tools/track_demo.py [--steps 60] [--splats 200000] [--out profiles/track_demo.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--splats", type=int, default=200_000)
ap.add_argument("--rot-deg", type=float, default=3.0, help="size of the rotation perturbation")
ap.add_argument("--shift", type=float, default=0.08, help="size of the translation perturbation (scene units)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H = 640, 360
KEYS = ("pos", "scale", "rotq", "sh", "opacity")


def exp_so3(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * (K @ K)


def apply_twist(Rc, p, xi):
    """[right up front]' = [right up front] exp([omega]x), position' = position + [right up front] tau"""
    return Rc @ exp_so3(xi[0:3]), p + Rc @ xi[3:6]


def cam12_of(Rc, p):
    return np.concatenate([p, Rc[:, 2], Rc[:, 1], Rc[:, 0]]).astype(np.float32)  # position, front, up, right


scene = L.synth_scene(1, 2001, args.splats)
t = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))
cam = L.get_lookat_cam([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0], width=W, height=H)
Rc_true = np.stack([np.array(cam.right[:], np.float64), np.array(cam.up[:], np.float64), np.array(cam.front[:], np.float64)], axis=1)
p_true = np.array(cam.position[:], np.float64)

with torch.no_grad():
    target = L.render_autograd_camera(r, cam, torch.from_numpy(cam12_of(Rc_true, p_true)), *[t[k] for k in KEYS])[0].clone()

rng = np.random.default_rng(7)
axis = rng.normal(size=3)
Rc, p = apply_twist(Rc_true, p_true, np.concatenate([np.radians(args.rot_deg) * axis / np.linalg.norm(axis),
                                                     args.shift * rng.normal(size=3) / np.sqrt(3.0)]))


def pose_error(Rc, p):
    c = np.clip((np.trace(Rc_true.T @ Rc) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(p - p_true))


lines = [f"bicycle stand-in, {args.splats} splats, {W}x{H}; perturbation {args.rot_deg} deg, {args.shift} units; "
         f"photometric loss, Adam on the twist (rates 2e-3 rad, 5e-3 units)"]
m, v = np.zeros(6), np.zeros(6)
rate = np.array([2e-3] * 3 + [5e-3] * 3)
loss, dL = torch.zeros(1, device=dev), torch.zeros(3, H, W, device=dev)
for step in range(args.steps + 1):
    c12 = torch.from_numpy(cam12_of(Rc, p)).requires_grad_(True)
    view = L.camera_with_vectors(cam, c12.detach().numpy())
    img = L.render_autograd_camera(r, cam, c12, *[t[k] for k in KEYS])[0]
    r.photometric_loss_backward(img.detach(), target, dL, loss)
    img.backward(dL)
    g6 = L.camera_grad_to_twist(view, c12.grad.numpy()).astype(np.float64)
    deg, dist = pose_error(Rc, p)
    lines.append(f"step {step:3d}   loss {float(loss):.6f}   rotation error {deg:8.4f} deg   position error {dist:.5f}   "
                 f"|dL/domega| {np.linalg.norm(g6[:3]):.3e}   |dL/dtau| {np.linalg.norm(g6[3:]):.3e}")
    print(lines[-1], flush=True)
    m = 0.9 * m + 0.1 * g6
    v = 0.999 * v + 0.001 * g6 * g6
    k = step + 1
    xi = -rate * (m / (1 - 0.9 ** k)) / (np.sqrt(v / (1 - 0.999 ** k)) + 1e-12)
    Rc, p = apply_twist(Rc, p, xi)

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
