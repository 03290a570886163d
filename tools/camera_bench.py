"""Times the camera gradient on the bicycle stand-in at 1920x1080 (the method of tools/maps_bench.py: events on the context's
stream around whole calls, the library's own event pairs for stages, median of --reps after warm-up):
    (a) lcgs_camera_backward alone, behind a backward, beside that backward's `preprocess_backward` stage
    (b) a tracking iteration, forward(keep_state) + lcgs_render_backward_camera, against forward(keep_state) +
        lcgs_render_backward on the same frame and the same dL_dimg
    python tools/camera_bench.py [--out profiles/camera_backward_bench.txt] [--splats N]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.reps >= 20
dev = torch.device("cuda", 0)
W, H, WARM = 1920, 1080, 5
KEYS = ("pos", "scale", "rotq", "sh", "opacity")

scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
cam = L.get_lookat_cam([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0], width=W, height=H)  # bench.py's view 0
img = torch.zeros(3, H, W, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
dL_img = torch.randn(3, H, W, device=dev, generator=g)
dL_d, dL_a = torch.randn(H, W, device=dev, generator=g), torch.randn(H, W, device=dev, generator=g)
grads = [torch.zeros_like(d[k]) for k in KEYS]
out12, out12b = torch.zeros(12, device=dev), torch.zeros(12, device=dev)


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
    return statistics.median(ms), min(ms)


def stages(fn):
    """median per stage of the library's own marks over the repetitions"""
    seen = {}
    for i in range(args.reps + WARM):
        fn()
        r.ctx.synchronize()
        if i >= WARM:
            for k, v in r.stage_times().items():
                seen.setdefault(k, []).append(v)
    return {k: (statistics.median(v), min(v)) for k, v in seen.items()}


lines = []
row = lambda name, t: lines.append(f"{name:72s} median {t[0] * 1e3:9.1f} us   best {t[1] * 1e3:9.1f} us   ({args.reps} calls)")
n = r.forward(cam, img, keep_state=True, sync=True)
stats = r.frame_stats()
lines.append(f"bicycle stand-in, {args.splats} splats, {W}x{H}: num_rendered {n}, {stats['num_visible']} on screen, "
             f"{stats['num_pairs']} pairs")

# ---- (a) the camera pass alone, behind a backward; its yardstick is the parameter pass over the same rows
r.set_profiling(True)
bwd = stages(lambda: r.backward(dL_img, *grads))
r.set_profiling(False)
r.forward(cam, img, keep_state=True, sync=True)
r.backward(dL_img, *grads)
row("(a) lcgs_render_backward stage `preprocess_backward`", bwd["preprocess_backward"])
cam_alone = timed(lambda: r.camera_backward(out12))
row("(a) lcgs_camera_backward alone (both kernels), behind lcgs_render_backward", cam_alone)
r.backward_maps(dL_img, dL_d, dL_a, *grads, mode="inv_z")
row("(a) lcgs_camera_backward alone, behind lcgs_render_backward_maps (inv_z)", timed(lambda: r.camera_backward(out12)))
lines.append(f"  camera pass / preprocess_backward stage = {cam_alone[0] / bwd['preprocess_backward'][0]:.2f}")

# ---- (b) a tracking iteration against a dense training iteration's forward + backward, same frame, same dL_dimg
def track():
    r.forward(cam, img, keep_state=True, sync=False)
    r.backward_camera(dL_img, None, None, out12b)


def dense():
    r.forward(cam, img, keep_state=True, sync=False)
    r.backward(dL_img, *grads)


t_track, t_dense = timed(track), timed(dense)
row("(b) forward(keep_state) + lcgs_render_backward_camera", t_track)
row("(b) forward(keep_state) + lcgs_render_backward", t_dense)
lines.append(f"  tracking iteration / dense iteration = {t_track[0] / t_dense[0]:.3f}")
r.forward(cam, img, keep_state=True, sync=True)
row("    lcgs_render_backward_camera alone (image)", timed(lambda: r.backward_camera(dL_img, None, None, out12b)))
row("    lcgs_render_backward alone", timed(lambda: r.backward(dL_img, *grads)))
row("    lcgs_render_backward_camera alone (image + depth + alpha)", timed(lambda: r.backward_camera(dL_img, dL_d, dL_a, out12b)))
row("    lcgs_render_backward_maps alone (image + depth + alpha)", timed(lambda: r.backward_maps(dL_img, dL_d, dL_a, *grads)))
r.backward(dL_img, *grads)
r.camera_backward(out12)
r.backward_camera(dL_img, None, None, out12b)
torch.cuda.synchronize()
lines.append(f"  the two routes' twelve numbers: max |difference| {float((out12 - out12b).abs().max()):.3e} "
             f"(max |value| {float(out12.abs().max()):.3e}; the colour walk's float atomics differ run to run)")

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
