"""Times the depth / alpha maps on the bicycle stand-in at 1920x1080, beside their yardsticks on the same frame, same run:
    lcgs_render_maps              beside the keep-state frame's `render` stage (the colour renderer over the same lists)
    the maps-backward kernel      beside `render_backward` (the colour walk), both from one lcgs_render_backward_maps call
Stage times are the library's own event pairs (lcgs_set_profiling: frames run in order); whole calls are timed with events on
the context's stream.  Median of --reps after warm-up.
    python tools/maps_bench.py [--out profiles/render_maps_bench.txt] [--splats N]"""
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
depth, alpha = torch.zeros(H, W, device=dev), torch.zeros(H, W, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
dL_img = torch.randn(3, H, W, device=dev, generator=g)
dL_d, dL_a = torch.randn(H, W, device=dev, generator=g), torch.randn(H, W, device=dev, generator=g)
grads = [torch.zeros_like(d[k]) for k in KEYS]


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
row = lambda name, t: lines.append(f"{name:64s} median {t[0] * 1e3:9.1f} us   best {t[1] * 1e3:9.1f} us   ({args.reps} calls)")
n = r.forward(cam, img, keep_state=True, sync=True)
stats = r.frame_stats()
lines.append(f"bicycle stand-in, {args.splats} splats, {W}x{H}: num_rendered {n}, {stats['num_visible']} on screen, "
             f"{stats['num_pairs']} pairs")

# ---- forward: the maps walk beside the frame's own renderer
r.set_profiling(True)
fwd = stages(lambda: r.forward(cam, img, keep_state=True, sync=True))
r.set_profiling(False)
r.forward(cam, img, keep_state=True, sync=True)
row("render stage of the keep-state frame (k_render_forward_b)", fwd["render"])
maps_both = timed(lambda: r.render_maps(depth, alpha, mode="z"))
row("lcgs_render_maps, depth + alpha, LCGS_DEPTH_Z", maps_both)
row("lcgs_render_maps, depth + alpha, LCGS_DEPTH_INV_Z", timed(lambda: r.render_maps(depth, alpha, mode="inv_z")))
row("lcgs_render_maps, alpha alone", timed(lambda: r.render_maps(None, alpha, mode="z")))
lines.append(f"  maps walk / render stage = {maps_both[0] / fwd['render'][0]:.2f}")

# ---- backward: the two-channel walk beside the three-channel one, stage by stage of one call
r.set_profiling(True)
bwd = stages(lambda: r.backward_maps(dL_img, dL_d, dL_a, *grads, mode="z"))
r.set_profiling(False)
for k in ("render_backward", "render_maps_backward", "preprocess_backward"):
    row(f"lcgs_render_backward_maps stage `{k}`", bwd[k])
lines.append(f"  maps backward kernel / render_backward = {bwd['render_maps_backward'][0] / bwd['render_backward'][0]:.2f}")
# whole calls (pipelined: the dense rows' zero-fill rides in the colour walk; without it the memsets run beside the maps walk)
row("lcgs_render_backward (colour alone)", timed(lambda: r.backward(dL_img, *grads)))
row("lcgs_render_backward_maps, image + depth + alpha", timed(lambda: r.backward_maps(dL_img, dL_d, dL_a, *grads)))
row("lcgs_render_backward_maps, depth + alpha (no image gradient)", timed(lambda: r.backward_maps(None, dL_d, dL_a, *grads)))
row("lcgs_render_backward_maps, alpha alone", timed(lambda: r.backward_maps(None, None, dL_a, *grads)))

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
