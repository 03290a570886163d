"""Times the depth-distortion map and its backward on the bicycle stand-in at 1920x1080 (the frame of tools/maps_bench.py), beside
their yardsticks on the same frame, same run:
    lcgs_render_distortion                      beside lcgs_render_maps (depth + alpha): the same walk, three accumulators for two
    lcgs_render_backward_distortion, 4 channels beside lcgs_render_backward_maps with depth + alpha (with and without an image gradient)
    the pre-walk's share                        the same call and its `render_maps_backward` stage with d_dL_ddist NULL (the
                                                two-channel kernel) against non-NULL (pre-walk + three-channel walk)
Whole calls are timed with events on the context's stream, stages are the library's own event pairs (lcgs_set_profiling).  The
candidates alternate: every round times each of them once (--reps calls after warm-up); a row is the median of the rounds'
medians with the rounds' spread.
    python tools/distortion_bench.py [--out profiles/distortion_bench.txt] [--splats N] [--rounds 3]"""
import argparse
import os
import statistics
import sys

import torch

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
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
CENTER = 3.5  # about the distance from the camera to the scene's centre

scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
cam = L.get_lookat_cam([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0], width=W, height=H)  # bench.py's view 0
img = torch.zeros(3, H, W, device=dev)
depth, alpha, dist = (torch.zeros(H, W, device=dev) for _ in range(3))
g = torch.Generator(device=dev).manual_seed(1)
dL_img = torch.randn(3, H, W, device=dev, generator=g)
dL_d, dL_a, dL_q = (torch.randn(H, W, device=dev, generator=g) for _ in range(3))
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
    return statistics.median(ms)


def stage(fn, name):
    """median of one stage of the library's own marks"""
    r.set_profiling(True)
    seen = []
    for i in range(args.reps + WARM):
        fn()
        r.ctx.synchronize()
        if i >= WARM:
            seen.append(r.stage_times()[name])
    r.set_profiling(False)
    fn()
    r.ctx.synchronize()
    return statistics.median(seen)


def alternate(candidates, measure=timed):
    """name -> the rounds' medians, every round timing each candidate once, in order"""
    out = {name: [] for name, _ in candidates}
    for _ in range(args.rounds):
        for name, fn in candidates:
            out[name].append(measure(fn))
    return out


lines = []


def rows(res):
    for name, ms in res.items():
        lines.append(f"{name:72s} median {statistics.median(ms) * 1e3:9.1f} us   rounds {min(ms) * 1e3:9.1f} .. {max(ms) * 1e3:9.1f} us")
    return {name: statistics.median(ms) for name, ms in res.items()}


n = r.forward(cam, img, keep_state=True, sync=True)
stats = r.frame_stats()
lines.append(f"bicycle stand-in, {args.splats} splats, {W}x{H}: num_rendered {n}, {stats['num_visible']} on screen, "
             f"{stats['num_pairs']} pairs; {args.rounds} alternating rounds of {args.reps} calls")

# ---- forward
m = rows(alternate([
    ("lcgs_render_maps, depth + alpha, LCGS_DEPTH_Z", lambda: r.render_maps(depth, alpha, mode="z")),
    ("lcgs_render_distortion, LCGS_DEPTH_Z, center 0", lambda: r.render_distortion(dist, mode="z", center=0.0)),
    (f"lcgs_render_distortion, LCGS_DEPTH_Z, center {CENTER}", lambda: r.render_distortion(dist, mode="z", center=CENTER)),
    (f"lcgs_render_distortion, LCGS_DEPTH_INV_Z, center {1 / CENTER:.3f}", lambda: r.render_distortion(dist, mode="inv_z", center=1 / CENTER)),
]))
lines.append(f"  distortion walk / maps walk = {m['lcgs_render_distortion, LCGS_DEPTH_Z, center 0'] / m['lcgs_render_maps, depth + alpha, LCGS_DEPTH_Z']:.2f}")

# ---- backward: whole calls
bd = lambda gi, gq: (lambda: r.backward_distortion(gi, dL_d, dL_a, gq, *grads, mode="z", center=CENTER))
m = rows(alternate([
    ("lcgs_render_backward_maps, image + depth + alpha", lambda: r.backward_maps(dL_img, dL_d, dL_a, *grads)),
    ("lcgs_render_backward_distortion, image + depth + alpha + dist", bd(dL_img, dL_q)),
    ("lcgs_render_backward_maps, depth + alpha (no image gradient)", lambda: r.backward_maps(None, dL_d, dL_a, *grads)),
    ("lcgs_render_backward_distortion, depth + alpha, d_dL_ddist NULL", bd(None, None)),
    ("lcgs_render_backward_distortion, depth + alpha + dist", bd(None, dL_q)),
    ("lcgs_render_backward_distortion, dist alone", lambda: r.backward_distortion(None, None, None, dL_q, *grads, center=CENTER)),
]))
a, b = m["lcgs_render_backward_distortion, depth + alpha, d_dL_ddist NULL"], m["lcgs_render_backward_distortion, depth + alpha + dist"]
lines.append(f"  whole call, d_dL_ddist non-NULL - NULL = {(b - a) * 1e3:.1f} us ({b / a:.2f} x)")

# ---- backward: the walk kernel itself, two channels against pre-walk + three channels
st = lambda fn: stage(fn, "render_maps_backward")
m = rows(alternate([
    ("stage `render_maps_backward`, depth + alpha, d_dL_ddist NULL", bd(None, None)),
    ("stage `render_maps_backward`, depth + alpha + dist", bd(None, dL_q)),
], measure=st))
a, b = m["stage `render_maps_backward`, depth + alpha, d_dL_ddist NULL"], m["stage `render_maps_backward`, depth + alpha + dist"]
fwd = statistics.median(alternate([("x", lambda: r.render_distortion(dist, mode="z", center=CENTER))])["x"])
lines.append(f"  kernel, pre-walk + third channel = {(b - a) * 1e3:.1f} us ({b / a:.2f} x; lcgs_render_distortion, the pre-walk's own walk "
             f"with a store, {fwd * 1e3:.1f} us)")

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
