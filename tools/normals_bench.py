"""Times the normal map and its backward on the bicycle stand-in at 1920x1080 (the frame of tools/maps_bench.py and
tools/distortion_bench.py), beside their yardsticks on the same frame, same run:
    lcgs_render_normals                          beside lcgs_render_maps (depth + alpha): the same walk, three accumulators for
                                                 two, a float4 staged per entry, plus the per-row pass in front
    lcgs_render_backward_normals, 5 channels     beside lcgs_render_backward_distortion, 4 channels (with and without an image
                                                 gradient), and the normal channel alone beside depth + alpha alone
    the walk kernel                              the `render_maps_backward` stage of the same call with d_dL_dnormal NULL (seven
                                                 sums per entry) against non-NULL (ten sums, sixteen flush lanes per entry)
    the two per-row passes                       the `splat_normals` and `normals_to_rot` stages
Whole calls are timed with events on the context's stream, stages are the library's own event pairs (lcgs_set_profiling).  The
candidates alternate: every round times each of them once (--reps calls after warm-up); a row is the median of the rounds'
medians with the rounds' spread.
    python tools/normals_bench.py [--out profiles/normals_bench.txt] [--splats N] [--rounds 3]"""
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
depth, alpha = (torch.zeros(H, W, device=dev) for _ in range(2))
normal = torch.zeros(3, H, W, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
dL_img, dL_n = (torch.randn(3, H, W, device=dev, generator=g) for _ in range(2))
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


def stage(name):
    """a measure: the median of one stage of the library's own marks"""
    def measure(fn):
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
    return measure


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
        lines.append(f"{name:76s} median {statistics.median(ms) * 1e3:9.1f} us   rounds {min(ms) * 1e3:9.1f} .. {max(ms) * 1e3:9.1f} us")
    return {name: statistics.median(ms) for name, ms in res.items()}


n = r.forward(cam, img, keep_state=True, sync=True)
stats = r.frame_stats()
lines.append(f"bicycle stand-in, {args.splats} splats, {W}x{H}: num_rendered {n}, {stats['num_visible']} on screen, "
             f"{stats['num_pairs']} pairs; {args.rounds} alternating rounds of {args.reps} calls; "
             f"{torch.cuda.get_device_name(0)}, clocks as the machine sets them (nothing pinned), nothing else on the stream")

# ---- forward
m = rows(alternate([
    ("lcgs_render_maps, depth + alpha, LCGS_DEPTH_Z", lambda: r.render_maps(depth, alpha, mode="z")),
    ("lcgs_render_normals", lambda: r.render_normals(normal)),
]))
lines.append(f"  normals call / maps walk = {m['lcgs_render_normals'] / m['lcgs_render_maps, depth + alpha, LCGS_DEPTH_Z']:.2f}")
fn = lambda: r.render_normals(normal)
m = rows(alternate([("stage `splat_normals` of lcgs_render_normals", fn)], measure=stage("splat_normals")))
m = rows(alternate([("stage `render_normals` of lcgs_render_normals", fn)], measure=stage("render_normals")))

# ---- backward: whole calls
bn = lambda gi, gd, ga, gq, gn: (lambda: r.backward_normals(gi, gd, ga, gq, gn, *grads, mode="z", center=CENTER))
m = rows(alternate([
    ("lcgs_render_backward_distortion, image + depth + alpha + dist", lambda: r.backward_distortion(dL_img, dL_d, dL_a, dL_q, *grads, mode="z", center=CENTER)),
    ("lcgs_render_backward_normals, image + depth + alpha + dist, d_dL_dnormal NULL", bn(dL_img, dL_d, dL_a, dL_q, None)),
    ("lcgs_render_backward_normals, image + depth + alpha + dist + normal", bn(dL_img, dL_d, dL_a, dL_q, dL_n)),
    ("lcgs_render_backward_distortion, depth + alpha + dist (no image gradient)", lambda: r.backward_distortion(None, dL_d, dL_a, dL_q, *grads, mode="z", center=CENTER)),
    ("lcgs_render_backward_normals, depth + alpha + dist + normal", bn(None, dL_d, dL_a, dL_q, dL_n)),
    ("lcgs_render_backward_maps, depth + alpha", lambda: r.backward_maps(None, dL_d, dL_a, *grads)),
    ("lcgs_render_backward_normals, depth + alpha + normal", bn(None, dL_d, dL_a, None, dL_n)),
    ("lcgs_render_backward_normals, normal alone", bn(None, None, None, None, dL_n)),
]))
a, b = m["lcgs_render_backward_distortion, image + depth + alpha + dist"], m["lcgs_render_backward_normals, image + depth + alpha + dist + normal"]
lines.append(f"  whole call, five channels - four = {(b - a) * 1e3:.1f} us ({b / a:.2f} x)")

# ---- backward: the walk kernel itself, seven sums against ten
m = rows(alternate([
    ("stage `render_maps_backward`, depth + alpha, d_dL_dnormal NULL", bn(None, dL_d, dL_a, None, None)),
    ("stage `render_maps_backward`, depth + alpha + normal", bn(None, dL_d, dL_a, None, dL_n)),
    ("stage `render_maps_backward`, depth + alpha + dist, d_dL_dnormal NULL", bn(None, dL_d, dL_a, dL_q, None)),
    ("stage `render_maps_backward`, depth + alpha + dist + normal", bn(None, dL_d, dL_a, dL_q, dL_n)),
], measure=stage("render_maps_backward")))
a, b = m["stage `render_maps_backward`, depth + alpha, d_dL_dnormal NULL"], m["stage `render_maps_backward`, depth + alpha + normal"]
lines.append(f"  kernel, normal channel on two channels = {(b - a) * 1e3:.1f} us ({b / a:.2f} x)")
a, b = m["stage `render_maps_backward`, depth + alpha + dist, d_dL_dnormal NULL"], m["stage `render_maps_backward`, depth + alpha + dist + normal"]
lines.append(f"  kernel, normal channel on three channels = {(b - a) * 1e3:.1f} us ({b / a:.2f} x)")

# ---- the two per-row passes of the backward
fn = bn(None, dL_d, dL_a, None, dL_n)
rows(alternate([("stage `splat_normals` of lcgs_render_backward_normals (writes n, clears dL/dn)", fn)], measure=stage("splat_normals")))
rows(alternate([("stage `normals_to_rot` of lcgs_render_backward_normals", fn)], measure=stage("normals_to_rot")))

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
