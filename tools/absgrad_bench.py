"""Times lcgs_absgrad_accumulate on the bicycle stand-in at 1920x1080 (the frame of tools/maps_bench.py and
tools/normals_bench.py), beside its two yardsticks on the same frame, same run:
    lcgs_absgrad_accumulate, whole call          colour only, and colour + depth + alpha; statistics + d_absgrad
    its stage `absgrad_walk` (clear + walk)      beside the `render_backward` stage of lcgs_render_backward and the
                                                 `render_maps_backward` stage of the two-channel lcgs_render_backward_maps: the
                                                 same per-entry work as the latter, two sums per (tile, entry) for seven, plus the
                                                 colour fetch
    its stage `absgrad_rows`                     the per-row pass (the reference radius, as lcgs_densify_accumulate's)
Whole calls are timed with events on the context's stream, stages are the library's own event pairs (lcgs_set_profiling).  The
candidates alternate: every round times each of them once (--reps calls after warm-up); a row is the median of the rounds'
medians with the rounds' spread.
    python tools/absgrad_bench.py [--out profiles/absgrad_bench.txt] [--splats N] [--rounds 3]"""
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

scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
P = d["opacity"].shape[0]
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
cam = L.get_lookat_cam([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0], width=W, height=H)  # bench.py's view 0
img = torch.zeros(3, H, W, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
dL_img = torch.randn(3, H, W, device=dev, generator=g)
dL_d, dL_a = (torch.randn(H, W, device=dev, generator=g) for _ in range(2))
grads = [torch.zeros_like(d[k]) for k in KEYS]
stats = {"grad_accum": torch.zeros(P, device=dev), "denom": torch.zeros(P, dtype=torch.int32, device=dev),
         "max_radii": torch.zeros(P, dtype=torch.int32, device=dev)}
absgrad = torch.zeros(P, 2, device=dev)


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


def alternate(candidates):
    """name -> the rounds' medians, every round timing each (name, fn, measure) once, in order"""
    out = {name: [] for name, _, _ in candidates}
    for _ in range(args.rounds):
        for name, fn, measure in candidates:
            out[name].append(measure(fn))
    return out


lines = []


def rows(res):
    for name, ms in res.items():
        lines.append(f"{name:76s} median {statistics.median(ms) * 1e3:9.1f} us   rounds {min(ms) * 1e3:9.1f} .. {max(ms) * 1e3:9.1f} us")
    return {name: (statistics.median(ms), max(ms) - min(ms)) for name, ms in res.items()}


n = r.forward(cam, img, keep_state=True, sync=True)
fs = r.frame_stats()
lines.append(f"bicycle stand-in, {args.splats} splats, {W}x{H}: num_rendered {n}, {fs['num_visible']} on screen, "
             f"{fs['num_pairs']} pairs; {args.rounds} alternating rounds of {args.reps} calls; "
             f"{torch.cuda.get_device_name(0)}, clocks as the machine sets them (nothing pinned), nothing else on the stream")

colour = lambda: r.absgrad_accumulate(dL_img, stats=stats, absgrad=absgrad)
three = lambda: r.absgrad_accumulate(dL_img, dL_d, dL_a, stats=stats, absgrad=absgrad)
maps_only = lambda: r.absgrad_accumulate(None, dL_d, dL_a, stats=stats, absgrad=absgrad)
backward = lambda: r.backward(dL_img, *grads)
backward_maps = lambda: r.backward_maps(None, dL_d, dL_a, *grads)

# ---- whole calls
rows(alternate([
    ("lcgs_render_backward (image)", backward, timed),
    ("lcgs_render_backward_maps, depth + alpha (no image gradient)", backward_maps, timed),
    ("lcgs_absgrad_accumulate, colour only", colour, timed),
    ("lcgs_absgrad_accumulate, colour + depth + alpha", three, timed),
    ("lcgs_absgrad_accumulate, depth + alpha (no colour staged)", maps_only, timed),
]))

# ---- the walk beside its two yardsticks, the kernels alone
m = rows(alternate([
    ("stage `render_backward` of lcgs_render_backward", backward, stage("render_backward")),
    ("stage `render_maps_backward` of lcgs_render_backward_maps, depth + alpha", backward_maps, stage("render_maps_backward")),
    ("stage `absgrad_walk` (clear + walk), colour only", colour, stage("absgrad_walk")),
    ("stage `absgrad_walk` (clear + walk), colour + depth + alpha", three, stage("absgrad_walk")),
    ("stage `absgrad_walk` (clear + walk), depth + alpha", maps_only, stage("absgrad_walk")),
]))
y, spread = m["stage `render_maps_backward` of lcgs_render_backward_maps, depth + alpha"]
for name in ("colour only", "colour + depth + alpha", "depth + alpha"):
    a, sa = m[f"stage `absgrad_walk` (clear + walk), {name}"]
    lines.append(f"  absgrad walk, {name} / two-channel maps-backward kernel = {a / y:.2f} ({(a - y) * 1e3:+.1f} us; the rounds' spreads "
                 f"{sa * 1e3:.1f} and {spread * 1e3:.1f} us)")
a, _ = m["stage `absgrad_walk` (clear + walk), colour only"]
lines.append(f"  absgrad walk, colour only / render-backward kernel = {a / m['stage `render_backward` of lcgs_render_backward'][0]:.2f}")

# ---- the per-row pass
rows(alternate([("stage `absgrad_rows`, statistics + d_absgrad", three, stage("absgrad_rows")),
                ("stage `absgrad_rows`, d_absgrad alone", lambda: r.absgrad_accumulate(dL_img, absgrad=absgrad), stage("absgrad_rows"))]))

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
