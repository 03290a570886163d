"""Times contribution-based pruning on the bicycle stand-in at 1920x1080:
    lcgs_contrib_accumulate and its two stages        beside lcgs_render_maps and the `render_maps_backward` stage, same frame, same run
    the eight C5 views accumulated                    rows kept under min_weight_max = 0.01 and under min_pixels = 1, and lcgs_prune's time
    forward frames/s of the scene before pruning      and of the pruned scene bound in its place, same view, alternated
Stage times are the library's own event pairs (lcgs_set_profiling: calls run in order); whole calls are timed with events on
the context's stream; frames/s is a host clock around --frames enqueued frames that ends in a synchronise.  Medians after warm-up.
    python tools/contrib_bench.py [--out profiles/contrib_bench.txt] [--splats N]"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H, WARM = 1920, 1080, 5
KEYS = ("pos", "scale", "rotq", "sh", "opacity")


def view_pose(k):
    """bench.py's C5 views: the base pose rotated about world-up (0, -1, 0) by k x 45 degrees"""
    a = math.radians(45.0 * k)
    c, s = math.cos(a), math.sin(a)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return (R @ np.array([-3.0, -0.5, 2.3])).tolist(), (R @ np.array([0.0, 0.0, 0.5])).tolist(), [0.0, -1.0, 0.0]


scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
P = args.splats
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
cams = [L.get_lookat_cam(*view_pose(k), width=W, height=H) for k in range(8)]
img = torch.zeros(3, H, W, device=dev)
depth, alpha = torch.zeros(H, W, device=dev), torch.zeros(H, W, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
dL_d, dL_a = torch.randn(H, W, device=dev, generator=g), torch.randn(H, W, device=dev, generator=g)
grads = [torch.zeros_like(d[k]) for k in KEYS]


def new_stats():
    return {"weight_sum": torch.zeros(P, device=dev), "weight_max": torch.zeros(P, device=dev),
            "pixels": torch.zeros(P, dtype=torch.int32, device=dev), "views": torch.zeros(P, dtype=torch.int32, device=dev)}


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
n = r.forward(cams[0], img, keep_state=True, sync=True)
fs = r.frame_stats()
lines.append(f"bicycle stand-in, {P} splats, {W}x{H}, view 0: num_rendered {n}, {fs['num_visible']} on screen, {fs['num_pairs']} pairs")

# ---- the walk beside its two yardsticks on the same kept frame
scratch = new_stats()
r.set_profiling(True)
st = stages(lambda: r.contrib_accumulate(scratch))
bwd = stages(lambda: r.backward_maps(None, dL_d, dL_a, *grads, mode="z"))
r.set_profiling(False)
r.forward(cams[0], img, keep_state=True, sync=True)
row("lcgs_contrib_accumulate stage `contrib_walk` (zero + walk)", st["contrib_walk"])
row("lcgs_contrib_accumulate stage `contrib_fold`", st["contrib_fold"])
whole = timed(lambda: r.contrib_accumulate(scratch))
row("lcgs_contrib_accumulate, all four statistics", whole)
row("lcgs_contrib_accumulate, weight_max alone", timed(lambda: r.contrib_accumulate({"weight_max": scratch["weight_max"]})))
maps = timed(lambda: r.render_maps(depth, alpha, mode="z"))
row("lcgs_render_maps, depth + alpha", maps)
row("lcgs_render_backward_maps stage `render_maps_backward`", bwd["render_maps_backward"])
lines.append(f"  contrib walk / maps walk = {st['contrib_walk'][0] / maps[0]:.2f}, contrib walk / maps backward walk = "
             f"{st['contrib_walk'][0] / bwd['render_maps_backward'][0]:.2f}")

# ---- the eight C5 views accumulated, the rules, the rewrite
stats = new_stats()
for cam in cams:
    r.forward(cam, img, keep_state=True, sync=True)
    r.contrib_accumulate(stats)
r.ctx.synchronize()
keep = torch.zeros(P, dtype=torch.uint8, device=dev)
kept = {}
for name, cfg in (("min_weight_max = 0.01", dict(min_weight_max=0.01)), ("min_pixels = 1", dict(min_pixels=1))):
    r.contrib_keep_mask(stats, keep, **cfg)
    r.ctx.synchronize()
    kept[name] = int(keep.sum())
    lines.append(f"eight C5 views accumulated: {kept[name]} of {P} rows kept under {name} ({100.0 * kept[name] / P:.1f} %)")
lines.append(f"  rows blended in 8 / 1-7 / 0 views: {int((stats['views'] == 8).sum())} / "
             f"{int(((stats['views'] > 0) & (stats['views'] < 8)).sum())} / {int((stats['views'] == 0).sum())}")
# the scene's own (activated) arrays go through the rewrite as `raw`: out_raw holds the kept rows bit for bit
cap = kept["min_weight_max = 0.01"]
zeros = {k: torch.zeros_like(d[k]) for k in KEYS}
outs = [{k: torch.empty((cap,) + tuple(d[k].shape[1:]), device=dev) for k in KEYS} for _ in range(4)]
ms = []
for i in range(args.reps // 3 + 2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_new = r.prune(stats, d, zeros, zeros, *outs, min_weight_max=0.01)
    torch.cuda.synchronize()
    if i >= 2:
        ms.append((time.perf_counter() - t0) * 1e3)
assert n_new == cap
lines.append(f"{'lcgs_prune, ' + str(P) + ' -> ' + str(n_new) + ' rows (raw, m, v, activated; one read-back)':64s} median "
             f"{statistics.median(ms):9.2f} ms   best {min(ms):9.2f} ms   ({len(ms)} calls)")

# ---- forward frames/s before and after, same view, alternated
del zeros, outs[1:], grads
pruned = outs[0]
r2 = L.Renderer(L.Context(0))
r2.bind_scene(*[pruned[k] for k in KEYS])


def fps(rr):
    for _ in range(50):
        rr.forward(cams[0], img, sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.frames):
        rr.forward(cams[0], img, sync=False)
    torch.cuda.synchronize()
    return args.frames / (time.perf_counter() - t0)


full_img = torch.zeros_like(img)
r.forward(cams[0], full_img, sync=True)
r2.forward(cams[0], img, sync=True)
diff = (img - full_img).abs()
runs = {"full": [], "pruned": []}
for _ in range(5):
    runs["full"].append(fps(r))
    runs["pruned"].append(fps(r2))
for name, rows in (("full", P), ("pruned", n_new)):
    v = runs[name]
    lines.append(f"forward frames/s, {name:6s} scene ({rows:8d} rows), view 0: median {statistics.median(v):8.1f}   "
                 f"min {min(v):8.1f}   max {max(v):8.1f}   (5 windows of {args.frames} frames, alternated)")
lines.append(f"  pruned / full = {statistics.median(runs['pruned']) / statistics.median(runs['full']):.3f}; view 0 of the pruned scene against "
             f"the full one: max |diff| {float(diff.max()):.3e}, mean |diff| {float(diff.mean()):.3e} (min_weight_max is lossy by design)")

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
