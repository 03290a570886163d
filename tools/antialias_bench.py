"""Times the antialiased raster mode (lcgs_set_raster_mode) beside the classic one on the bicycle stand-in at 1920x1080, same
run, same context, the two modes alternating:
    the forward frame                      (lcgs_render_forward, enqueue only)
    the keep-state forward + dense backward
    num_pairs                              (the compensated opacity prunes the rects harder)
and one quality line: the stand-in at 480x270 in both modes against the classic 1920x1080 frame box-averaged 4x4 (PSNR).
Whole calls are timed with events on the context's stream.  Median of --reps after warm-up.  Reports; asserts nothing.
    python tools/antialias_bench.py [--out profiles/antialias_bench.txt] [--splats N]"""
import argparse
import math
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
MODES = ("classic", "antialiased")
POSE = ([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0])  # bench.py's view 0

scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
r.bind_scene(*[d[k] for k in KEYS])
cam = L.get_lookat_cam(*POSE, width=W, height=H)
img = torch.zeros(3, H, W, device=dev)
dL_img = torch.randn(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
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


def step():
    r.forward(cam, img, keep_state=True, sync=False)
    r.backward(dL_img, *grads)


lines, frames, res = [], {}, {m: {} for m in MODES}
for rnd in range(2):  # (the modes alternate; the second round's figures are the ones reported)
    for mode in MODES:
        r.set_raster_mode(mode)
        n = r.forward(cam, img, keep_state=True, sync=True)
        st = r.frame_stats()
        res[mode].update(num_rendered=n, num_visible=st["num_visible"], num_pairs=st["num_pairs"])
        frames[mode] = img.clone()
        res[mode]["forward"] = timed(lambda: r.forward(cam, img, sync=False))
        res[mode]["step"] = timed(step)
lines.append(f"bicycle stand-in, {args.splats} splats, {W}x{H}, median / best of {args.reps} calls, modes alternating")
for mode in MODES:
    q = res[mode]
    lines.append(f"{mode:12s} num_rendered {q['num_rendered']}  on screen {q['num_visible']}  num_pairs {q['num_pairs']}")
    lines.append(f"{mode:12s} forward frame                       median {q['forward'][0] * 1e3:9.1f} us   best {q['forward'][1] * 1e3:9.1f} us")
    lines.append(f"{mode:12s} keep-state forward + dense backward median {q['step'][0] * 1e3:9.1f} us   best {q['step'][1] * 1e3:9.1f} us")
c, a = res["classic"], res["antialiased"]
lines.append(f"antialiased / classic: forward {a['forward'][0] / c['forward'][0]:.3f}, forward + backward "
             f"{a['step'][0] / c['step'][0]:.3f}, num_pairs {a['num_pairs'] / max(c['num_pairs'], 1):.3f}")

# ---- quality: a quarter-resolution frame against the box-averaged full-resolution classic frame
want = torch.nn.functional.avg_pool2d(frames["classic"][None], 4)[0]
small = L.get_lookat_cam(*POSE, width=W // 4, height=H // 4)
low = torch.zeros(3, H // 4, W // 4, device=dev)
for mode in MODES:
    r.set_raster_mode(mode)
    r.forward(small, low, sync=True)
    mse = float(((low - want) ** 2).mean())
    lines.append(f"{mode:12s} {W // 4}x{H // 4} frame vs the classic {W}x{H} frame box-averaged 4x4: PSNR "
                 f"{10 * math.log10(1.0 / max(mse, 1e-30)):.2f} dB")
r.set_raster_mode("classic")

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
