"""Times the point-cloud initialisation: lcgs_knn_mean_dist2 and the whole lcgs_scene_init_from_points, on the positions of the
bicycle stand-in (first 100 K, first 1 M, all 6 131 954) and on one adversarial cloud at 1 M (90 % of the points in a ball of
radius 1e-3, 10 % uniform in a cube of side 100); the same quantity composed in torch on the same GPU in the same run (chunked
torch.cdist + topk) where that finishes in reasonable time.  Median of --reps calls after warm-up, timed with events on the
context's stream; the per-stage split (box, sort, boxes, query, rows) is the context's own HIP-event profile of one more call.
    python tools/init_bench.py --case 100k|1m|bicycle|adversarial [--reps N] [--torch] [--out FILE (appended)]
One case per process, so that a driver can give every case a time limit of its own."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402

CASES = {"100k": 100_000, "1m": 1_000_000, "bicycle": 6_131_954, "adversarial": 1_000_000}
ap = argparse.ArgumentParser()
ap.add_argument("--case", required=True, choices=sorted(CASES))
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--torch", action="store_true", help="also time the torch composition (cdist + topk in row chunks)")
ap.add_argument("--torch-rows", type=int, default=2048, help="query rows per cdist call")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
n = CASES[args.case]


def cloud():
    if args.case == "adversarial":
        rng = np.random.default_rng(7)
        d = rng.normal(size=(n * 9 // 10, 3))
        ball = d / np.linalg.norm(d, axis=1, keepdims=True) * 1e-3 * rng.uniform(0, 1, (d.shape[0], 1)) ** (1 / 3) + 50.0
        pos = np.concatenate([ball, rng.uniform(0, 100, (n - d.shape[0], 3))]).astype(np.float32)
        return pos[rng.permutation(n)]
    return L.synth_scene(1, 2001, n)["pos"]  # conftest.BASELINE_SCENES["bicycle"]: kind 1, seed 2001


def timed(fn, reps, warm=2):
    ms = []
    for i in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def torch_composed(pos):
    """the 3DGS quantity with stock torch: squared distances of a block of rows to every point, the four smallest (the point
    itself is one of them), mean of the other three"""
    out = torch.empty(pos.shape[0], device=dev)
    for a in range(0, pos.shape[0], args.torch_rows):
        d = torch.cdist(pos[a:a + args.torch_rows], pos, compute_mode="donot_use_mm_for_euclid_dist")
        out[a:a + args.torch_rows] = (d.topk(4, dim=1, largest=False).values[:, 1:] ** 2).mean(dim=1)
    return out


pos = torch.from_numpy(cloud()).to(dev)
rgb = torch.rand(n, 3, device=dev)
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events above are on it)
feat = 48
raw = {"pos": torch.empty(n, 3, device=dev), "scale": torch.empty(n, 3, device=dev), "rotq": torch.empty(n, 4, device=dev),
       "sh": torch.empty(n, feat, device=dev), "opacity": torch.empty(n, device=dev)}
act = dict(raw, scale=torch.empty(n, 3, device=dev), rotq=torch.empty(n, 4, device=dev), opacity=torch.empty(n, device=dev))
lines = []
tag = f"{args.case:11s} n = {n:9d}"
med, best = timed(lambda: L.knn_mean_dist2(r.ctx, pos), args.reps)
lines.append(f"{tag}  lcgs_knn_mean_dist2               median {med:10.3f} ms   best {best:10.3f} ms   ({args.reps} calls)")
med, best = timed(lambda: r.init_from_points_into(pos, rgb, raw, act), args.reps)
lines.append(f"{tag}  lcgs_scene_init_from_points (deg 3) median {med:10.3f} ms   best {best:10.3f} ms   ({args.reps} calls)")
r.set_profiling(True)
r.init_from_points_into(pos, rgb, raw, act)
stages = r.stage_times()
r.set_profiling(False)
lines.append(f"{tag}  stages by HIP events (ms): " + ", ".join(f"{k} {v:.3f}" for k, v in stages.items()))
if args.torch:
    med, best = timed(lambda: torch_composed(pos), max(1, min(args.reps, 3)), warm=1)
    lines.append(f"{tag}  torch cdist + topk, {args.torch_rows} rows a call  median {med:10.3f} ms   best {best:10.3f} ms")
    ours, ref = L.knn_mean_dist2(r.ctx, pos), torch_composed(pos)
    torch.cuda.synchronize()
    rel = ((ours - ref).abs() / ref.clamp_min(1e-30)).max().item()
    lines.append(f"{tag}  largest relative difference to the torch composition {rel:.2e}")
text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "a") as f:
        f.write(text + "\n")
