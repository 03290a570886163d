"""Times the photometric loss at 1920x1080 and 800x800: lcgs_photometric_loss_backward, lcgs_l2_loss_backward and the same
loss composed in torch float32 on the GPU (five conv2d calls + autograd).  Same box, same run: median of --reps calls after
warm-up, timed with events on the context's stream.
    python tools/loss_bench.py [--out profiles/photometric_loss_bench.txt]
    python tools/loss_bench.py --kernels      per-pass kernel times: runs itself once under rocprofv3 --kernel-trace --stats
                                              and appends the rows of the three loss kernels"""
import argparse
import csv
import glob
import math
import os
import statistics
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--out", default=None)
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--library-only", action="store_true", help="(the run under the profiler) the library's loss alone")
args = ap.parse_args()
assert args.reps >= 20
dev = torch.device("cuda", 0)
LAMBDA = 0.2


def torch_composed(x, y, kernel):
    x = x.detach().requires_grad_(True)
    conv = lambda t: F.conv2d(t[None], kernel, padding=5, groups=3)[0]
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
    loss = (1 - LAMBDA) * (x - y).abs().mean() + LAMBDA * (1 - ssim.mean())
    loss.backward()
    return loss, x.grad


def timed(fn):
    ms = []
    for i in range(args.reps + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= 5:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


lines = []
r = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events above are on it)
w = torch.tensor([math.exp(-(k - 5) ** 2 / 4.5) for k in range(11)], dtype=torch.float64)
w = w / w.sum()
kernel = torch.outer(w, w).float().expand(3, 1, 11, 11).contiguous().to(dev)
for W, H in ((1920, 1080), (800, 800)):
    g = torch.Generator(device=dev).manual_seed(W)
    x, y = torch.rand(3, H, W, device=dev, generator=g), torch.rand(3, H, W, device=dev, generator=g)
    dL, loss = torch.empty_like(x), torch.zeros(1, device=dev)
    rows = [("lcgs_photometric_loss_backward", lambda: r.photometric_loss_backward(x, y, dL, loss, LAMBDA)),
            ("lcgs_photometric_loss_backward, evaluation only", lambda: r.photometric_loss_backward(x, y, None, loss, LAMBDA))]
    if not args.library_only:
        rows += [("lcgs_l2_loss_backward", lambda: r.l2_loss_backward(x, y, dL, loss)),
                 ("torch float32: conv2d x 5 + autograd", lambda: torch_composed(x, y, kernel))]
    for name, fn in rows:
        med, best = timed(fn)
        lines.append(f"{W}x{H}  {name:50s} median {med * 1e3:9.1f} us   best {best * 1e3:9.1f} us   ({args.reps} calls)")
    if not args.library_only:
        r.photometric_loss_backward(x, y, dL, loss, LAMBDA)
        ref_loss, ref_grad = torch_composed(x, y, kernel)
        torch.cuda.synchronize()
        lines.append(f"{W}x{H}  loss {loss.item():.7f} (torch float32 {ref_loss.item():.7f}), largest gradient difference "
                     f"{(dL - ref_grad).abs().max().item():.2e} of {ref_grad.abs().max().item():.2e}")

if args.kernels:  # one run of the library's calls under the profiler, in a fresh child process
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                        os.path.abspath(__file__), "--library-only", "--reps", str(args.reps)], check=True, timeout=600,
                       stdout=subprocess.DEVNULL)
        lines.append("per-pass kernel times of that sequence at both sizes (rocprofv3 --kernel-trace --stats):")
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "photometric" in row.get("Name", ""):
                    lines.append(f"  {row['Name'][:70]:70s} calls {row.get('Calls')}  avg {float(row.get('AverageNs', 0)) / 1e3:8.1f} us"
                                 f"  min {float(row.get('MinNs', 0)) / 1e3:8.1f} us  max {float(row.get('MaxNs', 0)) / 1e3:8.1f} us")

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
