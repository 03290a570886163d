"""Times the caller-supplied feature channels and their backward on the bicycle stand-in at 1920x1080 (the frame of
tools/maps_bench.py and tools/normals_bench.py) at K = 3, 16, 32, 64, beside their yardsticks on the same frame, same run:
    lcgs_render_features                         beside lcgs_render_normals' walk (its `render_normals` stage): at K = 3 the same
                                                 work -- three accumulated channels of a vector staged per entry
    lcgs_render_backward_features, full          (geometry rows and dL/dfeatures), features-only (grads NULL) and geometry-only
                                                 (d_dL_dfeatures NULL), beside the maps-backward kernel (`render_maps_backward`
                                                 stage) without and with the normal channel
    the clear of d_dL_dfeatures                  the `zero_features` stage (P x K floats)
    the chunk width CH                           4 / 8 / 16 forced through LCGS_FEATURES_CH (one context each: the hook is read
                                                 when a context is created) at K = 3 and K = 16, forward and full backward
Whole calls are timed with events on the context's stream, stages are the library's own event pairs (lcgs_set_profiling).  The
candidates alternate: every round times each of them once (--reps calls after warm-up); a row is the median of the rounds'
medians with the rounds' spread.
    python tools/features_bench.py [--out profiles/features_bench.txt] [--splats N] [--rounds 3]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H, WARM = 1920, 1080, 3
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
KS = (3, 16, 32, 64)

scene = L.synth_scene(1, 2001, args.splats)  # the mip360_bicycle stand-in of bench.py
d = {k: torch.from_numpy(scene[k]).to(dev) for k in KEYS}
P = d["pos"].shape[0]
cam = L.get_lookat_cam([-3.0, -0.5, 2.3], [0.0, 0.0, 0.5], [0.0, -1.0, 0.0], width=W, height=H)  # bench.py's view 0
img = torch.zeros(3, H, W, device=dev)


def renderer(ch=None):
    """a context with the frame kept; ch: the forced chunk width (None: the library's choice)"""
    if ch is None:
        os.environ.pop("LCGS_FEATURES_CH", None)
    else:
        os.environ["LCGS_FEATURES_CH"] = str(ch)
    rr = L.Renderer(L.Context(0))  # (the context takes torch's current stream: the events below are on it)
    os.environ.pop("LCGS_FEATURES_CH", None)
    rr.bind_scene(*[d[k] for k in KEYS])
    rr.forward(cam, img, keep_state=True, sync=True)
    return rr


r = renderer()
normal = torch.zeros(3, H, W, device=dev)
g = torch.Generator(device=dev).manual_seed(1)
dL_n = torch.randn(3, H, W, device=dev, generator=g)
dL_d, dL_a = (torch.randn(H, W, device=dev, generator=g) for _ in range(2))
grads = [torch.zeros_like(d[k]) for k in KEYS]


def timed(fn, rr=None):
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


def stage(name, rr=None):
    """a measure: the median of one stage of the library's own marks"""
    rr = rr or r

    def measure(fn):
        rr.set_profiling(True)
        seen = []
        for i in range(args.reps + WARM):
            fn()
            rr.ctx.synchronize()
            if i >= WARM:
                seen.append(rr.stage_times()[name])
        rr.set_profiling(False)
        fn()
        rr.ctx.synchronize()
        return statistics.median(seen)
    return measure


def alternate(candidates):
    """name -> the rounds' medians, every round timing each candidate once, in order; a candidate: (name, fn, measure)"""
    out = {name: [] for name, _, _ in candidates}
    for _ in range(args.rounds):
        for name, fn, measure in candidates:
            out[name].append(measure(fn))
    return out


lines = []


def rows(res):
    for name, ms in res.items():
        lines.append(f"{name:84s} median {statistics.median(ms) * 1e3:9.1f} us   rounds {min(ms) * 1e3:9.1f} .. {max(ms) * 1e3:9.1f} us")
    return {name: statistics.median(ms) for name, ms in res.items()}


stats = r.frame_stats()
lines.append(f"bicycle stand-in, {args.splats} splats, {W}x{H}: {stats['num_rendered']} rendered, {stats['num_visible']} on screen, "
             f"{stats['num_pairs']} pairs; {args.rounds} alternating rounds of {args.reps} calls; "
             f"{torch.cuda.get_device_name(0)}, clocks as the machine sets them (nothing pinned), nothing else on the stream")
lines.append("chunk width CH: the library takes 4 for K <= 4, 8 for K <= 8, 16 beyond; `CH = n`: forced (LCGS_FEATURES_CH)")

yard_fwd = ("yardstick: stage `render_normals` of lcgs_render_normals", lambda: r.render_normals(normal), stage("render_normals"))
bn = lambda gn: (lambda: r.backward_normals(None, dL_d, dL_a, None, gn, *grads))
yard_bwd = [("yardstick: stage `render_maps_backward`, depth + alpha", bn(None), stage("render_maps_backward")),
            ("yardstick: stage `render_maps_backward`, depth + alpha + normal", bn(dL_n), stage("render_maps_backward"))]

for K in KS:
    feats = torch.randn(P, K, device=dev, generator=g)
    fmap = torch.zeros(K, H, W, device=dev)
    dL_f = torch.randn(K, H, W, device=dev, generator=g)
    gfeat = torch.zeros(P, K, device=dev)
    none5 = (None,) * 5
    chunks = -(-K // (4 if K <= 4 else 8 if K <= 8 else 16))
    lines.append(f"---- K = {K} ({chunks} chunk{'s' if chunks > 1 else ''})")
    fwd = lambda rr: (lambda: rr.render_features(feats, fmap))
    full = lambda rr: (lambda: rr.backward_features(*none5, feats, dL_f, gfeat, *grads))
    m = rows(alternate([
        yard_fwd,
        (f"K = {K}: lcgs_render_features, whole call", fwd(r), timed),
        (f"K = {K}: stage `render_features`", fwd(r), stage("render_features")),
    ]))
    a, b = m[yard_fwd[0]], m[f"K = {K}: stage `render_features`"]
    lines.append(f"  forward walk / normals walk = {b / a:.2f}; per chunk {b / chunks * 1e3:.1f} us")
    m = rows(alternate(yard_bwd + [
        (f"K = {K}: lcgs_render_backward_features, full, whole call", full(r), timed),
        (f"K = {K}: stage `render_features_backward`, full (geometry + dL/dfeatures)", full(r), stage("render_features_backward")),
        (f"K = {K}: stage `zero_features` (clear of P x K floats)", full(r), stage("zero_features")),
        (f"K = {K}: lcgs_render_backward_features, features only (grads NULL), whole call",
         lambda: r.backward_features(*none5, feats, dL_f, gfeat), timed),
        (f"K = {K}: stage `render_features_backward`, features only",
         lambda: r.backward_features(*none5, feats, dL_f, gfeat), stage("render_features_backward")),
        (f"K = {K}: features only, accumulate (no clear), whole call",
         lambda: r.backward_features(*none5, feats, dL_f, gfeat, accumulate=True), timed),
        (f"K = {K}: lcgs_render_backward_features, geometry only (d_dL_dfeatures NULL), whole call",
         lambda: r.backward_features(*none5, feats, dL_f, None, *grads), timed),
        (f"K = {K}: stage `render_features_backward`, geometry only",
         lambda: r.backward_features(*none5, feats, dL_f, None, *grads), stage("render_features_backward")),
    ]))
    b = m[f"K = {K}: stage `render_features_backward`, full (geometry + dL/dfeatures)"]
    lines.append(f"  full backward walk / maps-backward kernel with the normal channel = {b / m[yard_bwd[1][0]]:.2f}; "
                 f"per chunk {b / chunks * 1e3:.1f} us")
    if K in (3, 16):  # the chunk width: every candidate beside the others, same run
        rs = {ch: renderer(ch) for ch in (4, 8, 16)}
        cand = []
        for ch, rr in rs.items():
            cand.append((f"K = {K}, CH = {ch}: stage `render_features`", fwd(rr), stage("render_features", rr)))
            cand.append((f"K = {K}, CH = {ch}: stage `render_features_backward`, full", full(rr), stage("render_features_backward", rr)))
        rows(alternate(cand))
        del rs
    del feats, fmap, dL_f, gfeat

text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
