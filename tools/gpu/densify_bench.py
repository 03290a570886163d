"""Times lcgs_densify on the 6.13 M-splat bicycle stand-in's size (roughly 10 % clone, 10 % split, 5 % pruned) against the same
rewrite composed from torch mask-indexing and cat, same box, same run: hipEvent median of 20 each.
    python tools/gpu/densify_bench.py [--out profiles/densify_bench.txt]
Both include the one device-to-host read of the new count (torch's mask-indexing synchronises for its sizes too)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

P, dev = args.splats, torch.device("cuda", 0)
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
shape = {"pos": (P, 3), "scale": (P, 3), "rotq": (P, 4), "sh": (P, 48), "opacity": (P,)}
CFG = dict(grad_threshold=2e-4, percent_dense=0.01, scene_extent=4.0, min_opacity=0.005, max_screen_size=0)
gen = torch.Generator(device=dev).manual_seed(1)
u = lambda *s: torch.rand(*s, device=dev, generator=gen)
raw = {"pos": u(P, 3) * 2 - 1, "rotq": u(P, 4) * 2 - 1, "sh": u(P, 48) - 0.5}
cat = torch.multinomial(torch.tensor([0.75, 0.10, 0.10, 0.05], device=dev), P, replacement=True, generator=gen)  # keep clone split prune
smax = torch.where(cat == 2, 0.06 + 0.2 * u(P), 0.004 + 0.02 * u(P))
raw["scale"] = torch.log(smax)[:, None] - u(P, 3) * 2
raw["scale"][:, 0] = torch.log(smax)
op = torch.where(cat == 3, 0.001 + 0.002 * u(P), 0.02 + 0.9 * u(P))
raw["opacity"] = torch.logit(op)
denom = torch.randint(1, 50, (P,), device=dev, dtype=torch.int32, generator=gen)
avg = torch.where((cat == 1) | (cat == 2), 4e-4 + 1e-3 * u(P), 1e-4 * u(P))
stats = {"grad_accum": avg * denom, "denom": denom, "max_radii": torch.zeros(P, dtype=torch.int32, device=dev)}
m = {k: torch.rand_like(t) * 1e-3 for k, t in raw.items()}
v = {k: torch.rand_like(t) * 1e-6 for k, t in raw.items()}
noise = torch.randn(P, 2, 3, device=dev, generator=gen)
n_act = torch.bincount(cat, minlength=4).tolist()
N = n_act[0] + 2 * n_act[1] + 2 * n_act[2]
CAP = N


def timed(fn):
    ms = []
    for i in range(args.reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if i >= 3:
            ms.append(a.elapsed_time(b))
        del out
    return float(np.median(ms))


# ---- the library
alloc = lambda: {k: torch.empty((CAP,) + shape[k][1:], device=dev) for k in KEYS}
o_raw, o_m, o_v, o_act = alloc(), alloc(), alloc(), alloc()
o_act["pos"], o_act["sh"] = o_raw["pos"], o_raw["sh"]
o_stats = {"grad_accum": torch.empty(CAP, device=dev), "denom": torch.empty(CAP, dtype=torch.int32, device=dev),
           "max_radii": torch.empty(CAP, dtype=torch.int32, device=dev)}
src_row = torch.empty(CAP, dtype=torch.int32, device=dev)
r = L.Renderer(L.Context(0))
new_n = []
hip_ms = timed(lambda: new_n.append(r.densify(stats, raw, m, v, o_raw, o_m, o_v, o_act, o_stats, noise=noise, src_row=src_row, **CFG)))
assert set(new_n) == {N}, (set(new_n), N)
del o_m, o_v, o_stats


# ---- the same rewrite out of torch mask-indexing and cat (INRIA-style: new rows appended)
def rot(q):
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
                        2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
                        2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y], 1).reshape(-1, 3, 3)


def torch_densify():
    a = torch.where(stats["denom"] > 0, stats["grad_accum"] / stats["denom"], 0.0)
    sm = torch.exp(raw["scale"]).max(dim=1).values
    prune = torch.sigmoid(raw["opacity"]) < CFG["min_opacity"]
    hot = (a >= CFG["grad_threshold"]) & ~prune
    big = sm > CFG["percent_dense"] * CFG["scene_extent"]
    stay, clone, split = ~prune & ~(hot & big), hot & ~big, hot & big
    R, s = rot(raw["rotq"][split]), torch.exp(raw["scale"][split])
    kids = [raw["pos"][split] + torch.bmm(R, (s * noise[split, k]).unsqueeze(-1)).squeeze(-1) for k in range(2)]
    out_raw, out_m, out_v = {}, {}, {}
    for k in KEYS:
        x = raw[k]
        c = kids if k == "pos" else ([x[split] - 0.47000363] * 2 if k == "scale" else [x[split]] * 2)
        out_raw[k] = torch.cat([x[stay], x[clone], c[0], c[1]])
        fresh = out_raw[k].shape[0] - int(stay.sum())
        out_m[k] = torch.cat([m[k][stay], torch.zeros((fresh,) + x.shape[1:], device=dev)])
        out_v[k] = torch.cat([v[k][stay], torch.zeros((fresh,) + x.shape[1:], device=dev)])
    act = {"scale": torch.exp(out_raw["scale"]), "rotq": out_raw["rotq"] / out_raw["rotq"].norm(dim=1, keepdim=True),
           "opacity": torch.sigmoid(out_raw["opacity"])}
    n = out_raw["opacity"].shape[0]
    fresh_stats = (torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    return out_raw, out_m, out_v, act, fresh_stats


assert torch_densify()[0]["opacity"].shape[0] == N
torch_ms = timed(torch_densify)

# bytes the library's path moves: classify reads scale + opacity + the statistics and writes count + action, the scan reads and
# writes a word; the scatter reads raw of every surviving source row and m / v of the kept ones, writes raw / m / v and the
# activated scale / rotation / opacity of every output row, the zero statistics and the source row
live, kept = P - n_act[3], n_act[0] + n_act[1]
moved = P * (12 + 4 + 12 + 4 + 1 + 8) + live * 236 + kept * 2 * 236 + N * (3 * 236 + 32 + 12 + 4)
lines = [f"lcgs_densify vs torch mask-indexing + cat, {P} splats (keep / clone / split / prune: {n_act}), {P} -> {N} rows, "
         f"hipEvent median of {args.reps}",
         f"lcgs_densify      {hip_ms:8.3f} ms   {moved / 1e9:.3f} GB moved   {moved / hip_ms / 1e9:.2f} TB/s = "
         f"{moved / hip_ms / 1e9 / 8.0 * 100:.0f} % of 8 TB/s",
         f"torch composition {torch_ms:8.3f} ms   ({torch_ms / hip_ms:.2f} x the library's time; its own traffic is not counted)"]
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
