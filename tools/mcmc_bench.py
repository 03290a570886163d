"""Times the 3DGS-MCMC steps on the 6.13 M-splat bicycle stand-in's size -- lcgs_mcmc_relocate with 5 % of the rows dead,
lcgs_mcmc_add of 5 %, lcgs_mcmc_noise -- against the same steps composed in torch (chunked multinomial: torch.multinomial takes
at most 2^24 categories; gather / scatter by index; the correction's double sum folded into one [rows, 51] product), same box,
same run: hipEvent median of 20 each.
    python tools/mcmc_bench.py [--out profiles/mcmc_bench.txt]
Relocation times include the one device-to-host read of the count on both sides (torch's nonzero synchronises for its sizes)."""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import luisacomputegaussiansplatting_amd as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--splats", type=int, default=6_131_954)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

P, dev = args.splats, torch.device("cuda", 0)
NEW = int(1.05 * P) - P
CAP = P + NEW
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
width = {"pos": 3, "scale": 3, "rotq": 4, "sh": 48, "opacity": 1}
MIN_OP, N_MAX, LR_POS, NOISE_LR = 0.005, 51, 1.6e-4, 5e5
gen = torch.Generator(device=dev).manual_seed(1)
u = lambda *s: torch.rand(*s, device=dev, generator=gen)


def rows(n_floats, fill):
    t = torch.zeros((CAP, n_floats) if n_floats > 1 else (CAP,), device=dev)
    t[:P] = fill
    return t


raw = {"pos": rows(3, u(P, 3) * 2 - 1), "scale": rows(3, torch.log(0.004 + 0.02 * u(P, 3))), "rotq": rows(4, u(P, 4) * 2 - 1),
       "sh": rows(48, u(P, 48) - 0.5)}
dead0 = u(P) < 0.05
raw["opacity"] = rows(1, torch.logit(torch.where(dead0, 0.001 + 0.002 * u(P), 0.02 + 0.9 * u(P))))
m = {k: torch.rand_like(t) * 1e-3 for k, t in raw.items()}
v = {k: torch.rand_like(t) * 1e-6 for k, t in raw.items()}
act = {"pos": raw["pos"], "sh": raw["sh"], "scale": torch.exp(raw["scale"]),
       "rotq": raw["rotq"] / raw["rotq"].norm(dim=1, keepdim=True).clamp_min(1e-20), "opacity": torch.sigmoid(raw["opacity"])}
saved = {k: raw[k].clone() for k in ("scale", "opacity")}  # what a relocation rewrites on live rows: restored between repeats
n_dead = int(dead0.sum())
view = lambda d: {k: t[:P] for k, t in d.items()}


def restore():
    for k, t in saved.items():
        raw[k].copy_(t)


def timed(fn, prep=None):
    ms = []
    for i in range(args.reps + 3):
        if prep:
            prep()
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
r = L.Renderer(L.Context(0))
moved = []
hip_relocate = timed(lambda: moved.append(r.mcmc_relocate(view(raw), view(m), view(v), view(act), min_opacity=MIN_OP, seed=7)), restore)
assert set(moved) == {n_dead}, (set(moved), n_dead)
hip_add = timed(lambda: r.mcmc_add(P, NEW, raw, m, v, act, min_opacity=MIN_OP, seed=7), restore)
hip_noise = timed(lambda: r.mcmc_noise(view(raw), view(act), lr_pos=LR_POS, step=1, seed=7))

# ---- the same steps composed in torch (after gsplat's MCMCStrategy; the correction's coefficients folded by the hockey-stick
# identity: sum_{i=k+1..n} C(i-1, k) = C(n, k+1))
COEF = torch.zeros(N_MAX + 1, N_MAX, dtype=torch.float64)
for n in range(1, N_MAX + 1):
    for k in range(n):
        COEF[n, k] = math.comb(n, k + 1) * (-1.0) ** k / math.sqrt(k + 1)
COEF = COEF.to(dev)


def chunked_multinomial(w, n, chunk=1 << 24):
    """n draws with replacement from weights w of any length"""
    if w.shape[0] <= chunk:
        return torch.multinomial(w, n, replacement=True)
    parts = list(torch.split(w, chunk))
    mass = torch.stack([p.sum() for p in parts])
    per = torch.bincount(torch.multinomial(mass, n, replacement=True), minlength=len(parts)).tolist()
    out = [torch.multinomial(p, c, replacement=True) + i * chunk for i, (p, c) in enumerate(zip(parts, per)) if c]
    return torch.cat(out)[torch.randperm(n, device=w.device)]


def corrected(src, count):
    x = raw["opacity"][src].double()
    n = count.clamp(max=N_MAX - 1) + 1
    o, q = torch.sigmoid(x), torch.sigmoid(-x)
    op = 1 - q ** (1.0 / n)
    D = (COEF[n] * torch.cumprod(op[:, None].expand(-1, N_MAX), dim=1)).sum(dim=1)
    oh = op.clamp(MIN_OP, 1 - 2.0 ** -23)
    return torch.log(o / D).float(), (torch.log(oh) - torch.log1p(-oh)).float()


def place(dst, src):
    count = torch.bincount(src, minlength=P)
    log_c, new_op = corrected(src, count[src])
    for k in ("pos", "rotq", "sh"):
        raw[k][dst] = raw[k][src]
    raw["scale"][dst] = raw["scale"][src] + log_c[:, None]
    raw["opacity"][dst] = new_op
    raw["scale"][src] = raw["scale"][dst]  # (duplicates in src write the same values)
    raw["opacity"][src] = new_op
    both = torch.cat([dst, src])
    for k in KEYS:
        m[k][both] = 0
        v[k][both] = 0
    act["scale"][both] = torch.exp(raw["scale"][both])
    act["rotq"][both] = raw["rotq"][both] / raw["rotq"][both].norm(dim=1, keepdim=True)
    act["opacity"][both] = torch.sigmoid(raw["opacity"][both])


def torch_relocate():
    o = torch.sigmoid(raw["opacity"][:P])
    dead = o <= MIN_OP
    dst, live = dead.nonzero(as_tuple=True)[0], (~dead).nonzero(as_tuple=True)[0]
    place(dst, live[chunked_multinomial(o[live], dst.shape[0])])
    return dst.shape[0]


def torch_add():
    o = torch.sigmoid(raw["opacity"][:P])
    live = (o > MIN_OP).nonzero(as_tuple=True)[0]
    place(torch.arange(P, P + NEW, device=dev), live[chunked_multinomial(o[live], NEW)])


def torch_noise():
    q = raw["rotq"][:P] / raw["rotq"][:P].norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
                     2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
                     2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y], 1).reshape(-1, 3, 3)
    M = R * torch.exp(raw["scale"][:P])[:, None, :]
    g = torch.sigmoid(-100.0 * (torch.sigmoid(raw["opacity"][:P]) - 0.005))  # = 1 / (1 + exp(-100 ((1 - o) - 0.995)))
    eps = torch.randn(P, 3, device=dev) * (g * (NOISE_LR * LR_POS))[:, None]
    t = (M * eps[:, :, None]).sum(dim=1)  # M^T eps, elementwise (torch.bmm over 6 M 3 x 3 matrices took 134 ms here)
    raw["pos"][:P] += (M * t[:, None, :]).sum(dim=2)


torch_relocate_ms = timed(torch_relocate, restore)
torch_add_ms = timed(torch_add, restore)
torch_noise_ms = timed(torch_noise)

row = sum(width.values()) * 4
# bytes the library's relocation moves: the weights pass reads opacity and writes weight + flag, the two scans read and write
# a word and a u64, the dead list reads two words per row; per relocated row one source row read, raw / m / v / activated
# scale, rotation, opacity of the destination written; the noise reads 44 bytes and writes 12 per row
reloc_bytes = P * (4 + 8 + 8 + 12 + 8 + 4) + n_dead * (row + 3 * row + 32)
noise_bytes = P * 56
lines = [f"3DGS-MCMC steps, {P} splats, {n_dead} dead ({100.0 * n_dead / P:.1f} %), growth by {NEW} rows; hipEvent median of {args.reps}",
         f"lcgs_mcmc_relocate {hip_relocate:8.3f} ms   torch composition {torch_relocate_ms:8.3f} ms   ({torch_relocate_ms / hip_relocate:.1f} x)"
         f"   ~{reloc_bytes / 1e9:.3f} GB moved, {reloc_bytes / hip_relocate / 1e9:.2f} TB/s",
         f"lcgs_mcmc_add      {hip_add:8.3f} ms   torch composition {torch_add_ms:8.3f} ms   ({torch_add_ms / hip_add:.1f} x)",
         f"lcgs_mcmc_noise    {hip_noise:8.3f} ms   torch composition {torch_noise_ms:8.3f} ms   ({torch_noise_ms / hip_noise:.1f} x)"
         f"   {noise_bytes / 1e9:.3f} GB moved, {noise_bytes / hip_noise / 1e9:.2f} TB/s = {noise_bytes / hip_noise / 1e9 / 8.0 * 100:.0f} % of 8 TB/s",
         "(the torch compositions' own traffic is not counted; both relocations include the read-back of the count)"]
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
