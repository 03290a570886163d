"""The yardstick of lcgs_adam_step: the contract in csrc/kernels/train.hip's header comment restated in torch (runs on the CPU,
and on the device for the two grid-stride cases).  Imports nothing from the package.

    pos, sh      raw == activated                 g_raw = g
    scale        s = exp(raw)                     g_raw = g s
    opacity      o = sigmoid(raw)                 g_raw = g o (1 - o)
    rotq         q = raw / |raw|                  g_raw = (g - q (q . g)) / |raw|
    m' = b1 m + (1 - b1) g_raw;  v' = b2 v + (1 - b2) g_raw^2;  raw' = raw - lr c1 m' / (sqrt(v') c2 + eps)
    c1 = 1 / (1 - b1^t), c2 = 1 / sqrt(1 - b2^t);  s, o, q are the STORED activated arrays, not recomputed from raw

Packs are dicts with the keys pos [P,3], scale [P,3], rotq [P,4], sh [P,F], opacity [P].

  step64(...)   one step in float64 from float32 inputs taken exactly; the scalars are the binary32 numbers that cross the ABI,
                c1 and c2 float64 functions of the binary32 betas.  -> {"raw", "m", "v", "act"} of packs
  step32(...)   the same with every operation a float32 tensor operation in the order launch.hpp::adam_update and the
                kernels write it.  Validates the bound; a diagnostic otherwise.
  bound(...)    per element, a first-order a-priori bound on |float32 result - step64| (below).  The GPU tests assert
                ASSERT_FACTOR = 2 x it; the factor covers second-order terms and nothing else.
  rows / compact: visible_only = 1 (only rows[...] are updated) and 2 (gradient row r belongs to splat rows[r]).

The bound, u = 2^-24 (every +, -, *, /, sqrt is one correctly rounded binary32 operation, relative error <= u):

  E_g (the activation chain)
    pos, sh   0
    scale     u |g_raw|                        one product
    opacity   3 u |g_raw|                      g o, 1 - o, their product
    rotq      ( |q_i| 4 u sum_j |q_j g_j|      q . g: a product and at most three additions per term
                + u |q_i (q . g)|              the product q_i (q . g)
                + 6 u |g_i - q_i (q . g)| ) / |raw|
                                               the subtraction (1), 1 / sqrt(sum of four squares) (4: a square and three
                                               additions per term = 4 u on the sum, halved by the root, + root + reciprocal),
                                               the last product (1).  Sums of magnitudes: the projection cancels when g || q.
  E_m = 2 u (|b1 m| + |(1 - b1) g_raw|) + (1 - b1) E_g + d1 |g_raw| + 2^-126
                                               two products and a sum (u |m'| <= u (|b1 m| + |(1 - b1) g_raw|));
                                               d1 = |fl(1 - b1) - (1 - b1)| (0 for beta >= 0.5, Sterbenz)
  E_v = 3 u v' + 2 (1 - b2) |g_raw| E_g + d2 g_raw^2 + 2^-126
                                               b2 v (1), ((1 - b2) g) g (2), the sum (1): u b2 v + 2 u (1 - b2) g^2 + u v' <= 3 u v'
  the floor 2^-126 makes the bound independent of whether subnormal intermediates are kept or flushed
  D = sqrt(v') c2 + eps as an interval: D_lo = (sqrt(max(v' - E_v, 0)) c2 (1 - 3 u) + eps)(1 - u), D_hi likewise upwards
                                               (root, the rounding of c2 to binary32, their product: 3 u; the sum: u)
  E_upd = 4 u |A| (|m'| + E_m) / D_lo          A = lr c1: rounding of c1, lr c1, A m', the quotient
          + |A| E_m / D_lo
          + |A m'| max(1 / D_lo - 1 / D, 1 / D - 1 / D_hi)
  E_raw = u |raw'| + E_upd                     the final subtraction
  E_act   pos, sh   E_raw (the same float)
          scale     exp(raw') (expm1(E_raw) + 2 u K) + 2^-126                    K = EXPF_ULPS
          opacity   o' ((1 - o') (expm1(E_raw) + 2 u K) + 2 u) + 2^-126          o' = 1 / (1 + e), e = expf(-raw'): the error of e
                                               reaches o' scaled by e / (1 + e) = 1 - o'; 1 + e and the reciprocal round once each
          rotq      sum_j |d_ij - q'_i q'_j| E_raw_j / |raw'| + 5 u |q'_i|       the Jacobian of x / |x|; 1 / sqrt(sum) (4), product (1)
          and E_act = inf where the float64 value + E_act leaves binary32's range (expf may then return inf)

EXPF_ULPS: the ROCm installation documents no ulp table for its device math library, so device expf was measured once on the
MI355X against float64 exp: 50 331 648 arguments drawn uniformly from [-20, 5] and rounded to binary32 (`act.scale` after an
lcgs_adam_step with g = m = v = 0 is expf(raw.scale)); the largest error was EXPF_ULPS_MEASURED = 0.8452 ulp of the result (mean
0.257, 6.3 % of the arguments above half an ulp), and EXPF_ULPS is twice that."""
import math

import torch

KEYS = ("pos", "scale", "rotq", "sh", "opacity")
ARRAYS = ("raw", "m", "v", "act")
LR = {"pos": 1.6e-4, "sh_dc": 2.5e-3, "sh_rest": 1.25e-4, "opacity": 5e-2, "scale": 5e-3, "rot": 1e-3}
U = 2.0 ** -24
FLOOR = 2.0 ** -126
FLT_MAX = 3.4028234663852886e38
EXPF_ULPS_MEASURED = 0.8452
EXPF_ULPS = 2.0 * EXPF_ULPS_MEASURED
ASSERT_FACTOR = 2.0
STEPS = (1, 2, 10, 1000, 30000)
EPSES = (1e-8, 1e-15)
CLASSES = ("general", "decay", "cancellation", "saturation")


def f32(x):
    """the binary32 number nearest to x, as a Python float"""
    return torch.tensor(float(x), dtype=torch.float32).item()


def scalars(step, lr=LR, betas=(0.9, 0.999), eps=1e-15):
    """what crosses the ABI (binary32) and the two bias corrections (float64 functions of the binary32 betas)"""
    b1, b2 = f32(betas[0]), f32(betas[1])
    assert step >= 1 and 0.0 < b1 < 1.0 and 0.0 < b2 < 1.0
    one = torch.tensor(1.0, dtype=torch.float32)
    return {"b1": b1, "b2": b2, "eps": f32(eps), "step": int(step), "lr": {k: f32(x) for k, x in lr.items()},
            "c1": 1.0 / (1.0 - b1 ** step), "c2": 1.0 / math.sqrt(1.0 - b2 ** step),
            # 1 - beta as the kernels form it, in binary32
            "omb1_32": (one - torch.tensor(b1, dtype=torch.float32)).item(),
            "omb2_32": (one - torch.tensor(b2, dtype=torch.float32)).item()}


def lr_columns(key, width, s, dtype, device):
    """the learning rate of every column of an attribute: SH columns 0..2 are the dc band, the others the rest, at every degree"""
    lr = s["lr"]
    if key == "sh":
        cols = [lr["sh_dc"]] * 3 + [lr["sh_rest"]] * (width - 3)
        return torch.tensor(cols, dtype=dtype, device=device)
    return torch.tensor(lr[{"pos": "pos", "scale": "scale", "rotq": "rot", "opacity": "opacity"}[key]], dtype=dtype, device=device)


def activate32(raw):
    """float32 activations of a raw pack (pos / sh are the same tensors)"""
    return {"pos": raw["pos"], "scale": torch.exp(raw["scale"]),
            "rotq": raw["rotq"] / raw["rotq"].norm(dim=1, keepdim=True), "sh": raw["sh"],
            "opacity": torch.sigmoid(raw["opacity"])}


# ------------------------------------------------------------------------------------------------ float64, with the bound
def attr64(key, g, raw, m, v, act, s, want_bound=True):
    """one attribute, all rows -> ({"raw", "m", "v", "act"} float64, the same keys' first-order bounds or None)"""
    g, raw, m, v, act = (t.double() for t in (g, raw, m, v, act))
    b1, b2, eps, c1, c2 = s["b1"], s["b2"], s["eps"], s["c1"], s["c2"]
    A = lr_columns(key, raw.shape[-1] if raw.dim() > 1 else 1, s, torch.float64, raw.device) * c1
    if key in ("pos", "sh"):
        gr, Eg = g, None
    elif key == "scale":
        gr = g * act
        Eg = U * gr.abs()
    elif key == "opacity":
        gr = g * act * (1.0 - act)
        Eg = 3.0 * U * gr.abs()
    else:
        inv = 1.0 / (raw * raw).sum(dim=1, keepdim=True).sqrt()
        qg = (act * g).sum(dim=1, keepdim=True)
        d = g - act * qg
        gr = d * inv
        Eg = inv * (act.abs() * (4.0 * U) * (act * g).abs().sum(dim=1, keepdim=True) + U * (act * qg).abs() + 6.0 * U * d.abs())
    m1 = b1 * m + (1.0 - b1) * gr
    v1 = b2 * v + (1.0 - b2) * gr * gr
    D = v1.sqrt() * c2 + eps
    raw1 = raw - A * m1 / D
    if key in ("pos", "sh"):
        act1 = raw1
    elif key == "scale":
        act1 = torch.exp(raw1)
    elif key == "opacity":
        act1 = 1.0 / (1.0 + torch.exp(-raw1))
    else:
        n1 = (raw1 * raw1).sum(dim=1, keepdim=True).sqrt()
        act1 = raw1 / n1
    out = {"raw": raw1, "m": m1, "v": v1, "act": act1}
    if not want_bound:
        return out, None
    zero = torch.zeros((), dtype=torch.float64, device=raw.device)
    Eg = zero if Eg is None else Eg
    d1, d2 = abs(s["omb1_32"] - (1.0 - b1)), abs(s["omb2_32"] - (1.0 - b2))
    Em = 2.0 * U * ((b1 * m).abs() + ((1.0 - b1) * gr).abs()) + (1.0 - b1) * Eg + d1 * gr.abs() + FLOOR
    Ev = 3.0 * U * v1 + 2.0 * (1.0 - b2) * gr.abs() * Eg + d2 * gr * gr + FLOOR
    D_lo = ((v1 - Ev).clamp_min(0.0).sqrt() * c2 * (1.0 - 3.0 * U) + eps) * (1.0 - U)
    D_hi = ((v1 + Ev).sqrt() * c2 * (1.0 + 3.0 * U) + eps) * (1.0 + U)
    Eupd = (4.0 * U * A.abs() * (m1.abs() + Em) / D_lo + A.abs() * Em / D_lo
            + (A * m1).abs() * torch.maximum(1.0 / D_lo - 1.0 / D, 1.0 / D - 1.0 / D_hi))
    Eraw = U * raw1.abs() + Eupd
    if key in ("pos", "sh"):
        Eact = Eraw
    elif key == "scale":
        Eact = act1 * (torch.expm1(Eraw) + 2.0 * U * EXPF_ULPS) + FLOOR
    elif key == "opacity":
        one_minus = 1.0 / (1.0 + torch.exp(raw1))
        Eact = act1 * (one_minus * (torch.expm1(Eraw) + 2.0 * U * EXPF_ULPS) + 2.0 * U) + FLOOR
    else:
        eye = torch.eye(4, dtype=torch.float64, device=raw.device)
        J = (eye[None] - act1[:, :, None] * act1[:, None, :]).abs()  # [P, i, j]
        Eact = (J * Eraw[:, None, :]).sum(dim=2) / n1 + 5.0 * U * act1.abs()
    if key in ("scale", "opacity"):
        Eact = torch.where(torch.nan_to_num(act1 + Eact, nan=math.inf) > FLT_MAX, torch.full_like(Eact, math.inf), Eact)
    return out, {"raw": Eraw, "m": Em, "v": Ev, "act": Eact}


# ------------------------------------------------------------------------------------------------ float32, the kernels' order
def attr32(key, g, raw, m, v, act, s, mutant=0):
    """one attribute, all rows, every operation a float32 tensor operation in the order the kernels write it.
    mutant 1 .. 6: the one-line kernel mutants of docs/TESTS.md "Optimiser step" (tests/test_adam_ref.py shows that the bound flags
    each): 1 bias corrections of step - 1, 2 eps inside the root, 3 the old m stored, 4 v without (1 - b2), 5 column 3 of SH at the
    dc rate, 6 the opacity chain with 1 + o."""
    for t in (g, raw, m, v, act):
        assert t.dtype == torch.float32
    dev = raw.device
    t32 = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
    b1, b2, eps = t32(s["b1"]), t32(s["b2"]), t32(s["eps"])
    one = t32(1.0)
    c1, c2 = t32(s["c1"]), t32(s["c2"])  # make_adam_step: the float64 value rounded once
    if mutant == 1 and s["step"] >= 2:
        c1, c2 = t32(1.0 / (1.0 - s["b1"] ** (s["step"] - 1))), t32(1.0 / math.sqrt(1.0 - s["b2"] ** (s["step"] - 1)))
    lr = lr_columns(key, raw.shape[-1] if raw.dim() > 1 else 1, s, torch.float32, dev)
    if mutant == 5 and key == "sh" and lr.numel() > 3:
        lr[3] = lr[0]
    if key == "scale":
        g = g * act
    elif key == "opacity":
        g = g * act * ((one + act) if mutant == 6 else (one - act))
    elif key == "rotq":
        x = [raw[:, i] for i in range(4)]
        inv = one / torch.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3])
        qg = act[:, 0] * g[:, 0] + act[:, 1] * g[:, 1] + act[:, 2] * g[:, 2] + act[:, 3] * g[:, 3]
        g = torch.stack([(g[:, i] - act[:, i] * qg) * inv for i in range(4)], dim=1)
    m1 = b1 * m + (one - b1) * g
    v1 = b2 * v + ((one if mutant == 4 else one - b2) * g) * g
    den = torch.sqrt(v1 + eps) * c2 if mutant == 2 else torch.sqrt(v1) * c2 + eps
    raw1 = raw - (lr * c1) * m1 / den
    if key in ("pos", "sh"):
        act1 = raw1
    elif key == "scale":
        act1 = torch.exp(raw1)
    elif key == "opacity":
        act1 = one / (one + torch.exp(-raw1))
    else:
        x = [raw1[:, i] for i in range(4)]
        n2 = one / torch.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3])
        act1 = torch.stack([x[i] * n2 for i in range(4)], dim=1)
    out = {"raw": raw1, "m": m.clone() if mutant == 3 else m1, "v": v1, "act": act1}
    assert all(t.dtype == torch.float32 for t in out.values())
    return out


# ------------------------------------------------------------------------------------------------ packs, row lists
def _rows_of(key, grad, raw, m, v, act, rows, compact):
    if rows is None:
        return grad[key], raw[key], m[key], v[key], act[key]
    rows = rows.long()
    g = grad[key][:rows.numel()] if compact else grad[key][rows]
    return g, raw[key][rows], m[key][rows], v[key][rows], act[key][rows]


def _scatter(full, rows, part, dtype):
    if rows is None:
        return part
    out = full.to(dtype).clone()
    out[rows.long()] = part
    return out


def attr64_rows(key, grad, raw, m, v, act, s, rows=None, compact=False, want_bound=True):
    """attr64 on the listed rows; the other rows keep their input and get a zero bound (they must be untouched bit for bit)"""
    out, bnd = attr64(key, *_rows_of(key, grad, raw, m, v, act, rows, compact), s, want_bound)
    full = {"raw": raw[key], "m": m[key], "v": v[key], "act": act[key]}
    out = {a: _scatter(full[a], rows, out[a], torch.float64) for a in ARRAYS}
    if bnd is not None:
        bnd = {a: _scatter(torch.zeros_like(full[a], dtype=torch.float64), rows, bnd[a], torch.float64) for a in ARRAYS}
    return out, bnd


def _per_key(fn):
    res = {a: {} for a in ARRAYS}
    for key in KEYS:
        for a, t in fn(key).items():
            res[a][key] = t
    return res


def step64(grad, raw, m, v, act, s, rows=None, compact=False):
    return _per_key(lambda key: attr64_rows(key, grad, raw, m, v, act, s, rows, compact, want_bound=False)[0])


def bound(grad, raw, m, v, act, s, rows=None, compact=False):
    """the first-order bound, per element, as {"raw", "m", "v", "act"} of packs"""
    return _per_key(lambda key: attr64_rows(key, grad, raw, m, v, act, s, rows, compact)[1])


def step32(grad, raw, m, v, act, s, rows=None, compact=False, mutant=0):
    def one(key):
        out = attr32(key, *_rows_of(key, grad, raw, m, v, act, rows, compact), s, mutant)
        full = {"raw": raw[key], "m": m[key], "v": v[key], "act": act[key]}
        return {a: _scatter(full[a], rows, out[a], torch.float32) for a in ARRAYS}

    return _per_key(one)


# ------------------------------------------------------------------------------------------------ the comparison
def compare(got, ref64, bnd, factor):
    """-> (worst |got - ref64| / (factor x bnd), elements outside).  Equal values (equal infinities included) differ by 0; a
    NaN is outside; an infinite bound (binary32's range left) admits any non-NaN value."""
    got, lim = got.double(), factor * bnd
    diff = torch.where(got == ref64, torch.zeros_like(ref64), (got - ref64).abs())
    bad = ~(diff <= lim)
    ratio = torch.where((diff == 0) | torch.isinf(lim), torch.zeros_like(diff), diff / lim)
    ratio = torch.where(bad, torch.full_like(ratio, math.inf), ratio)
    return (float(ratio.max()) if ratio.numel() else 0.0), int(bad.sum())


def check(got, grad, raw, m, v, act, s, rows=None, compact=False, factor=ASSERT_FACTOR):
    """`got` = {"raw", "m", "v", "act"} of packs after a step from the given inputs -> {(array, key): (worst ratio, elements
    outside)}, one attribute at a time (the float64 temporaries of a 16 M-row pack are freed in between)"""
    res = {}
    for key in KEYS:
        ref, bnd = attr64_rows(key, grad, raw, m, v, act, s, rows, compact)
        for a in ARRAYS:
            res[(a, key)] = compare(got[a][key], ref[a], bnd[a], factor)
    return res


def report(res, tag):
    worst = {a: max(res[(a, k)][0] for k in KEYS) for a in ARRAYS}
    print(f"[adam] {tag}: worst diff / bound  " + "  ".join(f"{a} {worst[a]:.3f}" for a in ARRAYS)
          + "  | act per attribute  " + "  ".join(f"{k} {res[('act', k)][0]:.3f}" for k in KEYS)
          + "  | raw per attribute  " + "  ".join(f"{k} {res[('raw', k)][0]:.3f}" for k in KEYS))
    return worst


def failures(res):
    return {k: x for k, x in res.items() if x[1] != 0}


# ------------------------------------------------------------------------------------------------ input classes
def _loguniform(shape, lo, hi, gen, device):
    e = torch.rand(shape, generator=gen, device=device, dtype=torch.float64) * (math.log10(hi) - math.log10(lo)) + math.log10(lo)
    return 10.0 ** e


def _signs(shape, gen, device):
    return torch.randint(0, 2, shape, generator=gen, device=device).double() * 2.0 - 1.0


def shapes(P, sh_floats):
    return {"pos": (P, 3), "scale": (P, 3), "rotq": (P, 4), "sh": (P, sh_floats), "opacity": (P,)}


def make_inputs(cls, P, sh_floats, seed, s, device="cpu"):
    """(grad, raw, m, v, act) float32 packs of one input class, each asserted to be what it claims.  `act` is the float32
    activation of raw (separate tensors for pos / sh too; the caller aliases them where it wants to).
      general        |g|, |m| log-uniform over 1e-12 .. 1e2 with random signs, v over 1e-24 .. 1e4; raw scale in [-10, 3], raw
                     opacity in [-15, 15], quaternion norms in {1e-3, 1, 1e3}
      decay          general with g = 0
      cancellation   b1 m + (1 - b1) g_raw cancels to 1e-6 of its terms (pos, scale, sh, opacity); rotation gradients parallel
                     to q within 1e-6 (their moments do not cancel too: the chain's error would then be the whole m')
      saturation     raw opacity +-15; v, g and m tiny so that sqrt(v') c2 lies within 1e-2 .. 1e2 of eps, on both sides (the
                     caller passes s with eps = 1e-15)"""
    gen = torch.Generator(device=device).manual_seed(seed)
    shp = shapes(P, sh_floats)
    f = lambda t: t.to(torch.float32)
    rnd = lambda k: torch.rand(shp[k], generator=gen, device=device, dtype=torch.float64)
    raw = {"pos": f(torch.randn(shp["pos"], generator=gen, device=device, dtype=torch.float64)),
           "scale": f(rnd("scale") * 13.0 - 10.0), "sh": f(0.3 * torch.randn(shp["sh"], generator=gen, device=device, dtype=torch.float64)),
           "opacity": f(rnd("opacity") * 30.0 - 15.0)}
    q = torch.randn(shp["rotq"], generator=gen, device=device, dtype=torch.float64)
    norms = torch.tensor([1e-3, 1.0, 1e3], dtype=torch.float64, device=device)[torch.randint(0, 3, (P, 1), generator=gen, device=device)]
    raw["rotq"] = f(q / q.norm(dim=1, keepdim=True) * norms)
    if cls == "saturation":
        raw["opacity"] = f(15.0 * _signs(shp["opacity"], gen, device))
    act = {k: t.clone() for k, t in activate32(raw).items()}
    g, m, v = {}, {}, {}
    for k in KEYS:
        if cls in ("general", "decay"):
            g[k] = f(_loguniform(shp[k], 1e-12, 1e2, gen, device) * _signs(shp[k], gen, device))
            m[k] = f(_loguniform(shp[k], 1e-12, 1e2, gen, device) * _signs(shp[k], gen, device))
            v[k] = f(_loguniform(shp[k], 1e-24, 1e4, gen, device))
            if cls == "decay":
                g[k] = torch.zeros_like(g[k])
        elif cls == "cancellation":
            g[k] = f(_loguniform(shp[k], 1e-6, 1.0, gen, device) * _signs(shp[k], gen, device))
            if k == "rotq":
                w = torch.randn(shp[k], generator=gen, device=device, dtype=torch.float64)
                qa = act[k].double()
                g[k] = f(g[k].double()[:, :1] * (qa + 1e-6 * w / w.norm(dim=1, keepdim=True)))
                m[k] = f(_loguniform(shp[k], 1e-6, 1.0, gen, device) * _signs(shp[k], gen, device))
            else:
                a = act[k].double()
                gr = {"pos": 1.0, "sh": 1.0, "scale": a, "opacity": a * (1.0 - a)}[k] * g[k].double()
                m[k] = f(-(1.0 - s["b1"]) * gr / s["b1"] * (1.0 + 1e-6))
            v[k] = f((m[k].double().abs() + g[k].double().abs()) ** 2 * _loguniform(shp[k], 0.1, 10.0, gen, device))
        elif cls == "saturation":
            target = s["eps"] * _loguniform(shp[k], 1e-2, 1e2, gen, device) / s["c2"]  # sqrt(v') aimed at
            v[k] = f(target * target)
            g[k] = f(target * _loguniform(shp[k], 0.1, 10.0, gen, device) * _signs(shp[k], gen, device))
            m[k] = f(target * _loguniform(shp[k], 0.1, 10.0, gen, device) * _signs(shp[k], gen, device))
        else:
            raise ValueError(cls)
    _assert_class(cls, g, raw, m, v, act, s)
    return g, raw, m, v, act


def _assert_class(cls, g, raw, m, v, act, s):
    inside = lambda t, lo, hi: bool(((t.double().abs() >= lo * (1 - 1e-6)) & (t.double().abs() <= hi * (1 + 1e-6))).all())
    for k in KEYS:
        assert all(bool(torch.isfinite(t[k]).all()) for t in (g, raw, m, v, act)) and bool((v[k] >= 0).all()), (cls, k)
    assert bool((raw["scale"] >= -10).all() and (raw["scale"] <= 3).all() and (raw["opacity"].abs() <= 15).all())
    n = raw["rotq"].double().norm(dim=1)
    assert bool((((n / 1e-3 - 1).abs() < 1e-6) | ((n - 1).abs() < 1e-6) | ((n / 1e3 - 1).abs() < 1e-6)).all())
    if cls in ("general", "decay"):
        for k in KEYS:
            assert inside(m[k], 1e-12, 1e2) and inside(v[k], 1e-24, 1e4), (cls, k)
            assert inside(g[k], 1e-12, 1e2) if cls == "general" else bool((g[k] == 0).all()), (cls, k)
    if cls == "cancellation":
        for k in KEYS:
            if k == "rotq":
                q, gg = act[k].double(), g[k].double()
                perp = gg - q * (q * gg).sum(dim=1, keepdim=True)
                assert bool((perp.norm(dim=1) <= 2e-6 * gg.norm(dim=1)).all()), k
                continue
            a = act[k].double()
            gr = {"pos": 1.0, "sh": 1.0, "scale": a, "opacity": a * (1.0 - a)}[k] * g[k].double()
            t1, t2 = s["b1"] * m[k].double(), (1.0 - s["b1"]) * gr
            live = t2 != 0
            assert bool(((t1 + t2).abs()[live] <= 2e-6 * t2.abs()[live]).all()) and bool((t1 * t2 <= 0).all()), k
    if cls == "saturation":
        assert abs(s["eps"] - 1e-15) < 1e-21
        assert bool((raw["opacity"].abs() == 15).all())
        one_minus = 1.0 - act["opacity"].double()
        few = torch.minimum(one_minus, act["opacity"].double())
        assert bool((few < 2.0 ** -21).all()) and bool((few > 0).all())  # o or 1 - o ~ 3e-7: a few bits below 1
        side = torch.cat([(attr64(k, g[k], raw[k], m[k], v[k], act[k], s, False)[0]["v"].sqrt() * s["c2"] > s["eps"]).reshape(-1)
                          for k in KEYS])
        assert 0 < int(side.sum()) < side.numel()  # eps dominates in some elements and not in others


# ------------------------------------------------------------------------------------------------ trajectories
def activate64(raw):
    raw = {k: t.double() for k, t in raw.items()}
    return {"pos": raw["pos"], "scale": torch.exp(raw["scale"]),
            "rotq": raw["rotq"] / (raw["rotq"] * raw["rotq"]).sum(dim=1, keepdim=True).sqrt(), "sh": raw["sh"],
            "opacity": 1.0 / (1.0 + torch.exp(-raw["opacity"]))}


def trajectory(raw0, grads_seq, dtype, lr=LR, betas=(0.9, 0.999), eps=1e-15):
    """steps 1 .. len(grads_seq) from zero moments, the restatement carrying its own state in `dtype` (float64: step64 from the
    exact activation of raw0; float32: step32 from activate32(raw0)) -> {"raw", "m", "v", "act"} of packs after the last step"""
    if dtype == torch.float64:
        raw, fn = {k: t.double() for k, t in raw0.items()}, step64
        act = activate64(raw)
    else:
        raw, fn = {k: t.clone() for k, t in raw0.items()}, step32
        act = activate32(raw)
    state = {"raw": raw, "m": {k: torch.zeros_like(t) for k, t in raw.items()},
             "v": {k: torch.zeros_like(t) for k, t in raw.items()}, "act": act}
    for step, g in enumerate(grads_seq, 1):
        state = fn(g, state["raw"], state["m"], state["v"], state["act"], scalars(step, lr, betas, eps))
    return state


def trajectory_bound(ref64, ref32):
    """the photometric suite's bar for one array: 3 E32 + 4 u S, E32 = max |float32 trajectory - float64 trajectory|, S = max
    |float64 trajectory| (the state is the kernel's own after the first step, so no a-priori bound applies)"""
    return 3.0 * float((ref32.double() - ref64).abs().max()) + 4.0 * U * float(ref64.abs().max())
