"""`-m gpu`: 3DGS-MCMC density control (lcgs_mcmc_relocate / _add / _noise / _regularize) against the restatement
in tests/mcmc_ref.py: the built-in sampler bit for bit, the binary64 relocation values to one binary32 ulp, the in-place
update's untouched rows, the edges, the SGLD noise, the regulariser, the image invariance the formulas exist for, and a short
end-to-end fit with a growing splat count.

The u64 scan of the weights works in blocks of SCAN_TILE = 1024 rows (kScanTile, csrc/kernels/scan.hip), its middle step
in passes of 1024 block sums: the sampler's sizes sit on both edges (1024 +- 1, and 1024^2 + 1 = 1 048 577 rows for the second
pass).

The weights are a function of the binary32 sigmoid as the DEVICE evaluates it (its expf may differ from NumPy's in the last
place), so the model takes that value from the library's own activation kernel: lcgs_opacity_reset with a ceiling above every
entry rewrites nothing but the activated opacity (_device_sigmoid)."""
import numpy as np
import pytest
import torch

import mcmc_ref as ref
from conftest import make_scene
from gpu_util import DEV, assert_image_parity, upload_scene

pytestmark = pytest.mark.gpu

KEYS = ("pos", "scale", "rotq", "sh", "opacity")
LR = {"pos": 1.6e-4, "sh_dc": 2.5e-3, "sh_rest": 1.25e-4, "opacity": 5e-2, "scale": 5e-3, "rot": 1e-3}
F32, F64 = np.float32, np.float64
SCAN_TILE = ref.SCAN_TILE
MIN_OP = 0.005
assert SCAN_TILE == 1024


def _activate(raw):
    return {"pos": raw["pos"], "scale": torch.exp(raw["scale"]),
            "rotq": raw["rotq"] / raw["rotq"].norm(dim=1, keepdim=True), "sh": raw["sh"],
            "opacity": torch.sigmoid(raw["opacity"])}


def _logit(o):
    o = np.asarray(o, F64)
    return (np.log(o) - np.log1p(-o)).astype(F32)


def _raw_scene(rng, P, feat, opacity_std=2.5):
    return {"pos": rng.normal(0, 1, (P, 3)).astype(F32), "scale": rng.normal(-4, 1, (P, 3)).astype(F32),
            "rotq": rng.normal(0, 1, (P, 4)).astype(F32), "sh": rng.normal(0, 0.3, (P, feat)).astype(F32),
            "opacity": rng.normal(0, opacity_std, P).astype(F32)}


def _device_sigmoid(lcgs, x):
    """act_sigmoid of raw opacities as the kernels evaluate it, through lcgs_opacity_reset on a scratch copy (NaN stays NaN)"""
    x = np.asarray(x, F32)
    nan = np.isnan(x)
    assert (x[~nan] < 16.0).all()  # below logit(1 - 2^-24) = 16.6: the reset's ceiling leaves every entry alone
    t = torch.from_numpy(np.where(nan, F32(0), x)).to(DEV)
    raw, act = t.clone(), torch.empty_like(t)
    r = lcgs.Renderer(lcgs.Context(0))
    r.opacity_reset({"opacity": raw}, {"opacity": torch.zeros_like(t)}, {"opacity": torch.zeros_like(t)}, {"opacity": act},
                    max_opacity=float(F32(1 - 2.0 ** -24)))
    r.ctx.synchronize()
    assert torch.equal(raw, t)
    o = act.cpu().numpy()
    o[nan] = np.nan
    return o


class Scene:
    """raw / m / v / activated device arrays of `cap` rows (the first P hold `raw`), moments filled with sentinels"""

    def __init__(self, raw, cap=None, alias=True, m_fill=3.0, v_fill=4.0, tail=5.0):
        P = raw["opacity"].shape[0]
        cap = P if cap is None else cap
        self.P, self.cap = P, cap

        def up(a, fill):
            t = torch.full((cap,) + a.shape[1:], fill, dtype=torch.float32, device=DEV)
            t[:P] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
            return t

        self.raw = {k: up(raw[k], tail) for k in KEYS}
        self.m = {k: torch.full_like(self.raw[k], m_fill) for k in KEYS}
        self.v = {k: torch.full_like(self.raw[k], v_fill) for k in KEYS}
        with np.errstate(all="ignore"):
            self.act = {k: t.clone() for k, t in _activate(self.raw).items()}
        if alias:
            self.act["pos"], self.act["sh"] = self.raw["pos"], self.raw["sh"]
        self.src_row = torch.full((cap,), -1, dtype=torch.int32, device=DEV)

    def packs(self):
        return self.raw, self.m, self.v, self.act

    def snapshot(self):
        return {name: {k: t.clone() for k, t in d.items()} for name, d in zip(("raw", "m", "v", "act"), self.packs())}

    def unchanged_since(self, snap, rows=slice(None)):
        for name, d in zip(("raw", "m", "v", "act"), self.packs()):
            for k in KEYS:
                a, b = d[k][rows].cpu().numpy().view(np.uint32), snap[name][k][rows].cpu().numpy().view(np.uint32)
                assert np.array_equal(a, b), (name, k)


def _cpu(d):
    return {k: t.cpu().numpy() for k, t in d.items()}


def _check_activated(raw, act, rows):
    ref_act = _activate({k: torch.from_numpy(a[rows].astype(F64)) for k, a in raw.items()})
    for k in KEYS:
        a, b = act[k][rows].astype(F64), ref_act[k].numpy()
        assert np.allclose(a, b, rtol=2e-5, atol=2e-6), ("activated " + k, np.abs(a - b).max())


# ------------------------------------------------------------------------------------------------------------ 1. the sampler
def _sampler_scene(P, seed):
    rng = np.random.default_rng(seed)
    raw = _raw_scene(rng, P, 3)
    if P >= 2:  # both ends of the cdf matter: a dead first row, a live last one
        raw["opacity"][0], raw["opacity"][-1] = F32(-9.0), F32(1.5)
    return raw


@pytest.mark.parametrize("P", [1, 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 100_003, SCAN_TILE * SCAN_TILE + 1])
def test_built_in_sampler_matches_the_model_bit_for_bit(lcgs, P):
    assert SCAN_TILE * SCAN_TILE + 1 < 1_100_000
    raw = _sampler_scene(P, 100 + P % 97)
    o = _device_sigmoid(lcgs, raw["opacity"])
    w, dead = ref.weights(o, MIN_OP)
    cdf = ref.cdf(w)
    D = int(dead.sum())
    r = lcgs.Renderer(lcgs.Context(0))
    # relocation: draw j fills the j-th dead row
    s = Scene(raw)
    n = r.mcmc_relocate(*s.packs(), min_opacity=MIN_OP, seed=77, src_row=s.src_row, sh_degree=0)
    r.ctx.synchronize()
    got = s.src_row.cpu().numpy()
    want = np.arange(P)
    if D and int(cdf[-1]):
        src = ref.draws(cdf, D, 77, ref.TAG_RELOCATE)
        want[np.nonzero(dead)[0]] = src
        assert n == D
        counts = np.bincount(got[dead], minlength=P)
        assert np.array_equal(counts, np.bincount(src, minlength=P))  # the per-row counts
    else:
        assert n == 0
    assert np.array_equal(got, want), int((got != want).sum())
    if P < 2:
        return
    assert D >= 1 and n == D
    # the same seed gives the same rows, another seed others
    again, other = Scene(raw), Scene(raw)
    r.mcmc_relocate(*again.packs(), min_opacity=MIN_OP, seed=77, src_row=again.src_row, sh_degree=0)
    r.mcmc_relocate(*other.packs(), min_opacity=MIN_OP, seed=78, src_row=other.src_row, sh_degree=0)
    r.ctx.synchronize()
    assert torch.equal(again.src_row, s.src_row)
    for k in KEYS:
        assert torch.equal(again.raw[k].view(torch.int32), s.raw[k].view(torch.int32)), k
    if D >= 8 and (w > 0).sum() >= 8:
        assert not torch.equal(other.src_row, s.src_row)
    # growth: the same weights, its own tag; a draw does not depend on how many are made (the launch shape)
    live = int((w > 0).sum())
    many, few = min(3 * SCAN_TILE + 5, max(P // 2, 1)), min(10, max(P // 2, 1))
    runs = {}
    for name, num_new in (("many", many), ("few", few)):
        g = Scene(raw, cap=P + num_new)
        r.mcmc_add(P, num_new, *g.packs(), min_opacity=MIN_OP, seed=77, src_row=g.src_row, sh_degree=0)
        r.ctx.synchronize()
        runs[name] = g.src_row.cpu().numpy()[:num_new]
        assert (g.src_row.cpu().numpy()[num_new:] == -1).all()
    want_add = ref.draws(cdf, many, 77, ref.TAG_ADD)
    assert np.array_equal(runs["many"], want_add) and np.array_equal(runs["few"], want_add[:few])
    print(f"[mcmc sampler] P={P}: {D} dead, {live} live, T={int(cdf[-1])}; {many} growth draws")


# ------------------------------------------------------------------------------------------------------------ 2. the values
COUNTS = (1, 2, 3, 50, 51, 52, 500)
OPACITIES = (0.0051, 0.02, 0.2, 0.5, 0.9, 0.999, 1 - 1e-7)


def _heaped(rng, feat, bystanders=700):
    """a scene whose dead rows heap onto 49 sources: every count of COUNTS at every opacity of OPACITIES -> (raw, src_in,
    source rows, their counts, dead rows ascending)"""
    pairs = [(c, o) for c in COUNTS for o in OPACITIES]
    n_dead = sum(c for c, _ in pairs)
    P = len(pairs) + n_dead + bystanders
    raw = _raw_scene(rng, P, feat)
    raw["opacity"] = _logit(rng.uniform(0.02, 0.98, P))  # bystanders: live, never drawn
    perm = rng.permutation(P)
    sources, dead_rows = perm[:len(pairs)], np.sort(perm[len(pairs):len(pairs) + n_dead])
    raw["opacity"][sources] = _logit(np.array([o for _, o in pairs], F32).astype(F64))
    raw["opacity"][dead_rows] = F32(-10.0)
    raw["opacity"][dead_rows[::7]] = np.nan
    counts = np.array([c for c, _ in pairs])
    src_in = rng.permutation(np.repeat(sources, counts)).astype(np.int32)
    return raw, src_in, sources, counts, dead_rows


@pytest.mark.parametrize("deg,alias", [(3, True), (1, False)])
def test_relocation_values_with_injected_sources(lcgs, deg, alias):
    rng = np.random.default_rng(40 + deg)
    feat = (deg + 1) ** 2 * 3
    raw, src_in, sources, counts, dead_rows = _heaped(rng, feat)
    P = raw["opacity"].shape[0]
    o_src = 1 / (1 + np.exp(-raw["opacity"][sources].astype(F64)))
    assert o_src.min() < 0.0052 and o_src.max() > 1 - 2e-7 and abs(o_src - 0.5).min() < 1e-6
    s = Scene(raw, alias=alias)
    before = s.snapshot()
    r = lcgs.Renderer(lcgs.Context(0))
    n = r.mcmc_relocate(*s.packs(), min_opacity=MIN_OP, n_max=51, src_in=torch.from_numpy(src_in).to(DEV), src_row=s.src_row,
                        sh_degree=deg)
    r.ctx.synchronize()
    assert n == dead_rows.size
    want_src = np.arange(P)
    want_src[dead_rows] = src_in
    assert np.array_equal(s.src_row.cpu().numpy(), want_src)
    g_raw, g_m, g_v, g_act = (_cpu(d) for d in s.packs())
    # the binary64 model, rounded once; one binary32 ulp for the device's pow / log against libm's in the last place
    log_c, raw_o, op, D = ref.relocated(raw["opacity"][sources], counts, 51, MIN_OP)
    want_scale = (raw["scale"][sources].astype(F64) + log_c[:, None]).astype(F32)
    want_op = raw_o.astype(F32)
    ds = np.abs(g_raw["scale"][sources].astype(F64) - want_scale.astype(F64)) / np.spacing(np.abs(want_scale)).astype(F64)
    do = np.abs(g_raw["opacity"][sources].astype(F64) - want_op.astype(F64))
    do_bound = np.spacing(np.abs(want_op)).astype(F64) + 1e-12
    print(f"[mcmc values] deg={deg}: {sources.size} sources, {n} copies; worst scale diff {ds.max():.2f} ulp, "
          f"opacity diff/bound {(do / do_bound).max():.2f}; log c in [{log_c.min():.4f}, {log_c.max():.4f}]")
    assert ds.max() <= 1.0, ds.max()
    assert (do <= do_bound).all(), (do / do_bound).max()
    assert (log_c < 0).all()
    # a copy's scale and opacity are its source's bit for bit; pos, rotq and sh are the source's ORIGINAL bits
    for k in ("scale", "opacity"):
        assert np.array_equal(g_raw[k][dead_rows].view(np.uint32), g_raw[k][src_in].view(np.uint32)), k
    for k in ("pos", "rotq", "sh"):
        assert np.array_equal(g_raw[k][dead_rows].view(np.uint32), raw[k][src_in].view(np.uint32)), k
    # moments: zero on sources and destinations; every other row, and its moments, untouched bit for bit
    touched = np.zeros(P, bool)
    touched[sources], touched[dead_rows] = True, True
    for k in KEYS:
        assert (g_m[k][touched] == 0).all() and (g_v[k][touched] == 0).all(), k
    s.unchanged_since(before, rows=torch.from_numpy(np.nonzero(~touched)[0]).to(DEV))
    for k in ("pos", "rotq", "sh"):  # a source keeps these
        assert np.array_equal(g_raw[k][sources].view(np.uint32), raw[k][sources].view(np.uint32)), k
    assert np.isfinite(g_raw["opacity"]).all()
    _check_activated(g_raw, g_act, slice(None))
    # no row is dead after the relocation, the sources clamped to min_opacity included (the liveness rule: at most one binary32
    # step up, inside the ulp above)
    clamped = op <= F64(F32(MIN_OP))
    assert clamped.sum() >= 7 and (_device_sigmoid(lcgs, g_raw["opacity"]) > F32(MIN_OP)).all()
    assert (g_raw["opacity"][sources][clamped] >= want_op[clamped]).all()


# ------------------------------------------------------------------------------------------------------------ 3. edges
def test_edges(lcgs):
    rng = np.random.default_rng(5)
    P, feat = 600, 12
    r = lcgs.Renderer(lcgs.Context(0))
    run = lambda s, **kw: r.mcmc_relocate(*s.packs(), min_opacity=kw.pop("min_opacity", MIN_OP), src_row=s.src_row, sh_degree=1, **kw)
    # no dead row, and every row dead: 0 and nothing written
    for fill in (rng.uniform(-2, 2, P).astype(F32), np.full(P, -12.0, F32)):
        raw = _raw_scene(rng, P, feat)
        raw["opacity"] = fill
        s = Scene(raw)
        snap = s.snapshot()
        assert run(s, seed=1) == 0
        r.ctx.synchronize()
        s.unchanged_since(snap)
        assert np.array_equal(s.src_row.cpu().numpy(), np.arange(P))
    # ... and growth from a scene without a live row is refused, nothing written
    g = Scene(raw, cap=P + 4)
    snap = g.snapshot()
    with pytest.raises(lcgs.LcgsError) as e:
        r.mcmc_add(P, 4, *g.packs(), sh_degree=1)
    r.ctx.synchronize()
    assert e.value.status == 8
    g.unchanged_since(snap)
    # one live row takes every draw
    raw = _raw_scene(rng, P, feat)
    raw["opacity"] = np.full(P, -12.0, F32)
    raw["opacity"][123] = F32(0.3)
    s = Scene(raw)
    assert run(s, seed=2) == P - 1
    r.ctx.synchronize()
    assert (s.src_row.cpu().numpy() == 123).all()
    got = _cpu(s.raw)
    want = ref.relocated(raw["opacity"][[123]], [P - 1])  # n = 51
    assert abs(float(got["opacity"][123]) - float(want[1][0])) <= np.spacing(F32(abs(want[1][0]))) + 1e-12
    assert (got["opacity"].view(np.uint32) == got["opacity"].view(np.uint32)[123]).all()
    # o exactly at min_opacity, and a NaN raw opacity: dead, relocated, never drawn
    raw = _raw_scene(rng, P, feat, opacity_std=1.0)
    raw["opacity"][10], raw["opacity"][20] = F32(-1.25), np.nan
    at = float(_device_sigmoid(lcgs, raw["opacity"][[10]])[0])
    o = _device_sigmoid(lcgs, raw["opacity"])
    assert (o[np.arange(P) != 20] >= F32(at)).sum() > 100 and (o < F32(at)).sum() > 20
    w, dead = ref.weights(o, at)
    assert dead[10] and dead[20] and (~dead).sum() > 100
    s = Scene(raw)
    assert run(s, seed=3, min_opacity=at) == int(dead.sum())
    r.ctx.synchronize()
    got = s.src_row.cpu().numpy()
    want = np.arange(P)
    want[dead] = ref.draws(ref.cdf(w), int(dead.sum()), 3, ref.TAG_RELOCATE)
    assert np.array_equal(got, want) and not dead[got].any()
    assert (_device_sigmoid(lcgs, s.raw["opacity"].cpu().numpy()) > F32(at)).all()  # ... and nobody is dead afterwards
    # P = 0
    empty = Scene({k: a[:0] for k, a in raw.items()})
    assert run(empty, seed=4) == 0
    r.mcmc_noise(empty.raw, empty.act, lr_pos=1e-4, step=1)
    r.mcmc_regularize({"opacity": empty.raw["opacity"], "scale": empty.raw["scale"]})
    # growth: capacity exact works; over by one is refused with the destinations (and everything else) unchanged
    raw = _raw_scene(rng, P, feat, opacity_std=1.0)
    num_new = 37
    g = Scene(raw, cap=P + num_new)
    r.mcmc_add(P, num_new, *g.packs(), seed=6, src_row=g.src_row, sh_degree=1)
    r.ctx.synchronize()
    src = g.src_row.cpu().numpy()[:num_new]
    got = _cpu(g.raw)
    assert src.min() >= 0 and src.max() < P
    for k in ("pos", "rotq", "sh"):
        assert np.array_equal(got[k][P:].view(np.uint32), raw[k][src].view(np.uint32)), k
    for k in ("scale", "opacity"):
        assert np.array_equal(got[k][P:].view(np.uint32), got[k][src].view(np.uint32)), k
    for k in KEYS:
        assert (g.m[k][P:] == 0).all() and (g.v[k][P:] == 0).all(), k
    _check_activated(got, _cpu(g.act), slice(None))
    g = Scene(raw, cap=P + num_new)
    snap = g.snapshot()
    with pytest.raises(lcgs.LcgsError) as e:
        r.mcmc_add(P, num_new + 1, *g.packs(), seed=6, src_row=g.src_row, sh_degree=1)
    r.ctx.synchronize()
    assert e.value.status == 5
    g.unchanged_since(snap)
    assert (g.src_row == -1).all()
    r.mcmc_add(P, 0, *g.packs(), seed=6, sh_degree=1)  # num_new = 0: nothing happens
    r.ctx.synchronize()
    g.unchanged_since(snap)
    # a bad entry of src_in: a row >= P, a dead row -> refused, nothing of the scene written
    raw["opacity"][:50] = F32(-12.0)
    for bad in (P, 7):
        s = Scene(raw)
        snap = s.snapshot()
        src_in = np.full(50, 300, np.int32)
        src_in[31] = bad
        with pytest.raises(lcgs.LcgsError) as e:
            run(s, src_in=torch.from_numpy(src_in).to(DEV))
        r.ctx.synchronize()
        assert e.value.status == 1, bad
        s.unchanged_since(snap)
        g = Scene(raw, cap=P + 50)
        snap = g.snapshot()
        with pytest.raises(lcgs.LcgsError) as e:
            r.mcmc_add(P, 50, *g.packs(), src_in=torch.from_numpy(src_in).to(DEV), sh_degree=1)
        r.ctx.synchronize()
        assert e.value.status == 1, bad
        g.unchanged_since(snap)


# ------------------------------------------------------------------------------------------------------------ 4. the noise
def test_noise_with_injected_normals(lcgs):
    """Bound per component: 3 x the binary32 NumPy model's own error against the binary64 model + 4 ulp of |pos|, |pos| the
    larger of the old and the new coordinate (the result is rounded on that grid).  The scene keeps a full-weight step below
    the coordinates it moves (|pos| in [0.5, 2], scales e^N(-4.5, 0.4)), as a trained scene does: the ulp term then covers an
    expf that differs from NumPy's in the last place where the model happens to be exact."""
    rng = np.random.default_rng(8)
    P = 6007
    raw = _raw_scene(rng, P, 3)
    raw["pos"] = (rng.choice([-1.0, 1.0], (P, 3)) * rng.uniform(0.5, 2.0, (P, 3))).astype(F32)
    raw["scale"] = rng.normal(-4.5, 0.4, (P, 3)).astype(F32)
    raw["opacity"] = _logit(np.concatenate([rng.uniform(1e-4, 0.004, P // 3), rng.uniform(0.004, 0.1, P // 3),
                                            rng.uniform(0.1, 0.995, P - 2 * (P // 3))]))
    eps = rng.normal(0, 1, (P, 3)).astype(F32)
    lr_pos = 1.6e-4
    new64, g64 = ref.noise_step(raw, eps, lr_pos, dtype=F64)
    new32, _ = ref.noise_step(raw, eps, lr_pos, dtype=F32)
    s = Scene(raw, alias=False)
    snap = s.snapshot()
    r = lcgs.Renderer(lcgs.Context(0))
    r.mcmc_noise(s.raw, s.act, lr_pos=lr_pos, step=1, noise=torch.from_numpy(eps).to(DEV))
    r.ctx.synchronize()
    got = s.raw["pos"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), s.act["pos"].cpu().numpy().view(np.uint32))
    for name, d in zip(("raw", "m", "v", "act"), s.packs()):  # nothing else moves, the moments least of all
        for k in KEYS:
            if k != "pos" or name in ("m", "v"):
                assert torch.equal(d[k].view(torch.int32), snap[name][k].view(torch.int32)), (name, k)
    scale_of = np.maximum(np.abs(raw["pos"].astype(F64)), np.abs(new64))
    bound = 3 * np.abs(new32.astype(F64) - new64) + 4 * np.spacing(scale_of.astype(F32)).astype(F64)
    ratio = np.abs(got.astype(F64) - new64) / bound
    o = 1 / (1 + np.exp(-raw["opacity"].astype(F64)))
    move = np.abs(got.astype(F64) - raw["pos"].astype(F64))
    print(f"[mcmc noise] worst diff/bound {ratio.max():.3f}; largest step {move.max():.3e}, of an opaque row "
          f"{move[o > 0.8].max():.3e}; gate in [{g64.min():.2e}, {g64.max():.3f}]")
    assert ratio.max() <= 1.0, ratio.max()
    # opaque rows stay where they are; dead-ish rows take the whole of Sigma eps (gate >= 1/2: it tends to 0.62 as o -> 0)
    smax = np.exp(raw["scale"].astype(F64)).max(axis=1)
    assert (o > 0.8).sum() > 300 and(move[o > 0.8] < 1e-30 * smax[o > 0.8, None]).all()
    low = o < 0.004
    assert low.sum() > 1000 and (g64[low] >= 0.5).all()
    R = ref.rotation(raw["rotq"].astype(F64), F64)
    full = 80.0 * np.einsum("nij,nj,nkj,nk->ni", R, np.exp(raw["scale"].astype(F64)) ** 2, R, eps.astype(F64))
    step64 = new64 - raw["pos"].astype(F64)
    assert (np.abs(step64[low]) >= 0.5 * np.abs(full[low]) * (1 - 1e-6)).all() and (np.abs(step64[low]) <= np.abs(full[low])).all()
    assert (move[low] > 0).mean() > 0.9


def test_built_in_normals(lcgs):
    rng = np.random.default_rng(9)
    P = 100_000
    raw = _raw_scene(rng, P, 3)
    raw["pos"][:] = 0  # the new position IS the step: no rounding against an old one
    raw["scale"] = rng.normal(-4, 0.5, (P, 3)).astype(F32)
    raw["opacity"][:] = F32(-12.0)
    r = lcgs.Renderer(lcgs.Context(0))
    runs = {}
    for name, seed, step, rows in (("a", 11, 3, P), ("b", 11, 3, P), ("seed", 12, 3, P), ("step", 11, 4, P), ("prefix", 11, 3, 1000)):
        s = Scene({k: a[:rows] for k, a in raw.items()})
        r.mcmc_noise(s.raw, s.act, lr_pos=1.6e-4, step=step, seed=seed)
        r.ctx.synchronize()
        runs[name] = s.raw["pos"].cpu().numpy()
    assert np.array_equal(runs["a"], runs["b"])
    assert not np.array_equal(runs["a"], runs["seed"]) and not np.array_equal(runs["a"], runs["step"])
    assert np.array_equal(runs["a"][:1000], runs["prefix"])  # a row's normals do not depend on P or the launch shape
    # back through Sigma^-1 = R S^-2 R^T and the gain: standard normals
    _, g64 = ref.noise_step(raw, np.zeros((P, 3), F32), 1.6e-4, dtype=F64)
    a = F64(F32(5e5) * F32(1.6e-4)) * g64
    R = ref.rotation(raw["rotq"].astype(F64), F64)
    z = np.einsum("nij,nj,nkj,nk->ni", R, np.exp(raw["scale"].astype(F64)) ** -2, R, runs["a"].astype(F64)) / a[:, None]
    mean, var = z.mean(axis=0), z.var(axis=0)
    corr = np.array([(z[:, 0] * z[:, 1]).mean(), (z[:, 0] * z[:, 2]).mean(), (z[:, 1] * z[:, 2]).mean()])
    print(f"[mcmc normals] mean {mean}, var {var}, cross moments {corr}")
    assert (np.abs(mean) <= 5 / np.sqrt(P)).all(), mean
    assert (np.abs(var - 1) <= 5 * np.sqrt(2 / P)).all(), var
    assert (np.abs(corr) <= 5 / np.sqrt(P)).all(), corr


# ------------------------------------------------------------------------------------------------------------ 5. the regulariser
def test_regulariser_is_exact(lcgs):
    rng = np.random.default_rng(10)
    r = lcgs.Renderer(lcgs.Context(0))
    for P in (1, 257, 20011):
        g = {"pos": rng.normal(size=(P, 3)), "scale": rng.normal(size=(P, 3)), "rotq": rng.normal(size=(P, 4)),
             "sh": rng.normal(size=(P, 12)), "opacity": rng.normal(size=P)}
        g = {k: a.astype(F32) for k, a in g.items()}
        d = {k: torch.from_numpy(a).to(DEV) for k, a in g.items()}
        lo, ls = 0.01, 0.03
        r.mcmc_regularize(d, lambda_opacity=lo, lambda_scale=ls)
        r.ctx.synchronize()
        add_o, add_s = F32(F64(F32(lo)) / P), F32(F64(F32(ls)) / (3.0 * P))  # single binary32 addends
        assert np.array_equal(d["opacity"].cpu().numpy(), g["opacity"] + add_o)
        assert np.array_equal(d["scale"].cpu().numpy(), g["scale"] + add_s)
        for k in ("pos", "rotq", "sh"):
            assert np.array_equal(d[k].cpu().numpy(), g[k]), k


# ------------------------------------------------------------------------------------------------------------ 6. the image
@pytest.mark.parametrize("copies", [1, 2, 4])
def test_relocation_leaves_the_image_nearly_unchanged(lcgs, oracle64, copies):
    """One isotropic splat at opacity 0.8 on 64 x 64, then `copies` dead rows relocated onto it.  The correction matches the
    splat's integral, not every pixel, so the bound is what the float64 oracle shows for the same comparison (the model's
    values) plus the 1e-4 parity bar."""
    W = H = 64
    pose = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])
    P = 1 + copies
    raw = {"pos": np.tile(np.array([[0.0, 0.0, 0.5]], F32), (P, 1)), "scale": np.full((P, 3), np.log(0.3), F32),
           "rotq": np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], F32), (P, 1)), "sh": np.zeros((P, 48), F32),
           "opacity": np.full(P, -20.0, F32)}
    raw["pos"][1:] += 5.0  # the dead rows lie elsewhere (and are invisible)
    raw["sh"][:, :3] = 1.0
    raw["opacity"][0] = _logit(0.8)
    s = Scene(raw)
    r = lcgs.Renderer(lcgs.Context(0))
    cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
    frames = []
    for step in range(2):
        r.bind_scene(*[s.act[k] for k in KEYS])
        img = torch.zeros(3, H, W, device=DEV)
        r.forward(cam, img, sync=True)
        frames.append(img.cpu().numpy().astype(F64))
        if step == 0:
            assert r.mcmc_relocate(*s.packs(), src_in=torch.zeros(copies, dtype=torch.int32, device=DEV)) == copies
            r.ctx.synchronize()
    assert frames[0].max() > 0.3  # the splat is on screen
    # the same comparison by the float64 oracle, on the model's values
    log_c, raw_o, _, _ = ref.relocated(raw["opacity"][[0]], [copies])
    act = lambda rw: {"pos": rw["pos"].astype(F64), "scale": np.exp(rw["scale"].astype(F64)), "rotq": rw["rotq"].astype(F64),
                      "sh": rw["sh"].astype(F64), "opacity": 1 / (1 + np.exp(-rw["opacity"].astype(F64)))}
    after = {k: np.repeat(a[:1].astype(F64), P, axis=0) for k, a in raw.items()}
    after["scale"] = after["scale"] + log_c[0]
    after["opacity"][:] = raw_o[0]
    ocam = oracle64.lookat(*pose, width=W, height=H)
    o_before, o_after = oracle64.render(act(raw), ocam)["img"], oracle64.render(act(after), ocam)["img"]
    residual = np.abs(o_after - o_before).max()
    diff = np.abs(frames[1] - frames[0]).max()
    print(f"[mcmc image] {copies} copies: frame moved by {diff:.3e}, the float64 oracle's by {residual:.3e}; c = {np.exp(log_c[0]):.4f}")
    print(f"[mcmc image] the first frame against the float64 oracle's: {np.abs(frames[0] - o_before).max():.3e}")
    assert diff <= residual + 1e-4, (diff, residual)


# ------------------------------------------------------------------------------------------------------------ 7. end to end
def test_lcgs_app_fits_with_mcmc_density_control(lcgs, tmp_path):
    """lcgs-app --fit --density mcmc --cap-max: the paper's schedule (first rewrite at step 500, then every 100) through the C++
    mirror; the last line but one reports the count, which reaches the cap and stops there."""
    import os
    import re
    import subprocess

    from conftest import ROOT

    app = os.path.join(ROOT, "luisacomputegaussiansplatting_amd", "lcgs-app")
    if not os.path.exists(app):
        lcgs.build_library()
    res = subprocess.run([app, "--synth", "0:20000:1001", "--res=320x240", "--out", str(tmp_path), "--world", "blender", "--pose", "lego",
                          "--fit", "600", "--density", "mcmc", "--cap-max", "20500"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    losses = [float(x) for x in re.findall(r"^step \d+ loss (\S+)$", res.stdout, flags=re.M)]
    assert len(losses) == 600 and np.isfinite(losses).all()
    m = re.search(r"^fit: mcmc density control: 20000 -> (\d+) splats \(cap 20500\), (\d+) rows relocated$", res.stdout, flags=re.M)
    assert m, res.stdout[-600:]
    assert int(m.group(1)) == 20500  # int(1.05 * 20000) = 21000 at step 500, cut to the cap; nothing more at step 600
    bad = subprocess.run([app, "--synth", "0:2000:1001", "--fit", "2", "--density", "adc"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "Invalid density control" in bad.stderr + bad.stdout


def test_fit_with_mcmc_density_control_end_to_end(lcgs, oracle):
    """A 300-splat scene (20 of them dead from the start) fitted to frames of a 2000-splat one under a cap of 600: fit_views,
    the regulariser, adam_step and the noise every step; relocation and growth every 20 steps, 60 steps.  Growth is by half
    (mcmc_num_new(growth=1.5)) so that three rewrites reach the cap.  After each rewrite: rebind, a synchronising frame, derived
    rows consistent, the frame bit-identical to the oracle's render of the downloaded arrays; the count never exceeds the cap
    and reaches it; no row is dead right after a relocation; losses finite.  (No claim about convergence.)"""
    rng = np.random.default_rng(31)
    W, H, CAP = 128, 96, 600
    poses = [([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1]), ([2.5, 1.5, 1.0], [0, 0, 0.5], [0, 0, 1]),
             ([0.5, -3.0, 1.5], [0, 0, 0.5], [0, 0, 1]), ([-1.5, 2.5, 2.0], [0, 0, 0.5], [0, 0, 1])]
    cams = [lcgs.get_lookat_cam(*p, width=W, height=H) for p in poses]
    target_scene = upload_scene(make_scene(rng, 2000, log_scale=(-3.2, 0.5)))
    rt = lcgs.Renderer(lcgs.Context(0))
    rt.bind_scene(*[target_scene[k] for k in KEYS])
    targets = []
    for cam in cams:
        img = torch.zeros(3, H, W, device=DEV)
        rt.forward(cam, img)
        targets.append(img)
    start = make_scene(rng, 300, log_scale=(-2.6, 0.4))
    start["opacity"][::15] = F32(0.001)
    n = 300
    raw0 = {"pos": start["pos"], "scale": np.log(start["scale"]), "rotq": start["rotq"] * F32(1.3), "sh": start["sh"],
            "opacity": _logit(start["opacity"])}
    s = Scene(raw0, cap=CAP, m_fill=0.0, v_fill=0.0, tail=0.0)
    view = lambda d, rows: {k: t[:rows] for k, t in d.items()}
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[view(s.act, n)[k] for k in KEYS])
    grads = {k: torch.zeros_like(t) for k, t in s.raw.items()}
    losses = torch.zeros(1, device=DEV)
    history, counts, relocated_rows = [], [n], 0
    lr = {k: 20 * x for k, x in LR.items()}
    for step in range(1, 61):
        j = step % len(cams)
        r.fit_views([cams[j]], [targets[j]], *[view(grads, n)[k] for k in KEYS], losses)
        r.mcmc_regularize(view(grads, n), lambda_opacity=0.01, lambda_scale=0.01)
        r.adam_step(view(grads, n), view(s.raw, n), view(s.m, n), view(s.v, n), view(s.act, n), step, lr, eps=1e-15)
        r.mcmc_noise(view(s.raw, n), view(s.act, n), lr_pos=LR["pos"], step=step, seed=5)
        history.append(losses.clone())
        if step % 20 == 0:
            dead_before = int((s.act["opacity"][:n] <= MIN_OP).sum())
            moved = r.mcmc_relocate(view(s.raw, n), view(s.m, n), view(s.v, n), view(s.act, n), min_opacity=MIN_OP, seed=step,
                                    src_row=s.src_row[:n])
            r.ctx.synchronize()
            assert moved == dead_before
            relocated_rows += moved
            src = s.src_row[:n].cpu().numpy()
            assert (src >= 0).all() and (src < n).all() and int((src != np.arange(n)).sum()) <= moved
            assert bool((s.act["opacity"][:n] > MIN_OP).all())  # no row is left dead
            num_new = lcgs.mcmc_num_new(n, CAP, growth=1.5)
            r.mcmc_add(n, num_new, *s.packs(), min_opacity=MIN_OP, seed=step, capacity=CAP)
            r.ctx.synchronize()
            print(f"[mcmc e2e] step {step}: {moved} rows relocated, {n} -> {n + num_new} rows")
            n += num_new
            counts.append(n)
            assert 0 < n <= CAP
            act = view(s.act, n)
            r.bind_scene(*[act[k] for k in KEYS])
            img = torch.zeros(3, H, W, device=DEV)
            assert r.forward(cams[0], img, sync=True) is not None  # a synchronising frame
            assert r.verify_derived() == 0
            scene = r.download_scene()
            for k in KEYS:
                assert np.array_equal(scene[k], act[k].cpu().numpy()), k
            assert_image_parity(img.cpu().numpy(), oracle.render(scene, oracle.lookat(*poses[0], width=W, height=H)))
    r.ctx.synchronize()
    hist = torch.cat(history).cpu().numpy()
    assert np.isfinite(hist).all()
    assert counts[-1] == CAP and max(counts) <= CAP, counts
    assert relocated_rows > 0  # the relocation had work to do
    for k in KEYS:
        assert torch.isfinite(s.raw[k][:n]).all(), k
    print(f"[mcmc e2e] counts {counts}; loss {hist[:4].mean():.5f} -> {hist[-4:].mean():.5f}")
