"""`-m gpu`: adaptive density control (lcgs_densify_accumulate, lcgs_densify, lcgs_opacity_reset) -- the
statistics against the oracles, the rewrite against a NumPy model written here (float32 decisions, float64 child positions),
the built-in sampler's determinism and moments, the opacity reset, and a short end-to-end fit with a changing splat count."""
import numpy as np
import pytest
import torch

from conftest import make_scene
from gpu_util import DEV, GRAD_ROW_CU, GRAD_ROW_K, U32, _oracles, assert_image_parity, upload_scene

pytestmark = pytest.mark.gpu

KEYS = ("pos", "scale", "rotq", "sh", "opacity")
LR = {"pos": 1.6e-4, "sh_dc": 2.5e-3, "sh_rest": 1.25e-4, "opacity": 5e-2, "scale": 5e-3, "rot": 1e-3}
F32 = np.float32
LN_1_6 = F32(np.log(np.float64(F32(1.6))))  # the kernel's ln 1.6: the double value rounded once to binary32


def _activate(raw):
    return {"pos": raw["pos"], "scale": torch.exp(raw["scale"]),
            "rotq": raw["rotq"] / raw["rotq"].norm(dim=1, keepdim=True), "sh": raw["sh"],
            "opacity": torch.sigmoid(raw["opacity"])}


def _new_stats(P):
    return {"grad_accum": torch.zeros(P, dtype=torch.float32, device=DEV), "denom": torch.zeros(P, dtype=torch.int32, device=DEV),
            "max_radii": torch.zeros(P, dtype=torch.int32, device=DEV)}


def _alloc(cap, feat, fill=0.0):
    shapes = {"pos": (cap, 3), "scale": (cap, 3), "rotq": (cap, 4), "sh": (cap, feat), "opacity": (cap,)}
    return {k: torch.full(shapes[k], fill, dtype=torch.float32, device=DEV) for k in KEYS}


# ------------------------------------------------------------------------------------------------------------ 1. statistics
POSES = [([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1]), ([2.5, 1.5, 1.0], [0, 0, 0.5], [0, 0, 1]), ([0.5, -3.0, 1.5], [0, 0, 0.5], [0, 0, 1])]


@pytest.mark.parametrize("owned", [False, True])
def test_statistics_against_the_oracles(lcgs, owned):
    """denom (views in which the row was on screen) / max_radii (largest oracle radius over those views) exactly, grad_accum row by row within the bound built from check_gradient_rows' ingredients on the two
    mean components: per view K |f32 oracle - f64 oracle| + c_u u A (A: the walk's rounding budget), times (W/2, H/2), summed
    over the views (|norm a - norm b| <= |a_x - b_x| + |a_y - b_y|).  owned: a Morton-ordered context-owned scene, rows mapped
    through permutation().  Measured worst diff/bound on the MI355X: 0.003 (docs/TESTS.md)."""
    o32, o64, _ = _oracles()
    rng = np.random.default_rng(3)
    P, W, H = 4000, 128, 96
    scene = make_scene(rng, P)
    scene["pos"][:1500] += 100.0  # far outside the frustum: never on screen
    r = lcgs.Renderer(lcgs.Context(0))
    if owned:
        r.upload_scene(scene)
        perm = r.permutation()
        assert perm is not None
        perm = perm.cpu().numpy().astype(np.int64)
    else:
        d = upload_scene(scene)
        r.bind_scene(*[d[k] for k in KEYS])
        perm = np.arange(P)
    stats = _new_stats(P)
    g = {k: torch.zeros_like(t) for k, t in upload_scene(scene).items()}
    want = np.zeros(P, np.float64)
    bound = np.zeros(P, np.float64)
    want_denom = np.zeros(P, np.int64)
    want_radii = np.zeros(P, np.int64)
    on_screen = np.zeros(P, bool)
    for j, pose in enumerate(POSES):
        cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
        dL = torch.from_numpy(np.random.default_rng(100 + j).normal(size=(3, H, W)).astype(F32)).to(DEV)
        img = torch.zeros(3, H, W, device=DEV)
        radii = torch.zeros(P, dtype=torch.int32, device=DEV)
        r.forward(cam, img, radii=radii, keep_state=True)
        r.backward(dL, *[g[k] for k in KEYS])
        r.densify_accumulate(stats)
        r.ctx.synchronize()
        rows = perm[r.visible_rows().cpu().numpy().astype(np.int64)]  # file rows of this frame's on-screen rows
        on_screen[rows] = True
        ocam = o32.lookat(*pose, width=W, height=H)
        gm = {}
        for name, o in (("f32", o32), ("f64", o64)):
            st = o.forward_state(scene, o.convert_camera(ocam))
            gm[name] = o.render_backward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"], st["opacity"],
                                         st["color"], st["final_T"], st["n_contrib"], dL.cpu().numpy())[0].astype(np.float64)
            if name == "f32":
                st32 = st
        A, _ = o64.render_backward_bound(W, H, np.zeros(3, F32), st32["ranges"], st32["point_list"], st32["means"], st32["conic"],
                                         st32["opacity"], st32["color"], st32["final_T"], st32["n_contrib"], dL.cpu().numpy())
        half = np.array([W / 2, H / 2])
        want += np.sqrt(((gm["f32"] * half) ** 2).sum(axis=1))
        bound += ((GRAD_ROW_K * np.abs(gm["f32"] - gm["f64"]) + GRAD_ROW_CU * U32 * A[:, 0:2]) * half).sum(axis=1)
        rad = st32["radii"].astype(np.int64)
        assert np.array_equal(rad, radii.cpu().numpy()[np.argsort(perm)] if owned else radii.cpu().numpy())
        # "on screen": the reference's radii are defined for splats that touch no tile too (the 1500 rows pushed out of the
        # frustum have radii > 0 in two of the views), so `radii > 0` alone is not it.  A row counts in a view when it is one
        # of the frame's on-screen rows; held against the oracle: every such row is in the oracle's pair lists with a
        # radius > 0, and every row of the oracle's lists that is NOT one (its opacity-pruned rect is empty) has exactly zero
        # 2-D mean gradients in the oracle's own backward -- it could not have contributed to grad_accum either way.
        vis, listed = np.zeros(P, bool), np.zeros(P, bool)
        vis[rows] = True
        listed[np.unique(st32["point_list"]).astype(np.int64)] = True
        assert (listed[vis]).all() and (rad[vis] > 0).all() and (rad[listed] > 0).all()
        assert (gm["f32"][listed & ~vis] == 0).all()
        print(f"[densify stats] owned={owned} view {j}: {int(vis.sum())} on-screen rows, {int((listed & ~vis).sum())} listed rows "
              f"with an empty pruned rect, {int(((rad > 0) & ~listed).sum())} rows with radii > 0 that touch no tile")
        want_denom += vis
        want_radii = np.maximum(want_radii, np.where(vis, rad, 0))
    got = {k: np.zeros(P, t.cpu().numpy().dtype) for k, t in stats.items()}
    for k, t in stats.items():
        got[k][perm] = t.cpu().numpy()  # library row r = file row perm[r]
    assert 0 < on_screen.sum() < P and not on_screen[:1500].any()
    print(f"[densify stats] owned={owned}: {int(on_screen.sum())} rows on some screen; denom mismatches "
          f"{int((want_denom != got['denom']).sum())}, max_radii mismatches {int((want_radii != got['max_radii']).sum())}")
    assert np.array_equal(got["denom"], want_denom)
    assert np.array_equal(got["max_radii"], want_radii)
    for k in got:
        assert (got[k][~on_screen] == 0).all(), k  # untouched rows are exactly zero
    diff = np.abs(got["grad_accum"].astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    print(f"[densify stats] owned={owned}: grad_accum worst diff/bound {ratio.max():.3f} (row {int(ratio.argmax())})")
    assert ratio.max() <= 1.0, (int(ratio.argmax()), float(ratio.max()), int((ratio > 1).sum()))
    assert (got["grad_accum"][on_screen] > 0).mean() > 0.5


# ------------------------------------------------------------------------------------------------------------ 2. state errors
def test_accumulate_needs_a_keep_state_frame_and_its_backward(lcgs):
    rng = np.random.default_rng(4)
    P, W, H = 500, 64, 48
    d = upload_scene(make_scene(rng, P))
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[d[k] for k in KEYS])
    stats = _new_stats(P)
    cam = lcgs.get_lookat_cam([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1], width=W, height=H)
    img = torch.zeros(3, H, W, device=DEV)
    with pytest.raises(lcgs.LcgsError) as e:
        r.densify_accumulate(stats)  # no frame at all
    assert e.value.status == 8
    r.forward(cam, img, keep_state=True)
    with pytest.raises(lcgs.LcgsError) as e:
        r.densify_accumulate(stats)  # a keep-state frame, but no backward yet
    assert e.value.status == 8
    g = {k: torch.zeros_like(d[k]) for k in KEYS}
    r.backward(torch.randn(3, H, W, device=DEV), *[g[k] for k in KEYS])
    r.densify_accumulate(stats)  # now it is fine
    r.forward(cam, img, keep_state=False)
    with pytest.raises(lcgs.LcgsError) as e:
        r.densify_accumulate(stats)  # the last frame kept no state
    assert e.value.status == 8
    r.ctx.synchronize()
    assert int(stats["denom"].sum()) > 0 and int(stats["denom"].max()) == 1


# ------------------------------------------------------------------------------------------------------------ 3. the rewrite
CFG = dict(grad_threshold=2e-4, percent_dense=0.01, scene_extent=4.0, min_opacity=0.005, max_screen_size=20)
REL = 1e-3  # no row's avg / smax / op may lie within this (relative) of a threshold: asserted


def _raw_scene(rng, P, feat):
    return {"pos": rng.normal(0, 1, (P, 3)).astype(F32), "scale": rng.normal(-4, 1, (P, 3)).astype(F32),
            "rotq": rng.normal(0, 1, (P, 4)).astype(F32), "sh": rng.normal(0, 0.3, (P, feat)).astype(F32),
            "opacity": rng.normal(0, 2, P).astype(F32)}


def _handmade(rng, P, feat, probs=None):
    """raw / m / v and statistics that give every action: ~10 % clone, ~10 % split, ~10 % pruned (a third by each reason, with
    the other criteria random: prune wins), ~5 % rows with denom = 0 and a large grad_accum."""
    raw = _raw_scene(rng, P, feat)
    m = {k: rng.normal(0, 1e-3, a.shape).astype(F32) for k, a in raw.items()}
    v = {k: (rng.normal(0, 1e-3, a.shape) ** 2).astype(F32) for k, a in raw.items()}
    cat = rng.choice(7, P, p=probs or [0.65, 0.10, 0.10, 0.034, 0.033, 0.033, 0.05])
    # 0 keep, 1 clone, 2 split, 3 prune by opacity, 4 by radius, 5 by extent, 6 never seen (denom 0)
    hot = np.where(cat == 1, True, np.where(cat == 2, True, np.where(cat == 0, False, rng.random(P) < 0.5)))
    big = np.where(cat == 1, False, np.where(cat == 2, True, rng.random(P) < 0.5))
    dense = F32(CFG["percent_dense"]) * F32(CFG["scene_extent"])
    huge = F32(0.1) * F32(CFG["scene_extent"])
    smax = np.where(cat == 5, rng.uniform(1.2 * huge, 3 * huge, P),
                    np.where(big, rng.uniform(1.3 * dense, 0.7 * huge, P), rng.uniform(0.1 * dense, 0.75 * dense, P)))
    axis = rng.integers(0, 3, P)
    scale = np.log(smax)[:, None] - rng.uniform(0.1, 2.0, (P, 3))
    scale[np.arange(P), axis] = np.log(smax)
    raw["scale"] = scale.astype(F32)
    op = np.where(cat == 3, rng.uniform(0.1, 0.8, P) * CFG["min_opacity"], rng.uniform(0.02, 0.98, P))
    raw["opacity"] = np.log(op / (1 - op)).astype(F32)
    denom = np.where(cat == 6, 0, rng.integers(1, 60, P)).astype(np.int32)
    avg = np.where(hot, rng.uniform(1.5, 10, P), rng.uniform(0, 0.7, P)) * CFG["grad_threshold"]
    grad_accum = np.where(denom > 0, avg * denom, 1.0).astype(F32)
    radii = np.where(cat == 4, rng.integers(CFG["max_screen_size"] + 1, 200, P), rng.integers(0, CFG["max_screen_size"] + 1, P))
    stats = {"grad_accum": grad_accum, "denom": denom, "max_radii": radii.astype(np.int32)}
    noise = rng.normal(0, 1, (P, 2, 3)).astype(F32)
    return raw, m, v, stats, noise


def _rot(q):
    """float64 rotation matrices of stored (r, x, y, z) quaternions, normalised"""
    q = q.astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w], -1),
                     np.stack([2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w], -1),
                     np.stack([2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y], -1)], 1)


def _model(raw, m, v, stats, noise, cfg=CFG):
    """The rewrite in NumPy: float32 for the decisions (every row asserted clear of its thresholds), float64 child positions.
    -> (actions, src_row, first-of-its-parent mask, out_raw, out_m, out_v, child position bound)."""
    P = raw["opacity"].shape[0]
    den = stats["denom"].astype(np.int64)
    avg = np.where(den > 0, stats["grad_accum"] / np.maximum(den, 1).astype(F32), F32(0)).astype(F32)
    smax = np.exp(raw["scale"]).max(axis=1).astype(F32)
    op = (F32(1) / (F32(1) + np.exp(-raw["opacity"]))).astype(F32)
    thr, dense = F32(cfg["grad_threshold"]), F32(cfg["percent_dense"]) * F32(cfg["scene_extent"])
    huge, min_op, mss = F32(0.1) * F32(cfg["scene_extent"]), F32(cfg["min_opacity"]), int(cfg["max_screen_size"])
    clear = lambda x, t: (np.abs(x.astype(np.float64) - float(t)) > REL * float(t)).all()
    assert clear(avg, thr) and clear(smax, dense) and clear(op, min_op) and (mss == 0 or clear(smax, huge))
    hot, big = avg >= thr, smax > dense
    prune = (op < min_op) | ((mss > 0) & ((stats["max_radii"] > mss) | (smax > huge)))
    action = np.where(prune, 0, np.where(~hot, 1, np.where(big, 3, 2)))
    emit = np.where(action >= 2, 2, action)
    src = np.repeat(np.arange(P), emit)
    first = np.concatenate([[True], src[1:] != src[:-1]]) if src.size else np.zeros(0, bool)
    a = action[src]
    out_raw = {k: raw[k][src].copy() for k in KEYS}
    out_raw["scale"][a == 3] = (raw["scale"][src] - LN_1_6)[a == 3]
    keep_moments = (a == 1) | ((a == 2) & first)
    out_m = {k: np.where(keep_moments.reshape((-1,) + (1,) * (m[k].ndim - 1)), m[k][src], F32(0)) for k in KEYS}
    out_v = {k: np.where(keep_moments.reshape((-1,) + (1,) * (v[k].ndim - 1)), v[k][src], F32(0)) for k in KEYS}
    # children: pos + R(q / |q|) (s * n_k) in float64; bound 16 u (|pos| + sum_j |R_ij| s_j |n_j|) per component
    kid = np.where(first, 0, 1)
    R = _rot(raw["rotq"][src])
    sn = np.exp(raw["scale"][src].astype(np.float64)) * noise[src, kid].astype(np.float64)
    child = raw["pos"][src].astype(np.float64) + np.einsum("nij,nj->ni", R, sn)
    cbound = 16 * U32 * (np.abs(raw["pos"][src].astype(np.float64)) + np.einsum("nij,nj->ni", np.abs(R), np.abs(sn)))
    pos64 = np.where((a == 3)[:, None], child, raw["pos"][src].astype(np.float64))
    return action, src, first, out_raw, out_m, out_v, pos64, np.where((a == 3)[:, None], cbound, 0.0)


def _run(lcgs, raw, m, v, stats, noise, cap, deg, cfg=CFG, seed=0, sentinel=None, alias=True):
    feat = raw["sh"].shape[1]
    t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for k, a in d.items()}
    d_raw, d_m, d_v, d_stats = t(raw), t(m), t(v), t(stats)
    fill = 0.0 if sentinel is None else sentinel
    o_raw, o_m, o_v, o_act = (_alloc(cap, feat, fill) for _ in range(4))
    if alias:
        o_act["pos"], o_act["sh"] = o_raw["pos"], o_raw["sh"]
    o_stats = {"grad_accum": torch.full((cap,), 7.0, device=DEV), "denom": torch.full((cap,), 7, dtype=torch.int32, device=DEV),
               "max_radii": torch.full((cap,), 7, dtype=torch.int32, device=DEV)}
    src_row = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    r = lcgs.Renderer(lcgs.Context(0))
    out = dict(raw=o_raw, m=o_m, v=o_v, act=o_act, stats=o_stats, src_row=src_row)
    try:
        n = r.densify(d_stats, d_raw, d_m, d_v, o_raw, o_m, o_v, o_act, o_stats, noise=None if noise is None else t({"n": noise})["n"],
                      src_row=src_row, sh_degree=deg, seed=seed, **cfg)
    except lcgs.LcgsError as e:
        r.ctx.synchronize()
        return e, out
    r.ctx.synchronize()
    return n, out


def _cpu(d):
    return {k: a.cpu().numpy() for k, a in d.items()}


def _check_activated(out_raw, out_act, n):
    ref = _activate({k: torch.from_numpy(a[:n].astype(np.float64)) for k, a in out_raw.items()})
    for k in KEYS:
        a, b = out_act[k][:n].astype(np.float64), ref[k].numpy()
        assert np.allclose(a, b, rtol=2e-5, atol=2e-6), ("activated " + k, np.abs(a - b).max())


@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("P", [1, 257, 20011])
def test_rewrite_matches_the_numpy_model(lcgs, P, deg):
    rng = np.random.default_rng(1000 * deg + P)
    feat = (deg + 1) ** 2 * 3
    raw, m, v, stats, noise = _handmade(rng, P, feat)
    action, src, first, w_raw, w_m, w_v, pos64, cbound = _model(raw, m, v, stats, noise)
    if P >= 257:
        assert all((action == a).sum() > 0 for a in range(4))
    cap = 2 * P + 5
    n, out = _run(lcgs, raw, m, v, stats, noise, cap, deg, alias=(deg == 3))
    assert n == src.size, (n, src.size)
    assert np.array_equal(out["src_row"].cpu().numpy()[:n], src)
    assert (out["src_row"].cpu().numpy()[n:] == -1).all()
    g_raw, g_m, g_v, g_act = (_cpu(out[k]) for k in ("raw", "m", "v", "act"))
    split = action[src] == 3
    for k in KEYS:
        rows = ~split if k == "pos" else np.ones(n, bool)
        assert np.array_equal(g_raw[k][:n][rows].view(np.uint32), w_raw[k][rows].view(np.uint32)), k  # bit for bit
        assert np.array_equal(g_m[k][:n].view(np.uint32), w_m[k].view(np.uint32)), "m " + k
        assert np.array_equal(g_v[k][:n].view(np.uint32), w_v[k].view(np.uint32)), "v " + k
        for g in (g_raw, g_m, g_v):
            assert (g[k][n:] == 0).all(), k  # nothing behind the new count
    for k, t in out["stats"].items():
        assert (t.cpu().numpy()[:n] == 0).all() and (t.cpu().numpy()[n:] == 7).all(), k
    _check_activated(g_raw, g_act, n)
    if split.any():
        diff = np.abs(g_raw["pos"][:n].astype(np.float64) - pos64)[split]
        ratio = (diff / cbound[split]).max()
        print(f"[densify rewrite] P={P} deg={deg}: {int(split.sum())} children, worst position diff/bound {ratio:.3f}; "
              f"actions {np.bincount(action, minlength=4).tolist()}")
        assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------------------------------------------ 4. edges
def test_rewrite_edges(lcgs):
    rng = np.random.default_rng(9)
    P, feat = 3001, 48
    # all pruned
    raw, m, v, stats, noise = _handmade(rng, P, feat, probs=[0, 0, 0, 1, 0, 0, 0])
    n, out = _run(lcgs, raw, m, v, stats, noise, P, 3, sentinel=5.0)
    assert n == 0 and all((out["raw"][k] == 5.0).all() for k in KEYS)
    # nothing hot, nothing pruned: the identity, bit for bit
    raw, m, v, stats, noise = _handmade(rng, P, feat, probs=[0.9, 0, 0, 0, 0, 0, 0.1])
    n, out = _run(lcgs, raw, m, v, stats, noise, P, 3)
    assert n == P and np.array_equal(out["src_row"].cpu().numpy(), np.arange(P))
    for name, want in (("raw", raw), ("m", m), ("v", v)):
        for k in KEYS:
            assert np.array_equal(out[name][k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), (name, k)
    # capacity: one short -> status 5 with the needed count and untouched destinations; exactly enough -> fine
    raw, m, v, stats, noise = _handmade(rng, P, feat)
    need = _model(raw, m, v, stats, noise)[1].size
    assert need != P
    e, out = _run(lcgs, raw, m, v, stats, noise, need - 1, 3, sentinel=5.0, alias=False)
    assert isinstance(e, lcgs.LcgsError) and e.status == 5 and e.needed == need
    for name in ("raw", "m", "v", "act"):
        assert all((out[name][k] == 5.0).all() for k in KEYS), name
    assert all((t == 7).all() for t in out["stats"].values()) and (out["src_row"] == -1).all()
    n, out = _run(lcgs, raw, m, v, stats, noise, need, 3)
    assert n == need
    # P = 0
    empty = {k: a[:0] for k, a in raw.items()}
    n, _ = _run(lcgs, empty, empty, empty, {k: a[:0] for k, a in stats.items()}, noise[:0], 4, 3)
    assert n == 0


# ------------------------------------------------------------------------------------------------------------ 5. the sampler
def test_built_in_sampler(lcgs):
    rng = np.random.default_rng(10)
    P, feat = 100_000, 3
    raw, m, v, stats, _ = _handmade(rng, P, feat, probs=[0, 0, 1, 0, 0, 0, 0])  # every row splits
    runs = {}
    for name, seed, rows in (("a", 11, P), ("b", 11, P), ("c", 12, P), ("prefix", 11, 1000)):
        cut = lambda d: {k: a[:rows] for k, a in d.items()}
        n, out = _run(lcgs, cut(raw), cut(m), cut(v), cut(stats), None, 2 * rows, 0, seed=seed)
        assert n == 2 * rows
        runs[name] = out["raw"]["pos"].cpu().numpy()
    assert np.array_equal(runs["a"], runs["b"])  # same seed: the same children
    assert not np.array_equal(runs["a"], runs["c"])  # another seed: others
    assert np.array_equal(runs["a"][:2000], runs["prefix"])  # a row's children do not depend on P
    # back through R^T and 1 / s: standard normals
    R = _rot(raw["rotq"])
    s = np.exp(raw["scale"].astype(np.float64))
    kids = runs["a"].astype(np.float64).reshape(P, 2, 3) - raw["pos"].astype(np.float64)[:, None, :]
    z = np.einsum("nji,nkj->nki", R, kids) / s[:, None, :]  # [P, child, axis]
    n_samples = 2 * P
    mean, var = z.reshape(-1, 3).mean(axis=0), z.reshape(-1, 3).var(axis=0)
    corr = (z[:, 0, :] * z[:, 1, :]).mean(axis=0)
    print(f"[densify sampler] mean {mean}, var {var}, child correlation {corr}")
    assert (np.abs(mean) <= 5 / np.sqrt(n_samples)).all(), mean
    assert (np.abs(var - 1) <= 5 * np.sqrt(2 / n_samples)).all(), var
    assert (np.abs(corr) <= 5 / np.sqrt(P)).all(), corr


# ------------------------------------------------------------------------------------------------------------ 6. opacity reset
def test_opacity_reset(lcgs):
    rng = np.random.default_rng(12)
    P = 20011
    raw = _raw_scene(rng, P, 48)
    t = lambda d: {k: torch.from_numpy(a.copy()).to(DEV) for k, a in d.items()}
    d_raw = t(raw)
    d_m = {k: torch.full_like(x, 3.0) for k, x in d_raw.items()}
    d_v = {k: torch.full_like(x, 4.0) for k, x in d_raw.items()}
    d_act = {k: x.clone() for k, x in _activate(d_raw).items()}
    before_act = {k: x.clone() for k, x in d_act.items()}
    r = lcgs.Renderer(lcgs.Context(0))
    r.opacity_reset(d_raw, d_m, d_v, d_act, max_opacity=0.01)
    r.ctx.synchronize()
    mo = np.float64(F32(0.01))
    ceiling = F32(np.log(mo / (1.0 - mo)))  # logit(max_opacity): the double value rounded once to binary32
    want = np.minimum(raw["opacity"], ceiling)
    assert (raw["opacity"] > ceiling).any() and (raw["opacity"] < ceiling).any()
    assert np.array_equal(d_raw["opacity"].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (d_m["opacity"] == 0).all() and (d_v["opacity"] == 0).all()
    for k in ("pos", "scale", "rotq", "sh"):
        assert torch.equal(d_raw[k].cpu(), torch.from_numpy(raw[k])) and (d_m[k] == 3.0).all() and (d_v[k] == 4.0).all(), k
        assert torch.equal(d_act[k], before_act[k]), k
    a, b = d_act["opacity"].cpu().numpy().astype(np.float64), 1 / (1 + np.exp(-want.astype(np.float64)))
    assert np.allclose(a, b, rtol=2e-5, atol=2e-6), np.abs(a - b).max()
    assert a.max() <= 0.01 * (1 + 1e-5)
    # only the opacity entries are needed
    only = lambda d: {"opacity": d["opacity"]}
    r.opacity_reset(only(d_raw), only(d_m), only(d_v), only(d_act), max_opacity=0.005)
    r.ctx.synchronize()
    assert float(d_act["opacity"].max()) <= 0.005 * (1 + 1e-5)


# ------------------------------------------------------------------------------------------------------------ 7. end to end
def test_fit_with_density_control_end_to_end(lcgs, oracle):
    """A 300-splat scene fitted to frames of a 2000-splat one: fit_views + adam_step with densify_accumulate every step and
    densify every 20 steps, 60 steps.  After each rewrite: rebind, a synchronising frame, derived rows consistent, the frame
    bit-identical to the oracle's render of the downloaded arrays, the count as d_src_row says; losses finite throughout.
    (No claim about convergence speed.)"""
    rng = np.random.default_rng(21)
    W, H, CAP = 128, 96, 4000
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
    n = 300
    sets = []
    for _ in range(2):  # two sets of arrays: the rewrite ping-pongs between them
        raw, m, v, act = (_alloc(CAP, 48) for _ in range(4))
        act["pos"], act["sh"] = raw["pos"], raw["sh"]
        sets.append(dict(raw=raw, m=m, v=v, act=act, stats=_new_stats(CAP)))
    cur = 0
    s0 = sets[0]
    s0["raw"]["pos"][:n] = torch.from_numpy(start["pos"]).to(DEV)
    s0["raw"]["scale"][:n] = torch.log(torch.from_numpy(start["scale"]).to(DEV))
    s0["raw"]["rotq"][:n] = torch.from_numpy(start["rotq"] * 1.3).to(DEV)
    s0["raw"]["sh"][:n] = torch.from_numpy(start["sh"]).to(DEV)
    s0["raw"]["opacity"][:n] = torch.logit(torch.from_numpy(start["opacity"]).to(DEV))
    for k in ("scale", "rotq", "opacity"):
        s0["act"][k][:n] = _activate({kk: s0["raw"][kk][:n] for kk in KEYS})[k]
    view = lambda d, rows: {k: t[:rows] for k, t in d.items()}
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[view(s0["act"], n)[k] for k in KEYS])
    grads = _alloc(CAP, 48)
    losses = torch.zeros(1, device=DEV)
    src_row = torch.zeros(CAP, dtype=torch.int32, device=DEV)
    history, counts = [], [n]
    lr = {k: 20 * x for k, x in LR.items()}
    for step in range(1, 61):
        s = sets[cur]
        j = step % len(cams)
        r.fit_views([cams[j]], [targets[j]], *[view(grads, n)[k] for k in KEYS], losses)
        r.densify_accumulate(view(s["stats"], n))
        r.adam_step(view(grads, n), view(s["raw"], n), view(s["m"], n), view(s["v"], n), view(s["act"], n), step, lr, eps=1e-15)
        history.append(losses.clone())
        if step % 20 == 0:
            o = sets[cur ^ 1]
            new_n = r.densify(view(s["stats"], n), view(s["raw"], n), view(s["m"], n), view(s["v"], n), o["raw"], o["m"], o["v"],
                              o["act"], o["stats"], grad_threshold=2e-4, percent_dense=0.01, scene_extent=3.0, min_opacity=0.005,
                              max_screen_size=64, seed=step, src_row=src_row)
            r.ctx.synchronize()
            src = src_row.cpu().numpy()[:new_n]
            uses = np.bincount(src, minlength=n)
            assert new_n == uses.sum() and uses.max() <= 2 and (np.diff(src) >= 0).all() and src.max() < n
            den = s["stats"]["denom"][:n].cpu().numpy()
            print(f"[densify e2e] step {step}: {n} -> {new_n} rows ({int((uses == 0).sum())} pruned, {int((uses == 2).sum())} "
                  f"cloned or split; {int((den > 0).sum())} rows seen)")
            assert int(o["stats"]["denom"][:new_n].sum()) == 0
            n, cur = new_n, cur ^ 1
            counts.append(n)
            assert 0 < n <= CAP
            act = view(o["act"], n)
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
    for k in KEYS:
        assert torch.isfinite(sets[cur]["raw"][k][:n]).all(), k
    print(f"[densify e2e] counts {counts}; loss {hist[:4].mean():.5f} -> {hist[-4:].mean():.5f}")
