"""`-m gpu`: per-splat blend-weight statistics of a keep-state frame (lcgs_contrib_accumulate), the keep mask and the pruning
rewrite on them (lcgs_contrib_keep_mask, lcgs_prune).

Statistics: weight_max, pixels and views equal tests/contrib_ref.py (the f32 oracle's one-hot composition) bit for bit on every
row; weight_sum within gamma_n x the float64 sum of the same bit-exact terms, n = the row's pixel count, no row excluded -- the
crowd (lists of five rounds, 413 rows that meet across tiles, 461 rows listed but never blended), four random draws with needles
and giants, two views, each member alone, a context-owned scene in spatial order, a frame that draws nothing, the call twice,
with and without a backward behind the frame.
Mask and prune: the numpy predicate on the reference statistics; the rewrite bit for bit against array[keep]; capacity; nothing
kept.  End to end: the crowd pruned by `pixels >= 1` over two views renders both views bit-identically.

The bound on a sum that starts from a value already in the array, or that two calls add to: any summation tree over k
non-negative terms obeys gamma_(k - 1) (Higham, section 4.2); with the header's convention (gamma_n for n terms) a row with n
blended pixels on top of one earlier value is held to gamma_(n + 1) x (value + reference)."""
import numpy as np
import pytest
import torch

import contrib_ref
import luisacomputegaussiansplatting_amd as L
import maps_ref
from gpu_util import BG, DEV, KEYS, cached, dev, random_draw, upload_scene

pytestmark = pytest.mark.gpu
SEEDS = (0, 1, 2, 3)  # 0, 3: anisotropic needles and a few giants that span many tiles
AWAY = ([1.6, 0.3, 0.9], [5.0, 1.0, 1.3], [0.0, 0.0, 1.0])  # the crowd behind the camera
NAMES = ("weight_sum", "weight_max", "pixels", "views")
LR = {"pos": 1.6e-4, "sh_dc": 2.5e-3, "sh_rest": 1.25e-4, "opacity": 5e-2, "scale": 5e-3, "rot": 1e-3}


class Frame:
    """one (scene, pose, resolution, fov, bg, scale modifier) with the oracle's per-row statistics, computed once"""

    def __init__(self, oracle, key, pose=None):
        if key == "crowd":
            self.scene, p, self.W, self.H = maps_ref.crowd()
            self.pose, self.fov, self.bg, self.sm = pose or p, None, BG, 1.0
        else:
            _, self.scene, self.W, self.H, self.pose, self.fov, self.bg, self.sm = random_draw(key)
        self.key, self.P = key, self.scene["pos"].shape[0]
        self.ocam = oracle.lookat(*self.pose, width=self.W, height=self.H, fov=self.fov)
        self.ref = contrib_ref.view_stats(oracle, self.scene, self.ocam, scale_modifier=self.sm)
        self.ref["views"] = (self.ref["pixels"] > 0).astype(np.uint32)

    def cam(self):
        return L.get_lookat_cam(*self.pose, width=self.W, height=self.H, fov=self.fov)

    def renderer(self, owned=False):
        """a fresh context with the scene bound (owned: uploaded, in spatial order) and the frame rendered"""
        r = L.Renderer(L.Context(0))
        if owned:
            r.upload_scene(self.scene)
        else:
            self.d = upload_scene(self.scene)
            r.bind_scene(*[self.d[k] for k in KEYS])
        return r, self.render(r)

    def render(self, r):
        img = torch.full((3, self.H, self.W), -1.0, device=DEV)
        assert r.forward(self.cam(), img, bg=self.bg, scale_modifier=self.sm, keep_state=True, sync=True) > 0, self.key
        return img


def _frame(oracle, key, pose=None):
    return cached(("contrib", key, str(pose)), lambda: Frame(oracle, key, pose))


def _stats(P, fill=None, names=NAMES):
    fill = fill or {}
    return {k: torch.full((P,), fill.get(k, 0), dtype=torch.float32 if k.startswith("weight") else torch.int32, device=DEV)
            for k in names}


def _host(stats):
    return {k: (t.cpu().numpy() if k.startswith("weight") else t.cpu().numpy().view(np.uint32)) for k, t in stats.items()}


def _accumulate(r, stats):
    r.contrib_accumulate(stats)
    r.ctx.synchronize()
    return _host(stats)


def _assert_stats(got, ref, tag, start=None):
    """got against a reference (contrib_ref.view_stats / accumulate) on top of `start` (the arrays' values before the calls)"""
    start = start or {}
    P = ref["pixels"].shape[0]
    for k in got:
        assert got[k].shape == (P,), (tag, k)
    if "pixels" in got:
        want = (np.uint32(start.get("pixels", 0)) + ref["pixels"]).astype(np.uint32)
        assert np.array_equal(got["pixels"], want), f"{tag} pixels: {int((got['pixels'] != want).sum())} of {P} rows differ"
    if "views" in got:
        want = (np.uint32(start.get("views", 0)) + ref["views"]).astype(np.uint32)
        assert np.array_equal(got["views"], want), f"{tag} views: {int((got['views'] != want).sum())} of {P} rows differ"
    if "weight_max" in got:
        want = np.maximum(np.float32(start.get("weight_max", 0)), ref["weight_max"])
        assert got["weight_max"].dtype == want.dtype == np.float32
        assert np.array_equal(got["weight_max"].view(np.uint32), want.view(np.uint32)), (
            f"{tag} weight_max: {int((got['weight_max'] != want).sum())} of {P} rows differ")
    if "weight_sum" in got:
        a = float(start.get("weight_sum", 0))
        want = a + ref["weight_sum"]
        bound = contrib_ref.sum_bound(want, ref["pixels"].astype(np.int64) + (1 if a else 0))
        diff = np.abs(got["weight_sum"].astype(np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
        print(f"[contrib] {tag} weight_sum: worst diff/bound {ratio.max():.3f} (row {int(ratio.argmax())}, "
              f"{int(ref['pixels'][ratio.argmax()])} pixels)")
        assert ratio.max() <= 1.0, f"{tag} weight_sum: {int((ratio > 1).sum())} rows over gamma_n, worst {ratio.max():.2f} x"
        untouched = ref["pixels"] == 0
        assert (got["weight_sum"][untouched] == np.float32(a)).all(), tag  # ... and untouched rows keep their bits


# ---------------------------------------------------------------------------------------------------------------- statistics
SENTINEL = {"weight_sum": 3.5, "weight_max": 0.25, "pixels": 7, "views": 5}


def test_crowd(lcgs, oracle):
    f = _frame(oracle, "crowd")
    listed = np.zeros(f.P, bool)
    listed[f.ref["listed"]] = True
    # a milder scene cannot replace the crowd unnoticed
    assert (listed & (f.ref["pixels"] == 0)).sum() >= 400 and (f.ref["tiles"] >= 2).sum() >= 300
    assert ((f.ref["weight_max"] > 0) & (f.ref["weight_max"] < 0.25)).any() and (f.ref["weight_max"] > 0.25).any()
    r, img = f.renderer()
    _assert_stats(_accumulate(r, _stats(f.P)), f.ref, "crowd")
    # rows the reference leaves alone must be UNTOUCHED, not rewritten with zeros: a second run on arrays that hold other values
    _assert_stats(_accumulate(r, _stats(f.P, SENTINEL)), f.ref, "crowd on sentinels", start=SENTINEL)
    assert np.array_equal(img.cpu().numpy(), oracle.render(f.scene, f.ocam, bg=f.bg)["img"])  # the colour frame is untouched


@pytest.mark.parametrize("seed", SEEDS)
def test_random_draws(lcgs, oracle, seed):
    f = _frame(oracle, seed)
    r, _ = f.renderer()
    _assert_stats(_accumulate(r, _stats(f.P)), f.ref, f"seed {seed}")


def test_two_views_accumulate(lcgs, oracle):
    f0, f1 = _frame(oracle, "crowd"), _frame(oracle, "crowd", contrib_ref.POSE2)
    ref = contrib_ref.accumulate([f0.ref, f1.ref])
    assert (ref["views"] == 2).any() and (ref["views"] == 1).any() and (ref["views"] == 0).any()
    r, _ = f0.renderer()
    stats = _stats(f0.P)
    r.contrib_accumulate(stats)
    f1.render(r)
    _assert_stats(_accumulate(r, stats), ref, "two views")


def test_each_member_alone(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer()
    for k in NAMES:
        got = _accumulate(r, _stats(f.P, names=(k,)))
        assert list(got) == [k]
        _assert_stats(got, f.ref, f"{k} alone")


def test_scene_in_spatial_order(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer(owned=True)  # context-owned, along a Morton curve
    perm = r.permutation()
    assert perm is not None
    perm = perm.cpu().numpy().astype(np.int64)
    assert not np.array_equal(perm, np.arange(f.P))
    got = _accumulate(r, _stats(f.P))
    in_file_order = {}
    for k, a in got.items():  # library row r = file row perm[r]
        in_file_order[k] = np.zeros_like(a)
        in_file_order[k][perm] = a
    _assert_stats(in_file_order, f.ref, "spatial order")


def test_frame_that_draws_nothing(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer()
    img = torch.full((3, f.H, f.W), -1.0, device=DEV)
    assert r.forward(L.get_lookat_cam(*AWAY, width=f.W, height=f.H), img, bg=f.bg, keep_state=True, sync=True) == 0
    got = _accumulate(r, _stats(f.P, SENTINEL))
    for k in NAMES:
        assert (got[k] == got[k].dtype.type(SENTINEL[k])).all(), k


def test_twice_on_one_frame(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer()
    stats = _stats(f.P)
    r.contrib_accumulate(stats)
    got = _accumulate(r, stats)
    twice = {"weight_sum": 2 * f.ref["weight_sum"], "weight_max": f.ref["weight_max"], "pixels": 2 * f.ref["pixels"],
             "views": 2 * f.ref["views"]}
    _assert_stats(got, twice, "twice")


def test_without_and_behind_a_backward(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r, _ = f.renderer()
    _assert_stats(_accumulate(r, _stats(f.P)), f.ref, "no backward")
    g = {k: torch.zeros_like(f.d[k]) for k in KEYS}
    r.backward(torch.randn(3, f.H, f.W, device=DEV), *[g[k] for k in KEYS])
    _assert_stats(_accumulate(r, _stats(f.P)), f.ref, "behind a backward")
    # ... and the backward's rows are not disturbed by the statistics: the same backward again gives the same gradients
    dL = torch.randn(3, f.H, f.W, device=DEV)
    r.backward(dL, *[g[k] for k in KEYS])
    r.contrib_accumulate(_stats(f.P))
    g2 = {k: torch.zeros_like(f.d[k]) for k in KEYS}
    r.backward(dL, *[g2[k] for k in KEYS])
    r.ctx.synchronize()
    assert all(torch.allclose(g[k], g2[k], rtol=1e-3, atol=1e-6) for k in KEYS)


def test_state_and_argument_errors(lcgs, oracle):
    f = _frame(oracle, "crowd")
    r = L.Renderer(L.Context(0))
    d = upload_scene(f.scene)
    r.bind_scene(*[d[k] for k in KEYS])
    stats = _stats(f.P)

    def refused(status, fn, *a, **kw):
        with pytest.raises(L.LcgsError) as e:
            fn(*a, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))

    refused(L.api.LCGS_ERR_STATE, r.contrib_accumulate, stats)  # no frame at all
    img = torch.zeros(3, f.H, f.W, device=DEV)
    r.forward(f.cam(), img, bg=f.bg, keep_state=False, sync=True)
    refused(L.api.LCGS_ERR_STATE, r.contrib_accumulate, stats)  # a frame without kept state
    f.render(r)
    refused(1, r.contrib_accumulate, {})                        # all four members NULL
    refused(1, r.contrib_accumulate, _stats(f.P - 1))           # not the bound scene's row count
    r.contrib_accumulate(stats)
    rows, recs = r.owner_project(0, f.cam(), 0, f.P, keep_state=True)
    r.owner_render(f.cam(), rows, recs, img, bg=f.bg, keep_state=True)
    refused(L.api.LCGS_ERR_STATE, r.contrib_accumulate, stats)  # a frame drawn from received records
    r.ctx.synchronize()
    _assert_stats(_host(stats), f.ref, "after the refusals")    # the refused calls touched nothing


# ------------------------------------------------------------------------------------------------------------ mask and prune
def _two_view_ref(oracle):
    f0, f1 = _frame(oracle, "crowd"), _frame(oracle, "crowd", contrib_ref.POSE2)
    ref = contrib_ref.accumulate([f0.ref, f1.ref])
    return f0, f1, {"weight_sum": ref["weight_sum"].astype(np.float32), "weight_max": ref["weight_max"], "pixels": ref["pixels"],
                    "views": ref["views"]}


def _device_stats(ref):
    return {k: dev(ref[k]) if k.startswith("weight") else dev(ref[k].view(np.int32)) for k in NAMES}


def test_keep_mask(lcgs, oracle):
    f0, _, ref = _two_view_ref(oracle)
    on_a_row = float(np.sort(ref["weight_max"][ref["weight_max"] > 0])[300])  # exactly a row's value: >= keeps that row
    configs = (dict(min_weight_max=0.01), dict(min_weight_max=on_a_row), dict(min_pixels=1, min_views=2),
               dict(min_weight_sum=0.5, min_weight_max=0.05, min_pixels=40, min_views=1))
    r = L.Renderer(L.Context(0))
    stats = _device_stats(ref)
    for cfg in configs:
        keep = torch.full((f0.P,), 9, dtype=torch.uint8, device=DEV)
        r.contrib_keep_mask(stats, keep, **cfg)
        r.ctx.synchronize()
        want = contrib_ref.keep_predicate(ref, **cfg)
        assert 0 < want.sum() < f0.P, cfg
        assert np.array_equal(keep.cpu().numpy(), want.astype(np.uint8)), cfg
    assert contrib_ref.keep_predicate(ref, min_weight_max=on_a_row)[ref["weight_max"] == np.float32(on_a_row)].all()
    # only the members a configuration names are needed; one it names and lacks is refused
    keep = torch.zeros(f0.P, dtype=torch.uint8, device=DEV)
    r.contrib_keep_mask({"pixels": stats["pixels"]}, keep, min_pixels=1)
    r.ctx.synchronize()
    assert np.array_equal(keep.cpu().numpy().astype(bool), ref["pixels"] >= 1)
    with pytest.raises(L.LcgsError) as e:
        r.contrib_keep_mask({"pixels": stats["pixels"]}, keep, min_views=1)
    assert e.value.status == 1


def _trained_source(r, P, seed=0):
    """raw / m / v / activated of P rows as init_from_points and one Adam step leave them (activated by the optimiser's own
    expressions)"""
    rng = np.random.default_rng(seed)
    pos, rgb = dev(rng.normal(0, 0.5, (P, 3)).astype(np.float32)), dev(rng.uniform(0, 1, (P, 3)).astype(np.float32))
    raw, act = r.init_from_points(pos, rgb)
    m, v = ({k: torch.zeros_like(raw[k]) for k in KEYS} for _ in range(2))
    grads = {k: dev(rng.normal(0, 1e-2, tuple(raw[k].shape)).astype(np.float32)) for k in KEYS}
    r.adam_step(grads, raw, m, v, act, step=1, lr=LR)
    r.ctx.synchronize()
    return raw, m, v, act


def _filled(cap, like, fill):
    return {k: torch.full((cap,) + tuple(like[k].shape[1:]), fill, dtype=torch.float32, device=DEV) for k in KEYS}


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_prune(lcgs, oracle):
    f0, _, ref = _two_view_ref(oracle)
    P = f0.P
    r = L.Renderer(L.Context(0))
    raw, m, v, act = _trained_source(r, P)
    stats = _device_stats(ref)
    keep = contrib_ref.keep_predicate(ref, min_weight_max=0.01)
    n_keep = int(keep.sum())
    assert 0 < n_keep < P
    cap = n_keep + 3
    outs = [_filled(cap, raw, fill) for fill in (11.0, 12.0, 13.0, 14.0)]
    src_row = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    n = r.prune(stats, raw, m, v, *outs, src_row=src_row, min_weight_max=0.01)
    r.ctx.synchronize()
    assert n == n_keep
    assert np.array_equal(src_row.cpu().numpy()[:n], np.nonzero(keep)[0]) and (src_row.cpu().numpy()[n:] == -1).all()
    for name, src, out, fill in (("raw", raw, outs[0], 11.0), ("m", m, outs[1], 12.0), ("v", v, outs[2], 13.0),
                                 ("activated", act, outs[3], 14.0)):
        for k in KEYS:
            assert np.array_equal(_bits(out[k])[:n], _bits(src[k])[keep]), (name, k)
            assert (out[k][n:] == fill).all(), (name, k)  # nothing past the new count
    # the source is untouched and activated really is another function of raw
    assert not np.array_equal(_bits(outs[3]["scale"])[:n], _bits(outs[0]["scale"])[:n])

    # one row short: the exact count, and no destination touched
    outs = [_filled(n_keep - 1, raw, fill) for fill in (11.0, 12.0, 13.0, 14.0)]
    src_row.fill_(-1)
    with pytest.raises(L.LcgsError) as e:
        r.prune(stats, raw, m, v, *outs, src_row=src_row, capacity=n_keep - 1, min_weight_max=0.01)
    r.ctx.synchronize()
    assert e.value.status == 5 and e.value.needed == n_keep
    for out, fill in zip(outs, (11.0, 12.0, 13.0, 14.0)):
        assert all(bool((out[k] == fill).all()) for k in KEYS)
    assert bool((src_row == -1).all())

    # every row dropped: 0 rows, LCGS_OK, nothing written
    assert r.prune(stats, raw, m, v, *outs, min_pixels=2 ** 31) == 0
    r.ctx.synchronize()
    assert all(bool((outs[0][k] == 11.0).all()) for k in KEYS)
    # nothing enabled: every row kept, in order
    outs = [_filled(P, raw, fill) for fill in (11.0, 12.0, 13.0, 14.0)]
    assert r.prune({}, raw, m, v, *outs) == P
    r.ctx.synchronize()
    assert all(np.array_equal(_bits(outs[0][k]), _bits(raw[k])) for k in KEYS)


def test_pruned_scene_renders_the_same_images(lcgs, oracle):
    """End to end: accumulate the crowd's two views, drop the rows no pixel blended, bind what is left, render both views again."""
    f0, f1, ref = _two_view_ref(oracle)
    r, img0 = f0.renderer()
    stats = _stats(f0.P)
    r.contrib_accumulate(stats)
    img1 = f1.render(r)
    r.contrib_accumulate(stats)
    # the scene's own (activated) arrays go through the rewrite as `raw`: out_raw holds its kept rows bit for bit
    zeros = {k: torch.zeros_like(f0.d[k]) for k in KEYS}
    outs = [_filled(f0.P, f0.d, 0.0) for _ in range(4)]
    n = r.prune(stats, f0.d, zeros, zeros, *outs, min_pixels=1)
    want = contrib_ref.keep_predicate(ref, min_pixels=1)
    assert n == int(want.sum()) and 0 < n < f0.P
    pruned = {k: outs[0][k][:n].contiguous() for k in KEYS}
    assert all(np.array_equal(_bits(pruned[k]), _bits(f0.d[k])[want]) for k in KEYS)
    r2 = L.Renderer(L.Context(0))
    r2.bind_scene(*[pruned[k] for k in KEYS])
    for f, full in ((f0, img0), (f1, img1)):
        assert np.array_equal(f.render(r2).cpu().numpy(), full.cpu().numpy()), f.pose
