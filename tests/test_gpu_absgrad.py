"""`-m gpu`: the AbsGS densification statistic (lcgs_absgrad_accumulate, kernels/absgrad.hip) against the reference
composed from the unchanged oracle (tests/absgrad_ref.py).  Every comparison is |kernel - f64 reference| / B <= 1 on every
component of every row, B the per-row bound of absgrad_ref.reference -- which the signed statistic and the one that takes the
absolute value per tile both miss on nearly every row (tests/test_absgrad_ref.py) -- and rows never on screen stay exactly as they
were.  Measured worst ratios on the MI355X are in docs/TESTS.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import absgrad_ref as R
import antialias_ref
from conftest import make_scene
from gpu_util import DEV, KEYS, _oracles, cached, upload_scene

pytestmark = pytest.mark.gpu
F32 = np.float32
SEVEN = 7.0


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _renderer(lcgs, scene, owned=False, raster=None):
    """(renderer, perm: library row r = file row perm[r], what must stay alive)"""
    r = lcgs.Renderer(lcgs.Context(0))
    if raster:
        r.set_raster_mode(raster)
    P = scene["pos"].shape[0]
    if owned:
        r.upload_scene(scene)
        perm = r.permutation()
        assert perm is not None
        return r, perm.cpu().numpy().astype(np.int64), None
    d = upload_scene(scene)
    r.bind_scene(*[d[k] for k in KEYS])
    return r, np.arange(P), d


def _frame(lcgs, r, W, H, pose=R.POSE, bg=R.BG):
    img = torch.zeros(3, H, W, device=DEV)
    r.forward(lcgs.get_lookat_cam(*pose, width=W, height=H), img, bg=bg, keep_state=True)
    return img


def _reference(tag, scene, W, H, di, dd, da, mode="z", pose=R.POSE, frame=R.Classic):
    def make():
        o32 = _oracles()[0]
        return R.reference(scene, o32.lookat(*pose, width=W, height=H), di, dd, da, mode=mode, bg=R.BG, frame=frame)

    return cached(("gpu_absgrad", tag), make)


def _file_rows(t, perm):
    a = t.cpu().numpy()
    out = np.zeros_like(a)
    out[perm] = a
    return out


def _check(tag, r, perm, ref, di, dd, da, mode="z"):
    """one call into zeros held to the bound, one into sevens: rows not on screen keep their bits"""
    P = perm.size
    out = torch.zeros(P, 2, device=DEV)
    mark = torch.full((P, 2), SEVEN, device=DEV)
    r.absgrad_accumulate(_t(di), _t(dd), _t(da), mode=mode, absgrad=out)
    r.absgrad_accumulate(_t(di), _t(dd), _t(da), mode=mode, absgrad=mark)
    r.ctx.synchronize()
    on = np.zeros(P, bool)
    on[perm[r.visible_rows().cpu().numpy().astype(np.int64)]] = True
    got, marked = _file_rows(out, perm), _file_rows(mark, perm)
    ratio = R.ratios(got, ref)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"[absgrad] {tag}: worst diff/B {ratio.max():.3f} (row {i[0]}, component {i[1]}); {int(on.sum())} of {P} rows on screen, "
          f"{int((ref['abs64'] > 0).any(axis=1).sum())} with a gradient")
    assert ratio.max() <= 1.0, (tag, i, float(ratio.max()), int((ratio > 1).sum()))
    assert (got[~on] == 0).all() and (marked[~on] == F32(SEVEN)).all()  # untouched, bit for bit
    assert not (ref["abs64"][~on] > 0).any()
    assert (marked[on] >= F32(SEVEN)).all() and (got >= 0).all()
    assert ((got > 0).any(axis=1) == (ref["abs64"] > 0).any(axis=1)).mean() > 0.98
    return got


# ------------------------------------------------------------------------------------------------ 1. colour only, two rounds
@pytest.mark.parametrize("owned", [False, True])
def test_colour_only_two_rounds(lcgs, owned):
    """24 x 20 (partial tiles in x and y), P = 300, every splat on one tile's list: the walk takes two rounds.  owned: a
    Morton-ordered context-owned scene, rows mapped through permutation()."""
    W, H = 24, 20
    scene = R.scene300()
    di, _, _ = R.gradients(W, H, 11, depth=False, alpha=False)
    ref = _reference("colour_24x20", scene, W, H, di, None, None)
    r, perm, keep = _renderer(lcgs, scene, owned)
    _frame(lcgs, r, W, H)
    nc = torch.zeros(H * W, dtype=torch.int32, device=DEV)
    r.last_state(None, nc)
    r.ctx.synchronize()
    assert int(nc.max()) > 256, int(nc.max())
    _check(f"colour 24x20 owned={owned}", r, perm, ref, di, None, None)


# ------------------------------------------------------------------------------------------------ 2. colour + depth + alpha
@pytest.mark.parametrize("mode", ["z", "inv_z"])
def test_colour_depth_alpha(lcgs, mode):
    W, H = 40, 24
    scene = R.scene300()
    di, dd, da = R.gradients(W, H, 12)
    ref = _reference(("three_40x24", mode), scene, W, H, di, dd, da, mode=mode)
    r, perm, keep = _renderer(lcgs, scene)
    _frame(lcgs, r, W, H)
    _check(f"colour+depth+alpha 40x24 {mode}", r, perm, ref, di, dd, da, mode)


# ------------------------------------------------------------------------------------------------ 3. map channels only
@pytest.mark.parametrize("which", ["depth", "alpha"])
def test_map_channels_only(lcgs, which):
    W, H = 40, 24
    scene = R.scene300()
    _, dd, da = R.gradients(W, H, 13, colour=False, depth=which == "depth", alpha=which == "alpha")
    ref = _reference(("maps_40x24", which), scene, W, H, None, dd, da)
    r, perm, keep = _renderer(lcgs, scene)
    _frame(lcgs, r, W, H)
    _check(f"{which} only 40x24", r, perm, ref, None, dd, da)


# ------------------------------------------------------------------------------------------------ 4. the antialiased frame
def test_antialiased_frame_colour_and_alpha(lcgs):
    W, H = 40, 24
    scene = R.scene300()
    di, _, da = R.gradients(W, H, 14, depth=False)
    ref = _reference("aa_40x24", scene, W, H, di, None, da, frame=antialias_ref.Antialiased)
    classic = _reference("aa_40x24_classic", scene, W, H, di, None, da)
    assert (np.abs(ref["abs64"] - classic["abs64"]) > ref["B"] + classic["B"]).any(axis=1).mean() > 0.5  # another frame altogether
    r, perm, keep = _renderer(lcgs, scene, raster="antialiased")
    _frame(lcgs, r, W, H)
    r.set_raster_mode("classic")  # the kept frame remembers its mode
    _check("antialiased colour+alpha 40x24", r, perm, ref, di, None, da)


# ------------------------------------------------------------------------------------------------ 5. stats over three views
POSES = [R.POSE, ([3.0, 0.5, -2.5], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]), ([-2.0, 2.0, 3.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])]


def _new_stats(P):
    return {"grad_accum": torch.zeros(P, dtype=torch.float32, device=DEV), "denom": torch.zeros(P, dtype=torch.int32, device=DEV),
            "max_radii": torch.zeros(P, dtype=torch.int32, device=DEV)}


def test_stats_over_three_views(lcgs):
    """denom and max_radii bit-equal to what lcgs_densify_accumulate wrote into a second statistics set on the same frames;
    grad_accum within (B_x W/2 + B_y H/2) summed over the views; d_absgrad called twice holds twice the reference within 2 B"""
    W, H = 64, 48
    scene = make_scene(np.random.default_rng(5), 340)
    scene["pos"][300:] += 100.0  # far outside the frustum: never on screen
    P = 340
    r, perm, d = _renderer(lcgs, scene)
    ours, theirs = _new_stats(P), _new_stats(P)
    g = {k: torch.zeros_like(d[k]) for k in KEYS}
    twice = torch.zeros(P, 2, device=DEV)
    refs = []
    on_screen = np.zeros(P, bool)
    for j, pose in enumerate(POSES):
        di = R.gradients(W, H, 20 + j, depth=False, alpha=False)[0]
        refs.append(_reference(("stats_64x48", j), scene, W, H, di, None, None, pose=pose))
        _frame(lcgs, r, W, H, pose=pose)
        r.backward(_t(di), *[g[k] for k in KEYS])
        r.densify_accumulate(theirs)
        r.absgrad_accumulate(_t(di), stats=ours, absgrad=twice if j == 2 else None)
        if j == 2:
            r.absgrad_accumulate(_t(di), absgrad=twice)
        r.ctx.synchronize()
        on_screen[r.visible_rows().cpu().numpy().astype(np.int64)] = True
    assert torch.equal(ours["denom"], theirs["denom"]) and torch.equal(ours["max_radii"], theirs["max_radii"])
    assert int(ours["denom"].max()) == 3 and 0 < on_screen.sum() < P and not on_screen[300:].any()
    for k, t in ours.items():
        assert (t.cpu().numpy()[~on_screen] == 0).all(), k
    want, bound = R.stats_bound(refs, W, H)
    diff = np.abs(ours["grad_accum"].cpu().numpy().astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    r2 = R.ratios(twice.cpu().numpy(), refs[2], scale=2.0)
    print(f"[absgrad] stats 3 x 64x48: grad_accum worst diff/bound {ratio.max():.3f} (row {int(ratio.argmax())}); "
          f"d_absgrad twice: worst diff/(2B) {r2.max():.3f}; {int(on_screen.sum())} rows on some screen")
    assert ratio.max() <= 1.0, (int(ratio.argmax()), float(ratio.max()))
    assert r2.max() <= 1.0, float(r2.max())
    # the statistic is not the 2020 one: the absolute sums exceed the norm of the summed gradient on most rows
    a, b = ours["grad_accum"].cpu().numpy(), theirs["grad_accum"].cpu().numpy()
    assert (a[on_screen] >= b[on_screen] * (1 - 1e-4)).all() and (a[on_screen] > 1.5 * b[on_screen]).mean() > 0.5


# ------------------------------------------------------------------------------------------------ 6. nothing disturbed
def test_nothing_a_later_call_reads_is_disturbed(lcgs):
    """forward, backward, densify_accumulate -> S1; absgrad_accumulate; densify_accumulate into fresh zeros -> S2: S1 == S2 bit
    for bit, and so is lcgs_camera_backward.  The call also works on a kept frame with no backward at all."""
    W, H = 40, 24
    scene = R.scene300()
    di, dd, da = R.gradients(W, H, 15)
    r, perm, d = _renderer(lcgs, scene)
    _frame(lcgs, r, W, H)
    P = 300
    early = torch.zeros(P, 2, device=DEV)
    r.absgrad_accumulate(_t(di), _t(dd), _t(da), absgrad=early)  # no backward yet
    g = {k: torch.zeros_like(d[k]) for k in KEYS}
    r.backward_maps(_t(di), _t(dd), _t(da), *[g[k] for k in KEYS])
    S1, S2 = _new_stats(P), _new_stats(P)
    cam1, cam2 = torch.zeros(12, device=DEV), torch.zeros(12, device=DEV)
    r.densify_accumulate(S1)
    r.camera_backward(cam1)
    late = torch.zeros(P, 2, device=DEV)
    r.absgrad_accumulate(_t(di), _t(dd), _t(da), stats=_new_stats(P), absgrad=late)
    r.densify_accumulate(S2)
    r.camera_backward(cam2)
    r.ctx.synchronize()
    for k in S1:
        assert torch.equal(S1[k], S2[k]), k
    assert float(S1["grad_accum"].sum()) > 0 and int(S1["denom"].sum()) > 0
    assert torch.equal(cam1.view(torch.int32), cam2.view(torch.int32)) and bool((cam1 != 0).any())
    ref = _reference(("three_40x24_15", "z"), scene, W, H, di, dd, da)
    for name, t in (("before any backward", early), ("behind a backward", late)):
        ratio = R.ratios(t.cpu().numpy(), ref)
        print(f"[absgrad] {name}: worst diff/B {ratio.max():.3f}")
        assert ratio.max() <= 1.0, name


# ------------------------------------------------------------------------------------------------ 7. state and arguments
def test_state_and_arguments(lcgs):
    W, H = 24, 20
    scene = R.scene300()
    P = 300
    r, perm, d = _renderer(lcgs, scene)
    di, dd, da = (_t(a) for a in R.gradients(W, H, 16))
    out = torch.full((P, 2), SEVEN, device=DEV)
    stats = {k: torch.full_like(t, 7) for k, t in _new_stats(P).items()}

    def refused(status, **kw):
        with pytest.raises(lcgs.LcgsError) as e:
            r.absgrad_accumulate(**kw)
        assert e.value.status == status, (e.value.status, str(e.value))

    refused(8, dL_dimg=di, absgrad=out)  # no frame at all
    img = torch.zeros(3, H, W, device=DEV)
    r.forward(lcgs.get_lookat_cam(*R.POSE, width=W, height=H), img, keep_state=False)
    refused(8, dL_dimg=di, absgrad=out)  # the last frame kept no state
    _frame(lcgs, r, W, H)
    refused(1, absgrad=out)  # all three gradients NULL
    refused(1, dL_dimg=di)  # both outputs NULL
    refused(1, dL_dimg=di, absgrad=torch.zeros(P + 1, 2, device=DEV))  # not the scene's row count
    refused(1, dL_dimg=di, stats={k: t[:P - 1] for k, t in stats.items()})
    lib, null = lcgs.load_library(), C.c_void_p(0)
    holed = lcgs.api._DensifyStats(C.c_void_p(stats["grad_accum"].data_ptr()), null, C.c_void_p(stats["max_radii"].data_ptr()))
    assert lib.lcgs_absgrad_accumulate(r.ctx._h, P, C.c_void_p(di.data_ptr()), 0, null, null, C.byref(holed), null) == 1
    assert lib.lcgs_absgrad_accumulate(r.ctx._h, P, C.c_void_p(di.data_ptr()), 2, null, null, None, C.c_void_p(out.data_ptr())) == 1
    assert lib.lcgs_absgrad_accumulate(None, P, C.c_void_p(di.data_ptr()), 0, null, null, None, C.c_void_p(out.data_ptr())) == 1
    r.ctx.synchronize()
    assert (out == SEVEN).all() and all((t == 7).all() for t in stats.values())  # nothing was written by any refused call
    r.absgrad_accumulate(di, dd, da, stats=stats, absgrad=out)  # ... and now it is fine
    r.ctx.synchronize()
    assert (out > SEVEN).any() and int(stats["denom"].max()) == 8
    # a frame that drew nothing (the scene behind the camera): LCGS_OK, outputs untouched
    out.fill_(SEVEN)
    for t in stats.values():
        t.fill_(7)
    _frame(lcgs, r, W, H, pose=([0.0, 0.0, -4.0], [0.0, 0.0, -8.0], [0.0, 1.0, 0.0]))
    assert r.frame_stats()["num_visible"] == 0
    r.absgrad_accumulate(di, dd, da, stats=stats, absgrad=out)
    r.ctx.synchronize()
    assert (out == SEVEN).all() and all((t == 7).all() for t in stats.values())
