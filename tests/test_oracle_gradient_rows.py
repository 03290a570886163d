"""`-m "not gpu"`: the per-row gradient checker (tests/gpu_util.py::check_gradient_rows) proven on the CPU before it judges a
kernel.  Honest answers -- other binary32 evaluations of the same frame -- lie inside every row's bound; wrong answers that
move a handful of rows, which the norm checks (gpu_util.check_gradients, test_gpu_backward._check) let through, are flagged
on exactly the rows they touch.

Cost of the bound, measured on a CPU host (the walk runs on one core): <= 1.1 s per random-sweep frame, 2.8 s for the 640 x 480
frame of 50 000 splats (the f64 walk with its two sums, the f32 forward by stages, eight f64 preprocess-backward runs for |J|);
the contracted oracle's backward (1.1 s there) comes on top where a caller does not already hold it."""
import numpy as np
import pytest
import torch

from conftest import make_scene
from gpu_util import (_oracles, check_gradients, gradient_row_bound, gradient_row_ratios,
                      random_draw)
from test_gpu_backward import POSE, _check

KEYS = ("pos", "scale", "rotq", "sh", "opacity")


def _frame(scene, W, H, pose, fov=None, bg=(0.1, 0.2, 0.3), sm=1.0, seed=0):
    o32, o64, o32c = _oracles()
    ocam = o32.lookat(*pose, width=W, height=H, fov=fov)
    cam64 = o64.lookat(*pose, width=W, height=H, fov=fov)
    dL = np.random.default_rng(seed).normal(size=(3, H, W)).astype(np.float32)
    kw = dict(bg=bg, scale_modifier=sm)
    r32 = o32.render_backward_full(scene, ocam, dL, **kw)
    r32c = o32c.render_backward_full(scene, o32c.convert_camera(ocam), dL, **kw)
    B, r64 = gradient_row_bound(scene, ocam, dL, ref32=r32, ref32c=r32c, cam64=cam64, **kw)
    return dict(scene=scene, ocam=ocam, cam64=cam64, dL=dL, kw=kw, r32=r32, r32c=r32c, r64=r64, B=B, W=W, H=H)


def _proxies(f):
    """binary32 answers that share the kernels' position -- the f32 oracle's forward state, bit for bit -- but not its
    rounding: the walk with libm's expf (another exp, as the kernels' hardware exp is) and the contracted-FMA build's walk,
    each followed by its own build's preprocess-backward -- by the f64 build's for splats whose filtered 2-D covariance has
    a trace over 455 px^2, as the kernels evaluate those rows in f64 (backward.hip, geom_backward: kGiantCovTrace)"""
    o32, o64, o32c = _oracles()
    st = o32.forward_state(f["scene"], f["ocam"], **f["kw"])
    out = {}
    for name, o, libm in (("libm-exp walk", o32, True), ("contracted walk", o32c, False)):
        o.set_blend_exp(libm)
        try:
            gm, gc, go, gcol = o.render_backward(f["W"], f["H"], np.asarray(f["kw"]["bg"], np.float32), st["ranges"],
                                                 st["point_list"], st["means"], st["conic"], st["opacity"], st["color"],
                                                 st["final_T"], st["n_contrib"], f["dL"])
        finally:
            o.set_blend_exp(False)
        sm = f["kw"]["scale_modifier"]
        g = o.preprocess_backward(f["scene"], o.convert_camera(f["ocam"]), st["radii"], gm, gc, gcol, scale_modifier=sm)
        g64 = o64.preprocess_backward(f["scene"], f["cam64"], st["radii"], gm, gc, gcol, scale_modifier=sm)
        _, _, cov = o32.project(f["scene"]["pos"], f["scene"]["scale"], f["scene"]["rotq"], f["ocam"], scale_modifier=sm)
        giant = cov[:, 0].astype(np.float64) + cov[:, 2] + 0.6 > 455.0  # (+ the 0.3 px^2 low-pass on both axes)
        for k in ("pos", "scale", "rotq", "sh"):
            g[k][giant] = g64[k][giant]
        g["opacity"] = go
        out[name] = g
    return out


def _worst(got, f):
    return {k: v[0] for k, v in gradient_row_ratios(got, f["B"], f["r64"]).items()}


def _flagged(got, f, k):
    return set(gradient_row_ratios({k: got[k]}, {k: f["B"][k]}, f["r64"])[k][2].tolist())


def _norms_catch(got, f):
    """(check_gradients catches it, _check catches it)"""
    P = f["scene"]["pos"].shape[0]
    radii = _oracles()[0].render(f["scene"], f["ocam"], **f["kw"])["radii"]
    caught = []
    try:
        check_gradients({k: torch.from_numpy(np.ascontiguousarray(got[k])) for k in KEYS}, f["r32"], f["r64"], P, radii, "mutation")
        caught.append(False)
    except AssertionError:
        caught.append(True)
    try:
        _check(got, f["r32"])
        caught.append(False)
    except AssertionError:
        caught.append(True)
    return tuple(caught)


HONEST_MARGIN = 0.8  # every honest answer at most this fraction of its bound (worst observed: see docs/TESTS.md)


def _honest(f, tag):
    answers = {"f32 oracle": f["r32"], "contracted f32 oracle": f["r32c"], **_proxies(f)}
    for name, g in answers.items():
        w = _worst(g, f)
        print(f"[gradient rows, honest] {tag} {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
        # the f32 oracles enter the noise term, so their rows sit at <= 1 / K by construction (a smoke check of the
        # plumbing); the two proxies are the real test of K and c_u: they share the noise term's forward, not its rounding
        assert max(w.values()) <= HONEST_MARGIN, (tag, name, w)


@pytest.mark.parametrize("seed", list(range(12)) + [100 + i for i in range(5)])
def test_honest_answers_lie_inside_every_row_bound_random_draws(seed):
    _, scene, W, H, pose, fov, bg, sm = random_draw(seed)
    _honest(_frame(scene, W, H, pose, fov=fov, bg=bg, sm=sm, seed=seed), f"draw {seed}")


@pytest.fixture(scope="module")
def big():
    """640 x 480, 50 000 splats, a few giants (screen-filling footprints near the camera)"""
    rng = np.random.default_rng(77)
    scene = make_scene(rng, 50_000, log_scale=(-4.2, 0.6))
    scene["pos"][:6] = rng.normal(0, 0.25, (6, 3)) + np.array(POSE[0]) * 0.55
    scene["scale"][:6] = np.exp(rng.normal(-1.5, 0.3, (6, 3)))
    return _frame(scene, 640, 480, POSE, seed=3)


@pytest.fixture(scope="module")
def partial():
    """333 x 201: the last tile column is 13 px wide, the last tile row 9 px high"""
    rng = np.random.default_rng(78)
    scene = make_scene(rng, 6000, spread=1.6, log_scale=(-4.0, 0.6))
    return _frame(scene, 333, 201, POSE, seed=4)


def test_honest_answers_lie_inside_every_row_bound_640x480(big):
    radii = _oracles()[0].render(big["scene"], big["ocam"], **big["kw"])["radii"]
    assert (radii > 64).sum() >= 3  # the giants are there
    _honest(big, "640x480")


def _zeroed(f, ys, xs):
    dL = f["dL"].copy()
    dL[:, ys, xs] = 0.0
    o32, o64, _ = _oracles()
    got = o32.render_backward_full(f["scene"], f["ocam"], dL, **f["kw"])
    part = np.zeros_like(f["dL"])
    part[:, ys, xs] = f["dL"][:, ys, xs]
    g_part = o64.render_backward_full(f["scene"], f["cam64"], part, **f["kw"])  # what the zeroed pixels contribute (linear in dL)
    return got, g_part


def _assert_flags_the_touched_rows(got, g_part, f):
    """every row whose contribution from the zeroed pixels exceeds twice its bound is flagged, and only rows that have one"""
    n_must = 0
    for k in KEYS:
        P = f["B"][k].shape[0]
        c = np.abs(g_part[k].astype(np.float64).reshape(P, -1))
        must = set(np.nonzero((c > 2.0 * f["B"][k]).any(axis=1))[0].tolist())
        touched = set(np.nonzero((c > 0).any(axis=1))[0].tolist())
        flagged = _flagged(got, f, k)
        assert must <= flagged, (k, sorted(must - flagged)[:10])
        assert flagged <= touched, (k, sorted(flagged - touched)[:10])
        n_must += len(must)
    assert n_must > 0
    return n_must


# what the two norm checks make of each mutation, as observed (check_gradients, _check): the gain of the per-row check
NORMS_CATCH = {
    "tile": (True, True),
    "last tile row": (True, True),
    "last tile column": (True, True),
    "scaled rows": (False, False),
    "swapped rows": (False, False),
    "sh channels": (False, False),
    "giant opacity": (False, False),
}


def test_a_zeroed_tile_is_flagged_on_its_rows(big):
    got, g_part = _zeroed(big, slice(16 * 14, 16 * 15), slice(16 * 20, 16 * 21))
    n = _assert_flags_the_touched_rows(got, g_part, big)
    print(f"[gradient rows, mutation] tile (20, 14) zeroed: {n} rows flagged as required; norms {_norms_catch(got, big)}")
    assert _norms_catch(got, big) == NORMS_CATCH["tile"]


@pytest.mark.parametrize("which", ["last tile row", "last tile column"])
def test_the_last_tile_row_and_column_zeroed_are_flagged(partial, which):
    """the last tile row / column that is rasterised: the partial strip behind it (9 rows, 13 columns here) never is -- the
    reference's own behaviour (tests/test_reference_png.py) -- and its pixels contribute nothing, which every row's bound
    holds exactly (a row with nothing to sum has bound 0)"""
    W, H = partial["W"], partial["H"]
    assert W % 16 and H % 16
    st = _oracles()[0].forward_state(partial["scene"], partial["ocam"], **partial["kw"])
    assert not st["n_contrib"][H - H % 16:].any() and not st["n_contrib"][:, W - W % 16:].any()
    y0, x0 = H - H % 16 - 16, W - W % 16 - 16
    ys, xs = (slice(y0, y0 + 16), slice(0, W)) if which == "last tile row" else (slice(0, H), slice(x0, x0 + 16))
    got, g_part = _zeroed(partial, ys, xs)
    n = _assert_flags_the_touched_rows(got, g_part, partial)
    print(f"[gradient rows, mutation] {which} zeroed: {n} rows flagged as required; norms {_norms_catch(got, partial)}")
    assert _norms_catch(got, partial) == NORMS_CATCH[which]


def _sharp_rows(f, k, n=1, rows=None):
    """the n rows whose largest |b64| / bound is largest (well-conditioned: a small relative change is far over the bound)"""
    b = np.abs(f["r64"][k].astype(np.float64).reshape(f["B"][k].shape[0], -1))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(f["B"][k] > 0, b / f["B"][k], 0.0).max(axis=1)
    if rows is not None:
        s = np.where(rows, s, -1.0)
    return [int(i) for i in np.argsort(-s)[:n]], s


def _copy(g):
    return {k: np.array(g[k], copy=True) for k in KEYS}


def test_one_row_scaled_by_1e_3_is_flagged_alone(big):
    got = _copy(big["r32"])
    picked = {}
    for k in KEYS:
        (i,), s = _sharp_rows(big, k)
        assert s[i] > 1e4
        got[k][i] *= np.float32(1.001)
        picked[k] = i
    for k in KEYS:
        assert _flagged(got, big, k) == {picked[k]}, k
    assert _norms_catch(got, big) == NORMS_CATCH["scaled rows"]


def test_two_swapped_rows_are_both_flagged(big):
    got = _copy(big["r32"])
    (i, j), _ = _sharp_rows(big, "pos", 2)
    got["pos"][[i, j]] = got["pos"][[j, i]]
    assert _flagged(got, big, "pos") == {i, j}
    assert _norms_catch(got, big) == NORMS_CATCH["swapped rows"]


def test_permuted_sh_channels_of_one_row_are_flagged(big):
    got = _copy(big["r32"])
    (i,), _ = _sharp_rows(big, "sh")
    row = got["sh"][i].reshape(16, 3)
    got["sh"][i] = row[:, [1, 2, 0]].reshape(-1)
    assert _flagged(got, big, "sh") == {i}
    assert _norms_catch(got, big) == NORMS_CATCH["sh channels"]


def test_a_giants_opacity_gradient_off_by_1e_2_is_flagged(big):
    radii = _oracles()[0].render(big["scene"], big["ocam"], **big["kw"])["radii"]
    got = _copy(big["r32"])
    (i,), s = _sharp_rows(big, "opacity", rows=radii > 64)
    assert radii[i] > 64 and s[i] > 100
    got["opacity"][i] *= np.float32(1.01)
    assert _flagged(got, big, "opacity") == {i}
    assert _norms_catch(got, big) == NORMS_CATCH["giant opacity"]


def test_the_bound_switch_leaves_the_default_walk_bit_identical(partial):
    o32, o64, _ = _oracles()
    for o in (o32, o64):
        o.set_backward_bound(True)
        o.set_backward_bound(False)
        cam = partial["ocam"] if o is o32 else partial["cam64"]
        g = o.render_backward_full(partial["scene"], cam, partial["dL"], **partial["kw"])
        ref = partial["r32"] if o is o32 else partial["r64"]
        assert all(np.array_equal(g[k], ref[k]) for k in KEYS)
    o64.set_backward_bound(True)
    try:
        assert o64.render_backward_full(partial["scene"], partial["cam64"], partial["dL"], **partial["kw"])["num_rendered"] == -1
    finally:
        o64.set_backward_bound(False)
