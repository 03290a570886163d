"""The feature channels' CPU reference (tests/features_ref.py) pinned without a GPU against the references it generalises: with
K = 3 and the rows' normals as features it is normals_ref's map bit for bit (and its backward's geometry rows but for the rotq
term of the normal's own value), with K = 1 and all-ones features it is the alpha map bit for bit; the map is linear in the
features, so <g, F(f + d) - F(f)> = <dL/df, d> in f64 to rounding; and the zero-padding of the last triple changes nothing."""
import numpy as np

import features_ref
import maps_ref
import normals_ref
from conftest import make_scene

POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])
P, W, H = 60, 24, 20


def _scene(dtype=np.float32):
    scene = make_scene(np.random.default_rng(3), P, spread=0.35, log_scale=(-2.2, 0.5))
    scene["opacity"] = np.clip(scene["opacity"], 0.05, 0.9)
    return {k: v.astype(dtype) for k, v in scene.items()}


def test_three_channels_of_the_rows_normals_are_the_normal_map(oracle):
    o, scene = oracle, _scene()
    cam = o.lookat(*POSE, width=W, height=H)
    ref, st, (n, k, flip) = normals_ref.forward(o, scene, cam)
    got, _ = features_ref.forward(o, scene, cam, n)
    assert got.dtype == ref.dtype == np.float32 and np.abs(ref).max() > 1e-2 and np.array_equal(got, ref)
    gn = np.random.default_rng(7).normal(size=(3, H, W)).astype(np.float32)
    a = features_ref.backward(o, scene, cam, n, gn)
    b = normals_ref.backward(o, scene, cam, gn)
    for key in ("pos", "scale", "sh", "opacity"):
        assert np.array_equal(a[key], b[key]), key
    assert a["opacity"].any() and a["pos"].any() and a[features_ref.FKEY].any()
    # the normal's own value reaches rotq; a caller's feature reaches nothing but its own gradient
    own = normals_ref.normal_to_rotq(o, scene, cam, a[features_ref.FKEY], k, flip)
    assert own.any() and np.array_equal(a["rotq"] + own, b["rotq"])


def test_one_channel_of_ones_is_the_alpha_map(oracle):
    o, scene = oracle, _scene()
    cam = o.lookat(*POSE, width=W, height=H)
    alpha = maps_ref.forward(o, scene, cam)[1]
    got, _ = features_ref.forward(o, scene, cam, np.ones((P, 1), np.float32))
    assert got.shape == (1, H, W) and alpha.max() > 0.5 and np.array_equal(got[0], alpha)
    ga = np.random.default_rng(8).normal(size=(H, W)).astype(np.float32)
    a = features_ref.backward(o, scene, cam, np.ones((P, 1), np.float32), ga[None])
    b = maps_ref.backward(o, scene, cam, None, ga)
    for key in ("pos", "scale", "rotq", "sh", "opacity"):
        assert np.array_equal(a[key], b[key]), key


def test_the_map_is_linear_in_the_features(oracle64):
    o, scene = oracle64, _scene(np.float64)
    cam = o.lookat(*POSE, width=W, height=H)
    rng = np.random.default_rng(9)
    for K in (1, 4, 7):
        f, d = rng.normal(size=(P, K)), rng.normal(size=(P, K))
        g = rng.normal(size=(K, H, W))
        lhs = float((g * (features_ref.forward(o, scene, cam, f + d)[0] - features_ref.forward(o, scene, cam, f)[0])).sum())
        gf = features_ref.backward(o, scene, cam, f, g)[features_ref.FKEY]
        rhs = float((gf * d).sum())
        scale = float(np.abs(gf * d).sum())
        assert gf.shape == (P, K) and scale > 0 and abs(lhs - rhs) <= 1e-11 * scale, (K, lhs, rhs, scale)
        # ... and dL/df does not depend on f: it is sum_p w g
        assert np.array_equal(gf, features_ref.backward(o, scene, cam, f + d, g)[features_ref.FKEY])


def test_zero_padding_of_the_last_triple_changes_nothing(oracle):
    o, scene = oracle, _scene()
    cam = o.lookat(*POSE, width=W, height=H)
    rng = np.random.default_rng(10)
    f4 = rng.normal(size=(P, 4)).astype(np.float32)
    g4 = rng.normal(size=(4, H, W)).astype(np.float32)
    f6 = np.concatenate([f4, np.zeros((P, 2), np.float32)], axis=1)
    g6 = np.concatenate([g4, np.zeros((2, H, W), np.float32)], axis=0)
    m4, m6 = features_ref.forward(o, scene, cam, f4)[0], features_ref.forward(o, scene, cam, f6)[0]
    assert np.array_equal(m4, m6[:4]) and not m6[4:].any() and m4[3].any()
    a, b = features_ref.backward(o, scene, cam, f4, g4), features_ref.backward(o, scene, cam, f6, g6)
    for key in ("pos", "scale", "rotq", "sh", "opacity"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a[features_ref.FKEY], b[features_ref.FKEY][:, :4]) and not b[features_ref.FKEY][:, 4:].any()
    # each channel is blended on its own: a column's map does not depend on its neighbours in the triple
    alone = features_ref.forward(o, scene, cam, f4[:, 1:2])[0]
    assert np.array_equal(alone[0], m4[1])


def test_row_bound_carries_the_feature_rows(oracle):
    scene = _scene()
    ocam = oracle.lookat(*POSE, width=W, height=H)
    rng = np.random.default_rng(12)
    f, g = rng.normal(size=(P, 5)).astype(np.float32), rng.normal(size=(5, H, W)).astype(np.float32)
    B, R = features_ref.row_bound(scene, ocam, f, g)
    assert B[features_ref.FKEY].shape == R[features_ref.FKEY].shape == (P, 5)
    r32 = features_ref.backward(oracle, scene, ocam, f, g)
    for key in B:  # the f32 reference itself sits inside the bound
        d = np.abs(r32[key].astype(np.float64).reshape(P, -1) - R[key])
        assert (d <= B[key]).all(), key
    # ... and the feature columns got the formula's budget, not a blanket: it scales with sum |w g| x the recursion depth (a row
    # whose terms cancel keeps the budget of its terms), so against the gradient itself it is small but not tiny
    # (tests/test_oracle_gradient_rows.py pins the formula and its constants)
    big = np.abs(R[features_ref.FKEY]) > 1e-3
    assert big.any() and (B[features_ref.FKEY] > 0).all() and np.median(B[features_ref.FKEY][big] / np.abs(R[features_ref.FKEY][big])) < 1e-2
    S = features_ref.sum_row_bounds([(B, R), maps_ref.row_bound(scene, ocam, None, g[0])])
    assert np.array_equal(S[0][features_ref.FKEY], B[features_ref.FKEY]) and (S[0]["pos"] >= B["pos"]).all()
    assert features_ref.FKEY not in features_ref.geometry_only((B, R))[0]


def test_noise_term_needs_both_channel_orders_on_a_needle_row(oracle):
    """features_ref.row_bound samples the binary32 builds in both channel orders: on draw 102 (needles and giants) at K = 17
    the f32 reference ITSELF, composed in another channel order (rng seed 3), leaves the bound that samples the given order
    alone -- dL/dscale of row 1154, 1.59 x -- and stays inside the one that samples both (0.49); everything else about the bound
    is maps_ref.row_bound's."""
    from gpu_util import random_draw

    _, scene, W_, H_, pose, fov, _, sm = random_draw(102)
    n, K = scene["pos"].shape[0], 17
    ocam = oracle.lookat(*pose, width=W_, height=H_, fov=fov)
    f = np.random.default_rng(41 + K).normal(size=(n, K)).astype(np.float32)
    g = np.random.default_rng(43 + K).normal(size=(K, H_, W_)).astype(np.float32)
    perm = np.random.default_rng(3).permutation(K)
    other = features_ref.backward(oracle, scene, ocam, f[:, perm], g[perm], scale_modifier=sm)

    def worst(bound):
        B, R = bound
        d = np.abs(other["scale"].astype(np.float64) - R["scale"])
        assert not d[B["scale"] == 0].any()  # (rows no pixel blends: exact zeros on both sides)
        ratio = d / np.where(B["scale"] > 0, B["scale"], 1.0)
        return float(ratio.max()), int(np.argmax(ratio.max(axis=1)))

    one = worst(features_ref.row_bound(scene, ocam, f, g, scale_modifier=sm, orders=[np.arange(K)]))
    both = worst(features_ref.row_bound(scene, ocam, f, g, scale_modifier=sm))
    print(f"[features noise term] the f32 reference in another channel order: {one[0]:.2f} of the one-order bound (row {one[1]}), "
          f"{both[0]:.2f} of the two-order bound")
    assert one[0] > 1.0 and one[1] == 1154 and scene["scale"][1154].max() > 50 * scene["scale"][1154].min()
    assert both[0] < 1.0
