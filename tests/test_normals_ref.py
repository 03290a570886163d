"""The normal map's CPU reference (tests/normals_ref.py) pinned without a GPU: splat_normals against the header's definition on
hand-made rows, and the f64 gradient against central differences of its own f64 forward, with the already-validated depth
channel of maps_ref.py through the identical procedure as the yardstick."""
import types

import numpy as np

import maps_ref
import normals_ref
from conftest import make_scene
from test_distortion_ref import _central_differences

POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])


def _rows(oracle, scale, rotq, pos, position=(0.0, 0.0, 0.0)):
    """splat_normals of hand-made rows for a camera at `position` whose view rows are the identity"""
    o = oracle
    cam = types.SimpleNamespace(position=list(position), right=[1.0, 0.0, 0.0], up=[0.0, 1.0, 0.0], front=[0.0, 0.0, 1.0])
    scene = {"scale": np.asarray(scale, np.float32), "rotq": np.asarray(rotq, np.float32), "pos": np.asarray(pos, np.float32)}
    return normals_ref.splat_normals(o, scene, cam)


def test_axis_is_the_shortest_with_ties_to_the_lower_index(oracle):
    ident = [1.0, 0.0, 0.0, 0.0]
    scale = [[0.1, 0.2, 0.3], [0.2, 0.1, 0.3], [0.3, 0.2, 0.1],  # each axis chosen
             [0.1, 0.1, 0.3], [0.3, 0.1, 0.1], [0.1, 0.3, 0.1], [0.2, 0.2, 0.2]]  # ties
    P = len(scale)
    pos = [[-1.0, -1.0, -1.0]] * P  # t = -1 for every axis of the identity rotation: never flipped
    n, k, flip = _rows(oracle, scale, [ident] * P, pos)
    assert k.tolist() == [0, 1, 2, 0, 1, 0, 0] and not flip.any()
    assert np.array_equal(n, np.eye(3, dtype=np.float32)[k])


def test_flip_turns_the_normal_to_the_camera_and_zero_or_nan_leave_it(oracle):
    ident = [1.0, 0.0, 0.0, 0.0]
    scale = [[0.1, 0.2, 0.3]] * 5  # axis 0: c = (1, 0, 0) and t = d0
    pos = [[2.0, 5.0, 5.0], [-2.0, 5.0, 5.0], [0.0, 5.0, 5.0], [np.nan, 5.0, 5.0], [3.5, 0.0, 0.0]]
    n, k, flip = _rows(oracle, scale, [ident] * 5, pos)
    assert k.tolist() == [0] * 5 and flip.tolist() == [True, False, False, False, True]
    assert np.array_equal(n[:, 0], np.float32([-1, 1, 1, 1, -1])) and not n[:, 1:].any()
    # the camera's position is subtracted: the same rows seen from x = 3 flip the other way
    flip3 = _rows(oracle, scale[:2], [ident] * 2, pos[:2], position=(3.0, 0.0, 0.0))[2]
    assert flip3.tolist() == [False, False]
    assert _rows(oracle, scale[:1], [ident], [[3.0, 0.0, 0.0]], position=(3.0, 0.0, 0.0))[2].tolist() == [False]  # t == 0


def test_unit_quaternions_give_unit_normals_that_face_the_camera(oracle):
    rng = np.random.default_rng(2)
    P = 300
    q = rng.normal(size=(P, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    scene = {"scale": rng.uniform(0.01, 1.0, (P, 3)).astype(np.float32), "rotq": q,
             "pos": rng.normal(size=(P, 3)).astype(np.float32)}
    cam = oracle.lookat(*POSE, width=24, height=20)
    n, k, flip = normals_ref.splat_normals(oracle, scene, cam)
    assert n.dtype == np.float32 and set(k.tolist()) == {0, 1, 2} and flip.any() and not flip.all()
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert (k == np.argmin(scene["scale"], axis=1)).all()
    # view space: the world normal is Rview^T n, its column is the rotation's, and it points to the camera's side
    Rv = np.stack([np.asarray(cam.right[:]), np.asarray(cam.up[:]), np.asarray(cam.front[:])]).astype(np.float64)
    c = n.astype(np.float64) @ Rv
    w, x, y, z = (q[:, j].astype(np.float64) for j in range(4))
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)  # [P, row, column]
    col = R[np.arange(P), :, k]
    assert np.abs(c - np.where(flip[:, None], -col, col)).max() < 1e-6
    d = scene["pos"].astype(np.float64) - np.asarray(cam.position[:], np.float64)
    assert ((c * d).sum(axis=1) <= 1e-6).all()
    # the decisions of another evaluation are taken as given
    n2, k2, f2 = normals_ref.splat_normals(oracle, scene, cam, decide=((k + 1) % 3, ~flip))
    assert (k2 == (k + 1) % 3).all() and (f2 == ~flip).all() and not np.array_equal(n2, n)


def test_reference_gradient_matches_central_differences_like_the_depth_channel_does(oracle64):
    """normals_ref.backward (f64) against central differences of normals_ref.forward (f64) with the axis and the flip held at
    the frame's own, 40 splats at 24 x 20, eight components per attribute; the same components through maps_ref.backward's
    depth channel are the yardstick, and the normal channel is held to 10 x its disagreement (as the distortion channel is).
    Measured (largest |fd - g| / max |g|; no component of the 32 drawn is skipped):
        depth channel 5.3e-10, normal channel 2.1e-10"""
    o = oracle64
    P, W, H = 40, 24, 20
    scene = {k: v.astype(np.float64) for k, v in make_scene(np.random.default_rng(3), P, spread=0.35, log_scale=(-2.2, 0.5)).items()}
    scene["opacity"] = np.clip(scene["opacity"], 0.05, 0.9)
    cam = o.lookat(*POSE, width=W, height=H)
    wrng = np.random.default_rng(11)
    wd, wn = wrng.normal(size=(H, W)), wrng.normal(size=(3, H, W))
    state = lambda sc: o.forward_state(sc, cam)
    dec = normals_ref.splat_normals(o, scene, cam)[1:]
    assert set(dec[0].tolist()) == {0, 1, 2} and dec[1].any() and not dec[1].all()
    g_depth = maps_ref.backward(o, scene, cam, wd, None)
    g_nrm = normals_ref.backward(o, scene, cam, wn, decide=dec)
    assert not g_nrm["sh"].any() and g_nrm["rotq"].any() and normals_ref.forward(o, scene, cam, decide=dec)[0].any()
    loss_depth = lambda sc: float((maps_ref.forward(o, sc, cam)[0] * wd).sum())
    loss_nrm = lambda sc: float((normals_ref.forward(o, sc, cam, decide=dec)[0] * wn).sum())
    e_depth, drawn, skipped = _central_differences(o, scene, cam, loss_depth, state, g_depth, np.random.default_rng(5), 8)
    e_nrm, drawn2, skipped2 = _central_differences(o, scene, cam, loss_nrm, state, g_nrm, np.random.default_rng(5), 8)
    print(f"[normals reference vs central differences] depth channel {e_depth:.3e}, normal channel {e_nrm:.3e}, "
          f"{skipped} of {drawn} components skipped")
    assert (drawn, skipped) == (drawn2, skipped2) and 4 * skipped <= drawn, (drawn, skipped)
    assert e_depth > 0 and e_nrm <= 10 * e_depth, (e_nrm, e_depth)
