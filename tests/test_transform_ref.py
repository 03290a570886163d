"""The restatement of the scene similarity transform (tests/transform_ref.py) against the mathematics, without a GPU and without
the library: the band matrices against the sixteen basis terms written out here, the binary32 row expressions against the binary64
ones, and the frame -- a transformed scene under the transformed camera is the original frame on both builds of the oracle, and is
NOT when the coefficients are left unrotated."""
import numpy as np
import pytest

import transform_ref as T
from conftest import make_scene

ROTATIONS = T.rotation_set()
ROT_IDS = [f"random{i}" for i in range(20)] + ["identity", "turn_x", "turn_y", "turn_z"]


def basis(d):
    """the sixteen expressions of gs_math.hpp's LCGS_SH_TERMS, binary64, constants read as binary64; d [n, 3] -> [n, 16]"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    C1, C2, C3 = T.C1, T.C2, T.C3
    return np.stack([
        np.full_like(x, 0.28209479177387814),
        -C1 * y, C1 * z, -C1 * x,
        C2[0] * x * y, C2[1] * y * z, C2[2] * (2.0 * zz - xx - yy), C2[3] * z * x, C2[4] * (xx - yy),
        C3[0] * y * (3.0 * xx - yy), C3[1] * x * y * z, C3[2] * y * (4.0 * zz - xx - yy),
        C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), C3[4] * x * (4.0 * zz - xx - yy), C3[5] * z * (xx - yy),
        C3[6] * x * (xx - 3.0 * yy)], axis=1)


def unit_directions(n, seed=7):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def test_basis_is_the_oracles(oracle64):
    """B as written above is what Oracle.sh_eval_dir sums.  The oracle holds the constants in binary32, this file in binary64:
    each term differs by at most 2^-24 relative, so |sum_k c_k B_k - oracle| <= 1.01 * 2^-24 * sum_k |c_k B_k| (+ binary64
    rounding of sixteen terms)."""
    rng = np.random.default_rng(11)
    d, sh = unit_directions(64, 12), rng.normal(0, 0.5, (64, 16, 3))
    B = basis(d)
    mine = np.einsum("nk,nkc->nc", B, sh)
    theirs = oracle64.sh_eval_dir(3, d, sh.reshape(64, 48))
    bound = 1.01 * T.U * np.einsum("nk,nkc->nc", np.abs(B), np.abs(sh)) + 1e-14
    assert (np.abs(mine - theirs) <= bound).all()
    assert np.abs(mine - theirs).max() > 1e-12  # (the two sets of constants do differ: the bound above is not slack)


@pytest.mark.parametrize("rot", ROTATIONS, ids=ROT_IDS)
def test_band_matrices_rotate_the_basis_and_are_orthogonal(rot):
    p = T.plan64(rot)
    d = unit_directions(256)
    B, BR = basis(d), basis(d @ p["Rh"].T)
    worst_fit = worst_orth = 0.0
    for l, D in zip((1, 2, 3), p["D"]):
        lo, hi = l * l, (l + 1) * (l + 1)
        worst_fit = max(worst_fit, float(np.abs(BR[:, lo:hi] - B[:, lo:hi] @ D.T).max()))
        worst_orth = max(worst_orth, float(np.abs(D @ D.T - np.eye(2 * l + 1)).max()))
    print(f"[band matrices] max |B(R d) - D B(d)| {worst_fit:.2e}, max |D D^T - I| {worst_orth:.2e}")
    assert worst_fit <= 1e-12 and worst_orth <= 1e-12
    # the rotation everything sees is a rotation, and it is the caller's to binary32 rounding of the caller's entries
    assert np.abs(p["Rh"] @ p["Rh"].T - np.eye(3)).max() <= 1e-15 and np.abs(p["Rh"] - rot.astype(np.float64)).max() <= 4e-7
    assert abs(np.linalg.norm(p["q"]) - 1.0) <= 1e-15 and p["q"][0] >= 0.0


def test_colour_is_invariant():
    """sum_k c'_k B_k(R d) = sum_k c_k B_k(d): the property the whole feature exists for, in binary64"""
    rng = np.random.default_rng(5)
    sh = rng.normal(0, 0.5, (40, 16, 3))
    d = unit_directions(40, 6)
    for rot in ROTATIONS[:6]:
        p = T.plan64(rot)
        sh2 = T.transform({"sh": sh}, p)["sh"]
        a = np.einsum("nk,nkc->nc", basis(d), sh)
        b = np.einsum("nk,nkc->nc", basis(d @ p["Rh"].T), sh2)
        assert np.abs(a - b).max() <= 1e-13


def test_every_shepperd_branch_gives_the_rotation_back():
    """rotations by 180 degrees (trace -1) about each axis and about a diagonal take the three branches that do not start from
    the trace"""
    for q in ([0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0.01, 0.2, 0.9, 0.4], [0.01, 0.2, 0.4, 0.9], [0.01, 0.9, 0.3, 0.2]):
        q = np.asarray(q, np.float64) / np.linalg.norm(q)
        R = T.rot_from_quat(*q)
        got = np.array(T.quat_from_rot(R))
        assert min(np.abs(got - q).max(), np.abs(got + q).max()) <= 1e-15
        assert np.abs(T.rot_from_quat(*got) - R).max() <= 1e-15


def test_binary32_rows_are_inside_the_forward_bound_of_the_binary64_rows():
    """A 48-coefficient row: c'_k is a left-to-right dot product of n = 2l + 1 terms whose D entries were each rounded once --
    the standard forward bound gamma_{n+1} sum_j |D[k][j]| |c_j|, gamma_m = m u / (1 - m u), u = 2^-24."""
    rng = np.random.default_rng(21)
    sh = rng.normal(0, 0.5, (500, 16, 3)).astype(np.float32)
    for rot in ROTATIONS:
        p = T.plan64(rot)
        got = T.transform({"sh": sh}, T.plan32(p))["sh"].astype(np.float64)
        ref = T.transform({"sh": sh}, p)["sh"]
        assert T.same_bits(got[:, 0, :].astype(np.float32), sh[:, 0, :])
        for l, D in zip((1, 2, 3), p["D"]):
            n, lo, hi = 2 * l + 1, l * l, (l + 1) * (l + 1)
            gamma = (n + 1) * T.U / (1 - (n + 1) * T.U)
            bound = gamma * np.einsum("kj,njc->nkc", np.abs(D), np.abs(sh[:, lo:hi, :].astype(np.float64)))
            assert (np.abs(got[:, lo:hi, :] - ref[:, lo:hi, :]) <= bound).all(), l


def test_positions_orientations_and_scales_follow_the_rotation():
    """binary64: pos' = s Rhat pos + t, and the covariance R' S'^2 R'^T of the transformed row is s^2 Rhat Sigma Rhat^T"""
    rng = np.random.default_rng(8)
    scene = make_scene(rng, 50)
    q64 = scene["rotq"].astype(np.float64)
    scene["rotq"] = q64 / np.linalg.norm(q64, axis=1, keepdims=True)  # (unit to binary64: R(Q q) = R(Q) R(q) holds for unit q)
    p = T.plan64(ROTATIONS[1], 2.5, (0.7, -1.3, 2.1))
    out = T.transform(scene, p)
    assert np.abs(out["pos"] - (2.5 * scene["pos"].astype(np.float64) @ p["Rh"].T + p["t"])).max() <= 1e-14
    for i in range(50):
        w, x, y, z = scene["rotq"][i].astype(np.float64)
        R0, R1 = T.rot_from_quat(w, x, y, z), T.rot_from_quat(*out["rotq"][i])
        S0, S1 = np.diag(scene["scale"][i].astype(np.float64) ** 2), np.diag(out["scale"][i] ** 2)
        want = 2.5 ** 2 * p["Rh"] @ R0 @ S0 @ R0.T @ p["Rh"].T
        assert np.abs(R1 @ S1 @ R1.T - want).max() <= 1e-12 * np.abs(want).max() + 1e-18


# ----------------------------------------------------------------------------------------------------------------- the frame
FRAME_CAP = 30  # 0.5 % of the 6 144 pixels may differ by more than 1e-4 (blend-threshold flips)


def _frame_inputs():
    scene = make_scene(np.random.default_rng(3), 400, log_scale=(-2.8, 0.6))
    rot = T.random_rotation(np.random.default_rng(77))
    return scene, rot, (0.7, -1.3, 2.1)


def _over_bar(orc, scene, scale, rotate_sh):
    scene0, rot, trans = scene
    cam = orc.lookat([3, 0.5, 1.2], [0, 0, 0.5], [0, 0, 1], 96, 64)
    p = T.plan64(rot, scale, trans)
    moved = T.transform(scene0, p, rotate_sh=rotate_sh)
    cam2 = orc.camera_from_dict(T.camera(orc.camera_to_dict(cam), p))
    a, b = orc.render(scene0, cam, sh_deg=3), orc.render(moved, cam2, sh_deg=3)
    diff = np.abs(a["img"].astype(np.float64) - b["img"].astype(np.float64)).max(axis=0)
    covered = float((a["final_T"] < 0.5).mean())
    print(f"[frame invariance] {orc.precision} scale {scale} rotate_sh {rotate_sh}: max diff {diff.max():.2e}, "
          f"{int((diff > 1e-4).sum())} of {diff.size} pixels beyond 1e-4; coverage {covered:.2f}")
    assert diff.size == 6144 and covered > 0.2  # (a fifth of the frame is more than half opaque: not two backgrounds compared)
    return int((diff > 1e-4).sum())


@pytest.mark.parametrize("scale", [1.0, 2.5])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_transformed_scene_under_the_transformed_camera_is_the_same_frame(oracle, oracle64, precision, scale):
    orc = oracle if precision == "f32" else oracle64
    assert _over_bar(orc, _frame_inputs(), scale, True) <= FRAME_CAP


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_unrotated_coefficients_fail_the_frame(oracle, oracle64, precision):
    """the same comparison with the SH rows copied: the cap is exceeded -- the test above can see the feature"""
    orc = oracle if precision == "f32" else oracle64
    assert _over_bar(orc, _frame_inputs(), 1.0, False) > FRAME_CAP
