"""lcgs_scene_transform and lcgs_scene_box_keep_mask on the GPU against tests/transform_ref.py: every output array is the binary32
restatement bit for bit in every mode, nothing outside an output is touched, and a bound scene transformed in place renders the
restated scene's frame under lcgs_camera_transform's camera -- the original frame."""
import numpy as np
import pytest
import torch

import transform_ref as T
from conftest import make_scene
from gpu_util import DEV, assert_image_parity

pytestmark = pytest.mark.gpu

KEYS = T.KEYS
GUARD = 64  # floats in front of and behind every output buffer
POISON = np.float32(-7.25e33)
ROT, SCALE, TRANS = T.random_rotation(np.random.default_rng(2025)), 2.5, (0.7, -1.3, 2.1)
COUNTS = [1, 63, 64, 65, 257, 1000]  # around one tile of the SH pass (kTransformTileRows = 64), several tiles, a partial last one


@pytest.fixture(scope="module")
def renderer(lcgs):
    return lcgs.Renderer(lcgs.Context(0))


def same(a, b):
    """bit for bit; a NaN is a NaN (its sign and payload are the producing unit's choice, not IEEE's)"""
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def guarded(a, offset=0):
    """a device copy of `a` with GUARD poisoned floats on either side (offset: further floats in front: 1 -> only 4-byte aligned);
    returns (the view, the whole buffer)"""
    a = np.ascontiguousarray(a, np.float32)
    flat = torch.full((a.size + 2 * GUARD + offset,), float(POISON), device=DEV)
    view = flat[GUARD + offset:GUARD + offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view, flat


def guards_intact(flat, n, offset=0):
    h = flat.cpu().numpy()
    return bool((h[:GUARD + offset] == POISON).all() and (h[GUARD + offset + n:] == POISON).all())


def structured_scene(P, deg, seed):
    """make_scene's rows at `deg`, with the rows the restatement's bits are most telling on: one 1 per band (a column of D_l), a
    non-unit quaternion, denormal and +-inf coefficients"""
    rng = np.random.default_rng(seed)
    s = make_scene(rng, P)
    K = (deg + 1) ** 2
    sh = s["sh"].reshape(P, 16, 3)[:, :K, :].copy()
    sh[0] = 0.0
    for l in range(1, deg + 1):
        sh[0, l * l + (l + seed) % (2 * l + 1), :] = 1.0
    if P > 2:
        s["rotq"][1] *= np.float32(3.5)
        sh[2, :, 0] = np.float32(1e-41) * rng.integers(-9, 10, K).astype(np.float32)  # denormals
        sh[2, :, 1] = np.float32(3e-39)
    if P > 4:
        sh[3, K - 1, 0], sh[3, min(1, K - 1), 1] = np.inf, -np.inf
        sh[4, :, 2] = np.nan
    s["sh"] = sh.reshape(P, K * 3)
    return s


def run(renderer, lcgs, xf, scene, deg, keys_out, in_place, offset=0):
    """-> ({key: result on the host} for every key, all guards intact)"""
    src = {k: guarded(scene[k], offset) for k in KEYS}
    if in_place:
        dst = {k: src[k] for k in keys_out}
    else:
        dst = {k: guarded(np.full_like(scene[k], 123.0), offset) for k in keys_out}
    renderer.scene_transform(xf, {k: v[0] for k, v in src.items()}, {k: v[0] for k, v in dst.items()}, sh_degree=deg)
    torch.cuda.synchronize()
    intact = all(guards_intact(flat, scene[k].size, offset) for store in (src, dst) for k, (_, flat) in store.items())
    out = {k: dst[k][0].cpu().numpy() for k in keys_out}
    untouched = {k: src[k][0].cpu().numpy() for k in KEYS if not (in_place and k in keys_out)}
    return out, untouched, intact


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("P", COUNTS)
def test_every_mode_is_the_restatement_bit_for_bit(renderer, lcgs, P, deg):
    scene = structured_scene(P, deg, 100 * deg + P)
    xf = lcgs.similarity(ROT, SCALE, TRANS)
    want = T.transform(scene, T.plan32(T.plan64(ROT, SCALE, TRANS)), sh_deg=deg)
    if deg >= 1:
        assert not same(want["sh"], scene["sh"])  # (a copy of the coefficients would not pass)
    modes = {"out of place": (KEYS, False), "in place": (KEYS, True), "sh only": (("sh",), False), "sh only, in place": (("sh",), True),
             "everything but sh": (("pos", "scale", "rotq", "opacity"), False)}
    for name, (keys_out, in_place) in modes.items():
        out, untouched, intact = run(renderer, lcgs, xf, scene, deg, keys_out, in_place)
        for k in keys_out:
            assert same(out[k], want[k]), (name, k)
        for k, v in untouched.items():
            assert same(v, scene[k]), (name, k, "an input changed")
        assert intact, (name, "guard floats changed")


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("P", [65, 257])
def test_arrays_that_are_only_4_byte_aligned(renderer, lcgs, P, deg):
    """every array one float past a 16-byte boundary: the passes' scalar paths, full tiles included"""
    scene = structured_scene(P, deg, 7 * deg + P)
    xf = lcgs.similarity(ROT, SCALE, TRANS)
    want = T.transform(scene, T.plan32(T.plan64(ROT, SCALE, TRANS)), sh_deg=deg)
    for in_place in (False, True):
        out, untouched, intact = run(renderer, lcgs, xf, scene, deg, KEYS, in_place, offset=1)
        assert all(same(out[k], want[k]) for k in KEYS) and intact
        assert all(same(v, scene[k]) for k, v in untouched.items())


@pytest.mark.parametrize("deg", [0, 3])
def test_identity_returns_every_array_bit_unchanged(renderer, lcgs, deg):
    scene = structured_scene(257, deg, 9)
    scene["sh"][4] = 0.25  # (0 * NaN is NaN whatever the matrix: the NaN row aside, the identity must not change a bit)
    out, _, intact = run(renderer, lcgs, lcgs.similarity(), scene, deg, KEYS, True)
    finite = np.isfinite(scene["sh"]).all(axis=1)
    for k in KEYS:
        rows = finite if k == "sh" else slice(None)
        assert T.same_bits(out[k][rows], scene[k][rows]), k
    assert intact


def test_the_library_plan_is_the_restatements(lcgs):
    """what the parity tests above stand on: for their rotation the kernels' plan is the restatement's, bit for bit"""
    plan, _ = lcgs.similarity_plan(lcgs.similarity(ROT, SCALE, TRANS))
    p = T.plan32(T.plan64(ROT, SCALE, TRANS))
    for got, want in ((plan.M, p["M"]), (plan.t, p["t"]), ([plan.s], [p["s"]]), (plan.q, p["q"]), (plan.D1, p["D"][0]),
                      (plan.D2, p["D"][1]), (plan.D3, p["D"][2])):
        assert T.same_bits(np.asarray(list(got), np.float32), np.asarray(want, np.float32).reshape(-1))


def test_empty_scene_launches_nothing(renderer, lcgs):
    e = {k: torch.empty((0, n), device=DEV) for k, n in zip(KEYS, (3, 3, 4, 48, 1))}
    renderer.scene_transform(lcgs.similarity(ROT), e)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- the frame
def test_bound_scene_transformed_in_place_renders_the_same_frame(renderer, lcgs, oracle):
    """Upload, render, transform the context's own arrays in place, render under lcgs_camera_transform's camera: the second frame
    is the f32 oracle's frame of the restated scene bit for bit (the derived rows were dropped and rebuilt), it is the first frame
    up to the project's image bar, and nothing derived is stale."""
    scene = make_scene(np.random.default_rng(3), 400, log_scale=(-2.8, 0.6))
    W, H = 96, 64
    pose = ([3, 0.5, 1.2], [0, 0, 0.5], [0, 0, 1])
    r = lcgs.Renderer(lcgs.Context(0))
    r.upload_scene(scene)
    cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
    first = torch.zeros(3, H, W, device=DEV)
    assert r.forward(cam, first, keep_state=True, sync=True) > 0 and r.verify_derived() == 0
    for scale in (1.0, 2.5):
        xf = lcgs.similarity(ROT, scale, TRANS)
        fresh = lcgs.Renderer(lcgs.Context(0))
        fresh.upload_scene(scene)
        fresh.forward(cam, torch.zeros(3, H, W, device=DEV), sync=True)  # (rows derived from the arrays about to be written)
        fresh.scene_transform(xf, fresh.scene_tensors())
        fresh.ctx.synchronize()
        assert fresh.verify_derived() == 0
        cam2 = lcgs.camera_transform(cam, xf)
        second = torch.zeros(3, H, W, device=DEV)
        assert fresh.forward(cam2, second, sync=True) > 0 and fresh.verify_derived() == 0
        moved = T.transform(scene, T.plan32(T.plan64(ROT, scale, TRANS)))
        ocam = oracle.camera_from_dict(cam2.to_dict())
        assert_image_parity(second.cpu().numpy(), oracle.render(moved, ocam, sh_deg=3))
        diff = (second - first).abs().amax(dim=0)
        over = int((diff > 1e-4).sum())
        print(f"[transformed frame] scale {scale}: max |second - first| {float(diff.max()):.2e}, {over} of {diff.numel()} pixels beyond 1e-4")
        assert over <= 30  # 0.5 % of 6 144: blend-threshold flips
        assert float((first.amax(dim=0) > 0.05).float().mean()) > 0.2  # (frames of the scene, not of the background)


# ------------------------------------------------------------------------------------------------------------------ the crop
def test_box_keep_mask_is_the_restatements(renderer, lcgs):
    rng = np.random.default_rng(31)
    P = 1000
    pos = make_scene(rng, P)["pos"]
    pos[3, 0] = np.nan
    pos[17, 2] = np.inf
    rot = T.random_rotation(rng)
    trans = (0.1, -0.2, -0.4)
    xf = lcgs.similarity(rot, 1.3, trans)
    plan = T.plan32(T.plan64(rot, 1.3, trans))
    b = np.abs(T.transform({"pos": pos}, plan)["pos"])
    on_face = [int(i) for i in np.nonzero((b[:, 1] < 0.6) & (b[:, 2] < 0.5) & (b[:, 0] > 0.3) & (b[:, 0] < 0.5))[0][:2]]
    boxes = [(float(b[on_face[0], 0]), 0.6, 0.5), (float("inf"), 0.3, float("inf")), (0.0, 0.0, 0.0),
             (0.5, float(b[on_face[1], 1]), float(b[on_face[1], 2]))]  # (a row on an edge: two faces at once)
    d_pos = torch.from_numpy(pos).to(DEV)
    for half in boxes:
        want = T.box_keep(pos, plan, half)
        for n, shift in ((P, 0), (P - 1, 1)):  # ... a count that is no multiple of four into bytes that are not 4-byte aligned
            buf = torch.full((n + 2 * GUARD + shift,), 0xAB, dtype=torch.uint8, device=DEV)
            keep = buf[GUARD + shift:GUARD + shift + n]
            renderer.scene_box_keep_mask(d_pos[:n], xf, half, keep)
            h = buf.cpu().numpy()
            assert (h[GUARD + shift:GUARD + shift + n] == want[:n]).all(), half
            assert (h[:GUARD + shift] == 0xAB).all() and (h[GUARD + shift + n:] == 0xAB).all()
        assert want[3] == 0 and want[17] == 0  # the NaN row and the row at infinity are dropped
    first = T.box_keep(pos, plan, boxes[0])
    assert first[on_face[0]] == 1 and 50 < first.sum() < 950  # exactly on a face: kept; the box cuts through the cloud
    assert T.box_keep(pos, plan, boxes[3])[on_face[1]] == 1


# ------------------------------------------------------------------------------------------------------------------ the tool
def test_transform_ply_tool_moves_crops_and_merges(lcgs, tmp_path, monkeypatch, capsys):
    """tools/transform_ply.py file to file, in process: two files, each under its own transform, cropped by one box, merged.
    Positions and coefficients are raw in the file: the restatement's bits.  Scale, opacity and rotation pass through log / logit /
    normalisation and back: |log s| <= 16 and |logit| <= 16 are rounded to binary32 once (half an ulp of 16 = 9.5e-7 absolute on
    the logarithm = relative on the scale, a quarter of it on the opacity) and the reader's exp / sigmoid / normalisation add a few
    2^-24: 2e-6 relative, 1e-6 absolute, 1e-6 absolute."""
    from tools import transform_ply as tool

    rng = np.random.default_rng(12)
    paths, scenes = [], []
    for name, P in (("a", 300), ("b", 200)):
        path = str(tmp_path / f"{name}.ply")
        lcgs.write_ply_raw(path, rng.normal(0, 0.6, (P, 3)), rng.normal(0, 1, (P, 3)), rng.normal(0, 0.2, (P, 45)), rng.normal(0, 2, P),
                           rng.normal(-3.5, 0.6, (P, 3)), rng.normal(0, 1, (P, 4)))
        r = lcgs.Renderer(lcgs.Context(0))
        assert r.load_ply(path, order="file") == P
        paths.append(path)
        scenes.append(r.download_scene())
    out = str(tmp_path / "out.ply")
    args = {"a": (["--rotate", "0.3", "-1", "0.5", "70"], 1.7, (0.2, 0.1, -0.3)), "b": (["--also-quat", "0.9", "0.1", "-0.3", "0.2"], 0.6, (-0.4, 0.0, 0.2))}
    crop_c, crop_h = (0.1, 0.0, -0.2), (1.2, float("inf"), 0.9)
    monkeypatch.setattr("sys.argv", ["transform_ply.py", paths[0], out, *args["a"][0], "--scale", "1.7", "--translate", "0.2", "0.1", "-0.3",
                                     "--also", paths[1], *args["b"][0], "--also-scale", "0.6", "--also-translate", "-0.4", "0.0", "0.2",
                                     "--crop", *[str(v) for v in crop_c + crop_h]])
    tool.main()
    rots = (tool.rotation_matrix(axis_angle=[0.3, -1, 0.5, 70]), tool.rotation_matrix(quat=[0.9, 0.1, -0.3, 0.2]))
    box = T.plan32(T.plan64(np.eye(3), 1.0, [-c for c in crop_c]))
    want = []
    for scene, rot, (_, scale, trans) in zip(scenes, rots, args.values()):
        moved = T.transform(scene, T.plan32(T.plan64(rot.astype(np.float32), scale, trans)))
        keep = T.box_keep(moved["pos"], box, crop_h) != 0
        assert 0 < keep.sum() < keep.size
        want.append({k: v[keep] for k, v in moved.items()})
    want = {k: np.concatenate([w[k] for w in want]) for k in KEYS}
    got = lcgs.read_gs_ply(out)
    assert got["pos"].shape == want["pos"].shape and f"{want['pos'].shape[0]} splats" in capsys.readouterr().out
    assert T.same_bits(got["pos"], want["pos"]) and T.same_bits(got["sh"], want["sh"])
    assert np.abs(got["scale"] / want["scale"] - 1).max() <= 2e-6
    assert np.abs(got["opacity"] - want["opacity"]).max() <= 1e-6
    unit = want["rotq"] / np.linalg.norm(want["rotq"].astype(np.float64), axis=1, keepdims=True)
    assert np.abs(got["rotq"] - unit).max() <= 1e-6
