"""`-m gpu`: a scene from a point cloud.  lcgs_knn_mean_dist2 against the brute-force float32 restatement (tests/knn_ref.py) with
ZERO tolerance -- the search is exact in the computed binary32 values, so pruning, chunking, the Morton sort and the order of the
input must leave no trace -- and lcgs_scene_init_from_points against 3DGS's create_from_pcd row by row, then as a scene that
renders and trains."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import DEV, assert_image_parity, dev
from knn_ref import mean_dist2_f32, mean_dist2_f64

pytestmark = pytest.mark.gpu

KEYS = ("pos", "scale", "rotq", "sh", "opacity")


def _chunk():
    import luisacomputegaussiansplatting_amd as L

    return L.api.LCGS_KNN_CHUNK  # the kernels' chunk size (include/lcgs_hip.h LCGS_KNN_CHUNK, static_assert-ed in abi_init.cpp)


def _blobs(rng):
    """three Gaussian blobs of sigma 1e-3, 1 and 100 + five outliers at distance 1e4: third-bests span ten orders of magnitude,
    so whether a far chunk is opened is decided by the bounds, not by luck"""
    parts = [rng.normal(0, s, (m, 3)) + c for s, m, c in ((1e-3, 1400, (0.3, 0.2, 0.1)), (1.0, 1400, (5, -3, 2)), (100.0, 1299, (-200, 50, 10)))]
    far = rng.normal(size=(5, 3))
    far *= 1e4 / np.linalg.norm(far, axis=1, keepdims=True)
    pos = np.concatenate(parts + [far]).astype(np.float32)
    return pos[rng.permutation(pos.shape[0])]


def _lattice(n):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def _plane_and_line(rng):
    plane = np.concatenate([rng.uniform(-2, 2, (3000, 2)), np.zeros((3000, 1))], axis=1)
    line = np.array([1.0, -2.0, 0.5]) + rng.uniform(-3, 3, (3000, 1)) * np.array([0.3, 0.5, -0.8])
    return np.concatenate([plane, line]).astype(np.float32)


def _make(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    C = _chunk()
    sizes = {"n1": 1, "n2": 2, "n3": 3, "n4": 4, "C-1": C - 1, "C": C, "C+1": C + 1, "2C+1": 2 * C + 1}
    if name in sizes:
        return rng.normal(0, 1, (sizes[name], 3)).astype(np.float32)
    if name == "uniform4096":
        return rng.uniform(0, 1, (4096, 3)).astype(np.float32)
    if name == "blobs4099":
        return _blobs(rng)
    if name == "lattice16":
        return _lattice(16)
    if name == "repeated4x1000":
        return np.repeat(rng.normal(0, 1, (1000, 3)).astype(np.float32), 4, axis=0)[rng.permutation(4000)]
    if name == "plane_and_line":
        return _plane_and_line(rng)
    raise KeyError(name)


CLOUDS = ("n1", "n2", "n3", "n4", "C-1", "C", "C+1", "2C+1", "uniform4096", "blobs4099", "lattice16", "repeated4x1000",
          "plane_and_line")


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(points, float32 restatement, float64 restatement): computed once, shared, read-only"""
    pos = _make(name)
    out = (pos, mean_dist2_f32(pos), mean_dist2_f64(pos))
    for a in out:
        a.setflags(write=False)
    return out


def _knn(lcgs, ctx, pos):
    out = lcgs.knn_mean_dist2(ctx, dev(pos))
    ctx.synchronize()
    return out.cpu().numpy()


def _assert_bits(got, want, tag):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        i = int(np.nonzero(~same)[0][0])
        raise AssertionError(f"{tag}: {int((~same).sum())} of {same.size} values differ from the float32 restatement; first at "
                             f"{i}: got {got[i]!r}, want {want[i]!r}")


@pytest.mark.parametrize("name", CLOUDS)
def test_knn_equals_the_float32_restatement_bit_for_bit(lcgs, name):
    pos, ref32, ref64 = _cloud(name)
    got = _knn(lcgs, lcgs.Context(0), pos)
    _assert_bits(got, ref32, name)
    nz = ref64 != 0
    assert np.allclose(got[nz], ref64[nz], rtol=1e-6, atol=0.0), name
    if name == "lattice16":
        assert (got == 1.0).all()
    if name == "repeated4x1000":
        assert not got.any()
    if name == "n1":
        assert got[0] == 0.0


def test_knn_is_independent_of_the_order_of_the_points(lcgs):
    pos, ref32, _ = _cloud("blobs4099")
    perm = np.random.default_rng(11).permutation(pos.shape[0])
    ctx = lcgs.Context(0)
    _assert_bits(_knn(lcgs, ctx, pos[perm]), _knn(lcgs, ctx, pos)[perm], "permuted blobs")
    _assert_bits(_knn(lcgs, ctx, pos[perm]), ref32[perm], "permuted blobs vs restatement")


def test_knn_non_finite_rows_give_zero_and_are_nobodys_neighbour(lcgs):
    rng = np.random.default_rng(12)
    pos = rng.normal(0, 1, (1000, 3)).astype(np.float32)
    bad = np.array([0, 1, 255, 256, 500, 777, 999])
    pos[bad] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 1], [1, np.nan, np.inf],
                [-np.inf, 2, 3]]
    got = _knn(lcgs, lcgs.Context(0), pos)
    keep = np.setdiff1d(np.arange(1000), bad)
    assert not got[bad].any() and keep.size == 993
    _assert_bits(got[keep], mean_dist2_f32(pos[keep]), "the 993 finite rows")


def test_knn_workspace_grows_and_is_reused(lcgs):
    rng = np.random.default_rng(13)
    big, small = rng.normal(0, 1, (5000, 3)).astype(np.float32), rng.normal(0, 1, (300, 3)).astype(np.float32)
    ctx = lcgs.Context(0)
    first, second, third = _knn(lcgs, ctx, big), _knn(lcgs, ctx, small), _knn(lcgs, ctx, big)
    _assert_bits(third, first, "5000 again")
    _assert_bits(second, mean_dist2_f32(small), "300 after 5000")
    _assert_bits(first, mean_dist2_f32(big), "5000")
    assert lcgs.knn_mean_dist2(ctx, torch.empty(0, 3, device=DEV)).shape == (0,)


# ---- lcgs_scene_init_from_points ------------------------------------------------------------------------------------------
def _init_cloud():
    """2000 points: 1900 uniform in a ball of radius 0.6 about (0, 0, 0.5) + 25 points four times each (duplicates: dist2 = 0)"""
    rng = np.random.default_rng(21)
    d = rng.normal(size=(1900, 3))
    ball = d / np.linalg.norm(d, axis=1, keepdims=True) * 0.6 * rng.uniform(0, 1, (1900, 1)) ** (1 / 3) + [0, 0, 0.5]
    dup = np.repeat(rng.normal(0, 0.2, (25, 3)) + [0, 0, 0.5], 4, axis=0)
    pos = np.concatenate([ball, dup]).astype(np.float32)
    order = rng.permutation(2000)
    return pos[order], rng.uniform(0, 1, (2000, 3)).astype(np.float32), np.nonzero(order >= 1900)[0]


def _ulps(got, want64):
    """|got - want| in units of the binary32 ulp at want"""
    want32 = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want32)).astype(np.float64)


_INIT_RESULTS = {}  # sh_degree -> the first variant's (raw, activated): the other variant must write the same rows


@pytest.mark.parametrize("aliased", [True, False])
@pytest.mark.parametrize("sh_degree", [3, 1])
def test_init_from_points_writes_create_from_pcd_rows(lcgs, sh_degree, aliased):
    """Raw scale: within 4 binary32 ulps of float64 log(sqrt(max(d2, min_dist2))), d2 the binary32 value the tests above pin.  The
    budget: sqrtf 1 (correctly rounded under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; its relative error reaches
    the logarithm as an ABSOLUTE error of the same size, below one ulp of the result because every expected value here has
    magnitude >= 1, asserted on the reference) + device logf 2 + the final rounding of the reference itself 1.  The HIP
    documentation's single-precision accuracy table (HIP math API, logf and sqrtf at 1 ulp) is within these figures; no copy
    of that table ships with the toolkit, so the issue's figures are kept as they were set.
    Activated scale / opacity: against the float64 activation of the raw values the call wrote, at the tolerance
    tests/test_gpu_train.py:75-77 holds the same two expressions to (rtol 2e-5, atol 2e-6)."""
    pos, rgb, dup_rows = _init_cloud()
    n, feat, min_dist2 = pos.shape[0], (sh_degree + 1) ** 2 * 3, 1e-7
    r = lcgs.Renderer(lcgs.Context(0))
    d_pos, d_rgb = dev(pos), dev(rgb)
    d2 = lcgs.knn_mean_dist2(r.ctx, d_pos).cpu().numpy()
    _assert_bits(d2, mean_dist2_f32(pos), "init cloud")
    assert not d2[dup_rows].any() and (d2[np.setdiff1d(np.arange(n), dup_rows)] > 0).all()
    if aliased:
        raw, act = r.init_from_points(d_pos, d_rgb, sh_degree=sh_degree, initial_opacity=0.1, min_dist2=min_dist2)
        assert act["pos"] is raw["pos"] and act["sh"] is raw["sh"]
    else:
        shapes = {"pos": (n, 3), "scale": (n, 3), "rotq": (n, 4), "sh": (n, feat), "opacity": (n,)}
        raw = {k: torch.full(s, 7.0, device=DEV) for k, s in shapes.items()}
        act = {k: torch.full(s, 9.0, device=DEV) for k, s in shapes.items()}
        r.init_from_points_into(d_pos, d_rgb, raw, act, sh_degree=sh_degree, initial_opacity=0.1, min_dist2=min_dist2)
    r.ctx.synchronize()
    raw, act = ({k: t.cpu().numpy() for k, t in d.items()} for d in (raw, act))
    # ---- bit-equal rows
    for d in (raw, act):
        assert np.array_equal(d["pos"], pos)
        sh = d["sh"].reshape(n, -1, 3)
        assert sh.shape[1] == (sh_degree + 1) ** 2
        assert np.array_equal(sh[:, 0, :], (rgb - np.float32(0.5)) / np.float32(0.28209479177387814))
        assert not sh[:, 1:, :].any()
        assert np.array_equal(d["rotq"], np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)))
    p = np.float64(np.float32(0.1))
    assert np.array_equal(raw["opacity"], np.full(n, np.float32(np.log(p / (1 - p)))))
    # ---- raw scale
    want = np.log(np.sqrt(np.maximum(d2.astype(np.float64), np.float64(np.float32(min_dist2)))))
    assert (np.abs(want) >= 1.0).all()  # (the cloud's nearest-neighbour distances are far below 1: see the docstring)
    assert np.array_equal(raw["scale"][:, 0], raw["scale"][:, 1]) and np.array_equal(raw["scale"][:, 0], raw["scale"][:, 2])
    u = _ulps(raw["scale"][:, 0], want)
    print(f"[init rows] deg {sh_degree}: raw scale worst {u.max():.2f} ulp; duplicates {_ulps(raw['scale'][dup_rows, 0], want[dup_rows]).max():.2f} ulp")
    assert u.max() <= 4.0, u.max()
    floor = 0.5 * np.log(np.float64(np.float32(min_dist2)))
    assert _ulps(raw["scale"][dup_rows, 0], np.full(dup_rows.size, floor)).max() <= 4.0
    # ---- activated values against the float64 activation of what the call wrote (tests/test_gpu_train.py:75-77)
    assert np.allclose(act["scale"].astype(np.float64), np.exp(raw["scale"].astype(np.float64)), rtol=2e-5, atol=2e-6)
    assert np.allclose(act["opacity"].astype(np.float64), 1 / (1 + np.exp(-raw["opacity"].astype(np.float64))), rtol=2e-5, atol=2e-6)
    # ---- aliased and separate packs hold the same rows
    other = _INIT_RESULTS.setdefault(sh_degree, (raw, act))
    for mine, theirs in zip((raw, act), other):
        for k in KEYS:
            assert np.array_equal(mine[k], theirs[k]), (k, "aliased vs separate packs")


def test_initialised_rows_are_a_scene_that_renders_and_trains(lcgs, oracle):
    pos, rgb, _ = _init_cloud()
    n, W, H = pos.shape[0], 128, 96
    pose = ([-2.2, -0.4, 1.6], [0, 0, 0.5], [0, 0, 1])
    r = lcgs.Renderer(lcgs.Context(0))
    raw, act = r.init_from_points(dev(pos), dev(rgb), sh_degree=3)
    r.bind_scene(*[act[k] for k in KEYS])
    img = torch.zeros(3, H, W, device=DEV)
    assert r.forward(lcgs.get_lookat_cam(*pose, width=W, height=H), img, keep_state=True, sync=True) > 0
    scene = r.download_scene()
    for k in KEYS:
        assert np.array_equal(scene[k], act[k].cpu().numpy()), k
    ref = oracle.render(scene, oracle.lookat(*pose, width=W, height=H))
    assert (ref["img"] != 0.0).any(), "the oracle's frame is all background: the pose does not see the cloud"
    assert_image_parity(img.cpu().numpy(), ref)
    # one optimiser step from zero moments
    grads = {k: torch.zeros_like(raw[k]) for k in KEYS}
    dL = torch.from_numpy(np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32)).to(DEV)
    r.backward(dL, *[grads[k] for k in KEYS])
    m, v = ({k: torch.zeros_like(raw[k]) for k in KEYS} for _ in range(2))
    lr = {"pos": 1.6e-4, "sh_dc": 2.5e-3, "sh_rest": 1.25e-4, "opacity": 5e-2, "scale": 5e-3, "rot": 1e-3}
    before = {k: raw[k].clone() for k in KEYS}
    r.adam_step(grads, raw, m, v, act, 1, lr)
    r.ctx.synchronize()
    for k in KEYS:
        assert torch.isfinite(raw[k]).all() and torch.isfinite(act[k]).all(), k
    assert any(not torch.equal(before[k], raw[k]) for k in KEYS), "the step moved nothing"
