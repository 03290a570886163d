"""A scene from a point cloud, without a GPU: the five entry points are exported, refuse bad arguments before anything touches a
device, and the two host-only ones (camera extent, point-cloud PLY reader) compute what they say."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("lcgs_knn_mean_dist2", "lcgs_scene_init_from_points", "lcgs_scene_extent", "lcgs_points_read_ply", "lcgs_points_free")


def test_symbols_are_exported_and_listed(lcgs):
    lib = lcgs.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
    for fn in ("knn_mean_dist2", "scene_extent", "read_points_ply"):
        assert callable(getattr(lcgs, fn))
    assert callable(lcgs.Renderer.init_from_points)
    hdr = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    assert int(re.search(r"#define\s+LCGS_KNN_CHUNK\s+(\d+)", hdr).group(1)) == lcgs.api.LCGS_KNN_CHUNK


def test_bad_arguments_are_refused_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    ctx, buf = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced: every call below is refused by its checks
    good = lcgs.api._InitConfig(0.1, 1e-7)
    nulls = lcgs.api._Params(None, None, None, None, None)
    pack = lcgs.api._Params(buf, buf, buf, buf, buf)
    p, cfg = C.byref(pack), C.byref(good)
    knn, init = lib.lcgs_knn_mean_dist2, lib.lcgs_scene_init_from_points
    assert knn(None, 4, buf, buf) == 1 and b"NULL" in lib.lcgs_last_error()
    assert knn(ctx, -1, buf, buf) == 1
    assert knn(ctx, 2 ** 31, buf, buf) == 1 and b"2^31" in lib.lcgs_last_error()
    assert knn(ctx, 2 ** 40, buf, buf) == 1
    assert knn(ctx, 4, None, buf) == 1 and knn(ctx, 4, buf, None) == 1
    assert knn(ctx, 0, None, None) == 0  # nothing to do, nothing touched
    assert init(None, 4, 3, buf, buf, cfg, p, p) == 1
    assert init(ctx, 4, 3, buf, buf, None, p, p) == 1
    assert init(ctx, 4, 3, buf, buf, cfg, None, p) == 1 and init(ctx, 4, 3, buf, buf, cfg, p, None) == 1
    assert init(ctx, -1, 3, buf, buf, cfg, p, p) == 1
    assert init(ctx, 4, 4, buf, buf, cfg, p, p) == 1 and init(ctx, 4, -1, buf, buf, cfg, p, p) == 1
    assert init(ctx, 4, 3, None, buf, cfg, p, p) == 1 and init(ctx, 4, 3, buf, None, cfg, p, p) == 1
    assert init(ctx, 4, 3, buf, buf, cfg, C.byref(nulls), p) == 1 and init(ctx, 4, 3, buf, buf, cfg, p, C.byref(nulls)) == 1
    for opacity in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert init(ctx, 4, 3, buf, buf, C.byref(lcgs.api._InitConfig(opacity, 1e-7)), p, p) == 1, opacity
    assert b"initial_opacity" in lib.lcgs_last_error()
    for floor in (0.0, -1e-7, float("nan")):
        assert init(ctx, 4, 3, buf, buf, C.byref(lcgs.api._InitConfig(0.1, floor)), p, p) == 1, floor
    assert b"min_dist2" in lib.lcgs_last_error()
    assert init(ctx, 0, 3, None, None, cfg, p, p) == 0


@pytest.mark.parametrize("n", [1, 2, 8])
def test_scene_extent_is_the_float64_formula_rounded_once(lcgs, n):
    rng = np.random.default_rng(n)
    positions = rng.normal(0, 3, (n, 3)).astype(np.float32)
    cams = [lcgs.get_lookat_cam(p, [0, 0, 0.5], [0, 0, 1], width=64, height=48) for p in positions]
    assert all(np.array_equal(np.array(c.position, np.float32), p) for c, p in zip(cams, positions))
    center, radius = lcgs.scene_extent(cams)
    p64 = positions.astype(np.float64)
    c64 = p64.mean(axis=0)
    r64 = 1.1 * np.linalg.norm(p64 - c64, axis=1).max()
    assert center.dtype == np.float32 and np.array_equal(center, c64.astype(np.float32))
    assert np.float32(radius) == np.float32(r64)
    assert (radius == 0.0) == (n == 1)


def test_scene_extent_refuses_no_cameras(lcgs):
    lib = lcgs.load_library()
    out = np.zeros(4, np.float32)
    cam = lcgs.Camera()
    assert lib.lcgs_scene_extent(0, C.byref(cam), out.ctypes.data, out.ctypes.data + 12) == 1
    assert lib.lcgs_scene_extent(1, None, out.ctypes.data, out.ctypes.data + 12) == 1
    assert lib.lcgs_scene_extent(1, C.byref(cam), None, out.ctypes.data + 12) == 1
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.scene_extent([])
    assert e.value.status == 1


# ---- the point-cloud reader against files written here -------------------------------------------------------------------
def _header(n, props, fmt="binary_little_endian"):
    return ("ply\nformat %s 1.0\ncomment a point cloud\nelement vertex %d\n" % (fmt, n) +
            "".join(f"property {t} {name}\n" for t, name in props) + "element face 0\nproperty list uchar int vertex_indices\nend_header\n")


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 5, (n, 3)), rng.integers(0, 256, (n, 3)).astype(np.uint8)


def test_read_points_ply_colmap_layout(lcgs, tmp_path):
    """binary little-endian, float xyz + float normals + uchar rgb: what COLMAP's model converter writes"""
    n = 1234
    xyz, rgb = _cloud(n, 0)
    xyz = xyz.astype(np.float32)
    props = [("float", k) for k in ("x", "y", "z", "nx", "ny", "nz")] + [("uchar", k) for k in ("red", "green", "blue")]
    rec = np.zeros(n, dtype=[("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)])
    rec["p"], rec["n"], rec["c"] = xyz, 7.0, rgb
    path = tmp_path / "colmap.ply"
    path.write_bytes(_header(n, props).encode() + rec.tobytes())
    got = lcgs.read_points_ply(str(path))
    assert got["pos"].dtype == got["rgb"].dtype == np.float32 and got["pos"].shape == got["rgb"].shape == (n, 3)
    assert np.array_equal(got["pos"], xyz)
    assert np.array_equal(got["rgb"], rgb.astype(np.float32) / np.float32(255))  # bit for bit
    assert got["rgb"].min() == 0.0 and got["rgb"].max() == 1.0


def test_read_points_ply_double_positions_and_other_order(lcgs, tmp_path):
    n = 77
    xyz, rgb = _cloud(n, 1)
    props = [("uchar", "red"), ("uchar", "green"), ("uchar", "blue"), ("short", "label"), ("double", "x"), ("double", "y"),
             ("double", "z")]
    rec = np.zeros(n, dtype=[("c", "u1", 3), ("l", "<i2"), ("p", "<f8", 3)])
    rec["c"], rec["l"], rec["p"] = rgb, -3, xyz
    path = tmp_path / "double.ply"
    path.write_bytes(_header(n, props).encode() + rec.tobytes())
    got = lcgs.read_points_ply(str(path))
    assert np.array_equal(got["pos"], xyz.astype(np.float32))
    assert np.array_equal(got["rgb"], rgb.astype(np.float32) / np.float32(255))


def test_read_points_ply_ascii(lcgs, tmp_path):
    n = 41
    xyz, rgb = _cloud(n, 2)
    xyz = xyz.astype(np.float32)
    props = [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    rows = "".join("%r %r %r %d %d %d\n" % (*[float(v) for v in p], *c) for p, c in zip(xyz, rgb))
    path = tmp_path / "ascii.ply"
    path.write_text(_header(n, props, "ascii") + rows)
    got = lcgs.read_points_ply(str(path))
    assert np.array_equal(got["pos"], xyz)
    assert np.array_equal(got["rgb"], rgb.astype(np.float32) / np.float32(255))


def test_read_points_ply_float_colours_are_taken_as_they_are(lcgs, tmp_path):
    n = 300
    rng = np.random.default_rng(3)
    xyz, rgb = rng.normal(size=(n, 3)).astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32)
    props = [("float", k) for k in ("x", "y", "z", "red", "green", "blue")]
    path = tmp_path / "float.ply"
    path.write_bytes(_header(n, props).encode() + np.concatenate([xyz, rgb], axis=1).astype("<f4").tobytes())
    got = lcgs.read_points_ply(str(path))
    assert np.array_equal(got["pos"], xyz) and np.array_equal(got["rgb"], rgb)


def test_read_points_ply_errors_and_empty(lcgs, tmp_path):
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.read_points_ply(str(tmp_path / "missing.ply"))
    assert e.value.status == 6
    no_z = tmp_path / "no_z.ply"
    props = [("float", "x"), ("float", "y"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    no_z.write_bytes(_header(1, props).encode() + struct.pack("<ffBBB", 1.0, 2.0, 3, 4, 5))
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.read_points_ply(str(no_z))
    assert e.value.status == 7 and "`z`" in str(e.value)
    short = tmp_path / "short.ply"
    props = [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    short.write_bytes(_header(2, props).encode() + struct.pack("<fffBBB", 1.0, 2.0, 3.0, 3, 4, 5))
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.read_points_ply(str(short))
    assert e.value.status == 7
    empty = tmp_path / "empty.ply"
    empty.write_bytes(_header(0, props).encode())
    got = lcgs.read_points_ply(str(empty))
    assert got["pos"].shape == got["rgb"].shape == (0, 3) and got["pos"].dtype == np.float32
    lib = lcgs.load_library()
    assert lib.lcgs_points_read_ply(None, None, None, None) == 1
    lib.lcgs_points_free(None, None)  # like free(): NULL is fine
