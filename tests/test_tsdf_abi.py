"""The TSDF / mesh entry points without a GPU: every argument check of lcgs_tsdf_integrate / _mesh_count / _mesh_extract that is
made before any device work (a stand-in context that is never dereferenced: the checks come first), the host PLY writer, and
the exported symbols."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

NAMES = ("lcgs_tsdf_integrate", "lcgs_tsdf_mesh_count", "lcgs_tsdf_mesh_extract", "lcgs_mesh_write_ply")
BAD = [float("nan"), float("inf"), 0.0, -1.0]


def test_exported_symbols_and_mirrors(lcgs):
    lib, api = lcgs.load_library(), lcgs.api
    for name in NAMES:
        assert name in api.EXPORTED_SYMBOLS and name in api.SIGNATURES and hasattr(lib, name)
    assert api.STRUCTS["lcgs_tsdf_volume"] is api._TsdfVolume and api.STRUCTS["lcgs_tsdf_config"] is api._TsdfConfig
    assert C.sizeof(api._TsdfVolume) == 56 and C.sizeof(api._TsdfConfig) == 12
    hdr = open(os.path.join(os.path.dirname(api.__file__), "..", "include", "lcgs_hip.h")).read()
    assert f"#define LCGS_TSDF_VIEW_CHUNK {api.LCGS_TSDF_VIEW_CHUNK}" in hdr
    for word in ("sparse or hashed volumes", "weight caps", "trilinear depth lookup", "median depth", "decimation or smoothing",
                 "lcgs-app flag", "any gradient"):
        assert word in hdr, word


class Call:
    """a valid lcgs_tsdf_integrate call on made-up addresses (never read: every check precedes the device work), one thing changed
    at a time"""

    def __init__(self, lcgs):
        self.L, self.lib, self.api = lcgs, lcgs.load_library(), lcgs.api
        self.ctx = C.create_string_buffer(1 << 16)  # the stand-in context
        self.n = 4 * 3 * 2
        self.vol = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, nx=4, ny=3, nz=2, d_tsdf=0x10000, d_weight=0x20000, d_rgb=0x30000)
        self.cfg = dict(trunc=0.2, depth_max=10.0, alpha_min=0.5)
        self.cams = [lcgs.get_lookat_cam([1, 1, 1], [0, 0, 0], [0, 0, 1], width=8, height=4) for _ in range(2)]
        self.depths, self.alphas, self.images = [0x40000, 0x50000], [0x60000, 0x70000], [0x80000, 0x90000]
        self.num_views = 2

    def run(self, ctx=True, vol=True, cfg=True, cams=True, table=True):
        a = self.api
        v = a._TsdfVolume(a._f3(self.vol["origin"]), *[self.vol[k] for k in ("voxel_size", "nx", "ny", "nz", "d_tsdf", "d_weight", "d_rgb")])
        c = a._TsdfConfig(*[self.cfg[k] for k in ("trunc", "depth_max", "alpha_min")])
        tab = lambda t: None if t is None else (C.c_void_p * len(t))(*t)
        st = self.lib.lcgs_tsdf_integrate(self.ctx if ctx else None, C.byref(v) if vol else None, C.byref(c) if cfg else None,
                                          self.num_views, (a.Camera * len(self.cams))(*self.cams) if cams else None,
                                          tab(self.depths) if table else None, tab(self.alphas), tab(self.images))
        return st, self.lib.lcgs_last_error().decode()


def test_integrate_refuses_bad_arguments_before_any_device_work(lcgs):
    def refused(what, **edit):
        c = Call(lcgs)
        run = {}
        for k, v in edit.items():
            if k in c.vol:
                c.vol[k] = v
            elif k in c.cfg:
                c.cfg[k] = v
            elif k in ("ctx", "vol", "cfg", "cams", "table"):
                run[k] = v
            else:
                setattr(c, k, v)
        st, msg = c.run(**run)
        assert st == 1 and msg.startswith("invalid argument") and what in msg, (edit, st, msg)

    for k in ("ctx", "cfg"):
        refused("NULL argument", **{k: False})
    refused("NULL volume", vol=False)
    refused("NULL cameras or d_depths", cams=False)
    refused("NULL cameras or d_depths", table=False)
    refused("NULL volume array", d_tsdf=None)
    refused("NULL volume array", d_weight=None)
    refused("NULL depth map", depths=[0x40000, None])
    for k in ("nx", "ny", "nz"):
        for bad in (0, -3):
            refused("dimension is below 1", **{k: bad})
    refused("more than 2^31 - 1 samples", nx=2048, ny=2048, nz=512, d_weight=0x1_0000_0000_0000, d_rgb=0x2_0000_0000_0000)
    for bad in BAD:
        refused("voxel_size", voxel_size=bad)
        for k in ("trunc", "depth_max", "alpha_min"):
            refused(k, **{k: bad})
    refused("origin", origin=(0.0, float("nan"), 0.0))
    refused("origin", origin=(float("inf"), 0.0, 0.0))
    refused("num_views is negative", num_views=-1)
    for k in ("width", "height"):
        c = Call(lcgs)
        setattr(c.cams[1], k, 0)
        st, msg = c.run()
        assert st == 1 and "width or height" in msg
    n = 24
    # volume arrays against each other (n floats, n floats, 3 n floats) ...
    refused("overlap each other", d_weight=0x10000 + 4 * (n - 1))
    refused("overlap each other", d_rgb=0x20000 - 4 * (3 * n - 1))
    refused("overlap each other", d_rgb=0x10000)
    # ... and against the maps of any view (8 x 4 pixels; the image is three planes)
    refused("overlaps an input map", depths=[0x40000, 0x10000 + 4 * (n - 1)])
    refused("overlaps an input map", alphas=[0x20000 - 4 * 31, 0x70000])
    refused("overlaps an input map", images=[0x80000, 0x30000 + 4 * (3 * n - 1)])
    refused("overlaps an input map", images=[0x30000 - 4 * 95, 0x90000])
    # adjacent is not overlapping: the checks pass and the call would reach the device -- not made here


def test_mesh_calls_refuse_bad_arguments_before_any_device_work(lcgs):
    lib, a = lcgs.load_library(), lcgs.api
    ctx = C.create_string_buffer(1 << 16)
    vol = a._TsdfVolume(a._f3((0, 0, 0)), 0.1, 4, 3, 2, 0x10000, 0x20000, None)
    nv, nt = C.c_uint64(7), C.c_uint64(7)
    out = (C.addressof(nv), C.addressof(nt))
    err = lambda: lib.lcgs_last_error().decode()
    assert lib.lcgs_tsdf_mesh_count(None, C.byref(vol), 1.0, *out) == 1
    assert lib.lcgs_tsdf_mesh_count(ctx, None, 1.0, *out) == 1 and "NULL volume" in err()
    assert lib.lcgs_tsdf_mesh_count(ctx, C.byref(vol), 1.0, None, out[1]) == 1
    assert lib.lcgs_tsdf_mesh_count(ctx, C.byref(vol), 1.0, out[0], None) == 1
    for bad in BAD:
        assert lib.lcgs_tsdf_mesh_count(ctx, C.byref(vol), bad, *out) == 1 and "weight_min" in err()
        assert lib.lcgs_tsdf_mesh_extract(ctx, C.byref(vol), bad, 10, 10, 0x50000, None, 0x60000, *out) == 1 and "weight_min" in err()
    assert lib.lcgs_tsdf_mesh_extract(None, C.byref(vol), 1.0, 10, 10, 0x50000, None, 0x60000, *out) == 1
    assert lib.lcgs_tsdf_mesh_extract(ctx, C.byref(vol), 1.0, 10, 10, None, None, 0x60000, *out) == 1 and "NULL output" in err()
    assert lib.lcgs_tsdf_mesh_extract(ctx, C.byref(vol), 1.0, 10, 10, 0x50000, None, None, *out) == 1 and "NULL output" in err()
    assert lib.lcgs_tsdf_mesh_extract(ctx, C.byref(vol), 1.0, 10, 10, 0x50000, 0x70000, 0x60000, *out) == 1 and "without colour" in err()
    bad_vol = a._TsdfVolume(a._f3((0, 0, 0)), 0.1, 4, 0, 2, 0x10000, 0x20000, None)
    assert lib.lcgs_tsdf_mesh_extract(ctx, C.byref(bad_vol), 1.0, 10, 10, 0x50000, None, 0x60000, *out) == 1 and "below 1" in err()
    assert (nv.value, nt.value) == (7, 7)  # a refused call writes nothing


def read_mesh_ply(path):
    """the test's own parser of the writer's layout -> (vertices [V, 3] float32, rgb [V, 3] uint8 or None, triangles [T, 3] int32)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    nt = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    props = [ln.split()[1:] for ln in lines if ln.startswith("property")]
    colour = ["uchar", "red"] in props
    assert props[:3] == [["float", "x"], ["float", "y"], ["float", "z"]] and props[-1] == ["list", "uchar", "int", "vertex_indices"]
    assert len(props) == (7 if colour else 4)
    vt = np.dtype([("p", "<f4", 3)] + ([("c", "u1", 3)] if colour else []))
    ft = np.dtype([("n", "u1"), ("i", "<i4", 3)])
    assert len(raw) == end + nv * vt.itemsize + nt * ft.itemsize
    v = np.frombuffer(raw, vt, nv, end)
    f = np.frombuffer(raw, ft, nt, end + nv * vt.itemsize)
    assert (f["n"] == 3).all()
    return v["p"].copy(), (v["c"].copy() if colour else None), f["i"].copy()


def test_mesh_ply_round_trip(lcgs, tmp_path):
    rng = np.random.default_rng(5)
    for nv, nt, colour in ((11, 7, True), (11, 7, False), (0, 0, True), (0, 0, False), (3, 0, True)):
        v = rng.normal(size=(nv, 3)).astype(np.float32)
        t = rng.integers(0, max(nv, 1), (nt, 3)).astype(np.uint32)
        c = rng.uniform(-0.2, 1.2, (nv, 3)).astype(np.float32) if colour else None
        if colour and nv:
            c[0] = [0.0, 1.0, np.nan]
            c[1] = [0.5, 127.4 / 255, 127.6 / 255]
        path = str(tmp_path / f"m_{nv}_{nt}_{colour}.ply")
        lcgs.write_mesh_ply(path, v, t, c)
        gv, gc, gt = read_mesh_ply(path)
        assert np.array_equal(gv.view(np.uint32), v.view(np.uint32)) and np.array_equal(gt, t.astype(np.int32))
        if colour:
            want = np.floor(np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0), 0, 1).astype(np.float32) * np.float32(255) + np.float32(0.5))
            assert np.array_equal(gc, want.astype(np.uint8)), (gc[:2], want[:2])
        else:
            assert gc is None


def test_mesh_ply_io_errors(lcgs, tmp_path):
    lib = lcgs.load_library()
    v, t = np.zeros((1, 3), np.float32), np.zeros((1, 3), np.uint32)
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.write_mesh_ply(str(tmp_path / "no_such_dir" / "m.ply"), v, t)
    assert e.value.status == 6
    assert lib.lcgs_mesh_write_ply(None, 0, None, None, 0, None) == 1
    assert lib.lcgs_mesh_write_ply(str(tmp_path / "x.ply").encode(), 1, None, None, 0, None) == 1
    assert lib.lcgs_mesh_write_ply(str(tmp_path / "x.ply").encode(), 0, None, None, 1, None) == 1
    assert not os.path.exists(tmp_path / "x.ply")
