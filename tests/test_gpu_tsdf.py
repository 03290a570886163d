"""TSDF fusion and the marching-tetrahedra mesh on the GPU (lcgs_tsdf_integrate, lcgs_tsdf_mesh_count / _extract) against their
NumPy restatement (tests/tsdf_ref.py): the volume bit for bit on every sample the restatement decides (the undecided ones -- a
pixel coordinate within 16 ulp of an integer, where the host's tanf may tip it -- hold one of the values the restatement allows;
their share is capped in tests/test_tsdf_ref.py), the mesh bit for bit and index for index, in order."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tsdf_ref as R
from gpu_util import DEV, dev
from test_tsdf_abi import read_mesh_ply

pytestmark = pytest.mark.gpu
CHUNK = R.VIEW_CHUNK


def u32(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def renderer(lcgs):
    assert lcgs.api.LCGS_TSDF_VIEW_CHUNK == CHUNK
    return lcgs.Renderer(lcgs.Context(0))


_DEVICE_MAPS = {}


def on_device(a):
    if a is None:
        return None
    if id(a) not in _DEVICE_MAPS:
        _DEVICE_MAPS[id(a)] = (a, dev(a))  # (the array is kept: its id stays its own)
    return _DEVICE_MAPS[id(a)][1]


def unaligned(n):
    """n zeroed device floats that start 4 bytes past a 16-byte boundary"""
    t = torch.zeros(n + 1, device=DEV)[1:]
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def integrate(lcgs, renderer, lattice, views, with_rgb=True, volume=None, splits=None, off_alignment=False):
    """the views through lcgs_tsdf_integrate, one call per entry of `splits` (view counts; default: one call) -> the volume"""
    origin, voxel, dims = R.LATTICES[lattice]
    n = dims[0] * dims[1] * dims[2]
    if volume is None:
        if off_alignment:
            volume = lcgs.TsdfVolume.from_tensors(origin, voxel, dims, unaligned(n), unaligned(n), unaligned(3 * n) if with_rgb else None)
        else:
            volume = lcgs.TsdfVolume(origin, voxel, dims, rgb=with_rgb, device=DEV)
    first = 0
    for count in splits or [len(views)]:
        vs = views[first:first + count]
        alphas, images = [on_device(v["alpha"]) for v in vs], [on_device(v["image"]) for v in vs]
        renderer.tsdf_integrate(volume, [v["cam"] for v in vs], [on_device(v["depth"]) for v in vs],
                                None if all(a is None for a in alphas) else alphas, None if all(i is None for i in images) else images,
                                trunc=R.CFG[0], depth_max=R.CFG[1], alpha_min=R.CFG[2])
        first += count
    assert first == len(views)
    renderer.ctx.synchronize()
    return volume


def state_bits(volume):
    return [None if t is None else u32(t).ravel() for t in (volume.tsdf, volume.weight, volume.rgb)]


def assert_volume_is_the_restatement(lcgs, lattice, views, volume, ref, with_rgb, tag):
    origin, voxel, dims = R.LATTICES[lattice]
    got = state_bits(volume)
    n = got[0].size
    rows = np.concatenate([got[0][:, None], got[1][:, None], got[2].reshape(n, 3) if with_rgb else np.zeros((n, 3), np.uint32)], axis=1)
    want = np.concatenate([u32(ref["tsdf"])[:, None], u32(ref["weight"])[:, None],
                           u32(ref["rgb"]) if with_rgb else np.zeros((n, 3), np.uint32)], axis=1)
    decided = ~ref["undecided"].any(axis=1)
    differ = (rows != want).any(axis=1)
    print(f"[tsdf] {tag}: {n} samples, {int((~decided).sum())} undecided, {int(differ.sum())} differ from the computed restatement, "
          f"{int((ref['weight'] > 0).sum())} touched")
    assert not (differ & decided).any(), (tag, np.nonzero(differ & decided)[0][:8], rows[differ & decided][:4], want[differ & decided][:4])
    for s in np.nonzero(~decided)[0]:  # one of the values the undecided views allow
        allowed = R.sample_outcomes(lcgs, origin, voxel, dims, views, R.CFG, int(s), ref["undecided"][s], with_rgb)
        assert rows[s].view(np.float32).tobytes() in allowed, (tag, int(s), rows[s].view(np.float32))


# ------------------------------------------------------------------------------------------------------------- integrate
@pytest.mark.parametrize("lattice", list(R.LATTICES))
@pytest.mark.parametrize("alpha, image", [(True, True), (False, True), (True, False)])
def test_integrate_is_the_restatement_bit_for_bit(lcgs, renderer, lattice, alpha, image):
    origin, voxel, dims = R.LATTICES[lattice]
    views = R.variant(R.views(lcgs, 5), alpha, image)
    with_rgb = image  # (a volume with colour and views without: the last case of the batching test)
    ref = R.integrate(lcgs, origin, voxel, dims, views, R.CFG, with_rgb=with_rgb)
    volume = integrate(lcgs, renderer, lattice, views, with_rgb)
    assert_volume_is_the_restatement(lcgs, lattice, views, volume, ref, with_rgb, f"{lattice} alpha={alpha} image={image}")
    w = volume.weight.cpu().numpy().ravel()
    assert np.array_equal(w, np.rint(w)) and w.max() <= 5 and (lattice == "one" or w.max() >= 2)  # weights are exact counts
    if lattice == "one":
        assert w[0] >= 1


def test_no_views_and_views_without_colour_leave_the_arrays_alone(lcgs, renderer):
    views = R.variant(R.views(lcgs, 5), True, False)
    volume = integrate(lcgs, renderer, "odd", views, with_rgb=True)
    assert not volume.rgb.any() and volume.weight.any()
    before = state_bits(volume)
    renderer.tsdf_integrate(volume, [], [], trunc=R.CFG[0], depth_max=R.CFG[1], alpha_min=R.CFG[2])
    renderer.ctx.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, state_bits(volume)))


# -------------------------------------------------------------------------------------------------------------- batching
def test_a_batch_leaves_the_bits_of_one_call_per_view(lcgs, renderer):
    every = R.views(lcgs, 2 * CHUNK + 3)
    for count in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        views = every[:count]
        batch = state_bits(integrate(lcgs, renderer, "odd", views))
        single = state_bits(integrate(lcgs, renderer, "odd", views, splits=[1] * count))
        assert all(np.array_equal(a, b) for a, b in zip(batch, single)), count
        split = state_bits(integrate(lcgs, renderer, "odd", views, splits=[40, count - 40]))
        assert all(np.array_equal(a, b) for a, b in zip(batch, split)), count
    # ... arrays 4 bytes off 16-byte alignment
    off = state_bits(integrate(lcgs, renderer, "odd", every, off_alignment=True))
    assert all(np.array_equal(a, b) for a, b in zip(batch, off))
    # ... and a second call on top of an existing volume continues the running mean
    volume = integrate(lcgs, renderer, "odd", every[:7])
    volume = integrate(lcgs, renderer, "odd", every[7:], volume=volume)
    assert all(np.array_equal(a, b) for a, b in zip(batch, state_bits(volume)))
    # the whole batch against the restatement as well
    origin, voxel, dims = R.LATTICES["odd"]
    ref = R.integrate(lcgs, origin, voxel, dims, every[:CHUNK + 1], R.CFG)
    assert_volume_is_the_restatement(lcgs, "odd", every[:CHUNK + 1], integrate(lcgs, renderer, "odd", every[:CHUNK + 1]), ref, True,
                                     f"odd, {CHUNK + 1} views")


# ------------------------------------------------------------------------------------------------------------------ mesh
def upload(lcgs, name):
    t, w, rgb, origin, voxel, dims = R.mesh_case(name)
    return lcgs.TsdfVolume.from_tensors(origin, voxel, dims, dev(t), dev(w), None if rgb is None else dev(rgb))


def raw_extract(lcgs, renderer, volume, cap_v, cap_t, colour):
    """lcgs_tsdf_mesh_extract into buffers pre-filled with a pattern -> (status, nv, nt, vertices, rgb, triangles)"""
    lib, a = lcgs.load_library(), lcgs.api
    v = torch.full((max(cap_v, 1), 3), -7.5, device=DEV)
    c = torch.full((max(cap_v, 1), 3), -7.5, device=DEV) if colour else None
    t = torch.full((max(cap_t, 1), 3), -77, dtype=torch.int32, device=DEV)
    nv, nt = C.c_uint64(123), C.c_uint64(456)
    vol = volume._struct()
    st = lib.lcgs_tsdf_mesh_extract(renderer.ctx._h, C.byref(vol), 1.0, cap_v, cap_t, a._ptr(v), a._ptr(c), a._ptr(t), C.addressof(nv),
                                    C.addressof(nt))
    renderer.ctx.synchronize()
    return st, nv.value, nt.value, v.cpu().numpy(), None if c is None else c.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("name", R.MESH_CASES)
def test_mesh_is_the_restatement_bit_for_bit_in_order(lcgs, renderer, name):
    t, w, rgb, origin, voxel, dims = R.mesh_case(name)
    ref = R.mesh(t, w, origin, voxel, dims, rgb=rgb)
    volume = upload(lcgs, name)
    nv, nt = renderer.tsdf_mesh_count(volume, 1.0)
    assert (nv, nt) == (len(ref["vertices"]), len(ref["triangles"]))
    vertices, colours, triangles = renderer.tsdf_mesh(volume, 1.0)
    assert vertices.shape == (nv, 3) and triangles.shape == (nt, 3) and triangles.dtype == torch.int64
    assert np.array_equal(u32(vertices), u32(ref["vertices"]))
    assert np.array_equal(triangles.cpu().numpy(), ref["triangles"])
    if rgb is None:
        assert colours is None
    else:
        assert np.array_equal(u32(colours), u32(ref["rgb"]))
    if name in ("cell_inside", "flat"):
        assert (nv, nt) == (0, 0)
    # the same again: same inputs, same bits (the scratch is reused)
    v2, c2, t2 = renderer.tsdf_mesh(volume, 1.0)
    assert torch.equal(v2, vertices) and torch.equal(t2, triangles)


def test_mesh_capacity_one_short_is_refused_with_the_counts_and_nothing_written(lcgs, renderer):
    volume = upload(lcgs, "sphere")
    nv, nt = renderer.tsdf_mesh_count(volume, 1.0)
    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1), (0, 0)):
        st, gv, gt, v, c, t = raw_extract(lcgs, renderer, volume, cap_v, cap_t, True)
        assert st == lcgs.api.LCGS_ERR_CAPACITY and (gv, gt) == (nv, nt)
        assert (v == -7.5).all() and (c == -7.5).all() and (t == -77).all()
    # the context's next call works, and capacities to spare leave the rest of the buffers alone
    st, gv, gt, v, c, t = raw_extract(lcgs, renderer, volume, nv + 3, nt + 2, True)
    tt, w, rgb, origin, voxel, dims = R.mesh_case("sphere")
    ref = R.mesh(tt, w, origin, voxel, dims, rgb=rgb)
    assert st == 0 and (gv, gt) == (nv, nt)
    assert np.array_equal(u32(v[:nv]), u32(ref["vertices"])) and np.array_equal(u32(c[:nv]), u32(ref["rgb"]))
    assert np.array_equal(t[:nt].astype(np.int64), ref["triangles"])
    assert (v[nv:] == -7.5).all() and (c[nv:] == -7.5).all() and (t[nt:] == -77).all()
    # weight_min above every weight: an empty mesh, LCGS_OK
    assert renderer.tsdf_mesh_count(volume, 1.5) == (0, 0)


# ------------------------------------------------------------------------------------------------------------ end to end
def shell_scene(P=4000, radius=0.5):
    """opaque splats flattened onto the sphere |X| = radius: the surface the renderer's depth maps see"""
    k = np.arange(P) + 0.5
    phi, theta = np.arccos(1 - 2 * k / P), np.pi * (1 + 5 ** 0.5) * k
    nrm = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)
    q = np.concatenate([1 + nrm[:, 2:3], -nrm[:, 1:2], nrm[:, 0:1], np.zeros((P, 1))], axis=1)  # rotates e_z onto the normal
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    sh = np.zeros((P, 48), np.float32)
    sh[:, :3] = 0.4 * nrm / 0.28209479177387814  # colour 0.5 + 0.4 n
    return {"pos": (radius * nrm).astype(np.float32), "scale": np.tile(np.float32([0.035, 0.035, 0.002]), (P, 1)),
            "rotq": q.astype(np.float32), "sh": sh, "opacity": np.full(P, 0.995, np.float32)}


def test_renderer_to_mesh_end_to_end(lcgs, renderer, tmp_path):
    scene = {k: dev(v) for k, v in shell_scene().items()}
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[scene[k] for k in ("pos", "scale", "rotq", "sh", "opacity")])
    W = H = 96
    eyes = [(1.6, 0.3, 0.4), (-1.5, 0.5, 0.3), (0.2, 1.7, -0.3), (0.4, -1.6, 0.5), (0.3, 0.5, 1.7), (-0.4, 0.3, -1.6)]
    cams = [lcgs.get_lookat_cam(list(e), [0.01, -0.02, 0.015], [0.0, 0.0, 1.0] if abs(e[2]) < 1 else [0.0, 1.0, 0.0], width=W, height=H,
                                fov=40.0) for e in eyes]
    origin, voxel, dims = (-0.78, -0.78, -0.78), 0.04, (40, 40, 40)
    volume = lcgs.TsdfVolume(origin, voxel, dims, rgb=True, device=DEV)
    maps = []
    for cam in cams:
        img, depth, alpha = torch.zeros(3, H, W, device=DEV), torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV)
        r.forward(cam, img, keep_state=True, sync=True)
        r.render_maps(depth, alpha, mode="z")
        maps.append((img, depth, alpha))
    cfg = (0.16, 10.0, 0.5)
    r.tsdf_integrate(volume, cams, [m[1] for m in maps], [m[2] for m in maps], [m[0] for m in maps], trunc=cfg[0], depth_max=cfg[1],
                     alpha_min=cfg[2])
    r.ctx.synchronize()
    views = [{"cam": c, "W": W, "H": H, "depth": m[1].cpu().numpy(), "alpha": m[2].cpu().numpy(), "image": m[0].cpu().numpy()}
             for c, m in zip(cams, maps)]
    ref = R.integrate(lcgs, origin, voxel, dims, views, cfg)
    decided = ~ref["undecided"].any(axis=1)
    assert decided.mean() > 0.98 and (ref["weight"] > 0).sum() > 1000 and (ref["weight"] >= 3).any()
    for got, want in zip(state_bits(volume), (ref["tsdf"], ref["weight"], ref["rgb"])):
        same = (got.reshape(decided.size, -1) == u32(want).reshape(decided.size, -1)).all(axis=1)
        assert same[decided].all(), int((~same[decided]).sum())
    vertices, colours, triangles = r.tsdf_mesh(volume, weight_min=1.0)
    assert vertices.shape[0] > 100 and triangles.shape[0] > 100 and colours.shape == vertices.shape  # not empty
    assert int(triangles.max()) == vertices.shape[0] - 1 and int(triangles.min()) == 0
    path = str(tmp_path / "shell.ply")
    lcgs.write_mesh_ply(path, vertices, triangles, colours)
    gv, gc, gt = read_mesh_ply(path)
    assert np.array_equal(u32(gv), u32(vertices)) and np.array_equal(gt.astype(np.int64), triangles.cpu().numpy())
    c = colours.cpu().numpy()
    assert np.array_equal(gc, np.floor(np.clip(np.nan_to_num(c), 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8))


def test_extract_mesh_tool(lcgs, golden_dir, tmp_path):
    from tools import extract_mesh

    cams = tmp_path / "cameras.txt"
    cams.write_text("\n".join(f"{x} {y} {z} 0.05 -0.03 0.5 0 0 1 55" for x, y, z in ((3.1, 0.4, 1.2), (-2.9, 0.6, 0.9), (0.3, 3.0, 1.4), (0.5, -3.2, 0.2))) + "\n")
    out = tmp_path / "mesh.ply"
    extract_mesh.main([os.path.join(golden_dir, "tiny_scene.ply"), str(cams), str(out), "--width", "160", "--height", "120",
                       "--resolution", "48", "--alpha-min", "0.2"])
    v, c, t = read_mesh_ply(str(out))  # (an empty mesh is allowed)
    assert c is not None and c.shape == v.shape and (t.size == 0 or (t.min() >= 0 and t.max() < len(v)))
