"""NumPy restatement of TSDF fusion and of the marching-tetrahedra mesh as include/lcgs_hip.h defines them (lcgs_tsdf_integrate,
lcgs_tsdf_mesh_count / _extract), in binary32 with the header's operation order (NumPy rounds every operation once and contracts
nothing) and in binary64.  No GPU: the view constants come from lcgs.world_to_local_matrix (the library's host code) and the
fov -> tangent path of csrc/host/camera.cpp restated with NumPy's tan, which may differ from the host's tanf in the last place --
hence `undecided` below: a (sample, view) pair whose pixel coordinate lies within 16 ulp of an integer, or whose alpha, depth or
signed distance lies within 16 ulp of its threshold.

The mesh half derives every triangle's winding from the GEOMETRY of its tetrahedron (midpoint vertices, integer arithmetic), not
from the parity rules the kernel uses: the two agree or the GPU test fails."""
import itertools

import numpy as np

U = 2.0 ** -24
VIEW_CHUNK = 42  # = kTsdfViewChunk (csrc/kernels/launch.hpp) = LCGS_TSDF_VIEW_CHUNK = api.LCGS_TSDF_VIEW_CHUNK
UNDECIDED = 16 * 2 * U  # 16 ulp, relative (an ulp is at most 2 U of the value)
PERMS = list(itertools.permutations(range(3)))  # lexicographic: the Kuhn split's six tetrahedra
POP7 = np.array([bin(m).count("1") for m in range(128)], np.int64)


# ------------------------------------------------------------------------------------------------------------ integrate
def view_constants(L, cam, dt=np.float32):
    """(rows [3, 3] = right, up, front; t [3]; inv_tanx, inv_tany) of a view: the binary32 values of make_cam_params
    (csrc/host/camera.cpp), widened for dt = float64"""
    m = L.world_to_local_matrix(cam)
    f = np.float32
    fovy = f(cam.fov) / f(180.0) * f(3.1415926536)
    tany = f(np.tan(fovy * f(0.5)))
    tanx = f(tany * f(cam.aspect_ratio))
    return m[:3, :3].astype(dt), m[:3, 3].astype(dt), dt(f(1.0) / tanx), dt(f(1.0) / tany)


def lattice(origin, voxel, dims, dt=np.float32):
    """X [n, 3] at dtype dt, sample-major (s = (k ny + j) nx + i): fl(origin + fl(voxel * i))"""
    nx, ny, nz = dims
    ax = [dt(np.float32(origin[c])) + dt(np.float32(voxel)) * np.arange(n).astype(dt) for c, n in enumerate((nx, ny, nz))]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([ax[0][i.ravel()], ax[1][j.ravel()], ax[2][k.ravel()]], axis=1)


def _near(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (np.abs(x - ref) <= UNDECIDED * np.maximum(np.abs(ref), np.abs(x)))


def _lookup(view, z, px, py, cfg, dt):
    """the depth lookup of pixels (px, py) for samples at view depth z -> (ok, t, rgb [n, 3] or None, undecided)"""
    W, H, depth, alpha, image = view["W"], view["H"], view["depth"], view["alpha"], view["image"]
    trunc, depth_max, alpha_min = (dt(np.float32(x)) for x in cfg)
    pix = py.astype(np.int64) * W + px
    with np.errstate(all="ignore"):
        d = depth.ravel()[pix].astype(dt)
        ok = np.ones(z.shape, bool)
        und = np.zeros(z.shape, bool)
        if alpha is not None:
            a = alpha.ravel()[pix].astype(dt)
            ok &= a >= alpha_min
            und |= _near(a, alpha_min)
            d = d / a
        ok &= np.isfinite(d) & (d > 0) & (d <= depth_max)
        und |= _near(d, depth_max)  # (d > 0: an ulp at 0 is 1.4e-45 -- no draw comes near it but exact zeros, which nothing moves)
        sdf = d - z
        ok &= ~(sdf < -trunc)
        und |= _near(sdf, -trunc)
        t = np.minimum(dt(1.0), sdf / trunc)
    rgb = None if image is None else image.reshape(3, -1)[:, pix].T.astype(dt)
    return ok, t, rgb, und


def project(L, X, view, dt=np.float32):
    """(z, ux, uy, inside [n], undecided [n]) of samples X in a view"""
    R, tr, itx, ity = view_constants(L, view["cam"], dt)
    W, H = view["W"], view["H"]
    with np.errstate(all="ignore"):
        v = [((R[a, 0] * X[:, 0] + R[a, 1] * X[:, 1]) + R[a, 2] * X[:, 2]) + tr[a] for a in range(3)]
        z = v[2]
        ux = ((v[0] / z) * itx + dt(1.0)) * (dt(0.5) * dt(W))
        uy = ((v[1] / z) * ity + dt(1.0)) * (dt(0.5) * dt(H))
        inside = (z > 0) & (ux >= 0) & (ux < dt(W)) & (uy >= 0) & (uy < dt(H))
        und = (z > 0) & (_near(ux, np.rint(ux.astype(np.float64))) | _near(uy, np.rint(uy.astype(np.float64))))
        # (0 and W are integers: the frustum's edges are covered; near 0 the relative test needs an absolute floor)
        und |= (z > 0) & ((np.abs(ux) <= 1e-5) | (np.abs(uy) <= 1e-5))
    return z, ux, uy, inside, und


def integrate(L, origin, voxel, dims, views, cfg, state=None, with_rgb=True, dt=np.float32):
    """lcgs_tsdf_integrate at dtype dt.  views: dicts cam, W, H, depth [H, W], alpha or None, image [3, H, W] or None; cfg =
    (trunc, depth_max, alpha_min); state = (tsdf, weight, rgb) to continue from.  Returns dict(tsdf [n], weight [n], rgb [n, 3] or
    None, undecided [n, V], applied [n, V])."""
    X = lattice(origin, voxel, dims, dt)
    n = X.shape[0]
    if state is None:
        tsdf, weight, rgb = np.zeros(n, dt), np.zeros(n, dt), (np.zeros((n, 3), dt) if with_rgb else None)
    else:
        tsdf, weight = np.array(state[0], dt).ravel(), np.array(state[1], dt).ravel()
        rgb = None if state[2] is None else np.array(state[2], dt).reshape(n, 3)
    und, applied = np.zeros((n, len(views)), bool), np.zeros((n, len(views)), bool)
    for k, view in enumerate(views):
        z, ux, uy, inside, u0 = project(L, X, view, dt)
        idx = np.nonzero(inside)[0]
        with np.errstate(all="ignore"):
            px, py = np.floor(ux[idx]).astype(np.int64), np.floor(uy[idx]).astype(np.int64)
            ok, t, img, u1 = _lookup(view, z[idx], px, py, cfg, dt)
            und[:, k] = u0
            und[idx, k] |= u1
            hit = idx[ok]
            w = weight[hit]
            w1 = w + dt(1.0)
            tsdf[hit] = (tsdf[hit] * w + t[ok]) / w1
            if rgb is not None and img is not None:
                rgb[hit] = (rgb[hit] * w[:, None] + img[ok]) / w1[:, None]
            weight[hit] = w1
            applied[hit, k] = True
    return {"tsdf": tsdf, "weight": weight, "rgb": rgb, "undecided": und, "applied": applied}


def sample_outcomes(L, origin, voxel, dims, views, cfg, s, und_row, with_rgb=True, start=None):
    """every (tsdf, weight, rgb bits) the header allows for sample s when its undecided views may each be skipped or read any
    pixel of the 3 x 3 neighbourhood of the computed one: a set of byte strings (binary32)"""
    dt = np.float32
    X = lattice(origin, voxel, dims, dt)[s:s + 1]
    options = []
    for k, view in enumerate(views):
        z, ux, uy, inside, _ = project(L, X, view, dt)
        opts = []
        if und_row[k]:
            opts.append(None)
            with np.errstate(all="ignore"):
                cx, cy = np.floor(ux.astype(np.float64)), np.floor(uy.astype(np.float64))
            if z[0] > 0 and np.isfinite(cx[0]) and np.isfinite(cy[0]):
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        px, py = int(cx[0]) + dx, int(cy[0]) + dy
                        if 0 <= px < view["W"] and 0 <= py < view["H"]:
                            ok, t, img, _ = _lookup(view, z, np.array([px]), np.array([py]), cfg, dt)
                            if ok[0]:
                                opts.append((t[0], None if img is None else img[0]))
        elif inside[0]:
            with np.errstate(all="ignore"):
                ok, t, img, _ = _lookup(view, z, np.floor(ux).astype(np.int64), np.floor(uy).astype(np.int64), cfg, dt)
            opts.append((t[0], None if img is None else img[0]) if ok[0] else None)
        else:
            opts.append(None)
        options.append(opts)
    out = set()
    for choice in itertools.product(*options):
        t, w, c = (dt(0), dt(0), np.zeros(3, dt)) if start is None else (dt(start[0]), dt(start[1]), np.array(start[2], dt))
        for o in choice:
            if o is None:
                continue
            w1 = w + dt(1)
            t = (t * w + o[0]) / w1
            if with_rgb and o[1] is not None:
                c = (c * w + o[1]) / w1
            w = w1
        out.add(np.array([t, w, *c], dt).tobytes())
    return out


# ----------------------------------------------------------------------------------------------------------------- mesh
def _corner_slices(dims, code):
    nx, ny, nz = dims
    dx, dy, dz = code & 1, (code >> 1) & 1, (code >> 2) & 1
    return (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))


def _tet_codes(q):
    a, b, _ = PERMS[q]
    return [0, 1 << a, (1 << a) | (1 << b), 7]


def _xyz(code):
    return np.array([code & 1, (code >> 1) & 1, (code >> 2) & 1], np.int64)


def _recipe(q, case):
    """the oriented cycle of tetrahedron q's sign case (bit i: corner i inside) as pairs of tetrahedron corners, from the
    geometry: vertices at the edges' midpoints, normal against (mean outside corner - mean inside corner), in integers"""
    codes = _tet_codes(q)
    ins = [i for i in range(4) if (case >> i) & 1]
    outs = [i for i in range(4) if not (case >> i) & 1]
    if len(ins) in (0, 4):
        return None
    if len(ins) == 2:
        cyc = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
    else:
        p, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
        cyc = [(p, r) for r in rest]
    mid = [_xyz(codes[i]) + _xyz(codes[j]) for i, j in cyc]  # x 2
    nrm = np.cross(mid[1] - mid[0], mid[2] - mid[0])
    direction = len(ins) * sum(_xyz(codes[i]) for i in outs) - len(outs) * sum(_xyz(codes[i]) for i in ins)
    dot = int(nrm @ direction)
    assert dot != 0
    return cyc if dot > 0 else [cyc[0]] + cyc[:0:-1]


def mesh(tsdf, weight, origin, voxel, dims, weight_min=1.0, rgb=None, dt=np.float32):
    """lcgs_tsdf_mesh_extract at dtype dt -> dict(vertices [V, 3], rgb [V, 3] or None, triangles [T, 3] int64, keys [V, 2] =
    (s_lo, dir), tri_dir [T, 3]: mean outside corner - mean inside corner of each triangle's tetrahedron, lattice units; tri_cell [T]:
    the linear index s of each triangle's cell's lowest corner)"""
    nx, ny, nz = dims
    n = nx * ny * nz
    t = np.asarray(tsdf, np.float32).reshape(nz, ny, nx)
    w = np.asarray(weight, np.float32).reshape(nz, ny, nx)
    empty = {"vertices": np.zeros((0, 3), dt), "rgb": None if rgb is None else np.zeros((0, 3), dt),
             "triangles": np.zeros((0, 3), np.int64), "keys": np.zeros((0, 2), np.int64), "tri_dir": np.zeros((0, 3)),
             "tri_cell": np.zeros(0, np.int64)}
    if min(dims) < 2:
        return empty
    with np.errstate(invalid="ignore"):
        good, inside = w >= np.float32(weight_min), t < 0
    valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        valid &= good[_corner_slices(dims, c)]
    mask = np.zeros((nz, ny, nx), np.int64)
    for c in range(7):
        for d in range(1, 8):
            if c & d == 0:
                cross = valid & (inside[_corner_slices(dims, c)] != inside[_corner_slices(dims, c | d)])
                mask[_corner_slices(dims, c)] |= cross.astype(np.int64) << (d - 1)
    mask = mask.ravel()
    base = np.cumsum(POP7[mask]) - POP7[mask]
    bits = (mask[:, None] >> np.arange(7)[None, :]) & 1
    s_lo, dbit = np.nonzero(bits)  # row-major: ascending (s_lo, dir)
    dirs = dbit + 1
    if s_lo.size == 0:
        return empty
    X = lattice(origin, voxel, dims, dt)
    off = lambda code: (code & 1) + ((code >> 1) & 1) * nx + ((code >> 2) & 1) * nx * ny
    s_hi = s_lo + off(dirs)
    tf = t.ravel().astype(dt)
    with np.errstate(all="ignore"):
        lam = tf[s_lo] / (tf[s_lo] - tf[s_hi])
        vertices = X[s_lo] + lam[:, None] * (X[s_hi] - X[s_lo])
        colours = None
        if rgb is not None:
            c = np.asarray(rgb, np.float32).reshape(n, 3).astype(dt)
            colours = c[s_lo] + lam[:, None] * (c[s_hi] - c[s_lo])
    # triangles
    kk, jj, ii = np.nonzero(valid)
    cell_s = (kk * ny + jj) * nx + ii
    cell_lin = (kk * (ny - 1) + jj) * (nx - 1) + ii
    ins_flat = inside.ravel()
    rows = []  # (cell_lin, q, sub, v0, v1, v2, dir3)
    vid = lambda s, lo, hi: base[s + off(lo)] + POP7[mask[s + off(lo)] & ((1 << ((hi ^ lo) - 1)) - 1)]
    for q in range(6):
        codes = _tet_codes(q)
        case = sum(ins_flat[cell_s + off(codes[i])].astype(np.int64) << i for i in range(4))
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)[0]
            if sel.size == 0:
                continue
            cyc = _recipe(q, cs)
            s = cell_s[sel]
            ids = np.stack([vid(s, codes[min(i, j)], codes[max(i, j)]) for i, j in cyc], axis=1)
            ins = [i for i in range(4) if (cs >> i) & 1]
            outs = [i for i in range(4) if not (cs >> i) & 1]
            direction = np.mean([_xyz(codes[i]) for i in outs], axis=0) - np.mean([_xyz(codes[i]) for i in ins], axis=0)
            r = np.arange(sel.size)
            first = np.argmin(ids, axis=1)
            ids = np.stack([ids[r, (first + m) % ids.shape[1]] for m in range(ids.shape[1])], axis=1)  # lowest id first, cycle kept
            if ids.shape[1] == 3:
                tris, subs = [ids], [np.zeros(sel.size, np.int64)]
            else:
                A, B = ids[:, [0, 1, 2]], ids[:, [0, 2, 3]]
                ka = np.sort(A[:, 1:], axis=1)
                kb = np.sort(B[:, 1:], axis=1)
                a_first = (ka[:, 0] < kb[:, 0]) | ((ka[:, 0] == kb[:, 0]) & (ka[:, 1] < kb[:, 1]))
                tris, subs = [A, B], [np.where(a_first, 0, 1), np.where(a_first, 1, 0)]
            for tri, sub in zip(tris, subs):
                rows.append((cell_lin[sel], np.full(sel.size, q), sub, tri, np.broadcast_to(direction, (sel.size, 3)), s))
    if not rows:
        tri_all, dir_all, cell_all = np.zeros((0, 3), np.int64), np.zeros((0, 3)), np.zeros(0, np.int64)
    else:
        cl, qq, sb = (np.concatenate([r[k] for r in rows]) for k in range(3))
        tri_all, dir_all = np.concatenate([r[3] for r in rows]), np.concatenate([r[4] for r in rows])
        order = np.lexsort((sb, qq, cl))
        tri_all, dir_all, cell_all = tri_all[order], dir_all[order], np.concatenate([r[5] for r in rows])[order]
    return {"vertices": vertices, "rgb": colours, "triangles": tri_all.astype(np.int64), "keys": np.stack([s_lo, dirs], axis=1),
            "tri_dir": dir_all, "tri_cell": cell_all}


def edges_of(triangles):
    """(unique undirected edges [E, 2], how many triangles share each)"""
    t = np.asarray(triangles, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0, return_counts=True)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)[np.asarray(triangles, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- cases
def sphere_volume(dims, center, radius, origin=(0.0, 0.0, 0.0), voxel=1.0, trunc=None):
    """analytic sphere TSDF (negative inside), weight 1 everywhere"""
    X = lattice(origin, voxel, dims, np.float64)
    d = np.linalg.norm(X - np.asarray(center, np.float64), axis=1) - radius
    if trunc:
        d = np.clip(d / trunc, -1, 1)
    return d.astype(np.float32), np.ones(d.shape, np.float32)


def torus_volume(dims, center, R, r, origin=(0.0, 0.0, 0.0), voxel=1.0):
    X = lattice(origin, voxel, dims, np.float64) - np.asarray(center, np.float64)
    d = np.sqrt((np.sqrt(X[:, 0] ** 2 + X[:, 1] ** 2) - R) ** 2 + X[:, 2] ** 2) - r
    return d.astype(np.float32), np.ones(d.shape, np.float32)


def exact_zero_sphere(dims=(20, 20, 20)):
    """x^2 + y^2 + z^2 - 25 about the lattice point (9, 9, 9): integers, exactly 0 on the 30 samples at distance 5"""
    X = lattice((0, 0, 0), 1.0, dims, np.float64) - 9.0
    d = (X ** 2).sum(axis=1) - 25.0
    assert (d == 0).sum() == 30
    return d.astype(np.float32), np.ones(d.shape, np.float32)


MESH_CASES = ("sphere", "torus", "zeros", "clipped", "hole", "cell_one", "cell_two", "cell_three", "cell_mixed", "cell_inside",
              "flat")


def mesh_case(name):
    """(tsdf, weight, rgb or None, origin, voxel, dims) of the mesh cases the CPU and GPU tests share"""
    rng = np.random.default_rng(sum(map(ord, name)))
    origin, voxel = (-0.31, 0.17, 0.05), 0.043
    if name == "sphere":
        dims = (20, 20, 20)
        t, w = sphere_volume(dims, (9.3, 9.6, 9.1), 6.37)
    elif name == "torus":
        dims = (20, 20, 20)
        t, w = torus_volume(dims, (9.4, 9.7, 9.2), 5.6, 2.3)
    elif name == "zeros":
        dims = (20, 20, 20)
        t, w = exact_zero_sphere(dims)
    elif name == "clipped":
        dims = (33, 18, 7)
        t, w = sphere_volume(dims, (15.2, 8.4, 3.3), 7.7)
    elif name == "hole":
        dims = (20, 20, 20)
        t, w = sphere_volume(dims, (9.3, 9.6, 9.1), 6.37)
        w = w.reshape(20, 20, 20).copy()
        w[8:12, 3:9, 12:17] = 0.0  # [k, j, i]: a block the surface passes through
        w = w.ravel()
    elif name.startswith("cell_"):
        dims = (2, 2, 2)
        t = {"cell_one": [-1, 2, 3, 1, 2, 5, 1, 1], "cell_two": [-1, -2, 3, 1, 2, 5, 1, 1], "cell_three": [1, 2, 3, 1, -2, 5, -1, -1],
             "cell_mixed": [-1, 2, -3, 1, 2, -5, 1, -0.0], "cell_inside": [-1, -2, -3, -1, -2, -5, -1, -1]}[name]
        t, w = np.array(t, np.float32), np.full(8, 2.0, np.float32)
    elif name == "flat":
        dims = (1, 5, 5)
        t, w = rng.normal(size=25).astype(np.float32), np.ones(25, np.float32)
    n = dims[0] * dims[1] * dims[2]
    rgb = rng.random((n, 3)).astype(np.float32) if name in ("sphere", "clipped", "hole", "cell_two") else None
    return t, w, rgb, origin, voxel, dims


LATTICES = {  # name -> (origin, voxel, dims)
    "odd": ((-0.9, -0.7, -0.55), 0.05, (37, 29, 23)),   # no dimension a multiple of 64: partial waves
    "one": ((0.28, 0.29, 0.31), 0.05, (1, 1, 1)),  # one sample just outside the sphere
    "long": ((-0.81, -0.023, -0.011), 0.0125, (130, 3, 2)),  # rows longer than two waves
}
CFG = (0.2, 10.0, 0.5)  # trunc, depth_max, alpha_min
_POSES = [  # eye, target, (W, H), fov
    ((1.7, 1.3, 0.9), (0.03, -0.02, 0.01), (64, 48), 50.0),
    ((-1.5, 0.8, -1.1), (0.1, 0.05, -0.03), (33, 17), 62.0),
    ((0.11, -0.07, 0.05), (0.9, 0.5, 0.31), (64, 48), 75.0),   # inside the volume: samples behind it
    ((2.0, -1.6, 1.2), (0.7, 1.3, 0.45), (33, 17), 35.0),     # looking past the volume: most rays leave the image
    ((1.2, -1.9, 1.4), (0.02, 0.01, -0.03), (1, 1), 40.0),    # a 1 x 1 map
]
_VIEWS = {}


def _maps(L, cam, rng):
    """depth (accumulated z = z alpha), alpha and image of a view of the sphere |X| = 0.5 over the plane z = -0.35, salted"""
    W, H = cam.width, cam.height
    R, t, itx, ity = view_constants(L, cam, np.float64)
    rx = ((np.arange(W) + 0.5) / W * 2 - 1) / itx
    ry = ((np.arange(H) + 0.5) / H * 2 - 1) / ity
    d = np.stack([np.broadcast_to(rx[None, :], (H, W)), np.broadcast_to(ry[:, None], (H, W)), np.ones((H, W))], axis=-1) @ R  # world
    C = np.array(list(cam.position), np.float64)
    b, c = d @ C, C @ C - 0.25
    a = (d * d).sum(-1)
    with np.errstate(all="ignore"):
        disc = b * b - a * c
        s1 = np.where(disc > 0, (-b - np.sqrt(disc)) / a, np.inf)
        s1 = np.where(s1 > 0, s1, np.inf)
        s2 = (-0.35 - C[2]) / d[..., 2]
        s2 = np.where(s2 > 0, s2, np.inf)
    z = np.minimum(s1, s2)
    z = np.where(np.isfinite(z), z, 0.0)
    alpha = rng.choice(np.array([0.3, 0.75, 0.97, 1.0], np.float32), size=(H, W), p=[0.15, 0.25, 0.3, 0.3]).astype(np.float32)
    alpha[rng.random((H, W)) < 0.001] = CFG[2]  # exact equality passes (and is undecided by the 16-ulp rule: kept rare)
    if W * H > 1:
        alpha[H - 1, 1] = CFG[2]
    depth = (z.astype(np.float32) * alpha).astype(np.float32)
    salt = rng.random((H, W))
    for lo, val in ((0.00, np.nan), (0.02, np.inf), (0.04, 0.0), (0.06, -0.7), (0.08, 37.0)):
        depth[(salt >= lo) & (salt < lo + 0.02)] = val
    return depth, alpha, rng.random((3, H, W)).astype(np.float32)


def views(L, count=5):
    """the first `count` views of the integrate cases: the five poses above, then repeats of them with perturbed poses that
    share the five's maps"""
    out = []
    for k in range(count):
        if k not in _VIEWS:
            rng = np.random.default_rng(9100 + k)
            eye, target, (W, H), fov = _POSES[k % 5]
            if k >= 5:
                eye = tuple(np.asarray(eye) + rng.normal(0, 0.03, 3))
                target = tuple(np.asarray(target) + rng.normal(0, 0.03, 3))
            cam = L.get_lookat_cam(list(map(float, eye)), list(map(float, target)), [0.0, 0.0, 1.0], width=W, height=H, fov=fov)
            depth, alpha, image = _maps(L, cam, rng) if k < 5 else (_VIEWS[k % 5][key] for key in ("depth", "alpha", "image"))
            _VIEWS[k] = {"cam": cam, "W": W, "H": H, "depth": depth, "alpha": alpha, "image": image}
        out.append(_VIEWS[k])
    return out


def variant(vs, alpha=True, image=True):
    return [dict(v, alpha=v["alpha"] if alpha else None, image=v["image"] if image else None) for v in vs]
