"""NumPy restatement of Mip-Splatting's 3-D smoothing filter as include/lcgs_hip.h defines it (lcgs_filter3d_accumulate /
_finalize / _apply / _backward), in binary32 with the header's operation order (NumPy rounds every operation once and contracts
nothing) and in binary64.  No GPU: the view constants come from lcgs.world_to_local_matrix (the library's host code, the very
rows and translation the kernels read) and the fov -> tangent path of csrc/host/camera.cpp restated with NumPy's tan, which may
differ from the host's tanf in the last place -- hence `undecided` below.

Error bounds of the binary32 forms against exact arithmetic, from counting roundings (u = 2^-24; b_k = s_k^2 + f^2 carries 1.5 u,
coef 4.75 u, the second gradient term about 9.5 u), rounded up to the next power of two so that they hold for any association:
scale_out 3 u, opacity_out 8 u, g_op' 8 u relative; g_s_k' 16 u (|first term| + |second term|)."""
import numpy as np

U = 2.0 ** -24
VIEW_CHUNK = 64  # = kFilter3dViewChunk (csrc/kernels/launch.hpp) = api.LCGS_FILTER3D_VIEW_CHUNK
BOUND_SCALE, BOUND_OPACITY, BOUND_G_OPACITY, BOUND_G_SCALE = 3 * U, 8 * U, 8 * U, 16 * U
UNDECIDED = 8 * U  # a comparison within this, relative, of equality may fall either way on the device


def view_constants(L, cam, dt=np.float32):
    """(rows [3, 3] = right, up, front; t [3]; limx, limy; focalx; tanfovx, tanfovy) of a view at dtype dt: the binary32 values of
    make_cam_params (csrc/host/camera.cpp), widened for dt = float64"""
    m = L.world_to_local_matrix(cam)  # (row, col): rows right | tx, up | ty, front | tz
    f = np.float32
    fovy = f(cam.fov) / f(180.0) * f(3.1415926536)
    tany = f(np.tan(fovy * f(0.5)))
    tanx = f(tany * f(cam.aspect_ratio))
    limx, limy = f(1.3) * tanx, f(1.3) * tany
    focalx = f(f(cam.width) / (f(2.0) * tanx))
    return m[:3, :3].astype(dt), m[:3, 3].astype(dt), dt(limx), dt(limy), dt(focalx), dt(tanx), dt(tany)


def accumulate(L, pos, cams, min_z=None, max_focal=0.0, dt=np.float32):
    """lcgs_filter3d_accumulate at dtype dt.  Returns dict(min_z [P], max_focal, z [P, V] (the view depths), seen [P, V],
    undecided [P, V]: any of the row's three comparisons with that view within UNDECIDED relative of equality)."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3).astype(dt)
    P, V = pos.shape[0], len(cams)
    mz = np.full(P, np.inf, dt) if min_z is None else np.asarray(min_z, dt).copy()
    z, seen, und = np.zeros((P, V), dt), np.zeros((P, V), bool), np.zeros((P, V), bool)
    focal = np.float32(max_focal)
    px, py, pz = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        for k, cam in enumerate(cams):
            R, t, limx, limy, fx, _, _ = view_constants(L, cam, dt)
            v = [((R[a, 0] * px + R[a, 1] * py) + R[a, 2] * pz) + t[a] for a in range(3)]  # gs_math.hpp view_transform
            lx, ly, near = limx * v[2], limy * v[2], dt(np.float32(0.2))
            s = (v[2] > near) & (np.abs(v[0]) <= lx) & (np.abs(v[1]) <= ly)  # a NaN fails every comparison
            w = [x.astype(np.float64) for x in (v[2], np.abs(v[0]), lx, np.abs(v[1]), ly)]
            und[:, k] = (np.abs(w[0] - float(near)) <= UNDECIDED * float(near)) | (np.abs(w[1] - w[2]) <= UNDECIDED * np.abs(w[2])) | \
                (np.abs(w[3] - w[4]) <= UNDECIDED * np.abs(w[4]))
            und[:, k] &= np.isfinite(w[1]) & np.isfinite(w[2]) & np.isfinite(w[3]) & np.isfinite(w[4])  # (infinities compare as they are)
            z[:, k], seen[:, k] = v[2], s
            mz = np.where(s & (v[2] < mz), v[2], mz)
            focal = max(focal, np.float32(fx))
    return {"min_z": mz, "max_focal": float(focal), "z": z, "seen": seen, "undecided": und}


def seen_in_pixels(L, pos, cams):
    """Mip-Splatting's compute_3D_filter statement of the rule, binary64: depth > 0.2 and the projected point inside the screen
    with a 15 % margin, -0.15 W <= x_pix <= 1.15 W (same for y), x_pix = x / z focal_x + W / 2.  [P, V] bool."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.zeros((pos.shape[0], len(cams)), bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k, cam in enumerate(cams):
            R, t, _, _, _, tanx, tany = view_constants(L, cam, np.float64)
            x, y, z = (pos @ R.T + t).T
            W, H = float(cam.width), float(cam.height)
            fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
            xp, yp = x / z * fx + W / 2.0, y / z * fy + H / 2.0
            out[:, k] = (z > float(np.float32(0.2))) & (xp >= -0.15 * W) & (xp <= 1.15 * W) & (yp >= -0.15 * H) & (yp <= 1.15 * H)
    return out


def finalize(min_z, max_focal, dt=np.float32):
    """lcgs_filter3d_finalize: ((finite min_z ? min_z : zmax) / max_focal) * c, c the binary32 nearest to sqrt(0.2) (dt = float64:
    sqrt(0.2) itself); zeros when no entry is finite"""
    mz = np.asarray(min_z, np.float32).astype(dt)
    finite = np.isfinite(mz)
    if not finite.any():
        return np.zeros(mz.shape, dt)
    c = np.float32(np.sqrt(0.2)) if dt is np.float32 else np.sqrt(0.2)
    return (np.where(finite, mz, mz[finite].max()) / dt(np.float32(max_focal))) * dt(c)


def _filtered(scale, filt, dt):
    s = np.asarray(scale, np.float32).reshape(-1, 3).astype(dt)
    f = np.asarray(filt, np.float32).reshape(-1).astype(dt)
    with np.errstate(all="ignore"):
        f2 = f * f
        a = s * s
        b = a + f2[:, None]
        sf = np.sqrt(b)
        r = a / b
        coef = np.sqrt((r[:, 0] * r[:, 1]) * r[:, 2])
    return s, f, f2, b, sf, coef


def apply(scale, opacity, filt, dt=np.float32):
    """lcgs_filter3d_apply -> (scale_out [P, 3], opacity_out [P]); rows with filt == 0 are the inputs' bits"""
    s, f, f2, b, sf, coef = _filtered(scale, filt, dt)
    o = np.asarray(opacity, np.float32).reshape(-1).astype(dt)
    ident = f == 0
    with np.errstate(all="ignore"):
        return np.where(ident[:, None], s, sf), np.where(ident, o, o * coef)


def backward(scale, opacity, filt, g_scale, g_opacity, dt=np.float32, terms=False):
    """lcgs_filter3d_backward on dense rows -> (g_scale' [P, 3], g_opacity' [P]) (terms: also |first term| + |second term| of
    g_scale', [P, 3]); rows with filt == 0 are the incoming gradients' bits"""
    s, f, f2, b, sf, coef = _filtered(scale, filt, dt)
    o = np.asarray(opacity, np.float32).reshape(-1).astype(dt)
    gs = np.asarray(g_scale, np.float32).reshape(-1, 3).astype(dt)
    go = np.asarray(g_opacity, np.float32).reshape(-1).astype(dt)
    ident = f == 0
    with np.errstate(all="ignore"):
        w = ((go * o) * coef) * f2
        t1, t2 = gs * (s / sf), w[:, None] / (s * b)
        out = np.where(ident[:, None], gs, t1 + t2), np.where(ident, go, go * coef)
    return (*out, np.where(ident[:, None], 0.0, np.abs(t1) + np.abs(t2))) if terms else out


def coef_by_determinants(scale, filt, dt=np.float32):
    """the opacity factor as Mip-Splatting writes it, sqrt(prod(s^2) / prod(s^2 + f^2)): what underflows for tiny scales"""
    s, f, f2, b, sf, coef = _filtered(scale, filt, dt)
    a = s * s
    with np.errstate(all="ignore"):
        return np.sqrt(((a[:, 0] * a[:, 1]) * a[:, 2]) / ((b[:, 0] * b[:, 1]) * b[:, 2]))


# ---------------------------------------------------------------------------------------------------------------- draws
def draw_rows(rng, P):
    """the log-normal draw the bounds were counted for: scales exp(N(-4, 2.5)), filters exp(N(-5, 2.5)), every tenth filter 0"""
    scale = np.exp(rng.normal(-4.0, 2.5, (P, 3))).astype(np.float32)
    filt = np.exp(rng.normal(-5.0, 2.5, P)).astype(np.float32)
    filt[::10] = 0.0
    opacity = (1 / (1 + np.exp(-rng.normal(0, 2, P)))).astype(np.float32)
    g_scale = rng.normal(0, 1, (P, 3)).astype(np.float32) * np.exp(rng.normal(0, 3, (P, 1))).astype(np.float32)
    g_opacity = rng.normal(0, 1, P).astype(np.float32) * np.exp(rng.normal(0, 3, P)).astype(np.float32)
    return scale, opacity, filt, g_scale, g_opacity


def draw_cameras(L, rng, n, center=(0.0, 0.0, 0.5)):
    """n random look-at cameras of mixed sizes and fovs around conftest.make_scene's cloud: some inside it, some looking past it,
    so that rows fall behind cameras, inside the 0.2 near limit and outside the margin"""
    cams = []
    for k in range(n):
        ang, elev, dist = rng.uniform(0, 2 * np.pi), rng.uniform(-0.7, 0.9), rng.uniform(0.05, 3.0)
        eye = np.asarray(center) + dist * np.array([np.cos(ang) * np.cos(elev), np.sin(ang) * np.cos(elev), np.sin(elev)])
        target = np.asarray(center) + rng.normal(0, 0.5, 3)
        W, H = int(rng.integers(17, 1300)), int(rng.integers(17, 900))
        cams.append(L.get_lookat_cam(eye.tolist(), target.tolist(), [0.0, 0.0, 1.0], width=W, height=H, fov=float(rng.uniform(20.0, 100.0))))
    return cams


ACC_SIZES = (1, 63, 64, 65, 255, 257, 70_001)
ACC_VIEWS = (0, 1, VIEW_CHUNK - 1, VIEW_CHUNK, VIEW_CHUNK + 1, 2 * VIEW_CHUNK + 1)
_CASES = {}


def accumulate_case(L, P):
    """the accumulate draw of size P that tests/test_filter3d_ref.py caps and tests/test_gpu_filter3d.py runs: (pos [P, 3], the
    2 VIEW_CHUNK + 1 cameras, accumulate()'s dict over all of them), computed once.  From 63 rows on, rows 5, 17 and 40 hold a
    NaN, a +inf and a -inf coordinate.  A prefix of the views is a prefix of the columns (min_z_of)."""
    if P not in _CASES:
        from conftest import make_scene

        rng = np.random.default_rng(7000 + P)
        pos = make_scene(rng, P)["pos"]
        if P >= 63:
            pos[5, 0], pos[17, 1], pos[40, 2] = np.nan, np.inf, -np.inf
        cams = draw_cameras(L, rng, ACC_VIEWS[-1])
        _CASES[P] = (pos, cams, accumulate(L, pos, cams))
    return _CASES[P]


def min_z_of(ref, first, last):
    """min_z (from +inf) over the views [first, last) of an accumulate() result"""
    z = np.where(ref["seen"][:, first:last], ref["z"][:, first:last], np.float32(np.inf))
    with np.errstate(invalid="ignore"):
        return np.minimum.reduce(z, axis=1, initial=np.float32(np.inf)).astype(np.float32)
