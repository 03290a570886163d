"""The reference of the normal map (include/lcgs_hip.h, kernels/maps.hip: lcgs_render_normals) and of its backward, composed
from the UNCHANGED CPU oracle the way distortion_ref.py composes the distortion map, and the per-row bound the kernels' gradients
are held to.  No GPU needed.

The per-splat normal (splat_normals) is the header's definition restated in numpy with the kernel's operation order: the axis k
of the smallest activated scale (ties to the lower index), column k of rot_from_quat's matrix from rotq as stored (w, x, y, z),
turned to face the camera (flipped iff (c0 d0 + c1 d1) + c2 d2 > 0, d = pos - camera position), taken to view space by the rows
right / up / front.  In binary32 it gives the kernel's bits (the build does not contract).  k and the flip are constants of the
frame: the f64 and the contracted builds take them from the binary32 evaluation instead of deciding again.
Forward: the oracle's forward state composited once more with the colour n over a zero background, every operation in o.dtype.
Backward, per oracle build: render_backward with that colour and the incoming dL_dnormal, the preprocess-backward with a zero
colour gradient, and the walk's colour-gradient columns (dL/dn) taken to rotq through dn/dq = Rview (+-) dc/dq, dc/dq the closed
form of column k.  The other channels of the same call are distortion_ref.backward's (or maps_ref.backward's), added.
Bound: maps_ref.row_bound's formula and constants.  A and F from the f64 walk over the f32 state with the colour n and the
incoming gradient; columns 6-8 are kept out of abs_jacobian_apply and sent to rotq through |Rview| |dc/dq|.  The other channels'
bounds are added with sum_row_bounds."""
import numpy as np

import distortion_ref
import maps_ref
from gpu_util import GRAD_ROW_CU, GRAD_ROW_FLOOR, GRAD_ROW_K, KEYS, U32, _oracles

MODES = maps_ref.MODES
sum_row_bounds = maps_ref.sum_row_bounds


def _dot3(a, b):
    """(a0 b0 + a1 b1) + a2 b2 over the last axis, in the operands' dtype"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _columns(q, dt):
    """rot_from_quat's three columns [P, 3 (column), 3 (component)] from rotq as stored (w, x, y, z), its expressions as they
    stand: 1 - 2 y y - 2 z z is ((1 - (2 y) y) - (2 z) z), 2 x y + 2 z w is ((2 x) y) + ((2 z) w)"""
    w, x, y, z = (q[:, j] for j in range(4))
    one, two = dt(1.0), dt(2.0)
    c0 = [one - two * y * y - two * z * z, two * x * y + two * z * w, two * x * z - two * y * w]
    c1 = [two * x * y - two * z * w, one - two * x * x - two * z * z, two * y * z + two * x * w]
    c2 = [two * x * z + two * y * w, two * y * z - two * x * w, one - two * x * x - two * y * y]
    out = np.stack([np.stack(c, axis=1) for c in (c0, c1, c2)], axis=1)
    assert out.dtype == dt
    return out


def _view_rows(o, cam):
    return np.stack([np.asarray(cam.right[:], o.dtype), np.asarray(cam.up[:], o.dtype), np.asarray(cam.front[:], o.dtype)])


def splat_normals(o, scene, cam, decide=None):
    """(n [P, 3] view space, k [P], flip [P] bool) in o.dtype; decide = (k, flip): taken as given instead of decided here"""
    dt = o.dtype
    pos = np.asarray(scene["pos"], dt).reshape(-1, 3)
    P = pos.shape[0]
    s = np.asarray(scene["scale"], dt).reshape(P, 3)
    q = np.asarray(scene["rotq"], dt).reshape(P, 4)
    cols = _columns(q, dt)
    if decide is None:
        k = np.zeros(P, np.int64)
        k = np.where(s[:, 1] < s[np.arange(P), k], 1, k)
        k = np.where(s[:, 2] < s[np.arange(P), k], 2, k)
    else:
        k = np.asarray(decide[0], np.int64)
    c = cols[np.arange(P), k]
    if decide is None:
        d = pos - np.asarray(cam.position[:], dt)[None, :]
        with np.errstate(invalid="ignore"):
            flip = _dot3(c, d) > 0  # (0 and NaN: unflipped)
    else:
        flip = np.asarray(decide[1], bool)
    c = np.where(flip[:, None], -c, c)
    Rv = _view_rows(o, cam)
    n = np.stack([_dot3(Rv[r][None, :], c) for r in range(3)], axis=1)
    assert n.dtype == dt
    return n, k, flip


def decisions(scene, ocam):
    """(k, flip) of the binary32 evaluation: what every build of the reference uses"""
    o32 = _oracles()[0]
    _, k, flip = splat_normals(o32, scene, o32.convert_camera(ocam))
    return k, flip


def _dcol_dq(q, k, dt):
    """d(column k) / d rotq, [P, 3 (component), 4 (w, x, y, z as stored)]"""
    w, x, y, z = (q[:, j] for j in range(4))
    zero = np.zeros_like(w)
    two, four = dt(2.0), dt(4.0)
    #            d/dw                 d/dx                      d/dy                      d/dz
    D0 = [[zero, zero, -four * y, -four * z], [two * z, two * y, two * x, two * w], [-two * y, two * z, -two * w, two * x]]
    D1 = [[-two * z, two * y, two * x, -two * w], [zero, -four * x, zero, -four * z], [two * x, two * w, two * z, two * y]]
    D2 = [[two * y, two * z, two * w, two * x], [-two * x, -two * w, two * z, two * y], [zero, -four * x, -four * y, zero]]
    D = np.stack([np.stack([np.stack(r, axis=1) for r in Dk], axis=1) for Dk in (D0, D1, D2)], axis=1)  # [P, 3 (k), 3, 4]
    return D[np.arange(q.shape[0]), k]


def normal_to_rotq(o, scene, cam, gn, k, flip):
    """dL/drotq [P, 4] from dL/dn [P, 3]: dL/dc = +-(right gn0 + up gn1 + front gn2), then (dc/dq)^T"""
    dt = o.dtype
    q = np.asarray(scene["rotq"], dt).reshape(-1, 4)
    gc = np.asarray(gn, dt) @ _view_rows(o, cam)
    gc = np.where(np.asarray(flip, bool)[:, None], -gc, gc)
    return np.einsum("pmj,pm->pj", _dcol_dq(q, k, dt), gc).astype(dt)


def compose(o, st, cam, n):
    """the map [3, H, W] in o.dtype of a forward state `st` (Oracle.forward_state's, or antialias_ref's)"""
    img = o.render_forward(cam.width, cam.height, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                           st["opacity"], n)[0]
    assert img.dtype == o.dtype
    return img


def forward(o, scene, cam, scale_modifier=1.0, sh_deg=3, decide=None):
    """(normal [3, H, W], forward state, (n, k, flip)) of oracle build `o`"""
    st = o.forward_state(scene, cam, scale_modifier=scale_modifier, sh_deg=sh_deg)
    sn = splat_normals(o, scene, cam, decide)
    return compose(o, st, cam, sn[0]), st, sn


def blended_rows(o, st, cam):
    """[P] bool: the rows some pixel blends (the sum of their weights over the frame is positive)"""
    W, H = cam.width, cam.height
    ones = np.ones((st["opacity"].shape[0], 3), o.dtype)
    gcol = o.render_backward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"], st["opacity"], ones,
                             st["final_T"], st["n_contrib"], np.ones((3, H, W), o.dtype))[3]
    return gcol[:, 0] > 0


def backward(o, scene, cam, dL_dnormal, dL_ddist=None, dL_ddepth=None, dL_dalpha=None, mode="z", center=0.0, scale_modifier=1.0,
             sh_deg=3, frame=maps_ref.Classic, walk=None, decide=None):
    """attribute -> gradient of <dL_dnormal, normal> + <dL_ddist, dist> + <dL_ddepth, depth> + <dL_dalpha, alpha> in oracle
    build `o` (its own forward); decide: the binary32 (k, flip) (None: the build's own -- the f32 build, or a test of this
    file); walk: a dict that receives the normal walk's own dL/dopacity row ("go")"""
    W, H = cam.width, cam.height
    st = frame.state(o, scene, cam, scale_modifier, sh_deg)
    n, k, flip = splat_normals(o, scene, cam, decide)
    gm, gc, go, gcol = o.render_backward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                                         st["opacity"], n, st["final_T"], st["n_contrib"], np.asarray(dL_dnormal, o.dtype))
    if walk is not None:
        walk["go"] = go
    gc, go = frame.augment(o, st, gc, go)
    g = o.preprocess_backward(scene, cam, st["radii"], gm, gc, np.zeros_like(gcol), scale_modifier=scale_modifier, sh_deg=sh_deg)
    g["rotq"] = g["rotq"] + normal_to_rotq(o, scene, cam, gcol, k, flip)
    g["opacity"] = go
    g["sh"] = np.zeros_like(g["sh"])
    other = None
    kw = dict(mode=mode, scale_modifier=scale_modifier, sh_deg=sh_deg, frame=frame)
    if dL_ddist is not None:
        other = distortion_ref.backward(o, scene, cam, dL_ddist, dL_ddepth, dL_dalpha, center=center, **kw)
    elif dL_ddepth is not None or dL_dalpha is not None:
        other = maps_ref.backward(o, scene, cam, dL_ddepth, dL_dalpha, **kw)
    if other is not None:
        g = {key: g[key] + other[key] for key in g}
    return g


def row_bound(scene, ocam, dL_dnormal, dL_ddist=None, dL_ddepth=None, dL_dalpha=None, mode="z", center=0.0, scale_modifier=1.0,
              sh_deg=3, other_bound=None, frame=maps_ref.Classic):
    """(per attribute [P, n] bound, f64 reference) for a normals backward without an image gradient.  other_bound: the
    (bound, reference) of the same call's other channels (distortion_ref.row_bound / maps_ref.row_bound), where the caller
    has it."""
    from oracle import abs_jacobian_apply

    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    cam64 = o64.convert_camera(ocam)
    dec = decisions(scene, ocam)
    kw = dict(scale_modifier=scale_modifier, sh_deg=sh_deg, frame=frame, decide=dec)
    r32 = backward(o32, scene, ocam, dL_dnormal, **kw)
    walk64 = {}
    r64 = backward(o64, scene, cam64, dL_dnormal, walk=walk64, **kw)
    r32c = backward(o32c, scene, o32c.convert_camera(ocam), dL_dnormal, **kw)
    # the rounding budget of the walk, over the binary32 state and the binary32 normals the kernels produce bit for bit
    W, H = ocam.width, ocam.height
    st = frame.state(o32, scene, ocam, scale_modifier, sh_deg)
    n32, k, _ = splat_normals(o32, scene, ocam, dec)
    A, F = o64.render_backward_bound(W, H, np.zeros(3, np.float32), st["ranges"], st["point_list"], st["means"], st["conic"],
                                     st["opacity"], n32, st["final_T"], st["n_contrib"], np.asarray(dL_dnormal, np.float32))
    A, F = (frame.augment_budget(o64, scene, cam64, st, X, scale_modifier) for X in (A, F))
    Az, Fz = A.copy(), F.copy()
    Az[:, 6:9] = 0.0
    Fz[:, 6:9] = 0.0
    JA, JF = abs_jacobian_apply(o64, scene, cam64, st["radii"], (Az, Fz), scale_modifier, sh_deg)
    # columns 6-8 (dL/dn) reach rotq through |Rview| and |dc/dq|
    q64 = np.asarray(scene["rotq"], np.float64).reshape(-1, 4)
    absD = np.abs(_dcol_dq(q64, k, np.float64))  # [P, 3, 4]
    absR = np.abs(_view_rows(o64, cam64))        # [3 (view component), 3 (world component)]
    JA["rotq"] = JA["rotq"] + np.einsum("pmj,pm->pj", absD, A[:, 6:9] @ absR)
    JF["rotq"] = JF["rotq"] + np.einsum("pmj,pm->pj", absD, F[:, 6:9] @ absR)
    P = q64.shape[0]
    extra = frame.conditioning(o64, scene, cam64, st["radii"], walk64["go"], scale_modifier, sh_deg)
    B, R = {}, {}
    for key in KEYS:
        b64 = r64[key].astype(np.float64).reshape(P, -1)
        noise = np.maximum(np.abs(r32[key].astype(np.float64).reshape(P, -1) - b64),
                           np.abs(r32c[key].astype(np.float64).reshape(P, -1) - b64))
        ja, jf = JA[key].reshape(P, -1), JF[key].reshape(P, -1)
        B[key] = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * ja + jf + GRAD_ROW_FLOOR * ja
        if extra is not None:
            B[key] = B[key] + extra[key].reshape(P, -1)
        R[key] = b64
    if dL_ddist is not None or dL_ddepth is not None or dL_dalpha is not None:
        if other_bound is None:
            kw = dict(mode=mode, scale_modifier=scale_modifier, sh_deg=sh_deg, frame=frame)
            other_bound = (distortion_ref.row_bound(scene, ocam, dL_ddist, dL_ddepth, dL_dalpha, center=center, **kw)
                           if dL_ddist is not None else maps_ref.row_bound(scene, ocam, dL_ddepth, dL_dalpha, **kw))
        return sum_row_bounds([(B, R), other_bound])
    return B, R
