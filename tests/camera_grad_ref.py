"""The reference of the camera gradient (include/lcgs_hip.h "camera gradient", kernels/camera_grad.hip), composed from the
UNCHANGED CPU oracle the way maps_ref.py is, and the bound the kernels' twelve numbers are held to.  No GPU needed.

The twelve numbers are the gradient w.r.t. lcgs_camera's position, front, up, right (that order) as independent reals.  Per
row: `contributions` restates the formulas of the header in numpy at the oracle's precision, linear in the row's ten 2-D
gradients (pixel mean 2, conic 3, opacity, colour 3, value).  `reference` feeds it the oracle's own walks over the oracle's
own forward state; its position columns are NOT the restatement but minus the rows of the oracle's own dL/dpos.
Bound per component k:
    GRAD_ROW_K noise[k] + GRAD_ROW_CU U32 JA[k] + JF[k] + GRAD_ROW_FLOOR JA[k] + U32 |r64[k]|
noise[k] = sum over rows of max(|c32 - c64|, |c32c - c64|): a sum of per-row absolute errors, not the error of the sum (which
can be near zero by cancellation, and the kernel's is another draw); JA / JF = sum over rows of |C64| A / |C64| F, A and F the
walks' rounding budgets over the binary32 state (maps_ref.row_bound's), C64 the per-row Jacobian from unit 2-D rows; the three
position components take the sum over rows of the existing per-row position bound.  Constants: gpu_util's, unchanged."""
import numpy as np

import maps_ref
from gpu_util import GRAD_ROW_CU, GRAD_ROW_FLOOR, GRAD_ROW_K, U32, _oracles, gradient_row_bound

FIELDS = ("position", "front", "up", "right")  # lcgs_camera's order
N2D = 10  # pixel mean 2, conic 3, opacity 1, colour 3, value 1


def cam12(cam):
    """the twelve numbers of a camera (any oracle's or the product's struct), float64"""
    return np.array([[float(x) for x in getattr(cam, f)] for f in FIELDS]).reshape(12)


def with_cam12(o, cam, v12):
    """a copy of `cam` in oracle o's struct whose four vectors are v12"""
    d = o.camera_to_dict(cam)
    v = np.asarray(v12, np.float64).reshape(4, 3)
    for k, f in enumerate(FIELDS):
        d[f] = [float(x) for x in v[k]]
    return o.camera_from_dict(d)


def _consts(o, cam):
    dt = o.dtype
    fovy = dt(cam.fov) / dt(180.0) * dt(np.float32(3.1415926536))  # (the oracle's constants are binary32 literals, widened)
    tany = dt(np.tan(fovy * dt(0.5)))
    tanx = dt(tany * dt(cam.aspect_ratio))
    return tanx, tany, dt(dt(cam.width) / (dt(2.0) * tanx)), dt(dt(cam.height) / (dt(2.0) * tany))


def geometry_terms(o, scene, cam, g2d, scale_modifier=1.0):
    """orc_preprocess_backward's geometry step in numpy at o.dtype, keeping what it drops: dict(dv [P, 3], dT0, dT1 [P, 3],
    j00, j11, j02, j12 [P], z [P], clx, cly [P])"""
    dt = o.dtype
    pos = np.asarray(scene["pos"], dt).reshape(-1, 3)
    P = pos.shape[0]
    scale = np.asarray(scene["scale"], dt).reshape(P, 3)
    rotq = np.asarray(scene["rotq"], dt).reshape(P, 4)
    g = np.asarray(g2d, dt).reshape(P, N2D)
    right, up, front, campos = (np.asarray(getattr(cam, f)[:], dt) for f in ("right", "up", "front", "position"))
    tanx, tany, fx, fy = _consts(o, cam)
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    t = [-dot(campos, right), -dot(campos, up), -dot(campos, front)]
    p = [pos[:, 0], pos[:, 1], pos[:, 2]]
    v = [ax[0] * p[0] + ax[1] * p[1] + ax[2] * p[2] + tt for ax, tt in zip((right, up, front), t)]
    limx, limy = dt(np.float32(1.3)) * tanx, dt(np.float32(1.3)) * tany
    rx, ry = v[0] / v[2], v[1] / v[2]
    clx = np.where(rx < -limx, -1, np.where(rx > limx, 1, 0))
    cly = np.where(ry < -limy, -1, np.where(ry > limy, 1, 0))
    tx = np.where(clx != 0, clx.astype(dt) * limx, rx) * v[2]
    ty = np.where(cly != 0, cly.astype(dt) * limy, ry) * v[2]
    tz = v[2]
    sm = dt(scale_modifier)
    sc = [sm * scale[:, k] for k in range(3)]
    w, x, y, z = rotq[:, 0], rotq[:, 1], rotq[:, 2], rotq[:, 3]
    one, two = dt(1.0), dt(2.0)
    R = [[one - two * y * y - two * z * z, two * x * y - two * z * w, two * x * z + two * y * w],
         [two * x * y + two * z * w, one - two * x * x - two * z * z, two * y * z - two * x * w],
         [two * x * z - two * y * w, two * y * z + two * x * w, one - two * x * x - two * y * y]]
    M = [[R[r][k] * sc[k] for k in range(3)] for r in range(3)]
    Sig = [[M[r][0] * M[k][0] + M[r][1] * M[k][1] + M[r][2] * M[k][2] for k in range(3)] for r in range(3)]
    j00, j11 = fx / tz, fy / tz
    j02, j12 = -fx * tx / (tz * tz), -fy * ty / (tz * tz)
    T0 = [right[r] * j00 + front[r] * j02 for r in range(3)]
    T1 = [up[r] * j11 + front[r] * j12 for r in range(3)]
    ST0 = [Sig[r][0] * T0[0] + Sig[r][1] * T0[1] + Sig[r][2] * T0[2] for r in range(3)]
    ST1 = [Sig[r][0] * T1[0] + Sig[r][1] * T1[1] + Sig[r][2] * T1[2] for r in range(3)]
    a, b, c = dot(T0, ST0) + dt(np.float32(0.3)), dot(T1, ST0), dot(T1, ST1) + dt(np.float32(0.3))
    D = a * c - b * b + dt(np.float32(1e-6))
    gA, gB, gC = g[:, 2], g[:, 3], g[:, 4]
    iD2 = one / (D * D)
    g00 = (-c * c * gA + b * c * gB + (D - a * c) * gC) * iD2
    g11 = ((D - a * c) * gA + a * b * gB - a * a * gC) * iD2
    g01 = (two * b * c * gA - (D + two * b * b) * gB + two * a * b * gC) * iD2
    dT0 = [two * g00 * ST0[r] + g01 * ST1[r] for r in range(3)]
    dT1 = [two * g11 * ST1[r] + g01 * ST0[r] for r in range(3)]
    dj00, dj02, dj11, dj12 = dot(right, dT0), dot(front, dT0), dot(up, dT1), dot(front, dT1)
    itz2 = one / (tz * tz)
    itz3 = itz2 / tz
    dtx, dty = dj02 * (-fx * itz2), dj12 * (-fy * itz2)
    dtz = dj00 * (-fx * itz2) + dj11 * (-fy * itz2) + dj02 * (two * fx * tx * itz3) + dj12 * (two * fy * ty * itz3)
    zero = np.zeros_like(dtx)
    dv = [np.where(clx != 0, zero, dtx), np.where(cly != 0, zero, dty),
          dtz + np.where(clx != 0, dtx * clx.astype(dt) * limx, zero) + np.where(cly != 0, dty * cly.astype(dt) * limy, zero)]
    gmx, gmy = g[:, 0], g[:, 1]
    pw = one / (v[2] + dt(np.float32(1e-6)))
    dv[0] = dv[0] + gmx * fx * pw
    dv[1] = dv[1] + gmy * fy * pw
    dv[2] = dv[2] + -(gmx * fx * v[0] + gmy * fy * v[1]) * pw * pw
    st = lambda l: np.stack(l, axis=1).astype(dt)
    return {"dv": st(dv), "dT0": st(dT0), "dT1": st(dT1), "j00": j00, "j11": j11, "j02": j02, "j12": j12, "z": v[2],
            "clx": clx, "cly": cly}


def contributions(o, scene, cam, radii, g2d, mode="z", scale_modifier=1.0, sh_deg=3):
    """[P, 12] per-row terms of the camera gradient in numpy at o.dtype, linear in the 2-D rows g2d [P, 10]; rows the forward
    wrote nothing for (radii <= 0) are zero"""
    dt = o.dtype
    pos = np.asarray(scene["pos"], dt).reshape(-1, 3)
    P = pos.shape[0]
    g = np.asarray(g2d, dt).reshape(P, N2D)
    on = np.asarray(radii) > 0
    with np.errstate(all="ignore"):
        t = geometry_terms(o, scene, cam, g, scale_modifier)
        gv, z = g[:, 9], t["z"]
        gz = gv if mode == "z" else -gv / (z * z)
        assert mode in maps_ref.MODES
        # the colour step's direction part of dL/dpos: the oracle's own, with the colour gradient alone
        gdir = o.preprocess_backward(scene, cam, radii, np.zeros((P, 2), dt), np.zeros((P, 3), dt), g[:, 6:9],
                                     scale_modifier=scale_modifier, sh_deg=sh_deg)["pos"]
        right, up, front, campos = (np.asarray(getattr(cam, f)[:], dt) for f in ("right", "up", "front", "position"))
        d = pos - campos[None, :]
        dv0, dv1, dv2 = t["dv"][:, 0:1], t["dv"][:, 1:2], (t["dv"][:, 2] + gz)[:, None]
        out = np.zeros((P, 12), dt)
        out[:, 0:3] = -(right[None, :] * dv0 + up[None, :] * dv1 + front[None, :] * dv2 + gdir)
        out[:, 3:6] = dv2 * d + t["j02"][:, None] * t["dT0"] + t["j12"][:, None] * t["dT1"]
        out[:, 6:9] = dv1 * d + t["j11"][:, None] * t["dT1"]
        out[:, 9:12] = dv0 * d + t["j00"][:, None] * t["dT0"]
    out[~on] = 0
    return out


def walk_rows(o, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """(2-D rows [P, 10], forward state) of oracle build `o`: its own forward state, its own render_backward walk for the image
    and -- with maps_ref's colour (v, 1, 0) over a zero background -- for the two map channels"""
    W, H = cam.width, cam.height
    st = o.forward_state(scene, cam, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    P = st["opacity"].shape[0]
    g = np.zeros((P, N2D), o.dtype)
    if dL_dimg is not None:
        gm, gc, go, gcol = o.render_backward(W, H, bg, st["ranges"], st["point_list"], st["means"], st["conic"], st["opacity"],
                                             st["color"], st["final_T"], st["n_contrib"], np.asarray(dL_dimg, o.dtype))
        g[:, 0:2] += gm
        g[:, 2:5] += gc
        g[:, 5] += go
        g[:, 6:9] += gcol
    if dL_ddepth is not None or dL_dalpha is not None:
        v, _ = maps_ref._value(o, scene, cam, mode, scale_modifier)
        gm, gc, go, gcol = o.render_backward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                                             st["opacity"], maps_ref._colour(v), st["final_T"], st["n_contrib"],
                                             maps_ref._dl3(o, dL_ddepth, dL_dalpha, H, W))
        g[:, 0:2] += gm
        g[:, 2:5] += gc
        g[:, 5] += go
        g[:, 9] += gcol[:, 0]
    return g, st


def oracle_dpos(o, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """[P, 3] rows of the oracle's own dL/dpos: render_backward_full, plus maps_ref.backward when map gradients are present"""
    P = np.asarray(scene["pos"]).reshape(-1, 3).shape[0]
    out = np.zeros((P, 3), o.dtype)
    if dL_dimg is not None:
        out = out + o.render_backward_full(scene, cam, dL_dimg, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)["pos"]
    if dL_ddepth is not None or dL_dalpha is not None:
        out = out + maps_ref.backward(o, scene, cam, dL_ddepth, dL_dalpha, mode, scale_modifier, sh_deg)["pos"]
    return out


def reference(o, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """(the twelve column sums in float64, the per-row terms [P, 12]) in oracle build `o`; the position columns are minus the
    rows of the oracle's own dL/dpos, not the restatement"""
    kw = dict(mode=mode, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    g, st = walk_rows(o, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, **kw)
    C = contributions(o, scene, cam, st["radii"], g, mode, scale_modifier, sh_deg)
    C[:, 0:3] = -oracle_dpos(o, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, **kw)
    return C.astype(np.float64).sum(axis=0), C


def unit_jacobian(o64, scene, cam64, radii, mode="z", scale_modifier=1.0, sh_deg=3):
    """C64 [P, 12, 10]: column s = contributions of unit 2-D rows (component s set to 1 on every row), as abs_jacobian_apply
    obtains the preprocess-backward's"""
    P = np.asarray(radii).shape[0]
    J = np.zeros((P, 12, N2D))
    for s in range(N2D):
        unit = np.zeros((P, N2D))
        unit[:, s] = 1.0
        J[:, :, s] = contributions(o64, scene, cam64, radii, unit, mode, scale_modifier, sh_deg)
    return J


def walk_budgets(scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """(A, F) [P, 10] of the walks over the f32 state (o64.render_backward_bound, exactly as maps_ref.row_bound and
    gradient_row_terms take them), the map walk's column 6 (dL/dv) sent to the value slot; and that state"""
    o32, o64, _ = _oracles()
    W, H = ocam.width, ocam.height
    st = o32.forward_state(scene, ocam, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    P = st["opacity"].shape[0]
    A, F = np.zeros((P, N2D)), np.zeros((P, N2D))
    if dL_dimg is not None:
        a, f = o64.render_backward_bound(W, H, np.asarray(bg, np.float32), st["ranges"], st["point_list"], st["means"],
                                         st["conic"], st["opacity"], st["color"], st["final_T"], st["n_contrib"],
                                         np.asarray(dL_dimg, np.float32))
        A[:, :9] += a
        F[:, :9] += f
    if dL_ddepth is not None or dL_dalpha is not None:
        v, _ = maps_ref._value(o32, scene, ocam, mode, scale_modifier)
        a, f = o64.render_backward_bound(W, H, np.zeros(3, np.float32), st["ranges"], st["point_list"], st["means"], st["conic"],
                                         st["opacity"], maps_ref._colour(v), st["final_T"], st["n_contrib"],
                                         maps_ref._dl3(o32, dL_ddepth, dL_dalpha, H, W))
        A[:, :6] += a[:, :6]
        F[:, :6] += f[:, :6]
        A[:, 9] += a[:, 6]
        F[:, 9] += f[:, 6]
    return A, F, st


def position_row_bound(scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """[P, 3]: the existing per-row bound of dL/dpos for this call"""
    if dL_ddepth is None and dL_dalpha is None:
        return gradient_row_bound(scene, ocam, dL_dimg, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)[0]["pos"]
    if dL_dimg is None:
        return maps_ref.row_bound(scene, ocam, dL_ddepth, dL_dalpha, mode, scale_modifier, sh_deg)[0]["pos"]
    return maps_ref.row_bound_with_image(scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, mode, bg, scale_modifier, sh_deg)[0]["pos"]


def bound(scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3, pos_bound=None):
    """(bound [12], r64 [12]) for one call; ocam: the f32 oracle's camera; pos_bound: position_row_bound of the same call when
    the caller has it"""
    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    cam64 = o64.convert_camera(ocam)
    kw = dict(mode=mode, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    r64, c64 = reference(o64, scene, cam64, dL_dimg, dL_ddepth, dL_dalpha, **kw)
    _, c32 = reference(o32, scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, **kw)
    _, c32c = reference(o32c, scene, o32c.convert_camera(ocam), dL_dimg, dL_ddepth, dL_dalpha, **kw)
    noise = np.maximum(np.abs(c32.astype(np.float64) - c64), np.abs(c32c.astype(np.float64) - c64)).sum(axis=0)
    A, F, st = walk_budgets(scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, **kw)
    J = np.abs(unit_jacobian(o64, scene, cam64, st["radii"], mode, scale_modifier, sh_deg))
    JA, JF = np.einsum("pks,ps->k", J, A), np.einsum("pks,ps->k", J, F)
    B = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * JA + JF + GRAD_ROW_FLOOR * JA
    if pos_bound is None:
        pos_bound = position_row_bound(scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, **kw)
    B[0:3] = np.asarray(pos_bound, np.float64).sum(axis=0)
    return B + U32 * np.abs(r64), r64
